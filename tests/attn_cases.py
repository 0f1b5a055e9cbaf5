"""Cases for attn_decode, attn_prefill and the composed prefill path.

The bound.  The output of softmax attention is a convex combination of V
rows, so |out| <= max|V| over the keys a row may attend.  Rounding the
output to bf16 costs at most 2**-9 * max|V|; attn_prefill (and the composed
path) also round P to bf16 before P.V while the normaliser stays fp32,
another 2**-9 * max|V| at most.  fp32 score and accumulation error is orders
of magnitude below that.  A correct kernel therefore stays under
2**-8 * max|V|; the tests allow BOUND = 2**-7 * max|V| per (batch row,
kv head), a factor of two above what the arithmetic explains.

The inputs.  Random K/V cannot see a wrong mask edge: one key in hundreds
moves the output by less than the bound.  Every case therefore plants probe
keys where the kernel decides something - the last key, the first key inside
the window and the one just outside it, both sides of tile and slice edges -
whose K rows score about 14 (or about the softcap) against every q head
while all other keys score about 0.  The probes share nearly all the softmax
mass; each attended probe carries at least 1/16 of it for every head
(asserted in test_attn_cases_cpu.py), so admitting one key too many, or
dropping one, moves the output by several times the bound.  V is uniform in
[-2, 2], so every V row is distinctive and max|V| is about 2.

Decode launch regimes pinned by DECODE_CASES (decode_launch mirrors the
heuristic of attn_decode_impl; `tiles` is the largest number of 256-key
tiles one block walks):
  ns1_*   B*Hkv = 528: nsplit == 1, one block walks 2 or 3 tiles
  s512_*  B*Hkv = 72: 512-key slices, two tiles per slice, host and device
  cap4k_* device position over a 4096-row cache: nsplit 8, per 512
  s256_*  the 256-key-slice regime of the older tests, one tile per slice
"""
import functools
import math
from collections import namedtuple

import torch

BF16 = torch.bfloat16
F64 = torch.float64
BOUND = 2.0 ** -7          # times max|V| over the keys a row may attend
MASS = 1.0 / 16            # least softmax mass of an attended probe key
DEFECT_FACTOR = 4.0        # every defect must miss the bound by this much
SCORE = 14.0               # raw probe score where there is no softcap
GAP = 0.7                  # between the two score levels probes alternate on
MAX_PROBES = 6             # attended probes per decode row
AD_TILE, AP_TILE, AP_QTILE = 256, 32, 64
# the wrong kernels test_attn_cases_cpu.py must see fail: as arguments of
# reference() / *_reference(), or of the tile walk online_softmax()
DEFECTS = ("no_softcap", "window+1", "window-1", "offset+1", "offset-1",
           "drop_last", "drop_first", "drop_tile", "no_factor", "no_alpha",
           "gqa_mod", "scale_dv")


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------

def allowed_keys(offsets, T, S, window):
    """[B, T, S] bool: row t of batch b sits at offsets[b] + t and attends
    keys [max(0, pos - window + 1), pos]."""
    qpos = (torch.as_tensor(offsets)[:, None, None]
            + torch.arange(T)[None, :, None])
    key = torch.arange(S)[None, None, :]
    ok = key <= qpos
    if window > 0:
        ok &= key > qpos - window
    return ok


def scores(q, k, scale, softcap=0.0, gqa_mod=False):
    """fp64 scaled (and softcapped) scores [B, Hkv, G, T, S]; q head h reads
    kv head h // G (h % Hkv under gqa_mod)."""
    B, Hq, T, Dk = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    qg = (q.view(B, G, Hkv, T, Dk).transpose(1, 2) if gqa_mod
          else q.view(B, Hkv, G, T, Dk))
    s = torch.einsum("bkgtd,bksd->bkgts", qg.to(F64), k.to(F64)) * scale
    if softcap > 0:
        s = softcap * torch.tanh(s / softcap)
    return s


def reference(q, k, v, scale, offsets, softcap=0.0, window=0, gqa_mod=False,
              drop=None):
    """fp64 masked softmax attention on bf16 inputs.  q [B, Hq, T, Dk],
    k [B, Hkv, S, Dk], v [B, Hkv, S, Dv]; offsets[b] is the position of
    row 0 of batch b.  drop: [B, T, S] bool of keys to mask on top.
    Returns (out [B, Hq, T, Dv], probabilities [B, Hq, T, S])."""
    B, Hq, T, _ = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    ok = allowed_keys(offsets, T, S, window)
    if drop is not None:
        ok = ok & ~drop
    s = scores(q, k, scale, softcap, gqa_mod)
    s = s.masked_fill(~ok[:, None, None], float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bkgts,bksd->bkgtd", p, v.to(F64))
    if gqa_mod:
        out, p = out.transpose(1, 2), p.transpose(1, 2)
    return out.reshape(B, Hq, T, -1), p.reshape(B, Hq, T, S)


def bounds(v, offsets, T, window):
    """[B, Hkv]: BOUND * max|V| over the keys any row of the batch row may
    attend."""
    ok = allowed_keys(offsets, T, v.shape[2], window).any(1)       # [B, S]
    vmax = v.to(F64).abs().amax(-1).masked_fill(~ok[:, None], 0.0)
    return BOUND * vmax.amax(-1)


def worst_ratio(got, want, bound):
    """max over (b, kv head) of max|got - want| / bound[b, kv head]."""
    B, Hq = got.shape[:2]
    Hkv = bound.shape[1]
    err = (got.to(F64) - want).abs().reshape(B, Hkv, -1).amax(-1)
    return (err / bound).max().item()


# --------------------------------------------------------------------------
# the kernels' tiling, emulated in fp64
# --------------------------------------------------------------------------

def online_softmax(s, v, slices, round_p=False, drop_tile=None,
                   no_alpha=False, no_factor=False, alphas=None):
    """s [..., R, S] masked scores, v [..., S, Dv] (broadcast over R rows).
    slices: a list of slices, each a list of (t0, t1) key tiles walked with
    a running (m, l, acc); the slice partials are combined with
    exp(m_s - m*).  round_p rounds P to bf16 for P.V only, as attn_prefill
    does.  The keyword defects: drop_tile = (slice, tile) skipped,
    no_alpha = acc not rescaled when the running max moves, no_factor =
    partials summed without exp(m_s - m*).  alphas: a list that receives
    the smallest rescale factor applied to a non-empty accumulator."""
    ninf = float("-inf")
    parts = []
    for si, tiles in enumerate(slices):
        m = torch.full(s.shape[:-1], ninf, dtype=F64)
        l = torch.zeros(s.shape[:-1], dtype=F64)
        acc = torch.zeros(*s.shape[:-1], v.shape[-1], dtype=F64)
        for ti, (t0, t1) in enumerate(tiles):
            if drop_tile == (si, ti):
                continue
            st = s[..., t0:t1]
            mnew = torch.maximum(m, st.amax(-1))
            live = mnew > ninf
            safe = torch.where(live, mnew, torch.zeros_like(mnew))
            alpha = torch.where(live, torch.exp(m - safe), torch.ones_like(m))
            if alphas is not None and (m > ninf).any():
                alphas.append(alpha[m > ninf].min().item())
            p = torch.exp(st - safe[..., None])
            l = l * alpha + p.sum(-1)
            if round_p:
                p = p.to(BF16).to(F64)
            if no_alpha:
                alpha = torch.ones_like(alpha)
            acc = acc * alpha[..., None] + p @ v[..., t0:t1, :]
            m = mnew
        parts.append((m, l, acc))
    mstar = torch.stack([m for m, _, _ in parts]).amax(0)
    num, den = 0.0, 0.0
    for m, l, acc in parts:
        w = torch.exp(m - mstar)
        if no_factor:
            w = torch.where(m > ninf, torch.ones_like(w), w)
        num, den = num + acc * w[..., None], den + l * w
    return num / den[..., None]


def decode_launch(B, Hkv, span):
    """(nsplit, per) of attn_decode_impl / attn_decode_kernel for a key span
    (the host length, or the cache capacity under a device position)."""
    slice_ = 256 if B * Hkv <= 64 else 512
    nsplit = min(8, max(1, 1024 // max(1, B * Hkv)),
                 max(1, -(-span // slice_)))
    if nsplit == 1:
        return 1, span
    return nsplit, -(-(-(-span // nsplit)) // AD_TILE) * AD_TILE


def decode_slices(L, window, nsplit, per):
    """The (t0, t1) tiles each slice's block walks for a row of length L."""
    lo0 = L - window if 0 < window < L else 0
    out = []
    for sp in range(nsplit):
        lo, hi = max(lo0, per * sp), min(L, per * (sp + 1))
        out.append([(t, min(t + AD_TILE, hi)) for t in range(lo, hi, AD_TILE)])
    return out


def prefill_slices(S):
    return [[(t, min(t + AP_TILE, S)) for t in range(0, S, AP_TILE)]]


# --------------------------------------------------------------------------
# decode cases
# --------------------------------------------------------------------------

# runs: (mode, lens, nsplit, tiles) with mode host | shared | ragged
DecodeCase = namedtuple(
    "DecodeCase", "name B Hq Hkv Dk Dv alias cap softcap window runs")


def _uni(B, L, host, dev):
    lens = (L,) * B
    return [("host", lens) + host, ("shared", lens) + dev,
            ("ragged", lens) + dev]


def _dc(name, B, Hq, Hkv, Dk, Dv, cap, runs, softcap=0.0, window=0,
        alias=False):
    return DecodeCase(name, B, Hq, Hkv, Dk, Dv, alias, cap, softcap, window,
                      runs)


DECODE_CASES = [
    # B*Hkv = 528 -> nsplit 1 in every mode; one block walks all tiles
    _dc("ns1_s300", 33, 16, 16, 64, 64, 520, _uni(33, 300, (1, 2), (1, 2))),
    _dc("ns1_s513", 33, 16, 16, 64, 64, 520, _uni(33, 513, (1, 3), (1, 3))),
    # window start 213: tiles [213, 469) and [469, 513)
    _dc("ns1_s513_w300_cap50", 33, 16, 16, 64, 64, 520,
        _uni(33, 513, (1, 2), (1, 2)), softcap=50.0, window=300),
    # B*Hkv = 72 -> 512-key slices; capacity 1025 gives the device modes
    # three slices, the last of one key
    _dc("s512_513_g2", 9, 16, 8, 64, 64, 1025,
        _uni(9, 513, (2, 2), (3, 2))),
    _dc("s512_600_g6_cap30", 9, 48, 8, 64, 64, 1025,
        _uni(9, 600, (2, 2), (3, 2)), softcap=30.0),
    # window start 925: slice 0 empty, slice 2 is key 1024 alone
    _dc("s512_1025_g7_w100", 9, 56, 8, 64, 64, 1025,
        _uni(9, 1025, (3, 1), (3, 1)), window=100),
    # window start 425: [425, 512), [512, 1024) in two tiles, [1024, 1025)
    _dc("s512_1025_g2_w600_cap50", 9, 16, 8, 64, 64, 1025,
        _uni(9, 1025, (3, 2), (3, 2)), softcap=50.0, window=600),
    # capacity 4096, B*Hkv <= 6: device modes run nsplit 8, per 512
    _dc("cap4k_mla32", 3, 32, 1, 576, 512, 4096,
        [("ragged", (1, 513, 4096), 8, 2)] + _uni(3, 4096, (8, 2), (8, 2)),
        alias=True),
    _dc("cap4k_mla16", 3, 16, 1, 576, 512, 4096,
        [("ragged", (256, 257, 700), 8, 2), ("ragged", (512, 1, 4096), 8, 2)],
        alias=True),
    # window start 3096 at L = 4096: slices 6 and 7, two tiles each
    _dc("cap4k_mla4_w1000", 3, 4, 1, 576, 512, 4096,
        [("ragged", (700, 4096, 513), 8, 2)], window=1000, alias=True),
    _dc("cap4k_g4_dv320", 3, 8, 2, 72, 320, 4096,
        [("ragged", (257, 512, 700), 8, 2)] + _uni(3, 700, (3, 1), (8, 2))),
    _dc("cap4k_g32_dv64", 3, 32, 1, 80, 64, 4096,
        [("ragged", (1, 256, 513), 8, 2)], alias=True),
    # window 100: at L = 700 the leading slices are empty (two of three on
    # the host, one of eight on the device); at 4096 only slice 7 runs
    _dc("cap4k_g8_w100_cap50", 3, 16, 2, 192, 128, 4096,
        [("ragged", (700, 1, 4096), 8, 1)] + _uni(3, 700, (3, 1), (8, 1)),
        softcap=50.0, window=100),
    _dc("cap4k_g16_w1", 3, 16, 1, 128, 256, 4096,
        [("ragged", (513, 257, 4096), 8, 1)] + _uni(3, 257, (2, 1), (8, 1)),
        window=1),
    # the 256-key-slice regime: capacity 1024 -> four one-tile slices
    _dc("s256_g1", 3, 4, 4, 128, 128, 1024,
        [("ragged", (1, 255, 257), 4, 1), ("ragged", (256, 257, 1), 4, 1)]
        + _uni(3, 1, (1, 1), (4, 1)) + _uni(3, 255, (1, 1), (4, 1))
        + _uni(3, 256, (1, 1), (4, 1)) + _uni(3, 257, (2, 1), (4, 1))),
    _dc("s256_g2_cap50", 3, 8, 4, 128, 128, 1024,
        [("ragged", (255, 256, 257), 4, 1)] + _uni(3, 257, (2, 1), (4, 1)),
        softcap=50.0),
    _dc("s256_g4_w300_cap30", 3, 8, 2, 128, 128, 1024,    # window >= S
        [("ragged", (1, 256, 257), 4, 1)] + _uni(3, 257, (2, 1), (4, 1)),
        softcap=30.0, window=300),
    _dc("s256_g7_w1", 3, 28, 4, 128, 128, 1024,
        [("ragged", (255, 256, 257), 4, 1)] + _uni(3, 256, (1, 1), (4, 1)),
        window=1),
]


def decode_runs():
    return [(c, mode, lens, ns, tiles) for c in DECODE_CASES
            for mode, lens, ns, tiles in c.runs]


def run_launch(case, mode, lens):
    """(nsplit, per) the binding picks for a run."""
    span = lens[0] if mode == "host" else case.cap
    return decode_launch(case.B, case.Hkv, span)


def decode_probes(case, L):
    """(attended probe keys, the key just outside the window or None) for a
    row of length L.  At most MAX_PROBES attended keys, kept in this order:
    the last key, the first key inside the window, both sides of the tile
    edges 255/256 and 511/512, then both sides of the slice edges of the
    host and the device launch from the top down."""
    lo = L - case.window if 0 < case.window < L else 0
    want = [L - 1, lo, 255, 256, 511, 512]
    edges = set()
    for span in (L, case.cap):
        nsplit, per = decode_launch(case.B, case.Hkv, span)
        edges |= {per * i for i in range(1, nsplit)}
    for e in sorted(edges, reverse=True):
        want += [e, e - 1]
    keep = []
    for j in want:
        if lo <= j < L and j not in keep and len(keep) < MAX_PROBES:
            keep.append(j)
    return keep, (lo - 1 if lo > 0 else None)


def _flatten(softcap):
    """d/dx of softcap * tanh(x / softcap) at x = softcap."""
    return math.cosh(1.0) ** -2 if softcap > 0 else 1.0


def _noise_sigma(Dk, nfeat, softcap):
    """q noise such that a key's (capped) score wanders by about 0.07
    between heads: heads of one group then weigh the probes differently,
    yet every probe keeps its share."""
    return 0.07 / _flatten(softcap) / (
        Dk ** -0.5 * math.sqrt(Dk - nfeat) * 2 / math.sqrt(3))


def _peak(softcap, level, unit):
    """K feature value of a probe: raw score SCORE (or the softcap) plus or
    minus what leaves the two levels GAP apart after the softcap, so that
    raw scores straddle the cap.  unit = scale * (q feature sum)."""
    half = GAP / 2 / _flatten(softcap)
    return ((softcap or SCORE) + (half if level % 2 == 0 else -half)) / unit


def _uniform(g, *shape):
    return torch.rand(*shape, generator=g) * 4 - 2


@functools.lru_cache(maxsize=4)
def decode_inputs(name, lens):
    """Seeded CPU tensors for one run: q [B, Hq, 1, Dk], kbuf and vbuf over
    the whole capacity (vbuf is kbuf[..., :Dv] when aliased), scale.  The
    last 8 K columns carry the probe signal: zero for ordinary keys, and for
    probe keys the value that scores about SCORE (or the softcap) against
    the 4.0 every q head holds there, on one of two levels."""
    c = next(c for c in DECODE_CASES if c.name == name)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7919 + sum(lens))
    scale = c.Dk ** -0.5
    q = torch.randn(c.B, c.Hq, 1, c.Dk, generator=g) \
        * _noise_sigma(c.Dk, 8, c.softcap)
    q[..., -8:] = 4.0
    kbuf = _uniform(g, c.B, c.Hkv, c.cap, c.Dk)
    kbuf[..., -8:] = 0.0
    for b, L in enumerate(lens):
        keys, outside = decode_probes(c, L)
        for j in keys + ([outside] if outside is not None else []):
            # the upper level for the last key, the key outside the window
            # and the odd 256-key tiles, the lower one for the first key of
            # the window: a block that walks from an even
            # tile into an odd one must rescale its accumulator
            low = j not in (L - 1, outside) and (
                j == keys[1] or j // AD_TILE % 2 == 0)
            kbuf[b, :, j, -8:] = _peak(c.softcap, int(low), scale * 8 * 4.0)
    kbuf = kbuf.to(BF16)
    vbuf = (kbuf[..., :c.Dv] if c.alias
            else _uniform(g, c.B, c.Hkv, c.cap, c.Dv).to(BF16))
    return q.to(BF16), kbuf, vbuf, scale


def decode_reference(case, lens, **kw):
    """reference() of a run, row by row over each row's own length:
    (out [B, Hq, Dv], p: list of [Hq, L_b], bound [B, Hkv])."""
    q, kbuf, vbuf, scale = decode_inputs(case.name, lens)
    kw.setdefault("softcap", case.softcap)
    kw.setdefault("window", case.window)
    kw.setdefault("scale", scale)
    drop_key = kw.pop("drop_key", None)
    outs, ps, bnd = [], [], []
    for b, L in enumerate(lens):
        drop = None
        if drop_key is not None and drop_key(L) is not None:
            drop = torch.zeros(1, 1, L, dtype=torch.bool)
            drop[..., drop_key(L)] = True
        o, p = reference(q[b:b + 1], kbuf[b:b + 1, :, :L], vbuf[b:b + 1, :, :L],
                         offsets=[L - 1], drop=drop, **kw)
        outs.append(o[0, :, 0])
        ps.append(p[0, :, 0])
        bnd.append(bounds(vbuf[b:b + 1, :, :L], [L - 1], 1, case.window)[0])
    return torch.stack(outs), ps, torch.stack(bnd)


def decode_emulation(case, mode, lens, rows=None, **defect):
    """The split-S launch of a run walked in fp64: out [B, Hq, Dv] (or the
    given batch rows only)."""
    q, kbuf, vbuf, scale = decode_inputs(case.name, lens)
    nsplit, per = run_launch(case, mode, lens)
    G = case.Hq // case.Hkv
    outs = []
    for b, L in enumerate(lens):
        if rows is not None and b not in rows:
            continue
        s = scores(q[b:b + 1], kbuf[b:b + 1, :, :L], scale, case.softcap)[0]
        ok = allowed_keys([L - 1], 1, L, case.window)[0]
        s = s.masked_fill(~ok, float("-inf"))[:, :, 0]          # [Hkv, G, L]
        o = online_softmax(s, vbuf[b, :, :L].to(F64),
                           decode_slices(L, case.window, nsplit, per),
                           **defect)
        outs.append(o.reshape(case.Hq, -1))
    return torch.stack(outs)


# --------------------------------------------------------------------------
# prefill cases
# --------------------------------------------------------------------------

PrefillCase = namedtuple(
    "PrefillCase", "name B Hq Hkv Dk Dv T offset cap softcap window")


def _pc(B, Hq, Hkv, Dk, Dv, T, offset, softcap=0.0, window=0, tag="pf"):
    name = f"{tag}_{Dk}x{Dv}_g{Hq // Hkv}_T{T}_o{offset}"
    name += (f"_w{window}" if window else "") \
        + (f"_cap{softcap:g}" if softcap else "")
    return PrefillCase(name, B, Hq, Hkv, Dk, Dv, T, offset,
                       (offset + T + 40) // 32 * 32, softcap, window)


PREFILL_PAIRS = [(32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128),
                 (128, 32), (128, 64), (128, 128), (192, 64), (192, 128),
                 (256, 256)]

PREFILL_CASES = (
    # every instantiation once: window and softcap alternate
    [_pc(2, 4, 2, dk, dv, 17, 31, softcap=(50.0, 0.0)[i % 2],
         window=(0, 20, 0)[i % 3]) for i, (dk, dv) in enumerate(PREFILL_PAIRS)]
    # wave edge, block edge, three blocks x offsets at the 32-key tile edges
    + [_pc(1, 4, 2, 128, 128, T, off, softcap=50.0 if off in (1, 32) else 0.0)
       for T in (1, 15, 16, 17, 64, 65, 130) for off in (0, 1, 31, 32, 64)]
    + [
        # s_lo > 0 in the third block only (64+128-40+1 = 153 -> 128)
        _pc(1, 4, 2, 128, 128, 130, 64, window=40),
        _pc(1, 4, 2, 128, 128, 130, 64, window=40, softcap=30.0),
        # s_lo > 0 from the first block on (96-33+1 = 64)
        _pc(1, 4, 2, 128, 128, 130, 96, window=33),
        _pc(1, 4, 2, 128, 128, 65, 32, window=1),
        _pc(1, 4, 2, 128, 128, 65, 31, window=32),
        _pc(2, 2, 2, 128, 128, 65, 31),
        _pc(2, 8, 1, 128, 128, 65, 31, softcap=50.0),
    ])

# shapes attn_prefill does not serve run the composed path of ops.attention
FALLBACK_CASES = [
    _pc(2, 4, 2, 48, 48, 17, 31, tag="fb"),
    _pc(2, 4, 2, 48, 48, 17, 31, softcap=50.0, window=20, tag="fb"),
    _pc(1, 4, 2, 48, 48, 65, 32, window=12, tag="fb"),
]


def _nfeat(case):
    """Period of the one-hot key signal: short cases need a short period for
    a row to see more than one marked key."""
    S = case.offset + case.T
    return min(16 if S <= 48 else 32 if S <= 96 else 64, case.Dk // 32 * 16)


def prefill_marks(case, t):
    """Key positions row t marks: its last key, the future key behind it,
    the first key in its window and the key just outside."""
    pos = case.offset + t
    marks = [pos, pos + 1]
    if case.window:
        marks += [pos - case.window + 1, pos - case.window]
    return [j for j in marks if j >= 0]


@functools.lru_cache(maxsize=4)
def prefill_inputs(case):
    """Seeded CPU tensors: q [B, Hq, T, Dk], kbuf/vbuf over the capacity,
    scale.  The last P K columns are one-hot in (key mod P); row t of q
    holds 4.0 in the columns of the keys it marks, so those keys (and the
    ones P, 2P, ... before them) score about SCORE or the softcap, on
    two alternating levels."""
    c = case
    g = torch.Generator().manual_seed(sum(map(ord, c.name)) * 104729)
    P = _nfeat(c)
    scale = c.Dk ** -0.5
    q = torch.randn(c.B, c.Hq, c.T, c.Dk, generator=g) \
        * _noise_sigma(c.Dk, P, c.softcap)
    q[..., -P:] = 0.0
    for t in range(c.T):
        for j in prefill_marks(c, t):
            q[:, :, t, c.Dk - P + j % P] = 4.0
    kbuf = _uniform(g, c.B, c.Hkv, c.cap, c.Dk)
    kbuf[..., -P:] = 0.0
    j = torch.arange(c.cap)
    for lvl in (0, 1):
        jj = j[(j + j // P) % 2 == lvl]
        kbuf[:, :, jj, c.Dk - P + jj % P] = _peak(c.softcap, lvl, scale * 4.0)
    vbuf = _uniform(g, c.B, c.Hkv, c.cap, c.Dv)
    return q.to(BF16), kbuf.to(BF16), vbuf.to(BF16), scale


def prefill_reference(case, d_offset=0, **kw):
    """reference() of a prefill case: (out, p, bound [B, Hkv]).  d_offset
    shifts causal_offset for the defects."""
    q, kbuf, vbuf, scale = prefill_inputs(case)
    S = case.offset + case.T
    kw.setdefault("softcap", case.softcap)
    kw.setdefault("window", case.window)
    kw.setdefault("scale", scale)
    out, p = reference(q, kbuf[:, :, :S], vbuf[:, :, :S],
                       offsets=[case.offset + d_offset] * case.B, **kw)
    return out, p, bounds(vbuf[:, :, :S], [case.offset] * case.B, case.T,
                          case.window)


def prefill_emulation(case, **defect):
    """The 32-key tile walk of attn_prefill in fp64 with P rounded to bf16
    for P.V: out [B, Hq, T, Dv].  (Tiles a row cannot see contribute
    nothing, so walking all of them equals the kernel's skipping.)"""
    q, kbuf, vbuf, scale = prefill_inputs(case)
    S = case.offset + case.T
    s = scores(q, kbuf[:, :, :S], scale, case.softcap)
    ok = allowed_keys([case.offset] * case.B, case.T, S, case.window)
    s = s.masked_fill(~ok[:, None, None], float("-inf"))
    o = online_softmax(s, vbuf[:, :, None, :S].to(F64), prefill_slices(S),
                       round_p=True, **defect)
    return o.reshape(case.B, case.Hq, case.T, -1)
