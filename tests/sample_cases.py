"""Cases for ops.sample_rows, shared by the CPU and GPU tests: an fp64
numpy implementation of the specification (reference.sample_rows'
docstring) and a builder that designs every row's top_p and u so that the
expected id is exact, not statistical.

Exactness condition, asserted by the builder for every sampled row
(normalized mass, fp64):
  * top_p sits at least MARGIN = 2e-3 from the nearest cumulative-mass
    boundary of the nucleus rule (the mass strictly above each tie class
    other than the top one, which is always kept);
  * u sits at least MARGIN from both ends of its target token's CDF
    interval over the kept set.
The builder places both at midpoints of gaps opened by tokens with
p >= 2 * MARGIN (2.02, so that rounding the midpoint to fp32 keeps it).
Why 2e-3: a worst-order (sequential) fp32 CDF differed from fp64 by at
most 1.2e-4 (V = 256 000, normal x 3, T = 1) and 1.1e-4 (V = 129 280,
normal x 4); 2e-3 is 16 times that, so any fp32 summation order picks the
same ids (test_sample_rows_cpu.py checks a sequential one).

DYADIC cases are the one exception, kept apart: rows whose probabilities
are powers of two, so every fp32 sum is exact in any order, with u * Z
exactly ON a CDF step.  Only they can tell ``>`` from ``>=`` in the pick
(under a 2e-3 margin the two agree by construction).

Rows: "staircase" rows put a handful of distinct heavy tokens at index 0,
V-1 and on both sides of a chunk boundary of the kernel (its 16 wave
chunks of ceil(V/16), its 64-lane tiles, its 1024-thread stride) over a
uniform tail; "normal" rows are seeded N(0, 1) * scale * T, scale 2..6.
"""

import functools
import math

import numpy as np

MARGIN = 2e-3
VOCABS = (1, 2, 63, 64, 65, 1000, 4099)
BIG_V = 129280
TEMPS = (0.0, 0.5, 1.0, 1.7)
KERNEL_BLOCK, KERNEL_WAVES, WAVE = 1024, 16, 64
MAX_BIAS, MAX_WINDOW = 32, 64

f32 = np.float32


# -- the specification in fp64 ------------------------------------------------

def apply_edits(x, bias_idx=None, bias_val=None, pen_idx=None, penalty=None,
                per_occurrence=False):
    """Step 1 on one fp32 row, in fp32 like the kernel (in place).
    per_occurrence is the negative control: the penalty once per window
    entry instead of once per distinct token."""
    if bias_idx is not None:
        for k, v in zip(bias_idx, bias_val):
            if k >= 0:
                x[k] = f32(x[k] + f32(v))
    if pen_idx is not None and f32(penalty) != f32(1.0):
        toks = [int(k) for k in pen_idx if k >= 0]
        if not per_occurrence:
            toks = sorted(set(toks))
        pen = f32(penalty)
        for k in toks:
            x[k] = f32(x[k] / pen) if x[k] > 0 else f32(x[k] * pen)
    return x


def keep_set(p, top_p):
    """Token i stays iff the mass of tokens with p_j > p_i is < top_p; the
    top class always stays."""
    vals, inv = np.unique(p, return_inverse=True)      # ascending classes
    mass = np.bincount(inv, weights=p, minlength=len(vals))
    above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])
    keep = above[inv] < top_p
    keep[inv == len(vals) - 1] = True
    return keep


def class_boundaries(p):
    """Mass strictly above every tie class but the top one, descending
    class order: where the kept set changes as top_p moves."""
    vals, inv = np.unique(p, return_inverse=True)
    mass = np.bincount(inv, weights=p, minlength=len(vals))[::-1]
    return np.cumsum(mass)[:-1], mass


def softmax64(x, T):
    z = x.astype(np.float64) / float(f32(T))
    e = np.exp(z - z.max())
    return e / e.sum()


def spec_row(x, T, top_p, u, ignore_nucleus=False, pick_ge=False):
    """Steps 2-5 on one edited fp32 row: (id, lse, keep or None).  The
    two flags are negative controls."""
    x64 = x.astype(np.float64)
    m = x64.max()
    lse = m + math.log(np.exp(x64 - m).sum())
    if float(T) <= 0.0:
        return int(np.argmax(x64)), lse, None
    p = softmax64(x, T)
    keep = np.ones(len(p), dtype=bool)
    if float(top_p) < 1.0 and not ignore_nucleus:
        keep = keep_set(p, float(f32(top_p)))
    kept = np.where(keep, p, 0.0)
    cdf = np.cumsum(kept)
    t = float(f32(u)) * cdf[-1]
    hit = keep & ((cdf >= t) if pick_ge else (cdf > t))
    idx = np.nonzero(hit)[0]
    tid = int(idx[0]) if len(idx) else int(np.nonzero(keep)[0][-1])
    return tid, lse, keep


def spec_case(case, **controls):
    """Expected (edited logits, ids, lse, keeps) of a case; inactive rows
    keep the case's initial ids / lse and keep None."""
    edit_kw = {k: controls.pop(k) for k in ("per_occurrence",)
               if k in controls}
    logits = case["logits"].copy()
    ids = case["ids_init"].copy()
    lse = case["lse_init"].astype(np.float64)
    keeps = [None] * len(ids)
    for b in range(len(ids)):
        if not case["active"][b]:
            continue
        apply_edits(
            logits[b],
            None if case["bias_idx"] is None else case["bias_idx"][b],
            None if case["bias_val"] is None else case["bias_val"][b],
            None if case["pen_idx"] is None else case["pen_idx"][b],
            None if case["penalty"] is None else case["penalty"][b],
            **edit_kw)
        ids[b], lse[b], keeps[b] = spec_row(
            logits[b], case["temperature"][b], case["top_p"][b],
            case["u"][b], **controls)
    return logits, ids, lse, keeps


# -- rows -----------------------------------------------------------------------

def staircase_positions(V, c):
    """Index 0, V-1, both sides of wave-chunk boundary c, of the first
    64-lane tile boundary and of the first block-stride boundary."""
    chunk = -(-V // KERNEL_WAVES)
    pos = {0, V - 1, c * chunk - 1, c * chunk, WAVE - 1, WAVE,
           KERNEL_BLOCK - 1, KERNEL_BLOCK}
    return sorted(k for k in pos if 0 <= k < V)


def staircase_row(V, T, c, rng):
    """Distinct heavy tokens (steps of 0.3 after the temperature) over a
    uniform tail at 0; which position gets which height is shuffled."""
    t_eff = T if T > 0 else 1.0
    pos = staircase_positions(V, c)
    heights = [t_eff * (math.log(V) + 3.0 - 0.3 * j) for j in range(len(pos))]
    x = np.zeros(V, dtype=f32)
    x[rng.permutation(pos)] = np.asarray(heights, dtype=f32)
    return x


def normal_row(V, T, scale, rng):
    t_eff = T if T > 0 else 1.0
    return (rng.standard_normal(V) * scale * t_eff).astype(f32)


# -- designing top_p and u --------------------------------------------------------

def design_top_p(x, T, kind, sel):
    """top_p of the wanted kind for an edited row: 0, 1, or the midpoint
    of a gap between two cumulative-mass boundaries opened by a class of
    mass >= 2 * MARGIN."""
    if kind == "zero":
        return f32(0.0)
    if kind == "one" or T <= 0:
        return f32(1.0)
    bounds, mass = class_boundaries(softmax64(x, T))
    edges = np.concatenate([[0.0], bounds, [1.0]])   # gap c is class c's
    wide = [c for c in range(len(mass)) if mass[c] >= 2.02 * MARGIN]
    assert wide, "no class with mass >= 4e-3"
    c = wide[sel % len(wide)]
    return f32(0.5 * (edges[c] + edges[c + 1]))


def top_p_margin(x, T, top_p):
    if T <= 0 or float(top_p) >= 1.0:
        return math.inf
    bounds, _ = class_boundaries(softmax64(x, T))
    if len(bounds) == 0:
        return math.inf
    return float(np.abs(bounds - float(top_p)).min())


def design_u(x, T, top_p, sel):
    """(u, margin): the midpoint of the CDF interval of a kept token with
    p / Z >= 2 * MARGIN."""
    if T <= 0:
        return f32(0.5), math.inf
    p = softmax64(x, T)
    keep = keep_set(p, float(top_p)) if float(top_p) < 1.0 \
        else np.ones(len(p), dtype=bool)
    kept = np.where(keep, p, 0.0)
    cdf = np.cumsum(kept) / kept.sum()
    lo = np.concatenate([[0.0], cdf[:-1]])
    cand = np.nonzero(keep & (cdf - lo >= 2.02 * MARGIN))[0]
    assert len(cand), "no kept token with p / Z >= 4e-3"
    t = cand[sel % len(cand)]
    u = f32(0.5 * (lo[t] + cdf[t]))
    return u, float(min(float(u) - lo[t], cdf[t] - float(u)))


def _finish(name, rows, bias=None, pen=None, seed=0):
    """Assemble a case from rows of (x, T, kind, active): apply the edits,
    design top_p and u on the edited row, assert the exactness condition
    and record the fp64 expectation."""
    rng = np.random.default_rng(seed)
    B, V = len(rows), len(rows[0][0])
    case = {
        "name": name,
        "logits": np.stack([r[0] for r in rows]).astype(f32),
        "temperature": np.asarray([r[1] for r in rows], dtype=f32),
        "active": np.asarray([r[3] for r in rows], dtype=np.int32),
        "top_p": np.ones(B, dtype=f32),
        "u": np.full(B, 0.5, dtype=f32),
        "ids_init": rng.integers(0, V, B).astype(np.int64),
        "lse_init": rng.standard_normal(B).astype(f32),
        "bias_idx": None, "bias_val": None, "pen_idx": None, "penalty": None,
    }
    if bias is not None:
        case["bias_idx"] = np.asarray(bias[0], dtype=np.int32)
        case["bias_val"] = np.asarray(bias[1], dtype=f32)
    if pen is not None:
        case["pen_idx"] = np.asarray(pen[0], dtype=np.int32)
        case["penalty"] = np.asarray(pen[1], dtype=f32)
    edited, _, _, _ = spec_case(case)
    for b, (_, T, kind, active) in enumerate(rows):
        if not active:
            # parameters that would sample if the row were (wrongly) run
            case["top_p"][b], case["u"][b] = f32(0.9), f32(0.3)
            continue
        T = float(f32(T))
        tp = design_top_p(edited[b], T, kind, sel=3 * b + seed)
        u, u_margin = design_u(edited[b], T, tp, sel=5 * b + seed + 1)
        assert top_p_margin(edited[b], T, tp) >= MARGIN, (name, b)
        assert u_margin >= MARGIN, (name, b)
        case["top_p"][b], case["u"][b] = tp, u
    (case["want_logits"], case["want_ids"], case["want_lse"],
     case["want_keep"]) = spec_case(case)
    return case


def _grid_case(V, seed):
    """Every temperature x every top_p kind, staircase and normal rows
    alternating, an inactive row after every third active one."""
    rng = np.random.default_rng(seed)
    rows, n = [], 0
    for T in TEMPS:
        for kind in ("zero", "mid", "one"):
            # top_p = 1 keeps the whole tail: only a staircase row has
            # targets with p >= 4e-3 at every V
            if kind == "one" or n % 2 == 0:
                x = staircase_row(V, T, c=1 + n % (KERNEL_WAVES - 1), rng=rng)
            else:
                x = normal_row(V, T, scale=2 + n % 5, rng=rng)
            rows.append((x, T, kind, 1))
            n += 1
            if n % 3 == 0:
                rows.append((normal_row(V, 1.0, 3, rng), 0.8, "mid", 0))
    return _finish(f"grid-V{V}", rows, seed=seed)


def _big_case():
    rng = np.random.default_rng(11)
    V = BIG_V
    rows = [
        (staircase_row(V, 1.7, c=KERNEL_WAVES - 1, rng=rng), 1.7, "one", 1),
        (normal_row(V, 1.0, 4, rng), 1.0, "mid", 1),
        (normal_row(V, 0.5, 6, rng), 0.5, "mid", 1),
    ]
    return _finish("big-V129280", rows, seed=11)


def _argmax_tie_case():
    """Greedy rows whose maximum occurs twice: the lowest index wins,
    across a wave chunk, a tile and the block stride."""
    V = 4099
    rows = []
    for pair in ((5, 4098), (63, 64), (1023, 1024), (256, 257), (2000, 70)):
        x = np.zeros(V, dtype=f32)
        x[list(pair)] = 4.5
        rows.append((x, 0.0, "one", 1))
    return _finish("argmax-ties", rows, seed=5)


def _edits_case():
    """Bias only, penalty only, both on one token, duplicate and -1 window
    entries, a penalized negative logit, penalty == 1, an inactive row
    whose edits must not be applied."""
    V, rng = 1000, np.random.default_rng(7)
    base = [normal_row(V, 1.0, 3, rng) for _ in range(7)]
    top = [int(np.argmax(x)) for x in base]
    low = [int(np.argmin(x)) for x in base]
    NB, W = 3, 6
    bias_idx = -np.ones((7, NB), dtype=np.int32)
    bias_val = np.zeros((7, NB), dtype=f32)
    pen_idx = -np.ones((7, W), dtype=np.int32)
    penalty = np.ones(7, dtype=f32)
    # 0: bias only — lifts a mid token to the top, sinks the old top
    bias_idx[0] = [500, -1, top[0]]
    bias_val[0] = [9.25, 0.0, -3.5]
    # 1: penalty only, distinct tokens
    pen_idx[1, :3] = [top[1], 17, 900]
    penalty[1] = 1.3
    # 2: bias and penalty on one token (bias first)
    bias_idx[2, 0], bias_val[2, 0] = top[2], 2.0
    pen_idx[2, 0], penalty[2] = top[2], 1.7
    # 3: duplicates and -1 pads between entries
    pen_idx[3] = [top[3], -1, top[3], 33, top[3], -1]
    penalty[3] = 1.5
    # 4: a penalized negative logit (x * pen) beside a positive one
    assert base[4][low[4]] < 0 < base[4][top[4]]
    pen_idx[4, :3] = [low[4], top[4], low[4]]
    penalty[4] = 2.0
    # 5: inactive, with edits that must not land
    bias_idx[5, 0], bias_val[5, 0] = top[5], -50.0
    pen_idx[5, 0], penalty[5] = top[5], 3.0
    # 6: a window with penalty == 1 is a no-op
    pen_idx[6, :2] = [top[6], 12]
    rows = [(base[b], T, kind, b != 5) for b, (T, kind) in enumerate(
        [(1.0, "mid"), (0.5, "mid"), (1.7, "mid"), (1.0, "zero"),
         (1.0, "mid"), (1.0, "mid"), (0.0, "one")])]
    return _finish("edits-V1000", rows, bias=(bias_idx, bias_val),
                   pen=(pen_idx, penalty), seed=7)


@functools.lru_cache(maxsize=None)
def cases():
    out = [_grid_case(V, seed=20 + i) for i, V in enumerate(VOCABS)]
    out += [_argmax_tie_case(), _edits_case(), _big_case()]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dyadic_cases():
    """u * Z exactly on a CDF step (see the module docstring): V equal
    logits, V a power of two, so every p is 1/V and every partial sum is
    exact in fp32 in any order."""
    out = []
    for V, u in ((2, 0.5), (4, 0.25), (64, 0.5), (128, 0.75)):
        case = {
            "name": f"dyadic-V{V}",
            "logits": np.full((1, V), 1.5, dtype=f32),
            "temperature": np.ones(1, dtype=f32),
            "top_p": np.ones(1, dtype=f32),
            "u": np.full(1, u, dtype=f32),
            "active": np.ones(1, dtype=np.int32),
            "ids_init": np.zeros(1, dtype=np.int64),
            "lse_init": np.zeros(1, dtype=f32),
            "bias_idx": None, "bias_val": None, "pen_idx": None,
            "penalty": None,
        }
        (case["want_logits"], case["want_ids"], case["want_lse"],
         case["want_keep"]) = spec_case(case)
        assert case["want_ids"][0] == int(u * V)   # the step's far side
        out.append(case)
    return tuple(out)


def torch_args(case, device="cpu"):
    """The case as ops.sample_rows arguments (fresh tensors)."""
    import torch

    def t(a):
        return None if a is None else torch.from_numpy(a.copy()).to(device)
    return dict(
        logits=t(case["logits"]), temperature=t(case["temperature"]),
        top_p=t(case["top_p"]), u=t(case["u"]), active=t(case["active"]),
        ids_out=t(case["ids_init"]), lse_out=t(case["lse_init"]),
        bias_idx=t(case["bias_idx"]), bias_val=t(case["bias_val"]),
        pen_idx=t(case["pen_idx"]), penalty=t(case["penalty"]))
