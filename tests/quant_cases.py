"""Shared exact-arithmetic inputs for the quantized GEMM / MoE kernel tests
(CPU sanity in test_quant_cases_cpu.py, GPU in test_quant_kernels_exact.py).

Every kernel here multiplies low-precision operands and accumulates in
fp32.  The inputs are chosen so that every dequantized weight, every
product and every partial sum is an integer multiple of one LSB and stays
below 2^24 LSBs; fp32 addition of such values is exact in ANY order (MFMA
internal order, parity-split chains, split-K atomics), so a correct kernel
must reproduce the fp64 reference bit for bit.

Weights: q uniform in [0, 2^bits); per (row, group) a scale s in
{1/4, 1/2, 1, 2} and a bias b = -m*s with integer m in [0, 2^bits), so
w = s*(q - m) with |q - m| <= 255: exact in bf16 (8-bit significand) and
fp16, as is b + off*s = (off - m)*s for the fp16 kernels' off = 8 / 128.
m[o, g] = (3*o + 5*g + r) mod 2^bits differs between neighbouring rows and
neighbouring groups, so a row- or group-index slip always changes values.
Activations are integers in [-2, 2] or one-hot rows.

Bit budget (LSB = 1/4 for the GEMVs: smallest scale times an integer x;
1/16 for the MoE down kernels, whose routing weights go down to 1/4).
"bound" is the worst case K * max|product| / LSB, "seen" the largest
sum_k |product| / LSB over the cases of this module
(test_quant_cases_cpu.py::test_bit_budget prints them):

    family                          longest K  bound (log2)  seen (log2)
    4-bit, dequantized weight           1024       17.9         15.2
    8-bit, dequantized weight           1024       22.0         19.3
    scalar w4a16, s*sum(q x) + b*sum(x)  384       21.6         19.9
    MoE down, 8-bit, two experts         384       23.6         21.0

Every builder asserts "seen" < 2^24 on the data it returns.  The seen
totals leave 3.0 bits (8-bit MoE down) to 8.8 bits (4-bit) under 2^24,
the worst-case bounds 0.4 to 6.1 bits.  Eight bits of headroom are not
reachable at 8 bits with scales up to 2 and |x| up to 2, and are not
needed: exactness only requires every partial sum below 2^24 LSBs.

At 8 bits a dense-integer output reaches ~10^4 and does not fit a bf16
significand, so the bf16-output GEMV cases with dense x are compared after
rounding BOTH sides to bf16 (the fp32 sum is still exact); a one-nibble
slip can hide behind that rounding, which is why every GEMV also gets the
one-hot sweep: y[m, :] = W[:, k_m] is exact in every output format and
ceil(K / M) offsets read back every (row, column) of the weight.

Gate-up constructions (h = silu(g) * u made exact).  x[t, 0] = 1 and x[t]
is one-hot at k_t in [1, H) otherwise.
  (a) constant gate: gate weights 32 in column 0, 0 elsewhere (code q = m);
      up weights 0 in column 0.  g = 32, silu(32) = 32 in fp32, so
      h = 32 * W_up[o, k_t].
  (b) saturated gate: up weights 1 in column 0, 0 elsewhere; gate 64 in
      column 0 with integer scales and m small enough that
      g = 64 + W_gate[o, k_t] >= 17.  In fp32 g / (1 + exp(-g)) == g for
      every integer 17 <= g < 2048 (exp(-17) < 2^-24), so h = g.

Section-4 arithmetic budget (fp16-dequant 4-bit kernels, random data).
The kernel forms w~ = fl16(s*(q-8) + fl16(b + 8s)): one fp16 rounding of
the bias constant, relative 2^-11 of |b + 8s|, and one of the fma result,
relative 2^-11 of |w| <= |s||q-8| + |b+8s|.  Summed over k with fp32
accumulation (negligible next to 2^-11):

    |got - ref64| <= u_out*|ref64| + 2 * 2^-11 * A,
    A = sum_k |x_k| * (|s||q-8| + |b+8s|)

with u_out = 2^-9 (bf16 out), 2^-11 (fp16 out), 0 (fp32 out).  For the
down kernel A is summed over a token's pairs with the routing weights.
For gate-up, with Bg, Bu the bounds on g and u and |silu'| <= 1.1:

    |h - h64| <= 2^-11*|h64| + 1.1*Bg*|u| + |silu(g)|*Bu + 1.1*Bg*Bu.

Measured (K = 384, seed 0): worst ratio of |error| to the bound for the
CPU emulation of the kernel's arithmetic / the same on an MI355X / share
of elements past the bound when the emulated bias is off by half a step
(b + 0.5 s):

    kernel             gs 32                gs 64                gs 128
    w4f16_gemv         0.42 / 0.42 / 90 %   0.41 / 0.41 / 92 %   0.46 / 0.46 / 94 %
    moe_w4f16_down     0.01 / 0.01 / 97 %   0.02 / 0.02 / 99 %   0.01 / 0.01 / 100 %
    moe_w4f16_gateup   0.03 / 0.03 / 63 %   0.02 / 0.02 / 67 %   0.02 / 0.02 / 70 %

(The GEMV ratio is dominated by the bf16 output rounding; the MoE kernels
store fp32 / fp16 and their dequant errors largely cancel over k.)
"""

import math

import torch

from mlx_sharding_amd.ops import reference as ref

BITS_GS = [(b, g) for b in (4, 8) for g in (32, 64, 128)]
BITS_GS_IDS = ["w%d-gs%d" % c for c in BITS_GS]
SCALES = (0.25, 0.5, 1.0, 2.0)
ROUTE_WTS = (1.0, 0.5, 0.25)
F24 = float(2 ** 24)

_PACK_DTYPE = ref.quantize(torch.zeros(1, 32), 32, 4)[0].dtype


def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _roundtrip(t64: torch.Tensor, dtype) -> bool:
    return torch.equal(t64.to(dtype).double(), t64)


def check_budget(abs_sum: torch.Tensor, lsb: float, what: str) -> float:
    """abs_sum: sum of |terms| per output; must stay under 2^24 LSBs.
    Returns the largest total in LSBs."""
    top = float(abs_sum.max()) / lsb
    assert top < F24, "%s: %.0f LSBs >= 2^24" % (what, top)
    return top


# --------------------------------------------------------------------------
# packing and weights
# --------------------------------------------------------------------------

def pack(q: torch.Tensor, bits: int) -> torch.Tensor:
    """Integer codes [..., K] -> little-endian u32 words [..., K*bits/32]
    (lowest bits = first element), in reference.quantize's dtype."""
    pw = 32 // bits
    assert q.shape[-1] % pw == 0
    qw = q.to(torch.int64).reshape(*q.shape[:-1], q.shape[-1] // pw, pw)
    shifts = torch.arange(0, 32, bits, dtype=torch.int64)
    packed = (qw << shifts).sum(-1) & 0xFFFFFFFF
    return packed.to(_PACK_DTYPE)


def unpack_natural(wq: torch.Tensor, bits: int) -> torch.Tensor:
    """Inverse of pack()."""
    shifts = torch.arange(0, 32, bits, dtype=torch.int64)
    w = wq.to(torch.int64) & 0xFFFFFFFF
    q = (w[..., None] >> shifts) & ((1 << bits) - 1)
    return q.reshape(*wq.shape[:-1], -1)


def unpack_repacked(rp: torch.Tensor, bits: int) -> torch.Tensor:
    """Codes in natural k order from ops.repack_w4 words, extracted the way
    the fp16 kernels do: 4-bit, the (lo, hi) halves of
    (w >> 4j) & 0x000F000F for j = 0..3; 8-bit, dq8_w8's
    (w0 >> 8j) & 0x00FF00FF then (w1 >> 8j) & 0x00FF00FF, j = 0..1."""
    w = rp.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if bits == 4:
        out = []
        for j in range(4):
            p = (w >> (4 * j)) & 0x000F000F
            out += [p & 0xFFFF, p >> 16]
        return torch.stack(out, -1).reshape(*rp.shape[:-1], -1)
    assert rp.shape[-1] % 2 == 0
    w = w.reshape(*rp.shape[:-1], -1, 2)
    out = []
    for half in range(2):
        for j in range(2):
            p = (w[..., half] >> (8 * j)) & 0x00FF00FF
            out += [p & 0xFFFF, p >> 16]
    return torch.stack(out, -1).reshape(*rp.shape[:-1], -1)


def finish_weights(q, s, m, gs: int, bits: int):
    """(q [O,K] codes, s [O,G] scales, m [O,G] integer zero points) ->
    (q, scales_bf16, biases_bf16, W64), with every exactness precondition
    asserted."""
    off = 8.0 if bits == 4 else 128.0
    s64 = s.double()
    b64 = -(m.double() * s64)
    sc, bi = s64.to(torch.bfloat16), b64.to(torch.bfloat16)
    assert torch.equal(sc.double(), s64) and torch.equal(bi.double(), b64)
    W64 = s64.repeat_interleave(gs, 1) * (
        q.double() - m.double().repeat_interleave(gs, 1))
    deq = ref.dequantize(pack(q, bits), sc, bi, gs, bits)
    assert torch.equal(deq.double(), W64), "reference.dequantize != W64"
    assert _roundtrip(W64, torch.bfloat16) and _roundtrip(W64, torch.float16)
    assert _roundtrip(b64 + off * s64, torch.float16)
    return q, sc, bi, W64


def exact_weights(O: int, K: int, gs: int, bits: int, seed: int = 0):
    """(q, scales_bf16, biases_bf16, W64) of the module docstring."""
    assert K % gs == 0
    g = _gen(O, K, gs, bits, seed)
    qmax = 1 << bits
    G = K // gs
    q = torch.randint(0, qmax, (O, K), generator=g)
    s = torch.tensor(SCALES)[torch.randint(0, 4, (O, G), generator=g)]
    r = int(torch.randint(0, qmax, (1,), generator=g))
    m = (3 * torch.arange(O)[:, None] + 5 * torch.arange(G)[None, :] + r) % qmax
    return finish_weights(q, s, m, gs, bits)


def exact_expert_weights(E, O, K, gs, bits, seed=0):
    """Stacked [E, ...] exact_weights, a different draw per expert."""
    parts = [exact_weights(O, K, gs, bits, 16 * seed + e) for e in range(E)]
    return tuple(torch.stack([p[i] for p in parts]) for i in range(4))


def random_q4(O: int, K: int, gs: int, seed: int = 0):
    """Section-4 weights: reference.quantize(randn * 0.05), 4-bit.  Returns
    (wq, scales_bf16, biases_bf16, q)."""
    g = _gen(O, K, gs, seed, 4)
    w = (torch.randn(O, K, generator=g) * 0.05).to(torch.bfloat16)
    wq, sc, bi = ref.quantize(w, gs, 4)
    return wq, sc, bi, unpack_natural(wq, 4)


# --------------------------------------------------------------------------
# activations
# --------------------------------------------------------------------------

def dense_int_x(M: int, K: int, seed: int = 0) -> torch.Tensor:
    """fp64 integers in [-2, 2]."""
    return torch.randint(-2, 3, (M, K), generator=_gen(M, K, seed, 7)).double()


def one_hot_x(M: int, K: int, offset: int) -> torch.Tensor:
    """fp64 [M, K], a single 1 in row m at column (offset + m) mod K."""
    x = torch.zeros(M, K, dtype=torch.float64)
    x[torch.arange(M), one_hot_cols(M, K, offset)] = 1.0
    return x


def one_hot_cols(M: int, K: int, offset: int) -> torch.Tensor:
    return (offset + torch.arange(M)) % K


def one_hot_offsets(M: int, K: int):
    """ceil(K / M) successive offsets: every column is read once."""
    return list(range(0, K, M))


def gemv_dense_case(M, O, K, gs, bits, seed=0):
    """(x64, q, sc, bi, W64, y64) with the fp32 budget asserted."""
    q, sc, bi, W64 = exact_weights(O, K, gs, bits, seed)
    x = dense_int_x(M, K, seed)
    y = x @ W64.t()
    check_budget(x.abs() @ W64.abs().t(), 0.25, "gemv dequantized")
    # the scalar kernel sums s*q*x and b*x separately
    qa = q.double() * sc.double().repeat_interleave(gs, 1)
    ba = bi.double().abs().repeat_interleave(gs, 1)
    check_budget(x.abs() @ (qa + ba).t(), 0.25, "gemv s*q*x + b*x")
    return x, q, sc, bi, W64, y


# --------------------------------------------------------------------------
# MoE sub-ranges, built by hand (independent of ops.make_expert_subranges)
# --------------------------------------------------------------------------

def build_subranges(plan):
    """plan: list of (expert, [tokens]) sub-ranges in slot order.  An empty
    token list is a padded cnt = 0 slot; ("gap", n) leaves n rows of the
    sorted arrays outside every sub-range (token 0, weight NaN).  Routing
    weights cycle through ROUTE_WTS.

    Returns ((sub_expert, sub_off, sub_cnt, sorted_tok, sorted_wt), live)
    where live is the bool mask of sorted rows inside a sub-range."""
    sub_e, sub_off, sub_cnt, stok, swt, live = [], [], [], [], [], []
    for e, toks in plan:
        if e == "gap":
            stok += [0] * toks
            swt += [float("nan")] * toks
            live += [False] * toks
            continue
        sub_e.append(e)
        sub_off.append(len(stok) if toks else 0)
        sub_cnt.append(len(toks))
        for t in toks:
            swt.append(ROUTE_WTS[len(stok) % len(ROUTE_WTS)])
            stok.append(t)
            live.append(True)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    return ((i32(sub_e), i32(sub_off), i32(sub_cnt), i32(stok),
             torch.tensor(swt, dtype=torch.float32)),
            torch.tensor(live))


# E = 3 everywhere; expert 1 is never used.  Token lists are not monotone,
# several tokens go to both experts, and the last two tokens of each plan
# are routed nowhere.
_E0_16 = [5, 3, 17, 0, 9, 12, 1, 20, 7, 14, 2, 19, 11, 8, 15, 4]
_E2_15 = [21, 6, 3, 18, 13, 16, 0, 9, 5, 20, 1, 12, 7, 19, 2]
PLAN16 = dict(N=24, plan=[(0, _E0_16), (0, [10]), (1, []), ("gap", 3),
                          (2, _E2_15), (0, [])])
PLAN4 = dict(N=9, plan=[(0, [3, 1, 2, 0]), (0, [4]), (1, []), ("gap", 2),
                        (2, [5, 1, 2, 3]), (2, [0]), (0, [])])
_P38 = torch.randperm(38, generator=_gen(38)).tolist()
_Q38 = torch.randperm(38, generator=_gen(39)).tolist()
PLAN32 = dict(N=40, plan=[(0, _P38[:32]), (0, _P38[32:33]), (1, []),
                          ("gap", 5), (2, _Q38[:17]), (2, _Q38[17:33]),
                          (0, [])])
N_EXPERTS = 3
UNUSED_EXPERT = 1


def plan_pairs(plan):
    """[(sorted row, expert, token)] of the live pairs."""
    out, p = [], 0
    for e, toks in plan:
        if e == "gap":
            p += toks
            continue
        for t in toks:
            out.append((p, e, t))
            p += 1
    return out


def dead_tokens(plan_d):
    used = {t for _, _, t in plan_pairs(plan_d["plan"])}
    dead = [t for t in range(plan_d["N"]) if t not in used]
    assert dead, "plan needs a token routed nowhere"
    return dead


def poison_rows(x: torch.Tensor, rows) -> torch.Tensor:
    x = x.clone()
    x[list(rows)] = float("nan")
    return x


def poison_expert(t: torch.Tensor, e: int = UNUSED_EXPERT) -> torch.Tensor:
    t = t.clone()
    t[e] = float("nan")
    return t


# --------------------------------------------------------------------------
# gate-up constructions
# --------------------------------------------------------------------------

def gateup_x(N: int, H: int, offset: int) -> torch.Tensor:
    """fp64 [N, H]: column 0 is 1, plus a 1 at gateup_cols(N, H, offset)."""
    x = torch.zeros(N, H, dtype=torch.float64)
    x[:, 0] = 1.0
    x[torch.arange(N), gateup_cols(N, H, offset)] = 1.0
    return x


def gateup_cols(N: int, H: int, offset: int) -> torch.Tensor:
    return 1 + (offset + torch.arange(N)) % (H - 1)


def gateup_offsets(plan_d, H: int):
    """The shortest stride-4/3/2/1 offset sweep after which every live
    expert has read every column 1..H-1 through some token."""
    pairs = plan_pairs(plan_d["plan"])
    for step in (4, 3, 2, 1):
        offs = list(range(0, H - 1, step))
        ok = True
        for e in {e for _, e, _ in pairs}:
            seen = {1 + (o + t) % (H - 1) for o in offs
                    for _, pe, t in pairs if pe == e}
            ok = ok and seen == set(range(1, H))
        if ok:
            return offs
    raise AssertionError("no sweep covers every column")


def _gate_group0(O, bits, kind, g):
    """Scale and zero point of group 0 so that s*(q0 - m) hits the column-0
    value (32 or 64) and, for (b), the rest of the group stays >= -47."""
    if kind == "a":
        pairs = [(4.0, 8), (8.0, 4)] if bits == 4 else [(1.0, 32), (2.0, 16)]
        m_hi = 7 if bits == 4 else 200
    else:
        # s*(q - m) >= -s*m >= -47
        pairs = [(8.0, 8), (16.0, 4)] if bits == 4 else [(1.0, 64), (2.0, 32)]
        m_hi = None
    pick = torch.randint(0, 2, (O,), generator=g)
    s0 = torch.tensor([pairs[int(i)][0] for i in pick])
    d0 = torch.tensor([pairs[int(i)][1] for i in pick])
    if m_hi is None:
        m_cap = torch.floor(47.0 / s0).long()
    else:
        m_cap = torch.full((O,), m_hi)
    m0 = (3 * torch.arange(O) + int(torch.randint(0, 64, (1,), generator=g))) \
        % (m_cap + 1)
    return s0, d0, m0


def gateup_weights(kind: str, I: int, H: int, gs: int, bits: int, seed: int = 0):
    """One expert's (gate, up) = ((q, sc, bi, W64), (q, sc, bi, W64)) for
    construction (a) or (b)."""
    g = _gen(I, H, gs, bits, seed, ord(kind))
    qmax = 1 << bits
    G = H // gs
    rows, grp = torch.arange(I)[:, None], torch.arange(G)[None, :]
    r = int(torch.randint(0, qmax, (1,), generator=g))
    # gate
    if kind == "a":
        s = torch.tensor(SCALES)[torch.randint(0, 4, (I, G), generator=g)]
        m = (3 * rows + 5 * grp + r) % qmax
        q = m.repeat_interleave(gs, 1).clone()          # code q = m: weight 0
    else:
        s = torch.tensor((1.0, 2.0))[torch.randint(0, 2, (I, G), generator=g)]
        m = (3 * rows + 5 * grp + r) % min(24, qmax)    # s*(q - m) >= -46
        q = torch.randint(0, qmax, (I, H), generator=g)
    s0, d0, m0 = _gate_group0(I, bits, kind, g)
    s[:, 0], m[:, 0] = s0, m0
    if kind == "a":
        q[:, :gs] = m0[:, None]
    q[:, 0] = m0 + d0
    assert int(q.max()) < qmax and int(q.min()) >= 0
    gate = finish_weights(q, s, m, gs, bits)
    # up
    uq, usc, ubi, _ = exact_weights(I, H, gs, bits, seed + 101)
    um = (-ubi.double() / usc.double()).long()
    uq = uq.clone()
    if kind == "a":
        uq[:, 0] = um[:, 0]                             # weight 0 in column 0
        us = usc.double()
    else:
        # 1 in column 0 (unit scale in group 0), 0 elsewhere
        uq = um.repeat_interleave(gs, 1).clone()
        us = usc.double().clone()
        us[:, 0] = 1.0
        um = um.clone()
        um[:, 0] = um[:, 0] % (qmax - 1)
        uq[:, :gs] = um[:, :1]
        uq[:, 0] = um[:, 0] + 1
    up = finish_weights(uq, us, um, gs, bits)
    if kind == "a":
        assert torch.all(gate[3][:, 0] == 32) and not gate[3][:, 1:].any()
        assert not up[3][:, 0].any()
    else:
        assert torch.all(gate[3][:, 0] == 64) and gate[3][:, 1:].min() >= -47
        assert torch.all(up[3][:, 0] == 1) and not up[3][:, 1:].any()
    return gate, up


def gateup_expert_weights(kind, E, I, H, gs, bits, seed=0):
    """Stacked over experts: (gate, up), each (q, sc, bi, W64) [E, ...]."""
    per = [gateup_weights(kind, I, H, gs, bits, 16 * seed + e) for e in range(E)]
    gate = tuple(torch.stack([p[0][i] for p in per]) for i in range(4))
    up = tuple(torch.stack([p[1][i] for p in per]) for i in range(4))
    return gate, up


def gateup_dense_weights(kind: str, E: int, I: int, H: int, seed: int = 0):
    """bf16-kernel version: small-integer dense (Wg64, Wu64) [E, I, H]."""
    g = _gen(E, I, H, seed, ord(kind), 3)
    if kind == "a":
        Wg = torch.zeros(E, I, H, dtype=torch.float64)
        Wg[..., 0] = 32.0
        Wu = torch.randint(-7, 8, (E, I, H), generator=g).double()
        Wu[..., 0] = 0.0
    else:
        Wg = torch.randint(-40, 101, (E, I, H), generator=g).double()
        Wg[..., 0] = 64.0
        Wu = torch.zeros(E, I, H, dtype=torch.float64)
        Wu[..., 0] = 1.0
    assert _roundtrip(Wg, torch.bfloat16) and _roundtrip(Wu, torch.bfloat16)
    return Wg, Wu


def gateup_expected(kind, Wg64, Wu64, plan_d, H, offset, out_dtype):
    """h64 [P, I] for the live sorted rows of the plan (other rows 0), with
    the exactness preconditions asserted: the closed form fits out_dtype
    and the fp64 silu(g)*u rounds to it."""
    pairs = plan_pairs(plan_d["plan"])
    P = build_subranges(plan_d["plan"])[1].numel()
    rows = torch.tensor([p for p, _, _ in pairs])
    es = torch.tensor([e for _, e, _ in pairs])
    ts = torch.tensor([t for _, _, t in pairs])
    ks = gateup_cols(plan_d["N"], H, offset)[ts]
    x = gateup_x(plan_d["N"], H, offset)[ts]
    gv = Wg64[es, :, 0] + Wg64[es, :, ks]
    uv = Wu64[es, :, 0] + Wu64[es, :, ks]
    assert torch.equal(gv, torch.einsum("pik,pk->pi", Wg64[es], x))
    assert torch.equal(uv, torch.einsum("pik,pk->pi", Wu64[es], x))
    if kind == "a":
        assert torch.all(gv == 32)
        live = 32.0 * uv
    else:
        assert torch.all(uv == 1) and gv.min() >= 17 and gv.max() < 2048
        assert torch.equal(gv, gv.round())
        live = gv
    true = gv / (1.0 + torch.exp(-gv)) * uv
    assert torch.equal(true.to(out_dtype), live.to(out_dtype))
    h = torch.zeros(P, Wg64.shape[1], dtype=torch.float64)
    h[rows] = live
    assert _roundtrip(h, out_dtype), "h does not fit the output format"
    return h


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------

def moe_linear_expected(W64, x64, plan_d):
    """Plain grouped GEMM y64 [P, O] (moe_w4_mfma): row p = W[e] @ x[tok]."""
    P = build_subranges(plan_d["plan"])[1].numel()
    y = torch.zeros(P, W64.shape[1], dtype=torch.float64)
    for p, e, t in plan_pairs(plan_d["plan"]):
        y[p] = W64[e] @ x64[t]
    return y


def down_expected(Wd64, h64, plan_d, lsb: float = 1.0 / 16):
    """out64 [N, H] = sum over pairs of wt * (Wd[e] @ h[p]); fp32 budget
    asserted (every weighted product is a multiple of lsb)."""
    subs, _ = build_subranges(plan_d["plan"])
    wt = subs[4].double()
    out = torch.zeros(plan_d["N"], Wd64.shape[1], dtype=torch.float64)
    mass = torch.zeros_like(out)
    for p, e, t in plan_pairs(plan_d["plan"]):
        out[t] += wt[p] * (Wd64[e] @ h64[p])
        mass[t] += wt[p] * (Wd64[e].abs() @ h64[p].abs())
    check_budget(mass, lsb, "moe down")
    assert _roundtrip(out, torch.float32)
    return out


def down_h(plan_d, I: int, seed: int = 0) -> torch.Tensor:
    """fp64 integers in [-2, 2], [P, I]."""
    P = build_subranges(plan_d["plan"])[1].numel()
    return dense_int_x(P, I, seed + 5)


# --------------------------------------------------------------------------
# case lists shared by the CPU and GPU modules
# --------------------------------------------------------------------------

DEQUANT_SHAPE = (20, 384)                               # O, H
SCALAR_GEMV = dict(Ms=(1, 7), O=20, H=384)
MFMA_GEMV = dict(Ms=(8, 33), O=72, Hs=(384, 1024))
# w4f16_gemv: gs -> H (split-K whose last split is a lone tail slice /
# two tail slices / whole batches)
W4F16_H = {32: 288, 64: 320, 128: 384}
W4F16_MS = (1, 17, 33, 64)
W4F16_O = 72
W4F16_DIRECT = dict(M=17, O=4096, H=128, gs=64)         # nsplit == 1
KSEG = dict(Ms=(1, 13, 64), N=80, K=512, ksegs=(1, 2))
# fp16 MoE kernels: gs -> inner dims (one 8-slice batch plus a tail; no tail)
MOE_F16_DIMS = {32: (288, 256), 64: (320, 256), 128: (384, 256)}
MOE_OUT = 72
# moe_w4_mfma: 8-slice batches only, and a batch plus a tail.  H = 288 is
# not a whole number of 64-wide groups, so gs 64 takes 320 for its tail.
MOE_W4_MFMA = [(b, g, h) for b in (4, 8)
               for g, hs in ((32, (256, 288)), (64, (256, 320))) for h in hs]
BF16_MOE = dict(H=416, I=96)
BF16_PLANS = {4: PLAN4, 16: PLAN16}
SCATTER = dict(H=36, P=7, K=3)
BUDGET_K = 384
BUDGET_O = 72


# --------------------------------------------------------------------------
# section 4: the arithmetic-budget bound
# --------------------------------------------------------------------------

U16 = 2.0 ** -11


def budget_mass(x64, q, sc, bi, gs: int):
    """A[m, o] = sum_k |x[m,k]| * (|s||q-8| + |b+8s|)."""
    s = sc.double().repeat_interleave(gs, 1)
    b = bi.double().repeat_interleave(gs, 1)
    return x64.abs() @ (s.abs() * (q.double() - 8).abs() + (b + 8 * s).abs()).t()


def budget_w64(q, sc, bi, gs: int):
    return (sc.double().repeat_interleave(gs, 1) * q.double()
            + bi.double().repeat_interleave(gs, 1))


def gemv_bound(ref64, A, u_out: float):
    return u_out * ref64.abs() + 2 * U16 * A


def gateup_bound(g64, u64, Ag, Au):
    Bg, Bu = 2 * U16 * Ag, 2 * U16 * Au
    silu = g64 / (1.0 + torch.exp(-g64))
    return (U16 * (silu * u64).abs() + 1.1 * Bg * u64.abs() + silu.abs() * Bu
            + 1.1 * Bg * Bu)


def budget_gemv_case(gs, seed=0):
    wq, sc, bi, q = random_q4(BUDGET_O, BUDGET_K, gs, seed)
    g = torch.Generator().manual_seed(seed + 11)
    x = torch.randn(64, BUDGET_K, generator=g).to(torch.float16)
    ref64 = x.double() @ budget_w64(q, sc, bi, gs).t()
    return wq, sc, bi, q, x, ref64, budget_mass(x.double(), q, sc, bi, gs)



def budget_moe_case(gs, seed=0):
    """Random 4-bit experts for the down and gate-up budget tests."""
    E, O, K = N_EXPERTS, BUDGET_O, BUDGET_K
    mats = {}
    for name, base in (("gate", 0), ("up", 1), ("down", 2)):
        parts = [random_q4(O, K, gs, 100 * seed + 10 * base + e) for e in range(E)]
        mats[name] = tuple(torch.stack([p[i] for p in parts]) for i in range(4))
    g = torch.Generator().manual_seed(seed + 17)
    P = build_subranges(PLAN16["plan"])[1].numel()
    x = torch.randn(PLAN16["N"], K, generator=g).to(torch.float16)
    hh = torch.randn(P, K, generator=g).to(torch.float16)
    return mats, x, hh



def budget_down_ref(mats, hh, gs):
    """(ref64, bound) [N, O] for the down kernel (fp32 out: u_out = 0)."""
    wq, sc, bi, q = mats["down"]
    subs, _ = build_subranges(PLAN16["plan"])
    N = PLAN16["N"]
    ref64 = torch.zeros(N, wq.shape[1], dtype=torch.float64)
    A = torch.zeros_like(ref64)
    for p, e, t in plan_pairs(PLAN16["plan"]):
        hp = hh[p:p + 1].double()
        wt = subs[4][p].double()
        ref64[t] += wt * (hp @ budget_w64(q[e], sc[e], bi[e], gs).t())[0]
        A[t] += wt * budget_mass(hp, q[e], sc[e], bi[e], gs)[0]
    return ref64, gemv_bound(ref64, A, 0.0)



def budget_gateup_ref(mats, x, gs):
    """(ref64, bound) [P, O] for the gate-up kernel (fp16 out)."""
    P = build_subranges(PLAN16["plan"])[1].numel()
    O = mats["gate"][0].shape[1]
    ref64 = torch.zeros(P, O, dtype=torch.float64)
    bound = torch.ones(P, O, dtype=torch.float64)
    for p, e, t in plan_pairs(PLAN16["plan"]):
        xt = x[t:t + 1].double()
        gq, gsc, gbi = (mats["gate"][i][e] for i in (3, 1, 2))
        uq, usc, ubi = (mats["up"][i][e] for i in (3, 1, 2))
        g64 = (xt @ budget_w64(gq, gsc, gbi, gs).t())[0]
        u64 = (xt @ budget_w64(uq, usc, ubi, gs).t())[0]
        ref64[p] = g64 / (1.0 + torch.exp(-g64)) * u64
        bound[p] = gateup_bound(g64, u64,
                                   budget_mass(xt, gq, gsc, gbi, gs)[0],
                                   budget_mass(xt, uq, usc, ubi, gs)[0])
    return ref64, bound



def log2_or_zero(v: float) -> float:
    return math.log2(v) if v > 0 else 0.0
