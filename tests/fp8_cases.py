"""Exact-arithmetic inputs for the FP8 block-quantized (W8A16) kernels:
fp8_block_dequant, fp8f16_gemv, moe_fp8f16_gateup(_acc), moe_fp8f16_down.
CPU sanity in test_fp8_cases_cpu.py, GPU in test_fp8_kernels_gpu.py.  The
sub-range plans and the gate-up helpers come from quant_cases.py.

Format: weight byte b is OCP e4m3 (float8_e4m3fn): sign b>>7, exponent
(b>>3)&15, mantissa b&7; value (1 + m/8) * 2^(e-7), or (m/8) * 2^-6 for
e = 0; 0x7F / 0xFF are NaN.  W[o, k] = value(b[o, k]) * s[o//128, k//128].

Codes.  ALL_CODES: the 254 finite bytes (0x80 = -0 and the subnormals
0x01..0x07 included).  SMALL_CODES: those whose value is a multiple of 1/8
with |v| <= 16.  Every dense-x case draws from SMALL_CODES only.

Scales.  Powers of two {1/4, 1/2, 1, 2}, one per (expert, row block, k
block), index (3*rb + 5*kb + 7*e + r) % 4: a slip to the next row block
(+3), the next k block (+1) or the next expert (+3) always lands on another
scale, a transposed (kb, rb) lookup whenever rb - kb is odd.

Budget.  With SMALL_CODES, LSB = 1/8 * 1/4 = 1/32 and integer |x| <= 2.
Worst case over K <= 384: 384 * 2 * 16 * 2 * 32 = 2^19.6 LSBs < 2^24, so
every fp32 partial sum is exact in any order (MFMA internal order, the
per-k-block partial sums, acc += s * partial with s a power of two,
split-K atomics) and a correct kernel equals the fp64 reference bit for
bit.  MoE down adds routing weights down to 1/4 (LSB 1/128) and up to two
experts per token: 2 * 2^19.6 * 4 = 2^22.6.  test_fp8_cases_cpu.py asserts
the bounds and prints the seen maxima (log2 LSBs):

    family            longest K   bound   seen
    gemv dense x         384       19.6   16.5
    moe down, 2 experts  384       22.6   19.4

One-hot sweeps draw weights from ALL_CODES (all 254 occur): one product
per output, and every e4m3 value times a power of two in [1/4, 2] is a
bf16, fp16 and fp32 value.

Gate-up constructions of quant_cases (x[t, 0] = 1 plus a one-hot column):
  (a) constant gate: gate weights 32 in column 0 (codes 128, 64, 32, 16
      under scales 1/4 .. 2), 0 elsewhere; up weights 0 in column 0, any
      finite code elsewhere.  h = 32 * W_up[o, k_t].
  (b) saturated gate: up weights 1 in column 0 (codes 4, 2, 1, 1/2), 0
      elsewhere; gate 64 in column 0 (codes 256 .. 32) and integer values
      n in [-44, 96] with at most 4 significant bits elsewhere (code n/s is
      then an e4m3 value).  g = 64 + n >= 20, so h = g.

Random-data bound.  Weights quantize_fp8_block(randn * 0.05), x randn
fp16, K = 384.  The conversion to fp16 is exact and a product of two fp16
values is exact in fp32, so the only error is fp32 accumulation: K product
additions and K/128 scale folds (one multiply-add each), each relative
2^-23 of a running sum bounded by A = sum_k |x_k||w_k| (this covers
truncating as well as round-to-nearest adders):

    |got - ref64| <= u_out * |ref64| + (K + K/128) * 2^-23 * A

u_out = 2^-9 (bf16 out), 2^-11 (fp16 out), 0 (fp32 out).  Gate-up
composes the two bounds Bg, Bu as quant_cases.gateup_bound does, plus
2^-25 absolute for fp16's subnormal spacing.  Worst |error| / bound, CPU
emulation of the kernels' declared arithmetic / measured on an MI355X:

    fp8f16_gemv        1.71 / 1.71   (see below)
    moe_fp8f16_down    <0.01 / <0.01
    moe_fp8f16_gateup  0.36 / 0.36

The GEMV ratio is above 1, for the emulation as for the kernel, and the
cause is the formula, not the arithmetic: bf16 has an 8-bit significand, so
a correctly rounded output is off by up to 2^-8 of its value (half an ulp of
2^-7 just above a power of two), twice the u_out = 2^-9 the formula grants.
The affine tests never saw this because their 2 * 2^-11 * A dequant term
dwarfs it; here the accumulation term is ~2^-14 * A and the output rounding
stands alone.  The tests therefore assert bf16_within() — the accumulation
bound with a correctly rounded output, which is tighter than the formula
with the right u_out — and print the formula's ratio next to it.
"""

import torch

import quant_cases as qc
from mlx_sharding_amd.ops import reference as ref

F8 = torch.float8_e4m3fn
BLOCK = 128
SCALES = (0.25, 0.5, 1.0, 2.0)
LSB = 1.0 / 32
DOWN_LSB = 1.0 / 128
NAN_CODE = 0x7F


def _code_table() -> torch.Tensor:
    """fp64 value of each byte, from the format's definition (NaN codes
    NaN)."""
    v = []
    for b in range(256):
        sgn = -1.0 if b >> 7 else 1.0
        e, m = (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            v.append(float("nan"))
        elif e == 0:
            v.append(sgn * (m / 8.0) * 2.0 ** -6)
        else:
            v.append(sgn * (1.0 + m / 8.0) * 2.0 ** (e - 7))
    return torch.tensor(v, dtype=torch.float64)


CODE_VALUE = _code_table()
ALL_CODES = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F])
SMALL_CODES = torch.tensor(
    [int(b) for b in ALL_CODES
     if abs(float(CODE_VALUE[b])) <= 16
     and float(CODE_VALUE[b]) * 8 == round(float(CODE_VALUE[b]) * 8)])
assert len(ALL_CODES) == 254
# value -> code for non-negative-zero values (0.0 maps to 0x00)
_VALUE_CODE = {float(CODE_VALUE[b]): int(b) for b in reversed(ALL_CODES.tolist())
               if b != 0x80}


def code_of(value: float) -> int:
    return _VALUE_CODE[float(value)]


def to_fp8(codes: torch.Tensor) -> torch.Tensor:
    """Integer byte codes -> float8_e4m3fn tensor with those bytes."""
    return codes.to(torch.uint8).contiguous().view(F8)


def nblk(n: int) -> int:
    return -(-n // BLOCK)


def scale_at(e, rb, kb, r: int):
    """fp64 scale of (expert, row block, k block) — defined for ANY index,
    so the slipped emulations can look past the stored array."""
    idx = (3 * rb + 5 * kb + 7 * e + r) % 4
    return torch.tensor(SCALES, dtype=torch.float64)[idx]


def make_scales(E, O: int, K: int, r: int) -> torch.Tensor:
    """fp32 [E, RB, KB] (or [RB, KB] when E is None)."""
    RB, KB = nblk(O), nblk(K)
    e = torch.arange(E or 1)[:, None, None]
    rb = torch.arange(RB)[None, :, None]
    kb = torch.arange(KB)[None, None, :]
    s = scale_at(e, rb, kb, r).float()
    return s if E is not None else s[0]


def expand_scales(s: torch.Tensor, O: int, K: int) -> torch.Tensor:
    s = s.double().repeat_interleave(BLOCK, -2).repeat_interleave(BLOCK, -1)
    return s[..., :O, :K]


def w64_of(codes: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The fp64 construction of the dequantized weight."""
    O, K = codes.shape[-2:]
    return CODE_VALUE[codes] * expand_scales(s, O, K)


def draw_codes(shape, pool: torch.Tensor, seed: int, cover: bool = False):
    """Codes drawn from pool; cover=True puts every pool code in at least
    once (spread over the tensor by a fixed permutation)."""
    g = qc._gen(*shape, len(pool), seed, 23)
    n = 1
    for d in shape:
        n *= d
    c = pool[torch.randint(0, len(pool), (n,), generator=g)]
    if cover:
        assert n >= len(pool)
        where = torch.randperm(n, generator=g)[: len(pool)]
        c[where] = pool
    c = c.reshape(shape)
    if cover:
        assert set(c.flatten().tolist()) == set(pool.tolist())
    return c


def exact_weight(O: int, K: int, E=None, seed: int = 0, pool=None,
                 cover: bool = False):
    """(codes, scales fp32, W64).  The dequantized weight is asserted to be
    a bf16, fp16 and fp32 value."""
    pool = SMALL_CODES if pool is None else pool
    shape = (O, K) if E is None else (E, O, K)
    codes = draw_codes(shape, pool, seed, cover)
    s = make_scales(E, O, K, seed % 4)
    W = w64_of(codes, s)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert qc._roundtrip(W, dt)
    return codes, s, W


def assert_small(codes: torch.Tensor):
    """Dense-x cases may only use SMALL_CODES."""
    assert set(codes.flatten().tolist()) <= set(SMALL_CODES.tolist())


# --------------------------------------------------------------------------
# case lists shared by the CPU and GPU modules
# --------------------------------------------------------------------------

DEQUANT_CASES = [(200, 384, None), (200, 384, 3), (20, 192, None)]
GEMV_MS = (1, 17, 33, 64)
GEMV_O = 200
GEMV_KS = (128, 384)
# direct bf16 store over two k-blocks: more row tiles than split-K allows
GEMV_DIRECT = dict(M=17, O=16400, K=256)       # nsplit == 1
GEMV_SPLIT = dict(M=17, O=200, K=384)          # nsplit > 1
MOE_I = 200
MOE_HS = (128, 384)
DOWN_H = 200
DOWN_IS = (128, 256, 384)
PLANS = {"plan16": qc.PLAN16, "plan32": qc.PLAN32}
E = qc.N_EXPERTS
BUDGET_K = 384
BUDGET_O = 200


def gemv_dense_case(M: int, O: int, K: int, seed: int = 0):
    """(x64, codes, scales, W64, y64) with the fp32 budget asserted."""
    codes, s, W = exact_weight(O, K, None, seed)
    assert_small(codes)
    x = qc.dense_int_x(M, K, seed)
    y = x @ W.t()
    top = qc.check_budget(x.abs() @ W.abs().t(), LSB, "fp8 gemv dense")
    return x, codes, s, W, y, top


def gemv_onehot_weight(O: int, K: int, seed: int = 0):
    return exact_weight(O, K, None, seed + 7, pool=ALL_CODES, cover=True)


# -- gate-up ---------------------------------------------------------------

_B_VALUES = [n for n in range(-44, 97)
             if n == 0 or (abs(n) >> max(0, abs(n).bit_length() - 4))
             << max(0, abs(n).bit_length() - 4) == abs(n)]


def gateup_weights(kind: str, I: int, H: int, seed: int = 0):
    """Stacked over E experts: (gate, up), each (codes, scales, W64), for
    construction (a) or (b) of the module docstring."""
    g = qc._gen(I, H, seed, ord(kind), 29)
    gs = make_scales(E, I, H, seed % 4)
    us = make_scales(E, I, H, (seed + 1) % 4)
    gsx = expand_scales(gs, I, H)
    usx = expand_scales(us, I, H)

    def codes_for(values64, sx):
        raw = values64 / sx
        return torch.tensor([code_of(v) for v in raw.flatten().tolist()]) \
            .reshape(values64.shape)

    if kind == "a":
        Wg = torch.zeros(E, I, H, dtype=torch.float64)
        Wg[..., 0] = 32.0
        gc = codes_for(Wg, gsx)
        uc = draw_codes((E, I, H), ALL_CODES, seed + 3, cover=True)
        uc[..., 0] = 0
    else:
        vals = torch.tensor(_B_VALUES, dtype=torch.float64)
        Wg = vals[torch.randint(0, len(vals), (E, I, H), generator=g)]
        Wg[..., 0] = 64.0
        gc = codes_for(Wg, gsx)
        Wu = torch.zeros(E, I, H, dtype=torch.float64)
        Wu[..., 0] = 1.0
        uc = codes_for(Wu, usx)
    gate = (gc, gs, w64_of(gc, gs))
    up = (uc, us, w64_of(uc, us))
    if kind == "a":
        assert torch.all(gate[2][..., 0] == 32) and not gate[2][..., 1:].any()
        assert not up[2][..., 0].any()
    else:
        assert torch.equal(gate[2], Wg) and gate[2][..., 1:].min() >= -47
        assert torch.all(up[2][..., 0] == 1) and not up[2][..., 1:].any()
    return gate, up


def poison_unused(codes: torch.Tensor, s: torch.Tensor):
    """The unused expert's weights become NaN codes, its scales NaN."""
    codes, s = codes.clone(), s.clone()
    codes[qc.UNUSED_EXPERT] = NAN_CODE
    s[qc.UNUSED_EXPERT] = float("nan")
    return codes, s


# -- down ------------------------------------------------------------------

def down_case(I: int, plan_d, seed: int = 0):
    """(codes, scales, W64 [E, H, I], h64 [P, I], out64 [N, H], top)."""
    codes, s, W = exact_weight(DOWN_H, I, E, seed + 11)
    assert_small(codes)
    h = qc.down_h(plan_d, I, seed)
    out = qc.down_expected(W, h, plan_d, lsb=DOWN_LSB)
    subs, _ = qc.build_subranges(plan_d["plan"])
    mass = torch.zeros_like(out)
    for p, e, t in qc.plan_pairs(plan_d["plan"]):
        mass[t] += subs[4][p].double() * (W[e].abs() @ h[p].abs())
    top = qc.check_budget(mass, DOWN_LSB, "fp8 moe down")
    return codes, s, W, h, out, top


# --------------------------------------------------------------------------
# emulation of the kernels' declared arithmetic (CPU)
# --------------------------------------------------------------------------

def emulate_linear(x64, codes, r: int, e: int = 0, slip=(0, 0),
                   transpose: bool = False) -> torch.Tensor:
    """y[m, o] in fp32 as the kernels form it: per 128-wide k-block an fp32
    partial sum of fp16 products from zero, then acc += s * partial.  slip
    = (d_rb, d_kb) / transpose look the scale up at a wrong block (negative
    controls)."""
    O, K = codes.shape
    x = x64.float()
    w = CODE_VALUE[codes].float()
    acc = torch.zeros(x.shape[0], O, dtype=torch.float32)
    for rb in range(nblk(O)):
        rows = slice(rb * BLOCK, min(O, (rb + 1) * BLOCK))
        for kb in range(nblk(K)):
            ks = slice(kb * BLOCK, min(K, (kb + 1) * BLOCK))
            part = x[:, ks] @ w[rows, ks].t()
            a, b = rb + slip[0], kb + slip[1]
            if transpose:
                a, b = b, a
            acc[:, rows] += scale_at(e, a, b, r).float() * part
    return acc


# --------------------------------------------------------------------------
# random-data bound
# --------------------------------------------------------------------------

U_BF16, U_FP16, U_ACC = 2.0 ** -9, 2.0 ** -11, 2.0 ** -23


def acc_bound(A: torch.Tensor, K: int) -> torch.Tensor:
    return (K + K // BLOCK) * U_ACC * A


def random_weight(O: int, K: int, E=None, seed: int = 0):
    """(w8, scale_inv, W64) from reference.quantize_fp8_block."""
    g = qc._gen(O, K, E or 0, seed, 31)
    shape = (O, K) if E is None else (E, O, K)
    w8, s = ref.quantize_fp8_block(torch.randn(*shape, generator=g) * 0.05)
    W = w8.double() * expand_scales(s, O, K)
    return w8, s, W


def random_gemv_case(seed: int = 0):
    w8, s, W = random_weight(BUDGET_O, BUDGET_K, None, seed)
    g = torch.Generator().manual_seed(seed + 11)
    x = torch.randn(64, BUDGET_K, generator=g).to(torch.float16)
    ref64 = x.double() @ W.t()
    A = x.double().abs() @ W.abs().t()
    return w8, s, x, ref64, acc_bound(A, BUDGET_K)


def gemv_formula_ratio(got_bf16, ref64, B) -> float:
    """Worst |error| / (2^-9 |ref64| + B), the stated formula."""
    return float(((got_bf16.double() - ref64).abs()
                  / (U_BF16 * ref64.abs() + B)).max())


def bf16_within(got_bf16, ref64, B) -> bool:
    """got is the round-to-nearest bf16 of SOME value within B of ref64:
    rounding is monotone, so that is RN(ref64 - B) <= got <= RN(ref64 + B).
    This is the accumulation bound B with a correctly rounded output and
    nothing else."""
    lo = (ref64 - B).float().to(torch.bfloat16).double()
    hi = (ref64 + B).float().to(torch.bfloat16).double()
    g = got_bf16.double()
    return bool(((lo <= g) & (g <= hi)).all())


def random_moe_case(seed: int = 0):
    """Random experts on PLAN16: ((w8, s, W64) for gate, up, down; x fp16
    [N, K]; hh fp16 [P, K])."""
    mats = {n: random_weight(BUDGET_O, BUDGET_K, E, seed + i)
            for i, n in enumerate(("gate", "up", "down"))}
    g = torch.Generator().manual_seed(seed + 17)
    P = qc.build_subranges(qc.PLAN16["plan"])[1].numel()
    x = torch.randn(qc.PLAN16["N"], BUDGET_K, generator=g).to(torch.float16)
    hh = torch.randn(P, BUDGET_K, generator=g).to(torch.float16)
    return mats, x, hh


def random_down_ref(mats, hh):
    """(ref64, bound) [N, O]; fp32 out."""
    W = mats["down"][2]
    subs, _ = qc.build_subranges(qc.PLAN16["plan"])
    ref64 = torch.zeros(qc.PLAN16["N"], W.shape[1], dtype=torch.float64)
    A = torch.zeros_like(ref64)
    for p, e, t in qc.plan_pairs(qc.PLAN16["plan"]):
        wt = subs[4][p].double()
        ref64[t] += wt * (W[e] @ hh[p].double())
        A[t] += wt * (W[e].abs() @ hh[p].double().abs())
    # one more rounding per pair for wt * acc and the atomic add
    return ref64, acc_bound(A, BUDGET_K) + 4 * U_ACC * A


def random_gateup_ref(mats, x):
    """(ref64, bound) [P, O]; fp16 out."""
    Wg, Wu = mats["gate"][2], mats["up"][2]
    P = qc.build_subranges(qc.PLAN16["plan"])[1].numel()
    ref64 = torch.zeros(P, Wg.shape[1], dtype=torch.float64)
    bound = torch.ones_like(ref64)
    for p, e, t in qc.plan_pairs(qc.PLAN16["plan"]):
        xt = x[t].double()
        g64, u64 = Wg[e] @ xt, Wu[e] @ xt
        Bg = acc_bound(Wg[e].abs() @ xt.abs(), BUDGET_K)
        Bu = acc_bound(Wu[e].abs() @ xt.abs(), BUDGET_K)
        silu = g64 / (1.0 + torch.exp(-g64))
        ref64[p] = silu * u64
        bound[p] = (U_FP16 * ref64[p].abs() + 2.0 ** -25 + 1.1 * Bg * u64.abs()
                    + silu.abs() * Bu + 1.1 * Bg * Bu)
    return ref64, bound


def emulate_moe_linear(x, w8, s):
    """fp32 [rows of x, O] with the kernels' arithmetic for one expert's
    stored (w8 [O, K], s [RB, KB]) and fp16 x."""
    O, K = w8.shape
    xf, w = x.float(), w8.float()
    acc = torch.zeros(x.shape[0], O, dtype=torch.float32)
    for rb in range(nblk(O)):
        rows = slice(rb * BLOCK, min(O, (rb + 1) * BLOCK))
        for kb in range(nblk(K)):
            ks = slice(kb * BLOCK, (kb + 1) * BLOCK)
            acc[:, rows] += s[rb, kb] * (xf[:, ks] @ w[rows, ks].t())
    return acc
