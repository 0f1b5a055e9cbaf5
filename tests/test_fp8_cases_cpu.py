"""CPU sanity for the FP8 block-quantized kernel cases (fp8_cases.py).

reference.dequantize_fp8_block equals the fp64 construction from the
format's definition; a torch emulation of the kernels' declared arithmetic
(per 128-wide k-block an fp32 partial sum from zero, then acc += s *
partial) equals the fp64 reference exactly on the cases
test_fp8_kernels_gpu.py runs — the proof that an inequality on the GPU is
the kernel's fault — and the same emulation reading the scale of a
transposed, next-row or next-k block does not.
"""

import math

import pytest
import torch

import fp8_cases as fc
import quant_cases as qc
from mlx_sharding_amd.ops import reference as ref

F8 = torch.float8_e4m3fn


# --------------------------------------------------------------------------
# the format
# --------------------------------------------------------------------------

def test_code_table_matches_torch_and_fp16():
    b = torch.arange(256)
    via_torch = fc.to_fp8(b).double()
    fin = torch.isfinite(fc.CODE_VALUE)
    assert int(fin.sum()) == 254 and set(b[~fin].tolist()) == {0x7F, 0xFF}
    assert torch.equal(via_torch[fin], fc.CODE_VALUE[fin])
    assert torch.isnan(via_torch[~fin]).all()
    # every finite code survives the round trip through fp16 (and bf16)
    v = fc.CODE_VALUE[fc.ALL_CODES]
    assert torch.equal(v.to(torch.float16).double(), v)
    assert torch.equal(v.to(torch.bfloat16).double(), v)
    # -0 and the subnormals are among them
    assert math.copysign(1.0, float(fc.CODE_VALUE[0x80])) == -1.0
    assert [float(fc.CODE_VALUE[c]) for c in range(1, 8)] == \
        [m / 8 * 2.0 ** -6 for m in range(1, 8)]


def test_small_codes():
    v = fc.CODE_VALUE[fc.SMALL_CODES]
    assert torch.equal(v * 8, (v * 8).round()) and float(v.abs().max()) == 16
    assert len(fc.SMALL_CODES) > 60


def test_scale_index_sees_slips():
    """Next row block, next k block and next expert always change the
    scale; a transposed lookup whenever rb - kb is odd."""
    for r in range(4):
        for e in range(3):
            for rb in range(3):
                for kb in range(4):
                    s = fc.scale_at(e, rb, kb, r)
                    assert s != fc.scale_at(e, rb + 1, kb, r)
                    assert s != fc.scale_at(e, rb, kb + 1, r)
                    assert s != fc.scale_at(e + 1, rb, kb, r)
                    if (rb - kb) % 2:
                        assert s != fc.scale_at(e, kb, rb, r)


@pytest.mark.parametrize("O,K,E", fc.DEQUANT_CASES)
def test_reference_dequant_equals_fp64_construction(O, K, E):
    """All 254 codes, partial last blocks in O and K, stacked."""
    codes, s, W = fc.exact_weight(O, K, E, pool=fc.ALL_CODES, cover=True)
    assert set(codes.flatten().tolist()) == set(fc.ALL_CODES.tolist())
    got = ref.dequantize_fp8_block(fc.to_fp8(codes), s)
    assert got.dtype == torch.float32 and got.shape == codes.shape
    assert torch.equal(got.double(), W)
    # -0 keeps its sign
    neg0 = codes == 0x80
    assert neg0.any() and torch.all(torch.signbit(got[neg0]))


def test_reference_dequant_rejects_wrong_scale_shape():
    codes, s, _ = fc.exact_weight(200, 384)
    with pytest.raises(ValueError):
        ref.dequantize_fp8_block(fc.to_fp8(codes), s.t().contiguous())
    with pytest.raises(ValueError):
        ref.dequantize_fp8_block(fc.to_fp8(codes), s[:1])


@pytest.mark.parametrize("shape", [(200, 300), (3, 130, 256), (128, 128)])
def test_quantize_round_trip(shape):
    """Block amax is reproduced exactly; elements outside the subnormal
    range of their block are within 2^-4 relative (3 mantissa bits)."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(*shape, generator=g) * 0.05
    w[..., :7, :9] = 0.0
    w8, s = ref.quantize_fp8_block(w)
    O, K = shape[-2:]
    assert w8.dtype == F8 and s.dtype == torch.float32
    assert s.shape == (*shape[:-2], fc.nblk(O), fc.nblk(K))
    d = ref.dequantize_fp8_block(w8, s)
    sx = fc.expand_scales(s, O, K).float()

    def block_amax(t):
        pad = torch.nn.functional.pad(
            t.abs(), (0, fc.nblk(K) * 128 - K, 0, fc.nblk(O) * 128 - O))
        return pad.reshape(*shape[:-2], fc.nblk(O), 128, fc.nblk(K), 128) \
            .amax(dim=(-3, -1))

    assert torch.equal(block_amax(d), block_amax(w))
    normal = (w / sx).abs() >= 2.0 ** -6
    rel = ((d - w).abs() / w.abs().clamp_min(1e-30))[normal]
    print("quantize_fp8_block %s: max rel err %.4f" % (shape, float(rel.max())))
    assert float(rel.max()) <= 2.0 ** -4
    # an all-zero block gets scale 1 and stays zero
    z8, zs = ref.quantize_fp8_block(torch.zeros(130, 128))
    assert torch.all(zs == 1) and not z8.float().any()


# --------------------------------------------------------------------------
# the kernel cases: emulation == reference, slipped emulation != reference
# --------------------------------------------------------------------------

SLIPS = {"transposed": dict(transpose=True), "rb+1": dict(slip=(1, 0)),
         "kb+1": dict(slip=(0, 1))}
_seen = {}


def _note(family, top):
    _seen[family] = max(_seen.get(family, 0.0), top)


def _check_linear(x64, codes, r, want64, e=0):
    got = fc.emulate_linear(x64, codes, r, e)
    assert torch.equal(got.double(), want64)
    for name, kw in SLIPS.items():
        bad = fc.emulate_linear(x64, codes, r, e, **kw)
        assert not torch.equal(bad.double(), want64), name


@pytest.mark.parametrize("K", fc.GEMV_KS)
@pytest.mark.parametrize("M", fc.GEMV_MS)
def test_gemv_dense_cases(M, K):
    x, codes, s, W, y, top = fc.gemv_dense_case(M, fc.GEMV_O, K)
    _note("gemv dense x", top)
    assert torch.equal(ref.fp8_block_linear(x.float(), fc.to_fp8(codes),
                                            s).double(), y)
    _check_linear(x, codes, 0, y)


@pytest.mark.parametrize("name", ("GEMV_DIRECT", "GEMV_SPLIT"))
def test_gemv_nsplit_cases(name):
    c = getattr(fc, name)
    x, codes, s, W, y, top = fc.gemv_dense_case(c["M"], c["O"], c["K"])
    _note("gemv dense x", top)
    _check_linear(x, codes, 0, y)


@pytest.mark.parametrize("K", fc.GEMV_KS)
def test_gemv_onehot_cases(K):
    codes, s, W = fc.gemv_onehot_weight(fc.GEMV_O, K)
    assert set(codes.flatten().tolist()) == set(fc.ALL_CODES.tolist())
    M = 64
    for off in qc.one_hot_offsets(M, K):
        x = qc.one_hot_x(M, K, off)
        want = W[:, qc.one_hot_cols(M, K, off)].t()
        assert torch.equal(x @ W.t(), want)
        assert qc._roundtrip(want, torch.bfloat16)
        got = fc.emulate_linear(x, codes, 7 % 4)
        assert torch.equal(got.double(), want)
    # the slips show on the whole sweep (a single offset may sit in a block
    # whose wrong scale happens to coincide)
    xs = torch.cat([qc.one_hot_x(M, K, o) for o in qc.one_hot_offsets(M, K)])
    _check_linear(xs, codes, 7 % 4, xs @ W.t())


@pytest.mark.parametrize("plan", list(fc.PLANS))
@pytest.mark.parametrize("H", fc.MOE_HS)
@pytest.mark.parametrize("kind", ("a", "b"))
def test_gateup_cases(kind, H, plan):
    plan_d = fc.PLANS[plan]
    gate, up = fc.gateup_weights(kind, fc.MOE_I, H)
    live = [e for e in range(fc.E) if e != qc.UNUSED_EXPERT]
    if kind == "a":
        assert set(up[0][live][..., 1:].flatten().tolist()) == \
            set(fc.ALL_CODES.tolist())
    for m in (gate, up):
        assert torch.equal(
            ref.dequantize_fp8_block(fc.to_fp8(m[0]), m[1]).double(), m[2])
    offs = qc.gateup_offsets(plan_d, H)
    seed = 0
    for off in offs[:: max(1, len(offs) // 6)]:
        want = qc.gateup_expected(kind, gate[2], up[2], plan_d, H, off,
                                  torch.float16)
        x = qc.gateup_x(plan_d["N"], H, off)
        for p, e, t in qc.plan_pairs(plan_d["plan"])[::5]:
            g = fc.emulate_linear(x[t:t + 1], gate[0][e], seed % 4, e)[0]
            u = fc.emulate_linear(x[t:t + 1], up[0][e], (seed + 1) % 4, e)[0]
            h = (g / (1.0 + torch.exp(-g)) * u).to(torch.float16)
            assert torch.equal(h.double(), want[p])
    # negative controls on the matrix that carries the data, whole sweep
    x = torch.cat([qc.gateup_x(plan_d["N"], H, o) for o in offs])
    for e in live:
        m, r = (up, 1) if kind == "a" else (gate, 0)
        _check_linear(x, m[0][e], r, x @ m[2][e].t(), e)


@pytest.mark.parametrize("plan", list(fc.PLANS))
@pytest.mark.parametrize("I", fc.DOWN_IS)
def test_down_cases(I, plan):
    plan_d = fc.PLANS[plan]
    codes, s, W, h, out, top = fc.down_case(I, plan_d)
    _note("moe down", top)
    subs, _ = qc.build_subranges(plan_d["plan"])
    r = 11 % 4
    for name, kw in [("ok", {})] + list(SLIPS.items()):
        got = torch.zeros(plan_d["N"], fc.DOWN_H, dtype=torch.float32)
        for p, e, t in qc.plan_pairs(plan_d["plan"]):
            y = fc.emulate_linear(h[p:p + 1], codes[e], r, e, **kw)[0]
            got[t] += subs[4][p] * y
        assert torch.equal(got.double(), out) == (name == "ok"), name


def test_bit_budget():
    """Worst-case bounds of the module docstring, and the seen maxima."""
    gemv_bound = 384 * 2 * 16 * 2 / fc.LSB
    down_bound = 2 * 384 * 2 * 16 * 2 / fc.DOWN_LSB
    assert gemv_bound < qc.F24 and down_bound < qc.F24
    print("fp8 gemv dense x: bound 2^%.1f" % math.log2(gemv_bound))
    print("fp8 moe down:     bound 2^%.1f" % math.log2(down_bound))
    for M in fc.GEMV_MS:
        _note("gemv dense x", fc.gemv_dense_case(M, fc.GEMV_O, 384)[5])
    for plan_d in fc.PLANS.values():
        _note("moe down", fc.down_case(384, plan_d)[5])
    for fam, top in _seen.items():
        print("fp8 %-14s seen 2^%.1f" % (fam, math.log2(top)))
        assert top < qc.F24


# --------------------------------------------------------------------------
# random-data bound: the emulated arithmetic sits inside it
# --------------------------------------------------------------------------

def test_random_bound_holds_for_emulation():
    w8, s, x, ref64, B = fc.random_gemv_case()
    got = fc.emulate_moe_linear(x, w8, s).to(torch.bfloat16)
    r_gemv = fc.gemv_formula_ratio(got, ref64, B)
    assert fc.bf16_within(got, ref64, B)
    # a perturbation of two accumulation bounds is caught
    assert not fc.bf16_within((ref64 + 3 * B + 2.0 ** -7 * ref64.abs())
                              .float().to(torch.bfloat16), ref64, B)
    mats, xm, hh = fc.random_moe_case()
    subs, _ = qc.build_subranges(qc.PLAN16["plan"])
    dref, dbound = fc.random_down_ref(mats, hh)
    gref, gbound = fc.random_gateup_ref(mats, xm)
    dgot = torch.zeros_like(dref, dtype=torch.float32)
    ggot = torch.zeros_like(gref, dtype=torch.float16)
    for p, e, t in qc.plan_pairs(qc.PLAN16["plan"]):
        dgot[t] += subs[4][p] * fc.emulate_moe_linear(
            hh[p:p + 1], mats["down"][0][e], mats["down"][1][e])[0]
        g = fc.emulate_moe_linear(xm[t:t + 1], mats["gate"][0][e],
                                  mats["gate"][1][e])[0]
        u = fc.emulate_moe_linear(xm[t:t + 1], mats["up"][0][e],
                                  mats["up"][1][e])[0]
        ggot[p] = (g / (1.0 + torch.exp(-g)) * u).to(torch.float16)
    live = torch.tensor([p for p, _, _ in qc.plan_pairs(qc.PLAN16["plan"])])
    r_down = float(((dgot.double() - dref).abs() / dbound.clamp_min(1e-30)).max())
    r_gu = float(((ggot.double() - gref).abs() / gbound)[live].max())
    print("worst |error| / bound (CPU emulation): gemv %.2f down %.2f "
          "gateup %.2f" % (r_gemv, r_down, r_gu))
    assert r_down <= 1 and r_gu <= 1
