"""Bit-exact tests of every quantized GEMM / MoE kernel variant.

Inputs come from quant_cases.py: every weight, product and partial sum is
exactly representable, so fp32 accumulation is exact in any order and each
kernel must equal the fp64 reference cast to its output dtype
(torch.equal, no tolerance).  test_quant_cases_cpu.py proves on the CPU
that the kernels' declared arithmetic is exact on these inputs.  The last
section is the one tolerance-based layer: an arithmetic budget for the
fp16-dequant 4-bit kernels on random data.
"""

import pytest
import torch

import quant_cases as qc
from mlx_sharding_amd import ops

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DEV = "cuda"


def ext():
    e = ops.hip_ext()
    assert e is not None, "HIP extension not built"
    return e


def assert_same(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = (got != want) | (got.isnan() != want.isnan())
        first = bad.nonzero()[0].tolist()
        pytest.fail("%s: %d of %d elements differ, first at %s: got %r want %r"
                    % (what, int(bad.sum()), bad.numel(), first,
                       got[tuple(first)].item(), want[tuple(first)].item()))


def packed(q, bits):
    return qc.pack(q, bits).to(DEV)


def repacked(q, bits):
    return ops.repack_w4(qc.pack(q, bits), bits).to(DEV)


def one_hot_sweep(fn, M, K, W64, in_dtype, out_dtype, what):
    """Run fn on ceil(K / M) one-hot activations; row m of call i must be
    column (offset_i + m) mod K of the weight, exactly."""
    offs = qc.one_hot_offsets(M, K)
    cols = torch.stack([qc.one_hot_cols(M, K, o) for o in offs])    # [n, M]
    assert set(cols.flatten().tolist()) == set(range(K))
    X = torch.zeros(len(offs), M, K, dtype=in_dtype)
    X.scatter_(2, cols[..., None], 1.0)
    Xd = X.to(DEV)
    got = torch.stack([fn(Xd[i]) for i in range(len(offs))])
    want64 = W64.t()[cols]                                          # [n, M, O]
    assert torch.equal(want64.to(out_dtype).double(), want64)
    assert_same(got, want64.to(out_dtype), what + " one-hot sweep")


# --------------------------------------------------------------------------
# dequant and the dense GEMVs
# --------------------------------------------------------------------------

@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_dequant_exact(bits, gs):
    O, H = qc.DEQUANT_SHAPE
    q, sc, bi, W64 = qc.exact_weights(O, H, gs, bits)
    got = ext().dequant(packed(q, bits), sc.to(DEV), bi.to(DEV), H, gs, bits)
    assert_same(got, W64.to(BF16), "dequant")


@pytest.mark.parametrize("M", qc.SCALAR_GEMV["Ms"])
@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_w4a16_gemv_scalar_exact(bits, gs, M):
    O, H = qc.SCALAR_GEMV["O"], qc.SCALAR_GEMV["H"]
    x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
    wq, scd, bid = packed(q, bits), sc.to(DEV), bi.to(DEV)
    fn = lambda xx: ext().w4a16_gemv(xx, wq, scd, bid, gs, bits)  # noqa: E731
    # both sides rounded to bf16: the fp32 sum is exact, |y| is not 8 bits
    assert_same(fn(x.to(BF16).to(DEV)), y.to(BF16), "scalar gemv dense")
    one_hot_sweep(fn, M, H, W64, BF16, BF16, "scalar gemv")


@pytest.mark.parametrize("H", qc.MFMA_GEMV["Hs"])
@pytest.mark.parametrize("M", qc.MFMA_GEMV["Ms"])
@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_w4a16_gemv_mfma_exact(bits, gs, M, H):
    O = qc.MFMA_GEMV["O"]
    nk = ext().w4a16_mfma_nsplit(M, O, H)
    assert (nk > 1) == (H == 1024), "H=1024 must split K, H=384 must not"
    x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
    wq, scd, bid = packed(q, bits), sc.to(DEV), bi.to(DEV)
    fn = lambda xx: ext().w4a16_gemv(xx, wq, scd, bid, gs, bits)  # noqa: E731
    assert_same(fn(x.to(BF16).to(DEV)), y.to(BF16), "mfma gemv dense")
    one_hot_sweep(fn, M, H, W64, BF16, BF16, "mfma gemv")


@pytest.mark.parametrize("M", qc.W4F16_MS)
@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_w4f16_gemv_exact(bits, gs, M):
    H, O = qc.W4F16_H[gs], qc.W4F16_O
    assert ext().w4f16_gemv_nsplit(M, O, H) == 3       # split-K, tails as planned
    x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
    rp, scd, bid = repacked(q, bits), sc.to(DEV), bi.to(DEV)
    fn = lambda xx: ext().w4f16_gemv(xx, rp, scd, bid, gs, bits)  # noqa: E731
    assert_same(fn(x.to(F16).to(DEV)), y.to(BF16), "w4f16 gemv dense")
    one_hot_sweep(fn, M, H, W64, F16, BF16, "w4f16 gemv")


@pytest.mark.parametrize("bits", (4, 8))
def test_w4f16_gemv_direct_store_exact(bits):
    c = qc.W4F16_DIRECT
    M, O, H, gs = c["M"], c["O"], c["H"], c["gs"]
    assert ext().w4f16_gemv_nsplit(M, O, H) == 1       # direct bf16 store
    x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
    rp, scd, bid = repacked(q, bits), sc.to(DEV), bi.to(DEV)
    fn = lambda xx: ext().w4f16_gemv(xx, rp, scd, bid, gs, bits)  # noqa: E731
    assert_same(fn(x.to(F16).to(DEV)), y.to(BF16), "w4f16 gemv direct dense")
    one_hot_sweep(fn, M, H, W64, F16, BF16, "w4f16 gemv direct")


@pytest.mark.parametrize("ksegs", qc.KSEG["ksegs"])
@pytest.mark.parametrize("M", qc.KSEG["Ms"])
@pytest.mark.parametrize("gs", (32, 64, 128))
def test_gemm_m64_kseg_w4_exact(gs, M, ksegs):
    N, K = qc.KSEG["N"], qc.KSEG["K"]
    x, q, sc, bi, W64, y = qc.gemv_dense_case(M, N, K, gs, 4)
    rp, scd, bid = repacked(q, 4), sc.to(DEV), bi.to(DEV)
    fn = lambda xx: ext().gemm_m64_kseg_w4(xx, rp, scd, bid, gs, ksegs)  # noqa: E731
    assert_same(fn(x.to(F16).to(DEV)), y.to(BF16), "kseg w4 dense")
    one_hot_sweep(fn, M, K, W64, F16, BF16, "kseg w4")


# --------------------------------------------------------------------------
# MoE kernels on hand-built sub-ranges
# --------------------------------------------------------------------------

def dev_subs(plan_d):
    subs, live = qc.build_subranges(plan_d["plan"])
    return tuple(t.to(DEV) for t in subs), live


def gateup_sweep(fn, kind, Wg64, Wu64, plan_d, H, in_dtype, out_dtype, what):
    """fn(x) -> h [P, I].  Every offset of the sweep; dead tokens' x rows
    are NaN; only the live sorted rows are compared."""
    _, live = qc.build_subranges(plan_d["plan"])
    dead = qc.dead_tokens(plan_d)
    offs = qc.gateup_offsets(plan_d, H)
    X = torch.stack([qc.poison_rows(qc.gateup_x(plan_d["N"], H, o), dead)
                     for o in offs]).to(in_dtype).to(DEV)
    want = torch.stack([qc.gateup_expected(kind, Wg64, Wu64, plan_d, H, o, out_dtype)
                        for o in offs]).to(out_dtype)
    got = torch.stack([fn(X[i]) for i in range(len(offs))])
    assert_same(got[:, live], want[:, live], what)


@pytest.mark.parametrize("kind", ("a", "b"))
@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_moe_w4f16_gateup_exact(bits, gs, kind):
    subs, _ = dev_subs(qc.PLAN16)
    P = subs[3].numel()
    for H in qc.MOE_F16_DIMS[gs]:
        gate, up = qc.gateup_expert_weights(kind, qc.N_EXPERTS, qc.MOE_OUT, H,
                                            gs, bits)
        gq, uq = repacked(gate[0], bits), repacked(up[0], bits)
        gsc, usc = (qc.poison_expert(t).to(DEV) for t in (gate[1], up[1]))
        gbi, ubi = gate[2].to(DEV), up[2].to(DEV)
        fn = lambda x: ext().moe_w4f16_gateup(  # noqa: E731
            x, gq, uq, gsc, gbi, usc, ubi, *subs[:4], P, gs, bits)
        gateup_sweep(fn, kind, gate[3], up[3], qc.PLAN16, H, F16, F16,
                     "moe_w4f16_gateup (%s) H=%d" % (kind, H))


@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_moe_w4f16_down_exact(bits, gs):
    subs, live = dev_subs(qc.PLAN16)
    N = qc.PLAN16["N"]
    for I in qc.MOE_F16_DIMS[gs]:
        q, sc, bi, W64 = qc.exact_expert_weights(qc.N_EXPERTS, qc.MOE_OUT, I,
                                                 gs, bits)
        h = qc.down_h(qc.PLAN16, I)
        want = qc.down_expected(W64, h, qc.PLAN16)
        hp = qc.poison_rows(h, (~live).nonzero().flatten().tolist())
        got = ext().moe_w4f16_down(hp.to(F16).to(DEV), repacked(q, bits),
                                   qc.poison_expert(sc).to(DEV), bi.to(DEV),
                                   *subs, N, gs, bits)
        assert_same(got, want.to(F32), "moe_w4f16_down I=%d" % I)
        assert not got[qc.dead_tokens(qc.PLAN16)].any()


@pytest.mark.parametrize("bits,gs,H", qc.MOE_W4_MFMA)
def test_moe_w4_mfma_exact(bits, gs, H):
    subs, live = dev_subs(qc.PLAN32)
    N, P, O = qc.PLAN32["N"], subs[3].numel(), qc.MOE_OUT
    dead = qc.dead_tokens(qc.PLAN32)
    q, sc, bi, W64 = qc.exact_expert_weights(qc.N_EXPERTS, O, H, gs, bits)
    wq, scd, bid = packed(q, bits), qc.poison_expert(sc).to(DEV), bi.to(DEV)
    fn = lambda x: ext().moe_w4_mfma(  # noqa: E731
        qc.poison_rows(x, dead).to(BF16).to(DEV), wq, scd, bid, *subs[:4], P,
        gs, bits)
    # dense integers: both sides rounded to bf16 (the fp32 sum is exact)
    x = qc.dense_int_x(N, H)
    want = qc.moe_linear_expected(W64, x, qc.PLAN32)
    qc.check_budget(qc.moe_linear_expected(W64.abs(), x.abs(), qc.PLAN32), 0.25,
                    "moe_w4_mfma")
    assert_same(fn(x)[live], want.to(BF16)[live], "moe_w4_mfma dense")
    for off in qc.one_hot_offsets(N, H):
        want = qc.moe_linear_expected(W64, qc.one_hot_x(N, H, off), qc.PLAN32)
        assert torch.equal(want.to(BF16).double(), want)
        assert_same(fn(qc.one_hot_x(N, H, off))[live], want.to(BF16)[live],
                    "moe_w4_mfma one-hot offset %d" % off)


@pytest.mark.parametrize("kind", ("a", "b"))
@pytest.mark.parametrize("max_tok", (4, 16))
def test_bf16_moe_gateup_exact(max_tok, kind):
    plan_d = qc.BF16_PLANS[max_tok]
    subs, _ = dev_subs(plan_d)
    H, I, P = qc.BF16_MOE["H"], qc.BF16_MOE["I"], subs[3].numel()
    Wg, Wu = qc.gateup_dense_weights(kind, qc.N_EXPERTS, I, H)
    gw, uw = (qc.poison_expert(w).to(BF16).to(DEV) for w in (Wg, Wu))
    fn = lambda x: ext().moe_gateup_grouped(  # noqa: E731
        x, gw, uw, *subs[:4], P, max_tok)
    gateup_sweep(fn, kind, Wg, Wu, plan_d, H, BF16, BF16,
                 "moe_gateup_grouped max_tok=%d (%s)" % (max_tok, kind))


@pytest.mark.parametrize("inner,outer", ((96, 416), (416, 96)))
@pytest.mark.parametrize("max_tok", (4, 16))
def test_bf16_moe_down_exact(max_tok, inner, outer):
    plan_d = qc.BF16_PLANS[max_tok]
    subs, live = dev_subs(plan_d)
    N = plan_d["N"]
    g = torch.Generator().manual_seed(3)
    Wd = torch.randint(-7, 8, (qc.N_EXPERTS, outer, inner), generator=g).double()
    h = qc.down_h(plan_d, inner)
    want = qc.down_expected(Wd, h, plan_d)
    hp = qc.poison_rows(h, (~live).nonzero().flatten().tolist())
    got = ext().moe_down_grouped(hp.to(BF16).to(DEV),
                                 qc.poison_expert(Wd).to(BF16).to(DEV), *subs,
                                 N, max_tok)
    assert_same(got, want.to(F32), "moe_down_grouped max_tok=%d" % max_tok)
    assert not got[qc.dead_tokens(plan_d)].any()


def test_scalar_grouped_kernels_refuse_h_not_multiple_of_8():
    """The max_tok <= 4 kernels read 8 elements at a time: the bindings
    must refuse H = 36 before any launch."""
    subs, _ = dev_subs(qc.PLAN4)
    N, P, E = qc.PLAN4["N"], subs[3].numel(), qc.N_EXPERTS
    x = torch.zeros(N, 36, dtype=BF16, device=DEV)
    w = torch.zeros(E, 8, 36, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="% 8"):
        ext().moe_gateup_grouped(x, w, w, *subs[:4], P, 4)
    h = torch.zeros(P, 36, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="% 8"):
        ext().moe_down_grouped(h, w, *subs, N, 4)
    # ... and an output dimension that is no multiple of 8
    x8 = torch.zeros(N, 64, dtype=BF16, device=DEV)
    w36 = torch.zeros(E, 36, 64, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="% 8"):
        ext().moe_gateup_grouped(x8, w36, w36, *subs[:4], P, 4)


def test_moe_w4_mfma_refuses_partial_group():
    """H = 288 is not a whole number of 64-wide groups: the kernel would
    index past the row's scales, so the binding must refuse."""
    subs, _ = dev_subs(qc.PLAN32)
    P, E, O, H = subs[3].numel(), qc.N_EXPERTS, 16, 288
    x = torch.zeros(qc.PLAN32["N"], H, dtype=BF16, device=DEV)
    wq = torch.zeros(E, O, H // 8, dtype=torch.int32, device=DEV)
    sb = torch.zeros(E, O, H // 64, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="H % gs"):
        ext().moe_w4_mfma(x, wq, sb, sb, *subs[:4], P, 64, 4)


# --------------------------------------------------------------------------
# prefill data movement
# --------------------------------------------------------------------------

def test_moe_scatter_rows_exact():
    H, P = qc.SCATTER["H"], qc.SCATTER["P"]
    g = torch.Generator().manual_seed(5)
    src = torch.randn(9, H, generator=g).to(BF16)
    src_idx = torch.tensor([4, 0, 8, 4, 2, 7, 1], dtype=torch.int32)
    dst_idx = torch.tensor([10, 3, 0, 12, 7, 1, 5], dtype=torch.int32)
    assert src_idx.numel() == P
    dst = torch.full((13, H), -7.0, dtype=BF16)
    want = dst.clone()
    want[dst_idx.long()] = src[src_idx.long()]
    got = dst.to(DEV)
    ext().moe_scatter_rows(src.to(DEV), got, src_idx.to(DEV), dst_idx.to(DEV))
    assert_same(got.view(torch.int16), want.view(torch.int16), "scatter rows")
    untouched = sorted(set(range(13)) - set(dst_idx.tolist()))
    assert torch.all(got[untouched].float() == -7.0)


def test_moe_gather_reduce_exact():
    H, N, K = qc.SCATTER["H"], qc.SCATTER["P"], qc.SCATTER["K"]
    g = torch.Generator().manual_seed(6)
    d = torch.randint(-8, 9, (23, H), generator=g).double()
    pos = torch.stack([torch.randperm(23, generator=g)[:K] for _ in range(N)])
    wts = torch.tensor(qc.ROUTE_WTS)[torch.randint(0, 3, (N, K), generator=g)]
    want = (wts.double()[..., None] * d[pos]).sum(1)
    assert torch.equal(want.to(BF16).double(), want)
    got = ext().moe_gather_reduce(d.to(BF16).to(DEV), pos.to(torch.int32).to(DEV),
                                  wts.to(DEV), N)
    assert_same(got, want.to(BF16), "gather reduce")


# --------------------------------------------------------------------------
# arithmetic budget of the fp16-dequant 4-bit kernels (random data)
# --------------------------------------------------------------------------

def assert_within(got, ref64, bound, what):
    err = (got.double().cpu() - ref64).abs()
    ratio = float((err / bound).max())
    print("%s: worst |error| / bound = %.3f" % (what, ratio))
    over = int((err > bound).sum())
    assert over == 0, "%s: %d elements past the bound, worst ratio %.3f" % (
        what, over, ratio)


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_w4f16_gemv_arithmetic_budget(gs):
    wq, sc, bi, q, x, ref64, A = qc.budget_gemv_case(gs)
    got = ext().w4f16_gemv(x.to(DEV), ops.repack_w4(wq, 4).to(DEV), sc.to(DEV),
                           bi.to(DEV), gs, 4)
    assert_within(got, ref64, qc.gemv_bound(ref64, A, 2.0 ** -9), "w4f16_gemv")


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_moe_w4f16_down_arithmetic_budget(gs):
    mats, x, hh = qc.budget_moe_case(gs)
    subs, _ = dev_subs(qc.PLAN16)
    wq, sc, bi, _ = mats["down"]
    ref64, bound = qc.budget_down_ref(mats, hh, gs)
    got = ext().moe_w4f16_down(hh.to(DEV), ops.repack_w4(wq, 4).to(DEV),
                               sc.to(DEV), bi.to(DEV), *subs, qc.PLAN16["N"],
                               gs, 4)
    used = bound > 0
    assert not got.cpu()[~used].any()
    assert_within(got.cpu()[used], ref64[used], bound[used], "moe_w4f16_down")


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_moe_w4f16_gateup_arithmetic_budget(gs):
    mats, x, hh = qc.budget_moe_case(gs)
    subs, live = dev_subs(qc.PLAN16)
    ref64, bound = qc.budget_gateup_ref(mats, x, gs)
    g, u = mats["gate"], mats["up"]
    got = ext().moe_w4f16_gateup(
        x.to(DEV), ops.repack_w4(g[0], 4).to(DEV), ops.repack_w4(u[0], 4).to(DEV),
        g[1].to(DEV), g[2].to(DEV), u[1].to(DEV), u[2].to(DEV), *subs[:4],
        subs[3].numel(), gs, 4)
    assert_within(got.cpu()[live], ref64[live], bound[live], "moe_w4f16_gateup")
