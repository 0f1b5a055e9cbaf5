"""The FP8 block-quantized (W8A16) kernels on the GPU, on the exact cases of
fp8_cases.py: every result must equal the fp64 reference bit for bit
(test_fp8_cases_cpu.py proves that on an emulation of the kernels' declared
arithmetic).  The random-data tests check the accumulation bound of the
fp8_cases docstring and print the worst |error| / bound.

Measured on an MI355X (seed 0, K = 384), worst |error| / bound:
fp8f16_gemv 1.71 against the stated formula with u_out = 2^-9 — bf16's unit
roundoff is 2^-8, the CPU emulation gives the same 1.71 (explained in
fp8_cases.py) and the asserted interval criterion holds; moe_fp8f16_down
below 0.01; moe_fp8f16_gateup 0.36.
"""

import pytest
import torch

import fp8_cases as fc
import quant_cases as qc
from mlx_sharding_amd import ops

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DEV = "cuda"
SENTINEL = 1234.0


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


def dev8(codes):
    return fc.to_fp8(codes).to(DEV)


def dev_subs(plan_d):
    subs, live = qc.build_subranges(plan_d["plan"])
    return tuple(t.to(DEV) for t in subs), live


# --------------------------------------------------------------------------
# dequant
# --------------------------------------------------------------------------

@pytest.mark.parametrize("O,K,E", fc.DEQUANT_CASES)
def test_dequant_exact(O, K, E):
    codes, s, W = fc.exact_weight(O, K, E, pool=fc.ALL_CODES, cover=True)
    got = ext().fp8_block_dequant(dev8(codes), s.to(DEV))
    assert_same(got, W.to(BF16), "fp8_block_dequant")
    neg0 = codes == 0x80
    assert torch.all(torch.signbit(got.cpu().float()[neg0]))
    assert_same(ops.dequantize_fp8_block(dev8(codes), s.to(DEV)), W.to(BF16),
                "ops.dequantize_fp8_block")


# --------------------------------------------------------------------------
# GEMV
# --------------------------------------------------------------------------

def _gemv_fn(codes, s):
    w, sd = dev8(codes), s.to(DEV)
    return lambda xx: ext().fp8f16_gemv(xx, w, sd)


@pytest.mark.parametrize("K", fc.GEMV_KS)
@pytest.mark.parametrize("M", fc.GEMV_MS)
def test_gemv_exact(M, K):
    O = fc.GEMV_O
    x, codes, s, W, y, _ = fc.gemv_dense_case(M, O, K)
    # both sides rounded to bf16: the fp32 sum is exact, |y| is not 8 bits
    assert_same(_gemv_fn(codes, s)(x.to(F16).to(DEV)), y.to(BF16),
                "fp8f16_gemv dense")
    # one-hot sweep over every column, all 254 codes
    codes, s, W = fc.gemv_onehot_weight(O, K)
    fn = _gemv_fn(codes, s)
    offs = qc.one_hot_offsets(M, K)
    cols = torch.stack([qc.one_hot_cols(M, K, o) for o in offs])
    assert set(cols.flatten().tolist()) == set(range(K))
    X = torch.zeros(len(offs), M, K, dtype=F16)
    X.scatter_(2, cols[..., None], 1.0)
    Xd = X.to(DEV)
    got = torch.stack([fn(Xd[i]) for i in range(len(offs))])
    want = W.t()[cols]
    assert torch.equal(want.to(BF16).double(), want)
    assert_same(got, want.to(BF16), "fp8f16_gemv one-hot sweep")


def test_gemv_direct_and_split_stores():
    d, sp = fc.GEMV_DIRECT, fc.GEMV_SPLIT
    assert ext().fp8f16_gemv_nsplit(d["M"], d["O"], d["K"]) == 1
    assert ext().fp8f16_gemv_nsplit(sp["M"], sp["O"], sp["K"]) > 1
    for c in (d, sp):
        x, codes, s, W, y, _ = fc.gemv_dense_case(c["M"], c["O"], c["K"])
        assert_same(_gemv_fn(codes, s)(x.to(F16).to(DEV)), y.to(BF16),
                    "fp8f16_gemv %r" % (c,))


# --------------------------------------------------------------------------
# MoE gate-up
# --------------------------------------------------------------------------

@pytest.mark.parametrize("plan", list(fc.PLANS))
@pytest.mark.parametrize("H", fc.MOE_HS)
@pytest.mark.parametrize("kind", ("a", "b"))
def test_moe_gateup_exact(kind, H, plan):
    plan_d = fc.PLANS[plan]
    subs, live = dev_subs(plan_d)
    P = subs[3].numel()
    gate, up = fc.gateup_weights(kind, fc.MOE_I, H)
    gc8, gs = fc.poison_unused(gate[0], gate[1])
    uc8, us = fc.poison_unused(up[0], up[1])
    gw, uw, gsd, usd = dev8(gc8), dev8(uc8), gs.to(DEV), us.to(DEV)
    dead = qc.dead_tokens(plan_d)
    offs = qc.gateup_offsets(plan_d, H)
    X = torch.stack([qc.poison_rows(qc.gateup_x(plan_d["N"], H, o), dead)
                     for o in offs]).to(F16).to(DEV)
    want = torch.stack([qc.gateup_expected(kind, gate[2], up[2], plan_d, H, o,
                                           F16) for o in offs]).to(F16)
    got = torch.stack([ext().moe_fp8f16_gateup(X[i], gw, uw, gsd, usd,
                                               *subs[:4], P)
                       for i in range(len(offs))])
    assert_same(got[:, live], want[:, live],
                "moe_fp8f16_gateup (%s) H=%d" % (kind, H))
    # rows outside every sub-range stay untouched.  The binding allocates
    # h itself, so pre-fill the block it will get: the caching allocator
    # hands a freed block of the same size straight back.
    del got
    h = torch.full((P, fc.MOE_I), SENTINEL, dtype=F16, device=DEV)
    ptr = h.data_ptr()
    del h
    h2 = ext().moe_fp8f16_gateup(X[0], gw, uw, gsd, usd, *subs[:4], P)
    assert h2.data_ptr() == ptr, "allocator did not recycle the sentinel block"
    assert (~live).any() and torch.all(h2.cpu()[~live] == SENTINEL)
    assert_same(h2[live], want[0][live], "gate-up rerun")


@pytest.mark.parametrize("plan", list(fc.PLANS))
def test_moe_gateup_acc_clears_nan_buffer(plan):
    """The _acc variant returns (h, acc) with acc zeroed by the launch: a
    NaN-filled block recycled by the allocator must come back all zero, for
    a buffer larger than the grid's thread count too."""
    plan_d = fc.PLANS[plan]
    subs, live = dev_subs(plan_d)
    P, N, H = subs[3].numel(), plan_d["N"], 128
    gate, up = fc.gateup_weights("a", fc.MOE_I, H)
    gw, uw = dev8(gate[0]), dev8(up[0])
    gsd, usd = gate[1].to(DEV), up[1].to(DEV)
    x = qc.gateup_x(N, H, 0).to(F16).to(DEV)
    want = qc.gateup_expected("a", gate[2], up[2], plan_d, H, 0, F16).to(F16)
    # grid = 4 x S blocks of 256 threads; Hout makes N * Hout exceed it
    for Hout in (fc.DOWN_H, 4099):
        junk = torch.full((N, Hout), float("nan"), device=DEV, dtype=F32)
        ptr = junk.data_ptr()
        del junk
        h, acc = ext().moe_fp8f16_gateup_acc(x, gw, uw, gsd, usd, *subs[:4],
                                             P, N, Hout)
        assert acc.shape == (N, Hout) and acc.dtype == F32
        assert acc.data_ptr() == ptr, "allocator did not recycle the NaN block"
        assert not acc.cpu().any() and not acc.cpu().isnan().any()
        assert_same(h[live], want[live], "gateup_acc h")


# --------------------------------------------------------------------------
# MoE down
# --------------------------------------------------------------------------

@pytest.mark.parametrize("plan", list(fc.PLANS))
@pytest.mark.parametrize("I", fc.DOWN_IS)
def test_moe_down_exact(I, plan):
    plan_d = fc.PLANS[plan]
    subs, live = dev_subs(plan_d)
    N = plan_d["N"]
    codes, s, W, h, want, _ = fc.down_case(I, plan_d)
    c8, s8 = fc.poison_unused(codes, s)
    dw, dsd = dev8(c8), s8.to(DEV)
    hp = qc.poison_rows(h, (~live).nonzero().flatten().tolist()).to(F16).to(DEV)
    got = ext().moe_fp8f16_down(hp, dw, dsd, *subs, N)
    assert_same(got, want.to(F32), "moe_fp8f16_down I=%d" % I)
    assert not got[qc.dead_tokens(plan_d)].any()
    # through a NaN-pre-filled accumulator cleared by gate-up's launch
    gate, up = fc.gateup_weights("a", fc.MOE_I, 128)
    x = qc.gateup_x(N, 128, 0).to(F16).to(DEV)
    junk = torch.full((N, fc.DOWN_H), float("nan"), device=DEV, dtype=F32)
    del junk
    _, acc = ext().moe_fp8f16_gateup_acc(
        x, dev8(gate[0]), dev8(up[0]), gate[1].to(DEV), up[1].to(DEV),
        *subs[:4], subs[3].numel(), N, fc.DOWN_H)
    got = ext().moe_fp8f16_down(hp, dw, dsd, *subs, N, acc)
    assert got.data_ptr() == acc.data_ptr()
    assert_same(got, want.to(F32), "moe_fp8f16_down (acc) I=%d" % I)


# --------------------------------------------------------------------------
# random data: the accumulation bound
# --------------------------------------------------------------------------

def test_random_layer_within_bound():
    w8, s, x, ref64, B = fc.random_gemv_case()
    got = ext().fp8f16_gemv(x.to(DEV), w8.to(DEV), s.to(DEV)).cpu()
    r_gemv = fc.gemv_formula_ratio(got, ref64, B)
    mats, xm, hh = fc.random_moe_case()
    subs, live = dev_subs(qc.PLAN16)
    P, N = subs[3].numel(), qc.PLAN16["N"]
    g, u, d = (tuple(t.to(DEV) for t in mats[n][:2])
               for n in ("gate", "up", "down"))
    dref, dbound = fc.random_down_ref(mats, hh)
    gref, gbound = fc.random_gateup_ref(mats, xm)
    dgot = ext().moe_fp8f16_down(hh.to(DEV), d[0], d[1], *subs, N).cpu()
    ggot = ext().moe_fp8f16_gateup(xm.to(DEV), g[0], u[0], g[1], u[1],
                                   *subs[:4], P).cpu()
    r_down = float(((dgot.double() - dref).abs()
                    / dbound.clamp_min(1e-30)).max())
    r_gu = float(((ggot.double() - gref).abs() / gbound)[live].max())
    print("worst |error| / bound (MI355X): gemv %.2f (stated formula) "
          "down %.2f gateup %.2f" % (r_gemv, r_down, r_gu))
    assert fc.bf16_within(got, ref64, B)
    assert r_down <= 1 and r_gu <= 1


# --------------------------------------------------------------------------
# graph capture
# --------------------------------------------------------------------------

def _capture_and_replay(call):
    eager = [t.clone() for t in call()]
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warmup allocs outside capture
            call()
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        out = call()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return eager, out


def test_gemv_splitk_under_graph_capture():
    c = fc.GEMV_SPLIT
    assert ext().fp8f16_gemv_nsplit(c["M"], c["O"], c["K"]) > 1
    x, codes, s, W, y, _ = fc.gemv_dense_case(c["M"], c["O"], c["K"])
    fn, xd = _gemv_fn(codes, s), x.to(F16).to(DEV)
    eager, out = _capture_and_replay(lambda: (fn(xd),))
    assert_same(out[0], eager[0], "gemv replay vs eager")
    assert_same(out[0], y.to(BF16), "gemv replay vs reference")


def test_gateup_acc_down_pair_under_graph_capture():
    plan_d = qc.PLAN16
    subs, live = dev_subs(plan_d)
    P, N, I = subs[3].numel(), plan_d["N"], 256
    # (a) gate-up at H = 384 feeding nothing, and the exact down case: the
    # pair shares the accumulator the way ops.grouped_expert_mlp_fp8_subs
    # uses it
    gate, up = fc.gateup_weights("a", fc.MOE_I, 384)
    gw, uw = dev8(gate[0]), dev8(up[0])
    gsd, usd = gate[1].to(DEV), up[1].to(DEV)
    x = qc.gateup_x(N, 384, 0).to(F16).to(DEV)
    hwant = qc.gateup_expected("a", gate[2], up[2], plan_d, 384, 0, F16).to(F16)
    codes, s, W, h, want, _ = fc.down_case(I, plan_d)
    dw, dsd = dev8(codes), s.to(DEV)
    hd = h.to(F16).to(DEV)

    def call():
        hh, acc = ext().moe_fp8f16_gateup_acc(x, gw, uw, gsd, usd, *subs[:4],
                                              P, N, fc.DOWN_H)
        return hh, ext().moe_fp8f16_down(hd, dw, dsd, *subs, N, acc)

    eager, out = _capture_and_replay(call)
    assert_same(out[0][live], eager[0][live], "gate-up replay vs eager")
    assert_same(out[0][live], hwant[live], "gate-up replay vs reference")
    assert_same(out[1], eager[1], "down replay vs eager")
    assert_same(out[1], want.to(F32), "down replay vs reference")


# --------------------------------------------------------------------------
# binding limits and dispatch
# --------------------------------------------------------------------------

def test_binding_limits():
    e = ext()
    codes, s, _ = fc.exact_weight(64, 256)
    w, sd = dev8(codes), s.to(DEV)
    x = torch.zeros(4, 256, dtype=F16, device=DEV)
    e.fp8f16_gemv(x, w, sd)
    with pytest.raises(RuntimeError, match="K % 128"):
        e.fp8f16_gemv(x[:, :192].contiguous(), w[:, :192].contiguous(),
                      sd.contiguous())
    with pytest.raises(RuntimeError, match="weight_scale_inv"):
        e.fp8f16_gemv(x, w, sd.t().contiguous())            # wrong shape
    with pytest.raises(RuntimeError, match="fp32"):
        e.fp8f16_gemv(x, w, sd.to(BF16))                    # wrong dtype
    with pytest.raises(RuntimeError, match="M <= 64"):
        e.fp8f16_gemv(torch.zeros(65, 256, dtype=F16, device=DEV), w, sd)
    with pytest.raises(RuntimeError, match="float8"):
        e.fp8f16_gemv(x, w.view(torch.uint8), sd)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.fp8f16_gemv(x, w.t(), sd)
    subs, _ = dev_subs(qc.PLAN16)
    P = subs[3].numel()
    c3, s3, _ = fc.exact_weight(40, 192, fc.E)
    xm = torch.zeros(qc.PLAN16["N"], 192, dtype=F16, device=DEV)
    with pytest.raises(RuntimeError, match="K % 128"):
        e.moe_fp8f16_gateup(xm, dev8(c3), dev8(c3), s3.to(DEV), s3.to(DEV),
                            *subs[:4], P)
    with pytest.raises(RuntimeError, match="K % 128"):
        e.moe_fp8f16_down(torch.zeros(P, 192, dtype=F16, device=DEV), dev8(c3),
                          s3.to(DEV), *subs, qc.PLAN16["N"])


def test_ops_dispatch_policy(monkeypatch):
    """Resident bf16 copy under the dq-cache budget; with none, the GEMV
    kernel for M <= 64 and dequant per call above it or off the kernel's
    shape limits."""
    calls = []
    real = ext()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not callable(fn):
                return fn

            def wrapped(*a, **k):
                calls.append(name)
                return fn(*a, **k)
            return wrapped

    monkeypatch.setattr(ops, "_EXT", Spy())
    w8, s, W = fc.random_weight(200, 256)
    want = None
    for M in (8, 80):
        x = (torch.randn(M, 256, generator=torch.Generator().manual_seed(M))
             .to(BF16))
        want = (x.double() @ W.t())
        tol = 2e-2 * float(want.abs().max())
        monkeypatch.setenv("MLXS_AMD_NO_DQ_CACHE", "1")
        wd = w8.to(DEV)
        calls.clear()
        y = ops.fp8_block_linear(x.to(DEV), wd, s.to(DEV))
        assert y.dtype == BF16 and not hasattr(wd, "_mlxs_dqw")
        assert ("fp8f16_gemv" in calls) == (M <= 64)
        assert ("fp8_block_dequant" in calls) == (M > 64)
        assert float((y.cpu().double() - want).abs().max()) <= tol
        monkeypatch.delenv("MLXS_AMD_NO_DQ_CACHE")
        calls.clear()
        for _ in range(2):
            y = ops.fp8_block_linear(x.to(DEV), wd, s.to(DEV))
        assert calls.count("fp8_block_dequant") == 1 and \
            "fp8f16_gemv" not in calls
        assert float((y.cpu().double() - want).abs().max()) <= tol
    # K % 128 != 0 never reaches the GEMV kernel
    monkeypatch.setenv("MLXS_AMD_NO_DQ_CACHE", "1")
    w8, s, W = fc.random_weight(72, 192)
    x = torch.randn(4, 192, generator=torch.Generator().manual_seed(1)).to(BF16)
    calls.clear()
    y = ops.fp8_block_linear(x.to(DEV), w8.to(DEV), s.to(DEV))
    assert "fp8f16_gemv" not in calls and "fp8_block_dequant" in calls
    want = x.double() @ W.t()
    assert float((y.cpu().double() - want).abs().max()) <= \
        2e-2 * float(want.abs().max())
