"""CPU sanity for the exact-arithmetic quantized-kernel cases.

A torch emulation of each kernel family's declared arithmetic (one fp16
rounding of s*(q-off) + (b + off*s), or one bf16 rounding of s*q + b, then
fp32 accumulation in a scrambled order over four partial chains) must equal
the fp64 reference exactly on the cases test_quant_kernels_exact.py runs:
that is the proof that an inequality on the GPU is the kernel's fault.  The
same emulation with a deliberate defect must break equality.
"""

import pytest
import torch

import quant_cases as qc
from mlx_sharding_amd import ops

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


# --------------------------------------------------------------------------
# emulation of the kernels' arithmetic
# --------------------------------------------------------------------------

def deq_f16(q, sc, bi, gs, bits, bias_shift=0.0):
    """fp16-dequant kernels (w4f16_dequant.h): the bias constant b + off*s
    is formed in fp32 and rounded to fp16, then ONE fp16 rounding of the
    fma.  bias_shift = 0.5 is the rejected folded-recentre design."""
    off = 8.0 if bits == 4 else 128.0
    s = sc.float()
    bc = (bi.float() + bias_shift * s + off * s).half()
    v = (s.half().double().repeat_interleave(gs, -1) * (q.double() - off)
         + bc.double().repeat_interleave(gs, -1))
    return v.half()


def deq_bf16(q, sc, bi, gs, bits, bias_shift=0.0):
    """bf16-dequant kernels (w4a16_mfma, moe_w4_mfma, dequant): fp32
    s*q + b, one bf16 rounding."""
    s = sc.float()
    b = bi.float() + bias_shift * s
    return (s.repeat_interleave(gs, -1) * q.float()
            + b.repeat_interleave(gs, -1)).bfloat16()


def acc_fp32(terms, seed=0, chunk=8, chains=4):
    """fp32 sum of terms[..., K] in a scrambled order: chunks of 8 dealt
    round-robin to four chains, the chains summed at the end."""
    K = terms.shape[-1]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    t = terms.float()[..., perm]
    acc = [torch.zeros(t.shape[:-1]) for _ in range(chains)]
    for i, c in enumerate(t.split(chunk, dim=-1)):
        acc[i % chains] = acc[i % chains] + c.sum(-1, dtype=F32)
    return (acc[0] + acc[2]) + (acc[1] + acc[3])


def emu_linear(x, wd, seed=0):
    """x [M, K] (any float dtype) times dequantized wd [O, K]: fp32
    products, fp32 accumulation.  Returns fp32 [M, O]."""
    return acc_fp32(x.float()[:, None, :] * wd.float()[None], seed)


def emu_scalar_gemv(x, q, sc, bi, gs, bits, seed=0, bias_shift=0.0):
    """w4a16 scalar path: per packed word, s*sum(q x) + b*sum(x) in fp32."""
    pw = 32 // bits
    M, K = x.shape
    xf = x.float()
    inner = (q.float()[None] * xf[:, None, :]).reshape(M, -1, K // pw, pw).sum(-1)
    xsum = xf.reshape(M, 1, K // pw, pw).sum(-1)
    s = sc.float().repeat_interleave(gs // pw, 1)
    b = (bi.float() + bias_shift * sc.float()).repeat_interleave(gs // pw, 1)
    return acc_fp32(s[None] * inner + b[None] * xsum, seed)


def silu32(g):
    return g / (1.0 + torch.exp(-g))


def emu_gateup(x, gate, up, subs, deq, gs, bits, out_dtype, **kw):
    """gate/up: (q, sc, bi) stacked over experts.  Returns [P, I]."""
    sub_e, sub_off, sub_cnt, stok, _ = subs
    h = torch.zeros(stok.numel(), gate[0].shape[1], dtype=out_dtype)
    for e, p0, cnt in zip(sub_e.tolist(), sub_off.tolist(), sub_cnt.tolist()):
        if cnt == 0:
            continue
        xs = x[stok[p0:p0 + cnt].long()]
        g = emu_linear(xs, deq(gate[0][e], gate[1][e], gate[2][e], gs, bits, **kw), 1)
        u = emu_linear(xs, deq(up[0][e], up[1][e], up[2][e], gs, bits, **kw), 2)
        h[p0:p0 + cnt] = (silu32(g) * u).to(out_dtype)
    return h


def emu_down(h, down, subs, N, deq, gs, bits, **kw):
    sub_e, sub_off, sub_cnt, stok, swt = subs
    out = torch.zeros(N, down[0].shape[1], dtype=F32)
    for e, p0, cnt in zip(sub_e.tolist(), sub_off.tolist(), sub_cnt.tolist()):
        if cnt == 0:
            continue
        acc = emu_linear(h[p0:p0 + cnt],
                         deq(down[0][e], down[1][e], down[2][e], gs, bits, **kw), 3)
        out.index_add_(0, stok[p0:p0 + cnt].long(), swt[p0:p0 + cnt, None] * acc)
    return out


def identity_sweep(wd):
    """All one-hot offsets at once: x = I, so y[k, o] = sum_k' I[k,k'] w[o,k']."""
    K = wd.shape[1]
    eye = torch.eye(K, dtype=F32)
    return torch.cat([emu_linear(eye[r:r + 64], wd, r) for r in range(0, K, 64)])


# --------------------------------------------------------------------------
# packing
# --------------------------------------------------------------------------

@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_pack_roundtrip(bits, gs):
    q, sc, bi, W64 = qc.exact_weights(20, 384, gs, bits)
    wq = qc.pack(q, bits)
    assert wq.dtype == ops.reference.quantize(torch.zeros(1, 32), 32, 4)[0].dtype
    assert wq.shape == (20, 384 * bits // 32)
    assert torch.equal(qc.unpack_natural(wq, bits), q)
    deq = ops.reference.dequantize(wq, sc, bi, gs, bits)
    assert deq.dtype == BF16 and torch.equal(deq.double(), W64)


@pytest.mark.parametrize("bits", (4, 8))
def test_repack_w4_layout(bits):
    """ops.repack_w4 output, read the way the fp16 kernels read it, is q in
    natural k order (2-D and stacked 3-D)."""
    q, _, _, _ = qc.exact_weights(20, 384, 64, bits)
    rp = ops.repack_w4(qc.pack(q, bits), bits)
    assert torch.equal(qc.unpack_repacked(rp, bits), q)
    q3 = qc.exact_expert_weights(3, 8, 64, 32, bits)[0]
    rp3 = ops.repack_w4(qc.pack(q3, bits), bits)
    assert rp3.shape == (3, 8, 64 * bits // 32)
    assert torch.equal(qc.unpack_repacked(rp3, bits), q3)


def test_subrange_builder():
    for plan_d, max_tok in ((qc.PLAN4, 4), (qc.PLAN16, 16), (qc.PLAN32, 32)):
        (se, so, sc_, st, sw), live = qc.build_subranges(plan_d["plan"])
        cnts = sc_.tolist()
        assert max(cnts) == max_tok and 1 in cnts
        assert 0 in cnts[1:-1] and cnts[-1] == 0      # pad inside and at the end
        assert qc.UNUSED_EXPERT not in se[sc_ > 0].tolist()
        toks = [t for _, _, t in qc.plan_pairs(plan_d["plan"])]
        assert len(set(toks)) < len(toks)              # a token on two experts
        assert toks != sorted(toks)
        assert len(qc.dead_tokens(plan_d)) >= 2
        assert int(live.sum()) == len(toks) < live.numel()
        assert torch.isnan(sw[~live]).all() and not torch.isnan(sw[live]).any()
        assert set(sw[live].tolist()) <= set(qc.ROUTE_WTS)
        for e, p0, c in zip(se.tolist(), so.tolist(), cnts):
            assert live[p0:p0 + c].all()


# --------------------------------------------------------------------------
# the emulation is exact on the GPU module's cases
# --------------------------------------------------------------------------

@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_emulated_dequant_exact(bits, gs):
    O, H = qc.DEQUANT_SHAPE
    q, sc, bi, W64 = qc.exact_weights(O, H, gs, bits)
    assert torch.equal(deq_bf16(q, sc, bi, gs, bits).double(), W64)
    assert torch.equal(deq_f16(q, sc, bi, gs, bits).double(), W64)


@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_emulated_scalar_gemv_exact(bits, gs):
    O, H = qc.SCALAR_GEMV["O"], qc.SCALAR_GEMV["H"]
    for M in qc.SCALAR_GEMV["Ms"]:
        x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
        got = emu_scalar_gemv(x.to(BF16), q, sc, bi, gs, bits)
        assert torch.equal(got.double(), y)            # exact in fp32
        assert torch.equal(got.to(BF16), y.to(BF16))
    eye = torch.eye(H, dtype=BF16)
    got = torch.cat([emu_scalar_gemv(eye[r:r + 64], q, sc, bi, gs, bits, r)
                     for r in range(0, H, 64)])
    assert torch.equal(got.double(), W64.t())


@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_emulated_mfma_gemv_exact(bits, gs):
    O = qc.MFMA_GEMV["O"]
    for H in qc.MFMA_GEMV["Hs"]:
        for M in qc.MFMA_GEMV["Ms"]:
            x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
            got = emu_linear(x.to(BF16), deq_bf16(q, sc, bi, gs, bits))
            assert torch.equal(got.double(), y)
        assert torch.equal(identity_sweep(deq_bf16(q, sc, bi, gs, bits)).double(),
                           W64.t())


@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_emulated_w4f16_gemv_exact(bits, gs):
    H, O = qc.W4F16_H[gs], qc.W4F16_O
    for M in qc.W4F16_MS:
        x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
        got = emu_linear(x.to(F16), deq_f16(q, sc, bi, gs, bits))
        assert torch.equal(got.double(), y)
    assert torch.equal(identity_sweep(deq_f16(q, sc, bi, gs, bits)).double(),
                       W64.t())


@pytest.mark.parametrize("bits", (4, 8))
def test_emulated_w4f16_direct_store_exact(bits):
    c = qc.W4F16_DIRECT
    x, q, sc, bi, W64, y = qc.gemv_dense_case(c["M"], c["O"], c["H"], c["gs"], bits)
    got = emu_linear(x.to(F16), deq_f16(q, sc, bi, c["gs"], bits))
    assert torch.equal(got.double(), y)


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_emulated_kseg_w4_exact(gs):
    N, K = qc.KSEG["N"], qc.KSEG["K"]
    for M in qc.KSEG["Ms"]:
        x, q, sc, bi, W64, y = qc.gemv_dense_case(M, N, K, gs, 4)
        got = emu_linear(x.to(F16), deq_f16(q, sc, bi, gs, 4))
        assert torch.equal(got.double(), y)
    assert torch.equal(identity_sweep(deq_f16(q, sc, bi, gs, 4)).double(), W64.t())


def _some_offsets(offs):
    return [offs[0], offs[len(offs) // 2], offs[-1]]


@pytest.mark.parametrize("kind", ("a", "b"))
@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_emulated_moe_w4f16_gateup_exact(bits, gs, kind):
    """Expected values are built (and their preconditions asserted) for
    every offset of the sweep; the emulation runs on three of them."""
    subs, live = qc.build_subranges(qc.PLAN16["plan"])
    for H in qc.MOE_F16_DIMS[gs]:
        gate, up = qc.gateup_expert_weights(kind, qc.N_EXPERTS, qc.MOE_OUT, H,
                                            gs, bits)
        offs = qc.gateup_offsets(qc.PLAN16, H)
        for off in offs:
            qc.gateup_expected(kind, gate[3], up[3], qc.PLAN16, H, off, F16)
        for off in _some_offsets(offs):
            want = qc.gateup_expected(kind, gate[3], up[3], qc.PLAN16, H, off, F16)
            x = qc.gateup_x(qc.PLAN16["N"], H, off).to(F16)
            got = emu_gateup(x, gate, up, subs, deq_f16, gs, bits, F16)
            assert torch.equal(got[live], want.to(F16)[live])


@pytest.mark.parametrize("bits,gs", qc.BITS_GS, ids=qc.BITS_GS_IDS)
def test_emulated_moe_w4f16_down_exact(bits, gs):
    subs, _ = qc.build_subranges(qc.PLAN16["plan"])
    for I in qc.MOE_F16_DIMS[gs]:
        down = qc.exact_expert_weights(qc.N_EXPERTS, qc.MOE_OUT, I, gs, bits)
        h = qc.down_h(qc.PLAN16, I)
        want = qc.down_expected(down[3], h, qc.PLAN16)
        got = emu_down(h.to(F16), down, subs, qc.PLAN16["N"], deq_f16, gs, bits)
        assert torch.equal(got.double(), want)
        assert not want[qc.dead_tokens(qc.PLAN16)].any()


@pytest.mark.parametrize("bits,gs,H", qc.MOE_W4_MFMA)
def test_emulated_moe_w4_mfma_exact(bits, gs, H):
    subs, live = qc.build_subranges(qc.PLAN32["plan"])
    N = qc.PLAN32["N"]
    q, sc, bi, W64 = qc.exact_expert_weights(qc.N_EXPERTS, qc.MOE_OUT, H, gs, bits)
    wd = torch.stack([deq_bf16(q[e], sc[e], bi[e], gs, bits)
                      for e in range(qc.N_EXPERTS)])
    assert torch.equal(wd.double(), W64)
    x = qc.dense_int_x(N, H)
    want = qc.moe_linear_expected(W64, x, qc.PLAN32)
    for p, e, t in qc.plan_pairs(qc.PLAN32["plan"])[::7]:
        got = emu_linear(x[t:t + 1].to(BF16), wd[e])[0]
        assert torch.equal(got.double(), want[p])
    for off in qc.one_hot_offsets(N, H):
        want = qc.moe_linear_expected(W64, qc.one_hot_x(N, H, off), qc.PLAN32)
        assert torch.equal(want.to(BF16).double(), want)


@pytest.mark.parametrize("max_tok", (4, 16))
def test_emulated_bf16_moe_exact(max_tok):
    plan_d = qc.BF16_PLANS[max_tok]
    subs, live = qc.build_subranges(plan_d["plan"])
    H, I, E, N = qc.BF16_MOE["H"], qc.BF16_MOE["I"], qc.N_EXPERTS, plan_d["N"]
    for kind in ("a", "b"):
        Wg, Wu = qc.gateup_dense_weights(kind, E, I, H)
        offs = qc.gateup_offsets(plan_d, H)
        for off in offs:
            qc.gateup_expected(kind, Wg, Wu, plan_d, H, off, BF16)
        off = offs[len(offs) // 2]
        want = qc.gateup_expected(kind, Wg, Wu, plan_d, H, off, BF16)
        x = qc.gateup_x(N, H, off)
        for p, e, t in qc.plan_pairs(plan_d["plan"]):
            g = emu_linear(x[t:t + 1], Wg[e], 1)
            u = emu_linear(x[t:t + 1], Wu[e], 2)
            assert torch.equal((silu32(g) * u).to(BF16)[0], want[p].to(BF16))
    for inner, outer in ((I, H), (H, I)):
        Wd = torch.randint(-7, 8, (E, outer, inner),
                           generator=torch.Generator().manual_seed(3)).double()
        h = qc.down_h(plan_d, inner)
        want = qc.down_expected(Wd, h, plan_d)
        got = torch.zeros(N, outer)
        for p, e, t in qc.plan_pairs(plan_d["plan"]):
            got[t] += subs[4][p] * emu_linear(h[p:p + 1], Wd[e], p)[0]
        assert torch.equal(got.double(), want)


def test_bit_budget():
    """Worst-case and seen totals in LSBs; the module docstring's table."""
    rows = []
    for bits in (4, 8):
        K = max(qc.MFMA_GEMV["Hs"])
        bound = K * 2.0 * ((1 << bits) - 1) * 2 / 0.25
        x, q, sc, bi, W64, y = qc.gemv_dense_case(33, qc.MFMA_GEMV["O"], K, 64, bits)
        seen = float((x.abs() @ W64.abs().t()).max()) / 0.25
        rows.append(("w%d dequantized" % bits, K, bound, seen))
    K = qc.SCALAR_GEMV["H"]
    x, q, sc, bi, W64, y = qc.gemv_dense_case(7, qc.SCALAR_GEMV["O"], K, 64, 8)
    mass = x.abs() @ (q.double() * sc.double().repeat_interleave(64, 1)
                      + bi.double().abs().repeat_interleave(64, 1)).t()
    rows.append(("scalar w8", K, K * 2 * (2.0 * 255 * 2) / 0.25,
                 float(mass.max()) / 0.25))
    I = 384
    down = qc.exact_expert_weights(qc.N_EXPERTS, qc.MOE_OUT, I, 128, 8)
    h = qc.down_h(qc.PLAN16, I)
    seen = 0.0
    subs, _ = qc.build_subranges(qc.PLAN16["plan"])
    mass = torch.zeros(qc.PLAN16["N"], qc.MOE_OUT, dtype=torch.float64)
    for p, e, t in qc.plan_pairs(qc.PLAN16["plan"]):
        mass[t] += subs[4][p].double() * (down[3][e].abs() @ h[p].abs())
    rows.append(("moe down w8", I, 2 * I * (2.0 * 255 * 2) * 16,
                 float(mass.max()) * 16))
    for name, K, bound, seen in rows:
        print("%-16s K=%4d bound 2^%.1f seen 2^%.1f"
              % (name, K, qc.log2_or_zero(bound), qc.log2_or_zero(seen)))
        assert seen <= bound < qc.F24


# --------------------------------------------------------------------------
# defects break equality
# --------------------------------------------------------------------------

def _bump(q, bits):
    q = q.clone()
    q[3, 41] = (q[3, 41] + 1) % (1 << bits)
    return q


def _swap_adjacent(q):
    q = q.clone()
    k = int((q[5, :-1] != q[5, 1:]).nonzero()[2])
    q[5, [k, k + 1]] = q[5, [k + 1, k]]
    return q


def _neighbour_group(t):
    t = t.clone()
    t[7, 1] = t[7, 2]
    return t


@pytest.mark.parametrize("arith", ("f16", "bf16", "scalar"))
@pytest.mark.parametrize("bits", (4, 8))
def test_defects_break_gemv_equality(arith, bits):
    gs, O, H, M = 64, 20, 384, 7
    x, q, sc, bi, W64, y = qc.gemv_dense_case(M, O, H, gs, bits)
    xdt = F16 if arith == "f16" else BF16
    deq = deq_f16 if arith == "f16" else deq_bf16

    def run(q_, sc_, bi_, xx, **kw):
        if arith == "scalar":
            return emu_scalar_gemv(xx.to(xdt), q_, sc_, bi_, gs, bits, **kw)
        return emu_linear(xx.to(xdt), deq(q_, sc_, bi_, gs, bits, **kw))

    eye = torch.eye(H, dtype=torch.float64)
    assert torch.equal(run(q, sc, bi, x).double(), y)
    assert torch.equal(run(q, sc, bi, eye).double(), W64.t())
    defects = {
        "bump": (_bump(q, bits), sc, bi, {}),
        "group": (q, _neighbour_group(sc), _neighbour_group(bi), {}),
        "swap-k": (_swap_adjacent(q), sc, bi, {}),
        "half-step": (q, sc, bi, {"bias_shift": 0.5}),
    }
    for name, (q_, sc_, bi_, kw) in defects.items():
        # the one-hot sweep sees every defect; the dense case in fp32 too
        assert not torch.equal(run(q_, sc_, bi_, eye, **kw).double(), W64.t()), name
        assert not torch.equal(run(q_, sc_, bi_, x, **kw).double(), y), name


@pytest.mark.parametrize("bits", (4, 8))
def test_defects_break_moe_equality(bits):
    gs, H = 64, 320
    plan_d = qc.PLAN16
    subs, live = qc.build_subranges(plan_d["plan"])
    N = plan_d["N"]
    down = qc.exact_expert_weights(qc.N_EXPERTS, qc.MOE_OUT, H, gs, bits)
    h = qc.down_h(plan_d, H)
    want_d = qc.down_expected(down[3], h, plan_d)
    gate, up = qc.gateup_expert_weights("b", qc.N_EXPERTS, qc.MOE_OUT, H, gs, bits)
    want_g = qc.gateup_expected("b", gate[3], up[3], plan_d, H, 8, F16).to(F16)
    x = qc.gateup_x(N, H, 8).to(F16)

    def run_down(dn=down, sb=subs, **kw):
        return emu_down(h.to(F16), dn, sb, N, deq_f16, gs, bits, **kw).double()

    def run_gu(gt=gate, sb=subs, **kw):
        return emu_gateup(x, gt, up, sb, deq_f16, gs, bits, F16, **kw)[live]

    assert torch.equal(run_down(), want_d)
    assert torch.equal(run_gu(), want_g[live])

    def swapped(i, a=0, b=1):
        t = subs[i].clone()
        t[[a, b]] = t[[b, a]]
        return subs[:i] + (t,) + subs[i + 1:]

    assert not torch.equal(run_down(sb=swapped(3)), want_d), "tokens swapped"
    assert not torch.equal(run_gu(sb=swapped(3)), want_g[live]), "tokens swapped"
    assert not torch.equal(run_down(sb=swapped(4)), want_d), "weights swapped"
    assert not torch.equal(run_down(bias_shift=0.5), want_d), "half step"
    assert not torch.equal(run_gu(bias_shift=0.5), want_g[live]), "half step"
    bumped = (torch.stack([_bump(q, bits) for q in down[0]]),) + down[1:]
    assert not torch.equal(run_down(dn=bumped), want_d), "bump"
    grp = (gate[0], torch.stack([_neighbour_group(t) for t in gate[1]]),
           torch.stack([_neighbour_group(t) for t in gate[2]]))
    # the sweep reads every column; group 1 of row 7 is hit at some offset
    hit = False
    for off in qc.gateup_offsets(plan_d, H):
        cols = set(qc.gateup_cols(N, H, off).tolist())
        if cols & set(range(gs, 2 * gs)):
            w = qc.gateup_expected("b", gate[3], up[3], plan_d, H, off, F16).to(F16)
            xo = qc.gateup_x(N, H, off).to(F16)
            g = emu_gateup(xo, grp, up, subs, deq_f16, gs, bits, F16)
            hit = hit or not torch.equal(g[live], w[live])
            if hit:
                break
    assert hit, "neighbouring group"


# --------------------------------------------------------------------------
# section 4: the arithmetic budget separates the two designs
# --------------------------------------------------------------------------

def _ratio_and_share(err, bound):
    return float((err / bound).max()), float((err > bound).double().mean())


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_budget_gemv(gs):
    wq, sc, bi, q, x, ref64, A = qc.budget_gemv_case(gs)
    bound = qc.gemv_bound(ref64, A, 2.0 ** -9)
    good = emu_linear(x, deq_f16(q, sc, bi, gs, 4)).to(BF16).double()
    bad = emu_linear(x, deq_f16(q, sc, bi, gs, 4, bias_shift=0.5)).to(BF16).double()
    r, _ = _ratio_and_share((good - ref64).abs(), bound)
    _, share = _ratio_and_share((bad - ref64).abs(), bound)
    print("w4f16_gemv gs%d: worst ratio %.2f, half-step share %.0f%%"
          % (gs, r, 100 * share))
    assert r <= 1.0 and share > 0.5


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_budget_moe_down(gs):
    mats, x, hh = qc.budget_moe_case(gs)
    subs, _ = qc.build_subranges(qc.PLAN16["plan"])
    ref64, bound = qc.budget_down_ref(mats, hh, gs)
    used = bound > 0
    dn = (mats["down"][3], mats["down"][1], mats["down"][2])
    good = emu_down(hh, dn, subs, qc.PLAN16["N"], deq_f16, gs, 4).double()
    bad = emu_down(hh, dn, subs, qc.PLAN16["N"], deq_f16, gs, 4,
                   bias_shift=0.5).double()
    assert not good[~used].any()
    r, _ = _ratio_and_share((good - ref64).abs()[used], bound[used])
    _, share = _ratio_and_share((bad - ref64).abs()[used], bound[used])
    print("moe_w4f16_down gs%d: worst ratio %.2f, half-step share %.0f%%"
          % (gs, r, 100 * share))
    assert r <= 1.0 and share > 0.5


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_budget_moe_gateup(gs):
    mats, x, hh = qc.budget_moe_case(gs)
    subs, live = qc.build_subranges(qc.PLAN16["plan"])
    ref64, bound = qc.budget_gateup_ref(mats, x, gs)
    gt = (mats["gate"][3], mats["gate"][1], mats["gate"][2])
    up = (mats["up"][3], mats["up"][1], mats["up"][2])
    good = emu_gateup(x, gt, up, subs, deq_f16, gs, 4, F16).double()
    bad = emu_gateup(x, gt, up, subs, deq_f16, gs, 4, F16, bias_shift=0.5).double()
    r, _ = _ratio_and_share((good - ref64).abs()[live], bound[live])
    _, share = _ratio_and_share((bad - ref64).abs()[live], bound[live])
    print("moe_w4f16_gateup gs%d: worst ratio %.2f, half-step share %.0f%%"
          % (gs, r, 100 * share))
    assert r <= 1.0 and share > 0.5
