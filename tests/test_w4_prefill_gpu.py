"""The wide-tile w4/w8 MoE prefill kernels (w4_prefill.hip) on the plans of
fp8_prefill_cases.py and the exact data of quant_cases.py: bit-equal to the
fp64 reference and to the 16-token kernels, which do not walk a sub-range
longer than 16 tokens and so get the plan re-cut to 16."""

import functools

import pytest
import torch

import fp8_prefill_cases as pc
import quant_cases as qc
from mlx_sharding_amd import ops
from test_quant_kernels_exact import (DEV, F16, F32, assert_same, dev_subs,
                                      ext, repacked)

pytestmark = pytest.mark.gpu

O, H_GU = 72, 384
CASES = [(b, g, p) for b, g in qc.BITS_GS for p in pc.PLAN_NAMES]


def plan_of(name):
    return pc.plans(ext().moe_w4f16_wide_tile())[name]


def cut16(plan_d):
    """The same sorted rows as sub-ranges of at most 16 tokens."""
    plan = []
    for e, toks in plan_d["plan"]:
        cut = e != "gap" and len(toks) > 16
        plan += [(e, toks[i:i + 16]) for i in range(0, len(toks), 16)] \
            if cut else [(e, toks)]
    return dict(N=plan_d["N"], plan=plan)


def dev3(q, sc, bi, bits):  # on the device, the unused expert's scales NaN
    return repacked(q, bits), qc.poison_expert(sc).to(DEV), bi.to(DEV)


@pytest.mark.parametrize("K", (128, 384))
@pytest.mark.parametrize("bits,gs,plan", CASES)
def test_down_wide_exact(bits, gs, plan, K):
    plan_d = plan_of(plan)
    subs, live = dev_subs(plan_d)
    N = plan_d["N"]
    q, sc, bi, W64 = qc.exact_expert_weights(qc.N_EXPERTS, O, K, gs, bits)
    h = qc.down_h(plan_d, K)
    want = qc.down_expected(W64, h, plan_d).to(F32)
    hp = qc.poison_rows(h, (~live).nonzero().flatten().tolist()).to(F16).to(DEV)
    w = dev3(q, sc, bi, bits)
    got = ext().moe_w4f16_down_wide(hp, *w, *subs, N, gs, bits)
    assert_same(got, want, "moe_w4f16_down_wide K=%d" % K)
    assert not got[qc.dead_tokens(plan_d)].any()
    old = ext().moe_w4f16_down(hp, *w, *dev_subs(cut16(plan_d))[0], N, gs, bits)
    assert_same(got, old, "wide vs 16-token down")


@functools.lru_cache(maxsize=None)
def gateup_mats(kind, gs, bits):
    gate, up = qc.gateup_expert_weights(kind, qc.N_EXPERTS, O, H_GU, gs, bits)
    return (dev3(*gate[:3], bits), dev3(*up[:3], bits)), gate[3], up[3]


@pytest.mark.parametrize("kind", ("a", "b"))
@pytest.mark.parametrize("bits,gs,plan", CASES)
def test_gateup_wide_exact(bits, gs, plan, kind):
    plan_d = plan_of(plan)
    subs, live = dev_subs(plan_d)
    subs16 = dev_subs(cut16(plan_d))[0]
    P = subs[3].numel()
    ((gq, gsc, gbi), (uq, usc, ubi)), Wg, Wu = gateup_mats(kind, gs, bits)
    offs = qc.gateup_offsets(plan_d, H_GU)
    X = pc.gateup_x_sweep(plan_d, H_GU, offs,
                          qc.dead_tokens(plan_d)).to(F16).to(DEV)
    want = pc.gateup_expected_sweep(kind, Wg, Wu, plan_d, H_GU, offs,
                                    F16).to(F16)
    got = torch.stack([ext().moe_w4f16_gateup_wide(
        X[i], gq, uq, gsc, gbi, usc, ubi, *subs[:4], P, gs, bits)
        for i in range(len(offs))])
    assert_same(got[:, live], want[:, live], "moe_w4f16_gateup_wide " + kind)
    old = torch.stack([ext().moe_w4f16_gateup(X[i], gq, uq, gsc, gbi, usc, ubi,
                                              *subs16[:4], P, gs, bits)
                       for i in range(0, len(offs), 8)])
    assert_same(got[::8][:, live], old[:, live], "wide vs 16-token gate-up")


@pytest.mark.parametrize("gs", (32, 64, 128))
def test_random_layer_within_bound(gs):
    """quant_cases section 4 (gemv_bound, gateup_bound) per sub-range."""
    plan_d = plan_of("wide_a")
    subs, live = dev_subs(plan_d)
    P, N, K = subs[3].numel(), plan_d["N"], qc.BUDGET_K
    mats = qc.budget_moe_case(gs)[0]
    g = torch.Generator().manual_seed(23)
    x, hh = (torch.randn(r, K, generator=g).to(F16) for r in (N, P))
    wt = subs[4].cpu().double()
    dref, dA = (torch.zeros(N, O, dtype=torch.float64) for _ in range(2))
    gref, gbound = (torch.ones(P, O, dtype=torch.float64) for _ in range(2))
    for e, rows, toks in pc.subrange_rows(plan_d["plan"]):
        gt, ut, dt = ((mats[n][3][e], mats[n][1][e], mats[n][2][e])
                      for n in ("gate", "up", "down"))     # (q, sc, bi)
        hp, w, ti = hh[rows].double(), wt[rows][:, None], torch.tensor(toks)
        dref.index_add_(0, ti, w * (hp @ qc.budget_w64(*dt, gs).t()))
        dA.index_add_(0, ti, w * qc.budget_mass(hp, *dt, gs))
        xt = x[toks].double()
        g64 = xt @ qc.budget_w64(*gt, gs).t()
        u64 = xt @ qc.budget_w64(*ut, gs).t()
        gref[rows] = g64 / (1.0 + torch.exp(-g64)) * u64
        gbound[rows] = qc.gateup_bound(g64, u64, qc.budget_mass(xt, *gt, gs),
                                       qc.budget_mass(xt, *ut, gs))
    dbound = qc.gemv_bound(dref, dA, 0.0)
    dv = {n: (ops.repack_w4(mats[n][0], 4).to(DEV), mats[n][1].to(DEV),
              mats[n][2].to(DEV)) for n in mats}
    ggot = ext().moe_w4f16_gateup_wide(
        x.to(DEV), dv["gate"][0], dv["up"][0], *dv["gate"][1:], *dv["up"][1:],
        *subs[:4], P, gs, 4).cpu().double()
    dgot = ext().moe_w4f16_down_wide(hh.to(DEV), *dv["down"], *subs, N, gs,
                                     4).cpu().double()
    rd = float(((dgot - dref).abs() / dbound.clamp_min(1e-30)).max())
    rg = float(((ggot - gref).abs() / gbound)[live].max())
    print("gs%d worst |error| / bound: down %.3f gateup %.3f" % (gs, rd, rg))
    assert rd <= 1 and rg <= 1


def test_binding_limits():
    plan_d = plan_of("wide_a")
    subs, _ = dev_subs(plan_d)
    P, N = subs[3].numel(), plan_d["N"]

    def args(K, wide=1):
        w = qc.exact_expert_weights(qc.N_EXPERTS, 40, K * wide, 64, 4)[:3]
        return (torch.zeros(N, K, dtype=F16, device=DEV),
                torch.zeros(P, K, dtype=F16, device=DEV), dev3(*w, 4))

    def both(match, x, hh, w, gs=64, bits=4, P_=P):
        e = ext()
        with pytest.raises(RuntimeError, match="gateup_wide.*" + match):
            e.moe_w4f16_gateup_wide(x, w[0], w[0], w[1], w[2], w[1], w[2],
                                    *subs[:4], P_, gs, bits)
        with pytest.raises(RuntimeError, match="down_wide.*" + match):
            e.moe_w4f16_down_wide(hh[:P_], *w, *subs, N, gs, bits)

    x, hh, w = args(256)
    both("K % 128", *args(192))
    both("gs must be", x, hh, w, gs=16)
    both("bits must be", x, hh, w, bits=3)
    both("contiguous", x, hh, (args(256, 2)[2][0][..., ::2], w[1], w[2]))
    both("P must be", x, hh, w, P_=P - 1)


def test_graph_capture_replays_match_eager():
    """The accumulator is zeroed inside the captured work."""
    plan_d = plan_of("wide_b")
    subs, _ = dev_subs(plan_d)
    P, N, K = subs[3].numel(), plan_d["N"], 128
    mats = [dev3(*qc.exact_expert_weights(qc.N_EXPERTS, K, K, 64, 4, s)[:3], 4)
            for s in range(3)]
    # |x| <= 1/8 keeps silu(g) * u far inside fp16
    x = (qc.dense_int_x(N, K) / 16).to(F16).to(DEV)

    def layer():
        h = ext().moe_w4f16_gateup_wide(
            x, mats[0][0], mats[1][0], *mats[0][1:], *mats[1][1:], *subs[:4],
            P, 64, 4)
        return ext().moe_w4f16_down_wide(h, *mats[2], *subs, N, 64, 4)

    eager = layer().clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = layer()
    for _ in range(2):
        graph.replay()
        assert_same(out, eager, "graph replay vs eager")
    assert eager.isfinite().all() and eager.any()
