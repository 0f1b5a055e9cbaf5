"""The wide-tile FP8 MoE prefill kernels (fp8_prefill.hip) on the GPU, on the
plans of fp8_prefill_cases.py built for the kernels' own tile: every result
on the exact cases must equal the fp64 reference bit for bit
(test_fp8_prefill_cpu.py proves that on an emulation of the declared
arithmetic), and must equal what the 16-token kernels give on the same
sub-range arrays.  The random-data test checks the accumulation bounds of
fp8_cases.py and prints the worst |error| / bound beside the 16-token
kernels' ratio.

Measured on an MI355X (seed 0, K = 384, TM = 64), worst |error| / bound,
wide (16-token): down 0.001 (0.001), gate-up 0.422 (0.422).
"""

import functools

import pytest
import torch

import fp8_cases as fc
import fp8_prefill_cases as pc
import quant_cases as qc
from mlx_sharding_amd import ops

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
DEV = "cuda"
SENTINEL = 1234.0


def ext():
    e = ops.hip_ext()
    assert e is not None, "HIP extension not built"
    return e


def tile() -> int:
    TM = ext().moe_fp8f16_wide_tile()
    assert TM >= 64 and TM % 16 == 0
    return TM


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


@functools.lru_cache(maxsize=None)
def gateup_mats(kind, H):
    """Device weights with the unused expert poisoned, and the fp64 pair."""
    gate, up = fc.gateup_weights(kind, fc.MOE_I, H)
    gc8, gs = fc.poison_unused(gate[0], gate[1])
    uc8, us = fc.poison_unused(up[0], up[1])
    return (dev8(gc8), dev8(uc8), gs.to(DEV), us.to(DEV)), gate[2], up[2]


@functools.lru_cache(maxsize=None)
def down_mats(I, plan):
    plan_d = pc.plans(tile())[plan]
    codes, s, W, h, want, _ = fc.down_case(I, plan_d)
    c8, s8 = fc.poison_unused(codes, s)
    _, live = qc.build_subranges(plan_d["plan"])
    hp = qc.poison_rows(h, (~live).nonzero().flatten().tolist())
    return dev8(c8), s8.to(DEV), hp.to(F16).to(DEV), want.to(F32)


# --------------------------------------------------------------------------
# gate-up
# --------------------------------------------------------------------------

@pytest.mark.parametrize("plan", pc.PLAN_NAMES)
@pytest.mark.parametrize("H", fc.MOE_HS)
@pytest.mark.parametrize("kind", ("a", "b"))
def test_gateup_wide_exact(kind, H, plan):
    plan_d = pc.plans(tile())[plan]
    subs, live = dev_subs(plan_d)
    P = subs[3].numel()
    (gw, uw, gsd, usd), Wg, Wu = gateup_mats(kind, H)
    dead = qc.dead_tokens(plan_d)
    offs = qc.gateup_offsets(plan_d, H)
    X = pc.gateup_x_sweep(plan_d, H, offs, dead).to(F16).to(DEV)
    want = pc.gateup_expected_sweep(kind, Wg, Wu, plan_d, H, offs,
                                    F16).to(F16)
    got = torch.stack([ext().moe_fp8f16_gateup_wide(X[i], gw, uw, gsd, usd,
                                                    *subs[:4], P)
                       for i in range(len(offs))])
    # dead tokens' NaN rows and the poisoned expert leave no trace
    assert not got[:, live].isnan().any()
    assert_same(got[:, live], want[:, live],
                "moe_fp8f16_gateup_wide (%s) H=%d %s" % (kind, H, plan))
    # the 16-token kernel walks the same sub-range arrays
    old = torch.stack([ext().moe_fp8f16_gateup(X[i], gw, uw, gsd, usd,
                                               *subs[:4], P)
                       for i in range(0, len(offs), 8)])
    assert_same(got[::8][:, live], old[:, live], "wide vs 16-token gate-up")
    # rows outside every sub-range stay untouched.  The binding allocates
    # h itself, so pre-fill the block it will get: the caching allocator
    # hands a freed block of the same size straight back.
    del got, old
    h = torch.full((P, fc.MOE_I), SENTINEL, dtype=F16, device=DEV)
    ptr = h.data_ptr()
    del h
    h2 = ext().moe_fp8f16_gateup_wide(X[0], gw, uw, gsd, usd, *subs[:4], P)
    assert h2.data_ptr() == ptr, "allocator did not recycle the sentinel block"
    assert int((~live).sum()) == 3 and torch.all(h2.cpu()[~live] == SENTINEL)
    assert_same(h2[live], want[0][live], "gate-up rerun")


# --------------------------------------------------------------------------
# down
# --------------------------------------------------------------------------

@pytest.mark.parametrize("plan", pc.PLAN_NAMES)
@pytest.mark.parametrize("I", fc.DOWN_IS)
def test_down_wide_exact(I, plan):
    plan_d = pc.plans(tile())[plan]
    subs, _ = dev_subs(plan_d)
    N = plan_d["N"]
    dw, dsd, hp, want = down_mats(I, plan)
    # a NaN block recycled by the allocator: the binding zero-fills out
    junk = torch.full((N, fc.DOWN_H), float("nan"), device=DEV, dtype=F32)
    del junk
    got = ext().moe_fp8f16_down_wide(hp, dw, dsd, *subs, N)
    assert_same(got, want, "moe_fp8f16_down_wide I=%d %s" % (I, plan))
    dead = qc.dead_tokens(plan_d)
    assert {N - 2, N - 1} <= set(dead) and not got[dead].any()
    old = ext().moe_fp8f16_down(hp, dw, dsd, *subs, N)
    assert_same(got, old, "wide vs 16-token down")


# --------------------------------------------------------------------------
# random data: the accumulation bounds, and the 16-token kernels beside
# --------------------------------------------------------------------------

def test_random_layer_within_bound():
    plan_d = pc.plans(tile())["wide_a"]
    mats, xm, hh = pc.random_case(plan_d)
    subs, live = dev_subs(plan_d)
    P, N = subs[3].numel(), plan_d["N"]
    g, u, d = (tuple(t.to(DEV) for t in mats[n][:2])
               for n in ("gate", "up", "down"))
    dref, dbound = pc.random_down_ref(mats, hh, plan_d)
    gref, gbound = pc.random_gateup_ref(mats, xm, plan_d)
    e = ext()
    xd, hd = xm.to(DEV), hh.to(DEV)
    ggot = e.moe_fp8f16_gateup_wide(xd, g[0], u[0], g[1], u[1], *subs[:4], P)
    gold = e.moe_fp8f16_gateup(xd, g[0], u[0], g[1], u[1], *subs[:4], P)
    dgot = e.moe_fp8f16_down_wide(hd, d[0], d[1], *subs, N).cpu()
    dold = e.moe_fp8f16_down(hd, d[0], d[1], *subs, N).cpu()

    def r_down(t):
        return float(((t.double() - dref).abs()
                      / dbound.clamp_min(1e-30)).max())

    def r_gu(t):
        return float(((t.cpu().double() - gref).abs() / gbound)[live].max())

    print("worst |error| / bound, wide (16-token): down %.3f (%.3f) "
          "gateup %.3f (%.3f)" % (r_down(dgot), r_down(dold), r_gu(ggot),
                                  r_gu(gold)))
    assert r_down(dgot) <= 1 and r_gu(ggot) <= 1
    # the same per-k-block structure: gate-up is bit-identical on any data
    assert_same(ggot[live], gold[live], "wide vs 16-token gate-up, random")


# --------------------------------------------------------------------------
# binding limits
# --------------------------------------------------------------------------

def test_binding_limits():
    e = ext()
    plan_d = pc.plans(tile())["wide_a"]
    subs, _ = dev_subs(plan_d)
    P, N = subs[3].numel(), plan_d["N"]
    c3, s3, _ = fc.exact_weight(40, 256, fc.E)
    w, sd = dev8(c3), s3.to(DEV)
    x = torch.zeros(N, 256, dtype=F16, device=DEV)
    hh = torch.zeros(P, 256, dtype=F16, device=DEV)
    e.moe_fp8f16_gateup_wide(x, w, w, sd, sd, *subs[:4], P)
    e.moe_fp8f16_down_wide(hh, w, sd, *subs, N)

    def both(match, wb, sb, xb=x, hb=hh, sub=subs):
        with pytest.raises(RuntimeError, match="moe_fp8f16_gateup_wide.*"
                           + match):
            e.moe_fp8f16_gateup_wide(xb, wb, wb, sb, sb, *sub[:4], P)
        with pytest.raises(RuntimeError, match="moe_fp8f16_down_wide.*"
                           + match):
            e.moe_fp8f16_down_wide(hb, wb, sb, *sub, N)

    # K = 192
    k192, s192, _ = fc.exact_weight(40, 192, fc.E)
    both("K % 128", dev8(k192), s192.to(DEV), x[:, :192].contiguous(),
         hh[:, :192].contiguous())
    # a non-contiguous weight
    wide, _, _ = fc.exact_weight(40, 512, fc.E)
    both("contiguous", dev8(wide)[..., ::2], sd)
    # a wrong scale shape
    both("weight_scale_inv", w, sd.transpose(1, 2).contiguous())
    # len(sorted_wt) != len(sorted_tok)
    with pytest.raises(RuntimeError, match="moe_fp8f16_down_wide.*sorted_wt"):
        e.moe_fp8f16_down_wide(hh, w, sd, *subs[:4], subs[4][:-1].contiguous(),
                               N)
