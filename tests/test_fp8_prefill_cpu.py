"""CPU sanity for the wide-tile FP8 MoE prefill cases (fp8_prefill_cases.py)
and for the prefill routing of ops.grouped_expert_mlp_fp8.

For both plans and both candidate tiles the fp32 exactness budget holds, an
emulation of the kernels' declared arithmetic over the plan equals the fp64
expectation bit for bit, and the two slips a tiled walk can make (losing
row TM of a walked sub-range; scattering a tail tile's clamped rows instead
of masking them) do not — so an inequality on the GPU is the kernel's
fault, and the cases can see those slips.
"""

import math

import pytest
import torch

import fp8_cases as fc
import fp8_prefill_cases as pc
import quant_cases as qc
from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

DOWN_BOUND = 2 * 384 * 2 * 16 * 2 / fc.DOWN_LSB   # fp8_cases: 2^22.6 LSBs


@pytest.mark.parametrize("TM", pc.TMS)
def test_plan_shapes(TM):
    a, b = pc.plans(TM)["wide_a"], pc.plans(TM)["wide_b"]
    assert a["N"] == b["N"] == 2 * TM + 26
    sa, live_a = qc.build_subranges(a["plan"])
    sb, live_b = qc.build_subranges(b["plan"])
    # the same sorted rows, cut differently
    assert torch.equal(sa[3], sb[3]) and torch.equal(live_a, live_b)
    assert torch.equal(sa[4][live_a], sb[4][live_b])
    assert sa[2].tolist() == [TM, 1, 0, TM - 1, TM, 17, 0]
    assert sb[2].tolist() == [TM, 1, 0, 2 * TM + 16, 0]
    assert int((~live_a).sum()) == 3 and live_a.numel() == 3 * TM + 20
    for d in (a, b):
        dead = qc.dead_tokens(d)
        assert {d["N"] - 2, d["N"] - 1} <= set(dead)
        e0 = [t for _, e, t in qc.plan_pairs(d["plan"]) if e == 0]
        e2 = [t for _, e, t in qc.plan_pairs(d["plan"]) if e == 2]
        assert e0 != sorted(e0) and e2 != sorted(e2)
        assert len(set(e0)) == len(e0) and len(set(e2)) == len(e2)
        assert len(set(e0) & set(e2)) > TM // 2
        assert qc.UNUSED_EXPERT not in {e for _, e, _ in
                                        qc.plan_pairs(d["plan"])}


@pytest.mark.parametrize("plan", pc.PLAN_NAMES)
@pytest.mark.parametrize("TM", pc.TMS)
@pytest.mark.parametrize("I", fc.DOWN_IS)
def test_down_cases(I, TM, plan):
    plan_d = pc.plans(TM)[plan]
    codes, s, W, h, out, top = fc.down_case(I, plan_d)
    print("fp8 moe down %s TM=%d I=%d: seen 2^%.1f of 2^%.1f LSBs"
          % (plan, TM, I, math.log2(top), math.log2(DOWN_BOUND)))
    assert top <= DOWN_BOUND < qc.F24
    got = pc.emulate_down(codes, s, h, plan_d, TM)
    assert torch.equal(got.double(), out)
    # the clamp slip shows on every plan (each has a sub-range whose length
    # is no multiple of 16), the dropped row where a sub-range is walked
    bad = pc.emulate_down(codes, s, h, plan_d, TM, slip="clamp_tail")
    assert not torch.equal(bad.double(), out)
    bad = pc.emulate_down(codes, s, h, plan_d, TM, slip="drop_row_tm")
    assert torch.equal(bad.double(), out) == (plan != "wide_b")


@pytest.mark.parametrize("plan", pc.PLAN_NAMES)
@pytest.mark.parametrize("TM", pc.TMS)
@pytest.mark.parametrize("kind", ("a", "b"))
def test_gateup_cases(kind, TM, plan):
    """The offset sweep covers every column for every live expert, the
    vectorised closed form equals quant_cases.gateup_expected, and the
    emulated gate / up products give it bit for bit."""
    H = 384
    plan_d = pc.plans(TM)[plan]
    gate, up = fc.gateup_weights(kind, fc.MOE_I, H)
    offs = qc.gateup_offsets(plan_d, H)
    print("gate-up %s TM=%d H=%d: %d one-hot offsets" % (plan, TM, H, len(offs)))
    some = [offs[0], offs[len(offs) // 2], offs[-1]]
    want = pc.gateup_expected_sweep(kind, gate[2], up[2], plan_d, H, some,
                                    torch.float16)
    for n, off in enumerate(some[:: 2]):
        assert torch.equal(want[2 * n], qc.gateup_expected(
            kind, gate[2], up[2], plan_d, H, off, torch.float16))
    for n, off in enumerate(some):
        x = qc.gateup_x(plan_d["N"], H, off).to(torch.float16)
        for e, rows, toks in pc.subrange_rows(plan_d["plan"]):
            g = fc.emulate_moe_linear(x[toks], fc.to_fp8(gate[0][e]),
                                      gate[1][e])
            u = fc.emulate_moe_linear(x[toks], fc.to_fp8(up[0][e]), up[1][e])
            h = (g / (1.0 + torch.exp(-g)) * u).to(torch.float16)
            assert torch.equal(h.double(), want[n][rows])


# --------------------------------------------------------------------------
# routing
# --------------------------------------------------------------------------

def test_route_truth_table():
    route = ops._fp8_prefill_route
    MIN = ops._MOE_GEMM_MIN_N
    assert MIN == 256
    for resident in (False, True):
        for kernel_ok in (False, True):
            for env in (None, "packed", "dense"):
                for pairs in (1, MIN - 1):
                    assert route(pairs, resident, kernel_ok, env) == "tiles16"
                for pairs in (MIN, 32768):
                    got = route(pairs, resident, kernel_ok, env)
                    if not kernel_ok or env == "dense":
                        want = "dense"
                    elif env == "packed":
                        want = "packed"
                    else:
                        want = "dense" if resident else "packed"
                    assert got == want, (pairs, resident, kernel_ok, env)
            for env in ("Packed", "1", "bf16"):
                for pairs in (1, MIN):
                    with pytest.raises(ValueError,
                                       match="MLXS_AMD_FP8_PREFILL"):
                        route(pairs, resident, kernel_ok, env)


def test_route_env_reading(monkeypatch):
    monkeypatch.delenv("MLXS_AMD_FP8_PREFILL", raising=False)
    assert ops._fp8_prefill_env() is None
    monkeypatch.setenv("MLXS_AMD_FP8_PREFILL", "")
    assert ops._fp8_prefill_env() is None
    monkeypatch.setenv("MLXS_AMD_FP8_PREFILL", "packed")
    assert ops._fp8_prefill_env() == "packed"


@pytest.mark.parametrize("env", (None, "packed", "dense"))
def test_cpu_path_unchanged(monkeypatch, env):
    """300 pairs on the CPU: the reference, whatever the variable says."""
    if env is None:
        monkeypatch.delenv("MLXS_AMD_FP8_PREFILL", raising=False)
    else:
        monkeypatch.setenv("MLXS_AMD_FP8_PREFILL", env)
    g = torch.Generator().manual_seed(3)
    E, H, I, N, K = 6, 128, 136, 100, 3
    mats = [ref.quantize_fp8_block(torch.randn(E, o, k, generator=g) * 0.05)
            for o, k in ((I, H), (I, H), (H, I))]
    x = torch.randn(N, H, generator=g)
    indices = torch.stack([torch.randperm(E, generator=g)[:K]
                           for _ in range(N)])
    weights = torch.rand(N, K, generator=g)
    assert indices.numel() == 300 >= ops._MOE_GEMM_MIN_N
    got = ops.grouped_expert_mlp_fp8(x, *mats, weights, indices)
    want = ref.grouped_expert_mlp_fp8(x, *mats, weights, indices)
    assert got.dtype == want.dtype and torch.equal(got, want)
