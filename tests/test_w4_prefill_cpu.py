"""The prefill routing of ops.grouped_expert_mlp_quant: _w4_prefill_route's
truth table and the MLXS_AMD_W4_PREFILL parsing."""

import pytest

from mlx_sharding_amd import ops

MIN = ops._MOE_GEMM_MIN_N


@pytest.mark.parametrize("pairs,resident,ok,env,want", [
    (MIN - 1, False, True, "packed", "tiles16"),
    (MIN - 1, True, True, None, "tiles16"),
    (MIN, False, True, None, "packed"),
    (MIN, True, True, None, "dense"),
    (MIN, True, True, "packed", "packed"),
    (MIN, False, True, "dense", "dense"),
    (MIN, False, False, None, "dense"),
    (MIN, False, False, "packed", "dense"),
])
def test_route_truth_table(pairs, resident, ok, env, want):
    assert ops._w4_prefill_route(pairs, resident, ok, env) == want


def test_env_parsing(monkeypatch):
    monkeypatch.delenv("MLXS_AMD_W4_PREFILL", raising=False)
    assert ops._w4_prefill_env() is None
    monkeypatch.setenv("MLXS_AMD_W4_PREFILL", "fast")
    for pairs in (1, MIN):
        with pytest.raises(ValueError, match="MLXS_AMD_W4_PREFILL"):
            ops._w4_prefill_route(pairs, False, True, ops._w4_prefill_env())
