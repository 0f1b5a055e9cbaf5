"""CPU checks for fused group-limited MoE gating: the model's dispatch
predicate, the new presets, and the sanity of the GPU test's inputs."""

import pytest
import torch

from moe_gate_cases import GRID, GRID_IDS, make_logits

from mlx_sharding_amd.config import ModelConfig
from mlx_sharding_amd.models.deepseek_v2 import DeepseekV2MoE
from mlx_sharding_amd.ops import reference as ref
from mlx_sharding_amd.utils.presets import get_preset


def _moe(cfg: ModelConfig) -> DeepseekV2MoE:
    with torch.device("meta"):
        return DeepseekV2MoE(cfg, lambda prefix: None, "model.layers.1.mlp")


def _cfg(**over) -> ModelConfig:
    raw = dict(get_preset("debug-deepseek-grouped").raw)
    raw.update(over)
    return ModelConfig.from_dict(raw)


def test_grouped_preset_fields():
    raw = get_preset("debug-deepseek-grouped").raw
    base = get_preset("debug-deepseek").raw
    changed = dict(n_routed_experts=96, num_experts_per_tok=4,
                   topk_method="group_limited_greedy", n_group=8,
                   topk_group=3, routed_scaling_factor=16.0,
                   norm_topk_prob=False)
    for k, v in changed.items():
        assert raw[k] == v, k
    for k, v in base.items():
        if k not in changed:
            assert raw[k] == v, k
    v2 = get_preset("deepseek-v2").raw
    assert (v2["n_routed_experts"], v2["n_group"], v2["topk_group"],
            v2["num_experts_per_tok"]) == (160, 8, 3, 6)
    assert v2["rope_scaling"]["mscale"] == v2["rope_scaling"]["mscale_all_dim"]


@pytest.mark.parametrize("n", [1, 64, 128])
def test_fused_gate_ok_grouped_preset(n):
    assert _moe(get_preset("debug-deepseek-grouped"))._fused_gate_ok(n)


def test_fused_gate_ok_v2_shape_and_256_greedy():
    v2 = _cfg(n_routed_experts=160, num_experts_per_tok=6, n_group=8,
              topk_group=3)
    assert _moe(v2)._fused_gate_ok(64)
    greedy = _cfg(n_routed_experts=256, num_experts_per_tok=8,
                  topk_method="greedy", n_group=1, topk_group=1)
    assert _moe(greedy)._fused_gate_ok(128)
    # plain greedy ignores the config's group fields, as the torch gate does
    odd = _cfg(n_routed_experts=100, topk_method="greedy", n_group=8)
    assert _moe(odd)._fused_gate_ok(4)


def test_fused_gate_ok_rejects_outside_limits():
    assert not _moe(get_preset("debug-deepseek-grouped"))._fused_gate_ok(129)
    assert not _moe(_cfg(n_routed_experts=257, topk_method="greedy",
                         n_group=1, topk_group=1))._fused_gate_ok(4)
    # E % n_group != 0
    assert not _moe(_cfg(n_routed_experts=100, n_group=8))._fused_gate_ok(4)
    # topk_group * (E / n_group) < top_k: 1 * 12 < 16 and 1 * 4 < 6
    assert not _moe(_cfg(topk_group=1, num_experts_per_tok=16))._fused_gate_ok(4)
    assert not _moe(_cfg(n_routed_experts=32, topk_group=1,
                         num_experts_per_tok=6))._fused_gate_ok(4)
    # group counts / kept groups outside the kernel's range
    assert not _moe(_cfg(n_routed_experts=128, n_group=64,
                         topk_group=8))._fused_gate_ok(4)
    assert not _moe(_cfg(topk_group=9))._fused_gate_ok(4)


@pytest.mark.parametrize("case", GRID, ids=GRID_IDS)
def test_gate_inputs_discriminate_groups(case):
    """The GPU test's logits have no ties, and wherever groups are dropped
    the group-limited selection differs from plain greedy for at least one
    token — a kernel that ignores groups cannot pass on them."""
    N, E, n_group, topk_group, K, norm, scaling, _ = case
    logits = make_logits(N, E).float()
    assert logits.shape == (N, E)
    for row in logits:
        assert row.unique().numel() == E
    _, idx_g = ref.moe_gate(logits, K, n_group, topk_group, scaling, norm)
    _, idx_p = ref.moe_gate(logits, K, 1, 1, scaling, norm)
    sets_g = [set(r.tolist()) for r in idx_g]
    sets_p = [set(r.tolist()) for r in idx_p]
    gsz = E // n_group
    for s in sets_g:  # the selection spans at most topk_group groups
        assert len({e // gsz for e in s}) <= topk_group
    if topk_group < n_group:
        assert any(a != b for a, b in zip(sets_g, sets_p))
    else:
        assert sets_g == sets_p
