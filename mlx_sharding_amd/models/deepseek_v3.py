"""DeepSeek-V3 / R1 stage model.

The V2 stack (MLA with q_lora_rank and YaRN, stacked `switch_mlp`
experts, the fused T == 1 decode path) with V3's router: sigmoid scores,
a learned per-expert `e_score_correction_bias` that steers selection
only, groups ranked by the sum of their two best biased scores
(`topk_method: "noaux_tc"`).  Absorbed (compressed-cache) decode is taken
up to 128 heads.

Checkpoints in the MLX / HF layout load directly: per-expert
`mlp.experts.E.*` stack into `switch_mlp.*`, `rotary_emb.inv_freq` and
the multi-token-prediction layers (`model.layers.i.*`, i >=
num_hidden_layers) are dropped.  The published FP8 block-quantized
checkpoints load the same way: `X.weight` (float8_e4m3fn) and
`X.weight_scale_inv` (fp32, one scale per 128x128 block) are the module
parameters' own names, per-expert scales stack to [E, RB, KB], and the
FP8 multi-token-prediction layers are dropped with the rest.
"""

from __future__ import annotations

from typing import Dict, Tuple

import torch
import torch.nn as nn

from ..config import ModelConfig, ShardSpec
from .deepseek_v2 import (DeepseekV2DecoderLayer, DeepseekV2MoE,
                          DeepseekV2StageModel, MLAAttention)


def _with_v3_defaults(cfg: ModelConfig) -> ModelConfig:
    """V3's router defaults for fields a config leaves out (the V2 classes
    default to V2-Lite's)."""
    raw = dict(cfg.raw)
    for key, val in (("n_routed_experts", 256), ("num_experts_per_tok", 8),
                     ("n_group", 8), ("topk_group", 4),
                     ("norm_topk_prob", True),
                     ("routed_scaling_factor", 2.5),
                     ("scoring_func", "sigmoid"),
                     ("topk_method", "noaux_tc"),
                     ("moe_intermediate_size", 2048)):
        if raw.get(key) is None:
            raw[key] = val
    return ModelConfig(cfg.model_type, raw)


class DeepseekV3Attention(MLAAttention):
    max_absorbed_heads = 128
    fuse_q_lora = True


class DeepseekV3MoE(DeepseekV2MoE):
    def __init__(self, cfg: ModelConfig, quant_for, prefix: str):
        cfg = _with_v3_defaults(cfg)
        scoring = cfg.get("scoring_func")
        method = cfg.get("topk_method")
        if scoring != "sigmoid":
            raise ValueError(
                f"deepseek_v3: scoring_func {scoring!r} not supported "
                f"(only 'sigmoid')")
        if method != "noaux_tc":
            raise ValueError(
                f"deepseek_v3: topk_method {method!r} not supported "
                f"(only 'noaux_tc')")
        super().__init__(cfg, quant_for, prefix)
        if self.n_group > 1 and (self.n_experts % self.n_group != 0
                                 or self.n_experts // self.n_group < 2):
            raise ValueError(
                f"deepseek_v3: n_group {self.n_group} must divide "
                f"n_routed_experts {self.n_experts} into groups of >= 2")
        # selection-only bias, fp32 whatever the model dtype; it lives on
        # the gate module so its key is the checkpoint's
        # `mlp.gate.e_score_correction_bias`
        self.gate.e_score_correction_bias = nn.Parameter(
            torch.zeros(self.n_experts, dtype=torch.float32),
            requires_grad=False)

    @property
    def e_score_correction_bias(self) -> torch.Tensor:
        return self.gate.e_score_correction_bias

    def _gate_groups(self) -> Tuple[int, int]:
        return self.n_group, self.topk_group

    def _fused_gate_ok(self, n_tokens: int) -> bool:
        # sigmoid mode ranks a group by its two best members
        return (super()._fused_gate_ok(n_tokens)
                and (self.n_group == 1
                     or self.n_experts // self.n_group >= 2))

    def _gate_kwargs(self) -> dict:
        # .float() is a no-op unless someone cast the whole module
        return {"scoring": "sigmoid",
                "e_bias": self.e_score_correction_bias.float()}


class DeepseekV3DecoderLayer(DeepseekV2DecoderLayer):
    attn_cls = DeepseekV3Attention
    moe_cls = DeepseekV3MoE


class DeepseekV3StageModel(DeepseekV2StageModel):
    model_type = "deepseek_v3"
    layer_cls = DeepseekV3DecoderLayer

    @classmethod
    def sanitize(cls, weights: Dict[str, torch.Tensor],
                 shard: ShardSpec) -> Dict[str, torch.Tensor]:
        for k in weights:
            if k.endswith((".embed_q.weight", ".unembed_out.weight",
                           ".embed_q.scales", ".unembed_out.scales")):
                raise ValueError(
                    f"deepseek_v3: checkpoint key {k!r} is the pre-absorbed "
                    f"embed_q/unembed_out layout of newer mlx_lm conversions, "
                    f"which is not supported; convert with kv_b_proj")
        # multi-token-prediction layers sit past num_hidden_layers
        n = shard.num_hidden_layers
        kept = {}
        for k, v in weights.items():
            if k.startswith("model.layers.") and int(k.split(".")[2]) >= n:
                continue
            kept[k] = v
        return super().sanitize(kept, shard)
