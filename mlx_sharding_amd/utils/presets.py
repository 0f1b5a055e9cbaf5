"""Named model-architecture presets for bench/tests (random-init weights;
there is no network for checkpoints).  Shapes follow the published HF
configs of the models BASELINE.json names."""

from __future__ import annotations

from ..config import FP8_QUANTIZATION_CONFIG, ModelConfig

PRESETS = {
    # headline model: DeepSeek-Coder-V2-Lite-Instruct (15.7B total, 2.4B active)
    "deepseek-v2-lite": {
        "model_type": "deepseek_v2",
        "hidden_size": 2048,
        "num_hidden_layers": 27,
        "intermediate_size": 10944,
        "moe_intermediate_size": 1408,
        "num_attention_heads": 16,
        "vocab_size": 102400,
        "rms_norm_eps": 1e-6,
        "rope_theta": 10000.0,
        "q_lora_rank": None,
        "kv_lora_rank": 512,
        "qk_nope_head_dim": 128,
        "qk_rope_head_dim": 64,
        "v_head_dim": 128,
        "n_routed_experts": 64,
        "n_shared_experts": 2,
        "num_experts_per_tok": 6,
        "n_group": 1,
        "topk_group": 1,
        "topk_method": "greedy",
        "norm_topk_prob": False,
        "routed_scaling_factor": 1.0,
        "first_k_dense_replace": 1,
        "moe_layer_freq": 1,
        "max_position_embeddings": 163840,
        "rope_scaling": {"type": "yarn", "factor": 40.0, "beta_fast": 32,
                         "beta_slow": 1, "mscale": 0.707, "mscale_all_dim": 0.707,
                         "original_max_position_embeddings": 4096},
    },
    # DeepSeek-V2 (236B total, 21B active): group-limited greedy routing
    # over 160 experts.  Shapes only; far too large to instantiate in tests.
    "deepseek-v2": {
        "model_type": "deepseek_v2",
        "hidden_size": 5120,
        "num_hidden_layers": 60,
        "intermediate_size": 12288,
        "moe_intermediate_size": 1536,
        "num_attention_heads": 128,
        "vocab_size": 102400,
        "rms_norm_eps": 1e-6,
        "rope_theta": 10000.0,
        "q_lora_rank": 1536,
        "kv_lora_rank": 512,
        "qk_nope_head_dim": 128,
        "qk_rope_head_dim": 64,
        "v_head_dim": 128,
        "n_routed_experts": 160,
        "n_shared_experts": 2,
        "num_experts_per_tok": 6,
        "n_group": 8,
        "topk_group": 3,
        "topk_method": "group_limited_greedy",
        "norm_topk_prob": False,
        "routed_scaling_factor": 16.0,
        "first_k_dense_replace": 1,
        "moe_layer_freq": 1,
        "max_position_embeddings": 163840,
        "rope_scaling": {"type": "yarn", "factor": 40.0, "beta_fast": 32,
                         "beta_slow": 1, "mscale": 1.0, "mscale_all_dim": 1.0,
                         "original_max_position_embeddings": 4096},
    },
    # DeepSeek-V3 / R1 (671B total, 37B active): sigmoid router with a
    # selection bias over 256 experts in 8 groups.  Shapes only.
    "deepseek-v3": {
        "model_type": "deepseek_v3",
        "hidden_size": 7168,
        "num_hidden_layers": 61,
        "intermediate_size": 18432,
        "moe_intermediate_size": 2048,
        "num_attention_heads": 128,
        "vocab_size": 129280,
        "rms_norm_eps": 1e-6,
        "rope_theta": 10000.0,
        "q_lora_rank": 1536,
        "kv_lora_rank": 512,
        "qk_nope_head_dim": 128,
        "qk_rope_head_dim": 64,
        "v_head_dim": 128,
        "n_routed_experts": 256,
        "n_shared_experts": 1,
        "num_experts_per_tok": 8,
        "n_group": 8,
        "topk_group": 4,
        "topk_method": "noaux_tc",
        "scoring_func": "sigmoid",
        "norm_topk_prob": True,
        "routed_scaling_factor": 2.5,
        "first_k_dense_replace": 3,
        "moe_layer_freq": 1,
        "max_position_embeddings": 163840,
        "rope_scaling": {"type": "yarn", "factor": 40.0, "beta_fast": 32,
                         "beta_slow": 1, "mscale": 1.0, "mscale_all_dim": 1.0,
                         "original_max_position_embeddings": 4096},
    },
    "llama-3-8b": {
        "model_type": "llama",
        "hidden_size": 4096,
        "num_hidden_layers": 32,
        "intermediate_size": 14336,
        "num_attention_heads": 32,
        "num_key_value_heads": 8,
        "vocab_size": 128256,
        "rms_norm_eps": 1e-5,
        "rope_theta": 500000.0,
        "max_position_embeddings": 8192,
    },
    "llama-3-70b": {
        "model_type": "llama",
        "hidden_size": 8192,
        "num_hidden_layers": 80,
        "intermediate_size": 28672,
        "num_attention_heads": 64,
        "num_key_value_heads": 8,
        "vocab_size": 128256,
        "rms_norm_eps": 1e-5,
        "rope_theta": 500000.0,
        "max_position_embeddings": 8192,
    },
    "gemma-2-9b": {
        "model_type": "gemma2",
        "hidden_size": 3584,
        "num_hidden_layers": 42,
        "intermediate_size": 14336,
        "num_attention_heads": 16,
        "num_key_value_heads": 8,
        "head_dim": 256,
        "vocab_size": 256000,
        "rms_norm_eps": 1e-6,
        "rope_theta": 10000.0,
        "query_pre_attn_scalar": 256,
        "attn_logit_softcapping": 50.0,
        "final_logit_softcapping": 30.0,
        "sliding_window": 4096,
        "max_position_embeddings": 8192,
    },
    "tinyllama-1.1b": {
        "model_type": "llama",
        "hidden_size": 2048,
        "num_hidden_layers": 22,
        "intermediate_size": 5632,
        "num_attention_heads": 32,
        "num_key_value_heads": 4,
        "vocab_size": 32000,
        "rms_norm_eps": 1e-5,
        "rope_theta": 10000.0,
    },
    # Qwen2-7B-Instruct shapes (config.json of Qwen/Qwen2-7B-Instruct);
    # llama-family remap with QKV-only attention biases
    "qwen2-7b": {
        "model_type": "qwen2",
        "hidden_size": 3584,
        "num_hidden_layers": 28,
        "intermediate_size": 18944,
        "num_attention_heads": 28,
        "num_key_value_heads": 4,
        "vocab_size": 152064,
        "rms_norm_eps": 1e-6,
        "rope_theta": 1000000.0,
        "tie_word_embeddings": False,
        "max_position_embeddings": 32768,
    },

    # small debug model (CPU-runnable; 8 layers so a CPU smoke of the
    # 8-stage pipeline gives every rank at least one layer)
    "debug-llama": {
        "model_type": "llama",
        "hidden_size": 256,
        "num_hidden_layers": 8,
        "intermediate_size": 512,
        "num_attention_heads": 8,
        "num_key_value_heads": 4,
        "vocab_size": 1024,
        "rms_norm_eps": 1e-5,
        "rope_theta": 10000.0,
    },
    "debug-deepseek": {
        "model_type": "deepseek_v2",
        "hidden_size": 128,
        "num_hidden_layers": 8,
        "intermediate_size": 256,
        "moe_intermediate_size": 64,
        "num_attention_heads": 4,
        "vocab_size": 512,
        "rms_norm_eps": 1e-6,
        "rope_theta": 10000.0,
        "q_lora_rank": None,
        "kv_lora_rank": 64,
        "qk_nope_head_dim": 32,
        "qk_rope_head_dim": 16,
        "v_head_dim": 32,
        "n_routed_experts": 8,
        "n_shared_experts": 1,
        "num_experts_per_tok": 2,
        "first_k_dense_replace": 1,
        "moe_layer_freq": 1,
        "rope_scaling": {"type": "yarn", "factor": 4.0, "beta_fast": 32,
                         "beta_slow": 1, "mscale": 0.707, "mscale_all_dim": 0.707,
                         "original_max_position_embeddings": 4096},
    },
}

# debug-deepseek with DeepSeek-V2's group-limited routing: 96 experts in
# 8 groups of 12 (more than one 64-lane register row in the fused gate)
PRESETS["debug-deepseek-grouped"] = dict(
    PRESETS["debug-deepseek"],
    n_routed_experts=96,
    num_experts_per_tok=4,
    topk_method="group_limited_greedy",
    n_group=8,
    topk_group=3,
    routed_scaling_factor=16.0,
    norm_topk_prob=False,
)

# debug-deepseek as a DeepSeek-V3: sigmoid router with a selection bias
# over 96 experts in 8 groups (more than one register row in the fused
# gate), a q_lora_rank, and 32 heads (the head-group decode path)
PRESETS["debug-deepseek-v3"] = dict(
    PRESETS["debug-deepseek"],
    model_type="deepseek_v3",
    q_lora_rank=48,
    num_attention_heads=32,
    n_routed_experts=96,
    num_experts_per_tok=4,
    topk_method="noaux_tc",
    scoring_func="sigmoid",
    n_group=8,
    topk_group=3,
    routed_scaling_factor=2.5,
    norm_topk_prob=True,
)


# debug-deepseek-v3 with every routed-expert GEMM on K % 128 == 0 (hidden
# 256, expert inner 128) — the shapes the FP8 block kernels serve
PRESETS["debug-deepseek-v3-fp8"] = dict(
    PRESETS["debug-deepseek-v3"],
    hidden_size=256,
    moe_intermediate_size=128,
)


def get_preset(name: str, quant: bool = False,
               group_size: int = 64, bits: int = 4,
               fp8: bool = False) -> ModelConfig:
    """fp8=True adds the FP8 block `quantization_config` stanza (128x128
    e4m3 blocks) instead of an affine `quantization` one."""
    raw = dict(PRESETS[name])
    if quant and fp8:
        raise ValueError("get_preset: quant and fp8 are exclusive")
    if quant:
        raw["quantization"] = {"group_size": group_size, "bits": bits}
    if fp8:
        raw["quantization_config"] = dict(FP8_QUANTIZATION_CONFIG)
    return ModelConfig.from_dict(raw)
