"""Shared set-up for the ragged batched-decode tests (CPU and GPU).

A pool of ``max_batch=4`` slots; three prompts of lengths 3, 7 and 12 are
prefilled through B=1 slot views into slots 0, 2 and 3 while slot 1 stays
idle, then 5 teacher-forced decode steps run with ``graph_pos`` as [4].
The reference is the same sequence run alone in a fresh B=1 cache.
"""

import torch

from conftest import init_model
from mlx_sharding_amd.config import ModelConfig
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.presets import get_preset

MAX_BATCH = 4
CAPACITY = 32
SLOTS = (0, 2, 3)
LENGTHS = (3, 7, 12)
N_STEPS = 5

TINY_LLAMA = {
    "model_type": "llama", "hidden_size": 64, "num_hidden_layers": 4,
    "intermediate_size": 128, "num_attention_heads": 4,
    "num_key_value_heads": 2, "vocab_size": 128,
    "rms_norm_eps": 1e-5, "rope_theta": 10000.0,
}
TINY_GEMMA2 = {
    "model_type": "gemma2", "hidden_size": 64, "num_hidden_layers": 4,
    "intermediate_size": 128, "num_attention_heads": 4,
    "num_key_value_heads": 2, "head_dim": 16, "vocab_size": 128,
    "rms_norm_eps": 1e-6, "rope_theta": 10000.0,
    "query_pre_attn_scalar": 16, "attn_logit_softcapping": 50.0,
    "final_logit_softcapping": 30.0, "sliding_window": 3,
}


def config_for(name: str) -> ModelConfig:
    if name == "llama":
        return ModelConfig.from_dict(TINY_LLAMA)
    if name == "gemma2":
        return ModelConfig.from_dict(TINY_GEMMA2)
    return get_preset(name)


def build_model(name: str, device="cpu"):
    cfg = config_for(name)
    m = init_model(get_model_class(cfg.model_type), cfg,
                   cfg.shard(0, cfg.num_hidden_layers))
    return m.to(device)


def sequences(vocab: int):
    """Seeded prompts and the forced decode tokens of every sequence."""
    g = torch.Generator().manual_seed(11)
    prompts = [torch.randint(0, vocab, (n,), generator=g).tolist()
               for n in LENGTHS]
    forced = [torch.randint(0, vocab, (N_STEPS,), generator=g).tolist()
              for _ in LENGTHS]
    return prompts, forced


@torch.no_grad()
def solo_run(model, prompt, forced):
    """[1 + N_STEPS] logits rows of one sequence alone in a B=1 cache."""
    dev = next(model.parameters()).device
    cache = model.make_cache(batch_size=1)
    out = [model(torch.tensor([prompt], device=dev), cache)[0, -1].float()]
    for t in forced:
        out.append(model(torch.tensor([[t]], device=dev), cache)[0, -1]
                   .float())
    return out


@torch.no_grad()
def ragged_run(model, prompts, forced):
    """The same sequences through the slot pool: per sequence, the
    prefill logits row and then one row per batched decode step."""
    dev = next(model.parameters()).device
    caches = model.make_cache(batch_size=MAX_BATCH)
    for c in caches:
        c.allocate(CAPACITY, MAX_BATCH)
    out = [[] for _ in prompts]
    pos = torch.zeros(MAX_BATCH, dtype=torch.int32, device=dev)
    inc = torch.zeros(MAX_BATCH, dtype=torch.int32, device=dev)
    for i, (slot, prompt) in enumerate(zip(SLOTS, prompts)):
        view = [c.slot(slot) for c in caches]
        h = model(torch.tensor([prompt], device=dev), view)
        out[i].append(h[0, -1].float())
        pos[slot] = len(prompt)
        inc[slot] = 1
    for c in caches:
        c.graph_pos = pos
    for step in range(N_STEPS):
        tok = torch.zeros(MAX_BATCH, 1, dtype=torch.long, device=dev)
        for i, slot in enumerate(SLOTS):
            tok[slot, 0] = forced[i][step]
        logits = model(tok, caches)[:, -1].float()
        pos.add_(inc)
        for i, slot in enumerate(SLOTS):
            out[i].append(logits[slot])
    return out
