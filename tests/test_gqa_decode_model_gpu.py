"""debug-llama-gqa (G = 4) and debug-gemma2 (G = 2, softcap, window 8)
decoding through the MFMA GQA kernel: the GPU model against the CPU model,
and the MLXS_AMD_GQA_MFMA switch."""
import functools

import pytest
import torch

from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.presets import get_preset

pytestmark = pytest.mark.gpu
DEV, STEPS = "cuda", 12


@functools.lru_cache(maxsize=None)
def _cpu_model_run(preset):
    """CPU prefill + STEPS greedy decode steps."""
    cfg = get_preset(preset)
    m = init_model(get_model_class(cfg.model_type), cfg,
                   cfg.shard(0, cfg.num_hidden_layers), seed=13)
    ids = torch.randint(0, cfg.vocab_size, (2, 7),
                        generator=torch.Generator().manual_seed(2))
    cache = m.make_cache(batch_size=2)
    rows, toks = [], []
    with torch.no_grad():
        h = m(ids, cache)
        for _ in range(STEPS):
            rows.append(h[:, -1].float())
            toks.append(h[:, -1].argmax(-1))
            h = m(toks[-1][:, None], cache)
        rows.append(h[:, -1].float())
    return cfg, m.state_dict(), ids, toks, rows


@pytest.mark.parametrize("mfma", ("1", "0"), ids=("mfma", "no_mfma"))
@pytest.mark.parametrize("preset", ("debug-llama-gqa", "debug-gemma2"))
def test_debug_gqa_decodes_through_gqa_decode(preset, mfma, monkeypatch):
    monkeypatch.setenv("MLXS_AMD_GQA_MFMA", mfma)
    cfg, sd, ids, toks, rows = _cpu_model_run(preset)
    m = get_model_class(cfg.model_type)(cfg, cfg.shard(0, cfg.num_hidden_layers))
    m.load_weights(sd)
    m = m.to(DEV).eval()
    cache = m.make_cache(batch_size=2)
    calls = []
    real = ops.hip_ext().gqa_decode
    monkeypatch.setattr(ops.hip_ext(), "gqa_decode",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    got = []
    with torch.no_grad():
        h = m(ids.to(DEV), cache)
        for t in toks:
            got.append(h[:, -1].float().cpu())
            h = m(t[:, None].to(DEV), cache)
        got.append(h[:, -1].float().cpu())
    assert len(calls) == (STEPS * cfg.num_hidden_layers if mfma == "1" else 0)
    for step, (a, b) in enumerate(zip(got, rows)):
        err, scale = (a - b).abs().max().item(), b.abs().max().item()
        print(f"step {step}: err {err:.3e} scale {scale:.3f}")
        assert err <= 6e-2 + 1e-2 * scale, (step, err, scale)
