"""debug-llama-gqa, a 5-token chunk over a 20-token cached prefix, bf16 and FP8
cache: the GPU model against the CPU model, and the MLXS_AMD_GQA_CHUNK switch."""
import pytest
import torch

from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.presets import get_preset

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPIED = ("gqa_chunk", "gqa_chunk_fp8", "kv_fp8_dequant", "attn_prefill")


@pytest.mark.parametrize("kv", ("bf16", "fp8"))
@pytest.mark.parametrize("env", ("1", "0"))
def test_debug_llama_chunk_over_prefix(env, kv, monkeypatch):
    monkeypatch.setenv("MLXS_AMD_GQA_CHUNK", env)
    if kv == "fp8":
        monkeypatch.setenv("MLXS_AMD_KV_DTYPE", "fp8")
    else:
        monkeypatch.delenv("MLXS_AMD_KV_DTYPE", raising=False)
    cfg = get_preset("debug-llama-gqa")
    cls = get_model_class(cfg.model_type)
    layers = cfg.shard(0, cfg.num_hidden_layers)
    cpu = init_model(cls, cfg, layers, seed=13)
    ids = torch.randint(0, cfg.vocab_size, (2, 26),
                        generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        want = cpu(ids, cpu.make_cache(batch_size=2)).float()[:, 20:]
    m = cls(cfg, layers)
    m.load_weights(cpu.state_dict())
    m = m.to(DEV).eval()
    cache = m.make_cache(batch_size=2)

    calls = {n: 0 for n in SPIED}
    for n in SPIED:
        def spy(*a, _n=n, _f=getattr(ops.hip_ext(), n), **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops.hip_ext(), n, spy)
    dev_ids, L = ids.to(DEV), cfg.num_hidden_layers
    with torch.no_grad():
        m(dev_ids[:, :20], cache)
        cold = dict(calls)
        got = [m(dev_ids[:, 20:25], cache)]
        chunk = {n: calls[n] - cold[n] for n in SPIED}
        got = torch.cat(got + [m(dev_ids[:, 25:], cache)], dim=1).float().cpu()
    # the cold prefill never takes the new kernel
    assert cold["gqa_chunk"] == cold["gqa_chunk_fp8"] == 0
    assert cold["attn_prefill"] == L
    new = "gqa_chunk_fp8" if kv == "fp8" else "gqa_chunk"
    if env == "1":
        assert chunk[new] == L and chunk["attn_prefill"] == 0
        assert chunk["kv_fp8_dequant"] == 0
    else:
        assert chunk["gqa_chunk"] == chunk["gqa_chunk_fp8"] == 0
        assert chunk["attn_prefill"] == L
    for pos in range(6):
        err = (got[:, pos] - want[:, pos]).abs().max().item()
        scale = want[:, pos].abs().max().item()
        assert err <= 6e-2 + 1e-2 * scale, (pos, err, scale)
