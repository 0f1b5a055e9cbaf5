"""debug-deepseek-v3 running a short chunk over a cached prefix through the
absorbed chunk kernel: the GPU model against the CPU model, and the switch."""
import pytest
import torch

from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.presets import get_preset

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("chunk", (True, False), ids=("chunk", "no_mla_chunk"))
def test_debug_v3_chunk_over_prefix(chunk, monkeypatch):
    if chunk:
        monkeypatch.delenv("MLXS_AMD_NO_MLA_CHUNK", raising=False)
    else:
        monkeypatch.setenv("MLXS_AMD_NO_MLA_CHUNK", "1")
    cfg = get_preset("debug-deepseek-v3")
    cls = get_model_class("deepseek_v3")
    layers = cfg.shard(0, cfg.num_hidden_layers)
    cpu = init_model(cls, cfg, layers, seed=13)
    ids = torch.randint(0, cfg.vocab_size, (2, 26),
                        generator=torch.Generator().manual_seed(3))
    with torch.no_grad():  # the CPU reference model on the same 25 + 1 tokens
        want = cpu(ids, cpu.make_cache(batch_size=2)).float()[:, 20:]
    m = cls(cfg, layers)
    m.load_weights(cpu.state_dict())
    m = m.to(DEV).eval()
    cache = m.make_cache(batch_size=2)

    calls = []
    real = ops.hip_ext().mla_chunk

    def spy(*args, **kwargs):
        calls.append(args[0].shape)
        return real(*args, **kwargs)

    monkeypatch.setattr(ops.hip_ext(), "mla_chunk", spy)
    dev_ids = ids.to(DEV)
    with torch.no_grad():
        m(dev_ids[:, :20], cache)
        got = torch.cat([m(dev_ids[:, 20:25], cache),
                         m(dev_ids[:, 25:], cache)], dim=1).float().cpu()
    assert len(calls) == (cfg.num_hidden_layers if chunk else 0)
    for pos in range(6):
        err = (got[:, pos] - want[:, pos]).abs().max().item()
        scale = want[:, pos].abs().max().item()
        print(f"position {20 + pos}: err {err:.3e} scale {scale:.3f}")
        assert err <= 6e-2 + 1e-2 * scale, (pos, err, scale)
