"""The decode fusions are GPU-only: the CPU/reference path must not notice
MLXS_AMD_NO_DECODE_FUSE, and the new keyword arguments must be inert there.
"""

import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref


def test_switch_reads_environment(monkeypatch):
    monkeypatch.delenv("MLXS_AMD_NO_DECODE_FUSE", raising=False)
    assert ops.decode_fuse_enabled()
    monkeypatch.setenv("MLXS_AMD_NO_DECODE_FUSE", "1")
    assert not ops.decode_fuse_enabled()


def test_rms_norm_residual_want_f16_is_inert_on_cpu():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 1, 64, generator=g).bfloat16()
    r = torch.randn(3, 1, 64, generator=g).bfloat16()
    w = torch.rand(64, generator=g).bfloat16()
    y, h = ops.rms_norm_residual(x, r, w, 1e-6, 0.0, want_f16=True)
    assert torch.equal(h, x + r)
    assert torch.equal(y, ref.rms_norm(x + r, w, 1e-6, 0.0))
    assert not hasattr(y, "_mlxs_f16")


def test_cpu_decode_ignores_switch(tiny_deepseek_config, monkeypatch):
    from conftest import init_model
    from mlx_sharding_amd.models import get_model_class
    cfg = tiny_deepseek_config
    m = init_model(get_model_class("deepseek_v2"), cfg,
                   cfg.shard(0, cfg.num_hidden_layers), seed=3)
    ids = torch.randint(0, 128, (2, 4), generator=torch.Generator().manual_seed(1))

    def run():
        cache = m.make_cache(batch_size=2)
        with torch.no_grad():
            out = [m(ids, cache)[:, -1]]
            for _ in range(2):
                out.append(m(out[-1].argmax(-1)[:, None], cache)[:, -1])
        return torch.stack(out)

    monkeypatch.delenv("MLXS_AMD_NO_DECODE_FUSE", raising=False)
    a = run()
    monkeypatch.setenv("MLXS_AMD_NO_DECODE_FUSE", "1")
    assert torch.equal(a, run())
