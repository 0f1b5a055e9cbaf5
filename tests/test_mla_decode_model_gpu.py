"""debug-deepseek-v3 decoding through the MFMA absorbed-MLA kernel: the GPU
model against the CPU model, and the routing switch."""
import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.presets import get_preset
from test_deepseek_v3_gpu import _cpu_model_run  # the shared CPU reference run

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 8   # decode steps in _cpu_model_run


@pytest.mark.parametrize("mfma", (True, False), ids=("mfma", "no_mla_mfma"))
@pytest.mark.parametrize("fuse", (True, False), ids=("fused", "no_decode_fuse"))
def test_debug_v3_decodes_through_mla_decode(fuse, mfma, monkeypatch):
    for name, on in (("MLXS_AMD_NO_DECODE_FUSE", fuse),
                     ("MLXS_AMD_NO_MLA_MFMA", mfma)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "1")
    sd, ids, toks, rows = _cpu_model_run()
    cfg = get_preset("debug-deepseek-v3")
    m = get_model_class("deepseek_v3")(cfg, cfg.shard(0, cfg.num_hidden_layers))
    m.load_weights(sd)
    m = m.to(DEV).eval()
    cache = m.make_cache(batch_size=2)

    calls = []
    real = ops.hip_ext().mla_decode

    def spy(*args, **kwargs):
        calls.append(args[0].shape)
        return real(*args, **kwargs)

    monkeypatch.setattr(ops.hip_ext(), "mla_decode", spy)
    got = []
    with torch.no_grad():
        h = m(ids.to(DEV), cache)
        for t in toks:
            got.append(h[:, -1].float().cpu())
            h = m(t[:, None].to(DEV), cache)
        got.append(h[:, -1].float().cpu())
    assert len(calls) == (STEPS * cfg.num_hidden_layers if mfma else 0)
    for step, (a, b) in enumerate(zip(got, rows)):
        err = (a - b).abs().max().item()
        scale = b.abs().max().item()
        print(f"step {step}: err {err:.3e} scale {scale:.3f}")
        assert err <= 6e-2 + 1e-2 * scale, (step, err, scale)
