"""debug-deepseek-h16 (16 heads, rows (80, 64)) decoding through the 16-head
MFMA kernel: the GPU model against the CPU model, and the routing switch."""
import functools

import pytest
import torch

from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.presets import get_preset

pytestmark = pytest.mark.gpu
DEV, STEPS = "cuda", 8


@functools.lru_cache(maxsize=None)
def _cpu_model_run():
    """CPU prefill + STEPS greedy decode steps."""
    cfg = get_preset("debug-deepseek-h16")
    m = init_model(get_model_class("deepseek_v2"), cfg,
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


@pytest.mark.parametrize("mfma", (True, False), ids=("mfma", "no_mla_mfma"))
@pytest.mark.parametrize("fuse", (True, False), ids=("fused", "no_decode_fuse"))
def test_debug_h16_decodes_through_mla_decode(fuse, mfma, monkeypatch):
    for name, on in (("MLXS_AMD_NO_DECODE_FUSE", fuse),
                     ("MLXS_AMD_NO_MLA_MFMA", mfma)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "1")
    cfg, sd, ids, toks, rows = _cpu_model_run()
    m = get_model_class("deepseek_v2")(cfg, cfg.shard(0, cfg.num_hidden_layers))
    m.load_weights(sd)
    m = m.to(DEV).eval()
    cache = m.make_cache(batch_size=2)
    calls = []
    real = ops.hip_ext().mla_decode
    monkeypatch.setattr(ops.hip_ext(), "mla_decode",
                        lambda *a, **kw: calls.append(1) or real(*a, **kw))
    got = []
    with torch.no_grad():
        h = m(ids.to(DEV), cache)
        for t in toks:
            got.append(h[:, -1].float().cpu())
            h = m(t[:, None].to(DEV), cache)
        got.append(h[:, -1].float().cpu())
    assert len(calls) == (STEPS * cfg.num_hidden_layers if mfma else 0)
    for step, (a, b) in enumerate(zip(got, rows)):
        err, scale = (a - b).abs().max().item(), b.abs().max().item()
        print(f"step {step}: err {err:.3e} scale {scale:.3f}")
        assert err <= 6e-2 + 1e-2 * scale, (step, err, scale)
