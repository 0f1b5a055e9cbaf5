"""debug-deepseek-v3-fp8 with FP8 block-quantized weights: the GPU model
against the CPU model, teacher-forced prefill + 8 decode steps at B = 2,
within test_debug_v3_gpu_matches_cpu's 6e-2 + 1e-2 * max|ref|, in three
configurations: default, dq-cache disabled (memory-tight: the fp8 GEMV
carries the dense projections) and MLXS_AMD_NO_DECODE_FUSE=1.  Spies check
that the FP8 expert kernels ran on every MoE layer of every step."""

import functools

import pytest
import torch

from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.loading import make_quant_predicate, quantize_weights
from mlx_sharding_amd.utils.presets import get_preset

pytestmark = pytest.mark.gpu

DEV = "cuda"
PRESET = "debug-deepseek-v3-fp8"
F8 = torch.float8_e4m3fn


def _fp8_model(sd, cfg):
    cls = get_model_class("deepseek_v3")
    m = cls(cfg, cfg.shard(0, cfg.num_hidden_layers),
            quant_for=make_quant_predicate(cfg, sd))
    m.load_weights(sd)
    return m.eval()


@functools.lru_cache(maxsize=None)
def _cpu_model_run():
    """The preset with load-time FP8 weights on the CPU: prefill + 8 greedy
    decode steps.  Returns (fp8 state dict, config, ids, tokens, logits)."""
    dense_cfg = get_preset(PRESET)
    assert dense_cfg.hidden_size == 256 and \
        dense_cfg["moe_intermediate_size"] == 128
    dense = init_model(get_model_class("deepseek_v3"), dense_cfg,
                       dense_cfg.shard(0, dense_cfg.num_hidden_layers), seed=13)
    sd = {k: v.clone() for k, v in dense.state_dict().items()}
    cfg = get_preset(PRESET)
    quantize_weights(sd, cfg, fmt="fp8")
    assert cfg.quantization == get_preset(PRESET, fp8=True).quantization
    m = _fp8_model(sd, cfg)
    assert m.model.layers["1"].mlp.switch_mlp.gate_proj.weight.dtype == F8
    ids = torch.randint(0, cfg.vocab_size, (2, 7),
                        generator=torch.Generator().manual_seed(2))
    cache = m.make_cache(batch_size=2)
    rows, toks = [], []
    with torch.no_grad():
        h = m(ids, cache)
        for _ in range(8):
            rows.append(h[:, -1].float())
            toks.append(h[:, -1].argmax(-1))
            h = m(toks[-1][:, None], cache)
        rows.append(h[:, -1].float())
    return sd, cfg, ids, toks, rows


class _Spy:
    """Counts calls into the HIP extension by name."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn

        def wrapped(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return wrapped


@pytest.mark.parametrize("mode", ("default", "no_dq_cache", "no_decode_fuse"))
def test_debug_v3_fp8_gpu_matches_cpu(mode, monkeypatch):
    monkeypatch.delenv("MLXS_AMD_NO_DECODE_FUSE", raising=False)
    monkeypatch.delenv("MLXS_AMD_NO_DQ_CACHE", raising=False)
    monkeypatch.delenv("MLXS_AMD_MOE_RESIDENT", raising=False)
    if mode == "no_dq_cache":
        monkeypatch.setenv("MLXS_AMD_NO_DQ_CACHE", "1")
    if mode == "no_decode_fuse":
        monkeypatch.setenv("MLXS_AMD_NO_DECODE_FUSE", "1")
    sd, cfg, ids, toks, rows = _cpu_model_run()
    m = _fp8_model(sd, cfg).to(DEV)
    assert m._use_absorbed()
    cache = m.make_cache(batch_size=2)
    assert all(c.n_kv_heads == 1 for c in cache)
    assert m.cache_specs()[0] == (1, 64 + 16, 0)

    real = ops.hip_ext()
    assert real is not None, "HIP extension not built"
    spy = _Spy(real)
    monkeypatch.setattr(ops, "_EXT", spy)
    n_moe = cfg.num_hidden_layers - 1
    got, per_step = [], []
    with torch.no_grad():
        h = m(ids.to(DEV), cache)
        for t in toks:
            got.append(h[:, -1].float().cpu())
            spy.calls.clear()
            h = m(t[:, None].to(DEV), cache)
            per_step.append(list(spy.calls))
        got.append(h[:, -1].float().cpu())
    for calls in per_step:
        gu = calls.count("moe_fp8f16_gateup") + \
            calls.count("moe_fp8f16_gateup_acc")
        assert gu == n_moe and calls.count("moe_fp8f16_down") == n_moe, calls
        if mode == "no_decode_fuse":
            assert calls.count("moe_fp8f16_gateup_acc") == 0
        else:
            assert calls.count("moe_fp8f16_gateup_acc") == n_moe
        assert not any(c.startswith(("moe_w4", "moe_gateup", "moe_down"))
                       for c in calls)
        if mode == "no_dq_cache":
            assert calls.count("fp8f16_gemv") >= 4 * cfg.num_hidden_layers
        else:
            assert "fp8f16_gemv" not in calls
    for step, (a, b) in enumerate(zip(got, rows)):
        err = (a - b).abs().max().item()
        scale = b.abs().max().item()
        print(f"{mode} step {step}: err {err:.3e} scale {scale:.3f}")
        assert err <= 6e-2 + 1e-2 * scale, (step, err, scale)
