"""debug-deepseek-v3-fp8 (hidden 256, expert inner 128) with affine w4/w8
weights, prefill at B = 2, T = 65 (520 token-expert pairs): which expert
route ran on every MoE layer, and last-position logits against the same
quantized model on the CPU.  The yardstick is the parent's dense route,
measured in the same test: packed error <= 2 x dense error + 1e-3.
Measured on an MI355X: packed 9.8e-04, dense 7.3e-04, both formats."""

import functools

import pytest
import torch

from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.utils.loading import quantize_weights
from mlx_sharding_amd.utils.presets import get_preset
from test_fp8_model_gpu import DEV, PRESET, _fp8_model as _model
from test_fp8_prefill_model_gpu import _Spy

pytestmark = pytest.mark.gpu

B, T = 2, 65
ENVS = ("MLXS_AMD_NO_DQ_CACHE", "MLXS_AMD_DQ_CACHE_GB", "MLXS_AMD_W4_PREFILL",
        "MLXS_AMD_NO_FUSED_ROUTE", "MLXS_AMD_MOE_RESIDENT")
PACKED = ({"MLXS_AMD_NO_DQ_CACHE": "1"}, {"MLXS_AMD_DQ_CACHE_GB": "0"},
          {"MLXS_AMD_W4_PREFILL": "packed"})
DENSE = ({"MLXS_AMD_W4_PREFILL": "dense"}, {})


@functools.lru_cache(maxsize=None)
def _cpu_prefill(bits, gs):
    """(state dict, config, ids, last-position logits of the CPU model)."""
    cfg = get_preset(PRESET)
    dense = init_model(get_model_class("deepseek_v3"), cfg,
                       cfg.shard(0, cfg.num_hidden_layers), seed=13)
    sd = {k: v.clone() for k, v in dense.state_dict().items()}
    quantize_weights(sd, cfg, group_size=gs, bits=bits)
    m = _model(sd, cfg)
    ids = torch.randint(0, cfg.vocab_size, (B, T),
                        generator=torch.Generator().manual_seed(5))
    assert ids.numel() * cfg["num_experts_per_tok"] >= ops._MOE_GEMM_MIN_N
    with torch.no_grad():
        return sd, cfg, ids, m(ids, m.make_cache(batch_size=B))[:, -1].float()


def _gpu_prefill(quant, env, monkeypatch):
    """(error against the CPU model, extension spy, torch helpers called)."""
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    sd, cfg, ids, ref = _cpu_prefill(*quant)
    m = _model(sd, cfg).to(DEV)
    spy, helpers = _Spy(ops.hip_ext()), []
    with monkeypatch.context() as mp:
        mp.setattr(ops, "_EXT", spy)
        for name in ("expert_dequant", "make_expert_subranges"):
            real = getattr(ops, name)
            mp.setattr(ops, name, lambda *a, _n=name, _f=real, **k:
                       helpers.append(_n) or _f(*a, **k))
        with torch.no_grad():
            got = m(ids.to(DEV), m.make_cache(batch_size=B))[:, -1]
    return (got.float().cpu() - ref).abs().max().item(), spy, helpers


@pytest.mark.parametrize("quant", ((4, 64), (8, 128)), ids=("w4", "w8"))
def test_prefill_routes_and_accuracy(quant, monkeypatch):
    n_moe = _cpu_prefill(*quant)[1].num_hidden_layers - 1
    dense_err = None
    for env in DENSE + PACKED:
        err, spy, helpers = _gpu_prefill(quant, env, monkeypatch)
        wide = (spy.count("moe_w4f16_gateup_wide"),
                spy.count("moe_w4f16_down_wide"))
        gemm = (spy.count("moe_scatter_rows"), spy.count("moe_gather_reduce"))
        print("%r %r: max |logit error| %.2e" % (quant, env, err))
        if env in DENSE:  # as on the parent
            assert wide == (0, 0) and gemm == (n_moe, n_moe), (env, spy.calls)
            dense_err = err if dense_err is None else dense_err
        else:
            assert wide == (n_moe, n_moe) and gemm == (0, 0), (env, spy.calls)
            assert helpers == [], (env, helpers)
            assert err <= 2 * dense_err + 1e-3, (env, err, dense_err)


def test_unknown_value_raises(monkeypatch):
    monkeypatch.setenv("MLXS_AMD_W4_PREFILL", "fast")
    sd, cfg, ids, _ = _cpu_prefill(4, 64)
    m = _model(sd, cfg).to(DEV)
    with torch.no_grad(), pytest.raises(ValueError,
                                        match="MLXS_AMD_W4_PREFILL"):
        m(ids.to(DEV), m.make_cache(batch_size=B))
