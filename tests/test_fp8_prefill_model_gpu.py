"""debug-deepseek-v3-fp8 prefill through the packed wide-tile FP8 expert
kernels: GPU last-position logits against the CPU model within
test_fp8_model_gpu.py's 6e-2 + 1e-2 * max|ref|, with the dq-cache disabled
(MLXS_AMD_NO_DQ_CACHE=1), with no budget (MLXS_AMD_DQ_CACHE_GB=0) and with
MLXS_AMD_FP8_PREFILL=packed; each error is printed beside the dense route's
(MLXS_AMD_FP8_PREFILL=dense).  A spy on the extension checks which route
ran on every MoE layer.

Prefill only, B = 2, T = 65.  The MoE block sends up to 128 tokens through
the fused gate and the 16-token kernels whatever the pair count, so the
prompt has to exceed 128 tokens to reach ops.grouped_expert_mlp_fp8 at all:
130 tokens x top-4 = 520 pairs >= 256.
"""

import functools

import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.utils.presets import get_preset
from test_fp8_model_gpu import DEV, PRESET, _fp8_model, _cpu_model_run

pytestmark = pytest.mark.gpu

B, T = 2, 65
ENVS = ("MLXS_AMD_NO_DQ_CACHE", "MLXS_AMD_DQ_CACHE_GB", "MLXS_AMD_FP8_PREFILL",
        "MLXS_AMD_NO_DECODE_FUSE", "MLXS_AMD_MOE_RESIDENT")
MODES = {
    "no_dq_cache": {"MLXS_AMD_NO_DQ_CACHE": "1"},
    "dq_cache_0gb": {"MLXS_AMD_DQ_CACHE_GB": "0"},
    "forced_packed": {"MLXS_AMD_FP8_PREFILL": "packed"},
    "forced_dense": {"MLXS_AMD_FP8_PREFILL": "dense"},
    "default": {},
}


class _Spy:
    """Records (name, dims of the first tensor argument) of every call into
    the HIP extension."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not callable(fn):
            return fn

        def wrapped(*a, **k):
            dims = next((t.dim() for t in a if isinstance(t, torch.Tensor)),
                        None)
            self.calls.append((name, dims))
            return fn(*a, **k)
        return wrapped

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


@functools.lru_cache(maxsize=None)
def _cpu_prefill():
    """(fp8 state dict, config, ids, last-position logits of the CPU model)."""
    sd, cfg = _cpu_model_run()[:2]
    assert cfg["num_experts_per_tok"] == 4
    m = _fp8_model(sd, cfg)
    ids = torch.randint(0, cfg.vocab_size, (B, T),
                        generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = m(ids, m.make_cache(batch_size=B))[:, -1].float()
    assert ids.numel() * 4 >= ops._MOE_GEMM_MIN_N and ids.numel() > 128
    return sd, cfg, ids, ref


def _gpu_prefill(mode, monkeypatch):
    """(error against the CPU model, scale, spy) of one GPU prefill."""
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    for name, val in MODES[mode].items():
        monkeypatch.setenv(name, val)
    sd, cfg, ids, ref = _cpu_prefill()
    m = _fp8_model(sd, cfg).to(DEV)
    real = ops.hip_ext()
    assert real is not None, "HIP extension not built"
    spy = _Spy(real)
    monkeypatch.setattr(ops, "_EXT", spy)
    with torch.no_grad():
        got = m(ids.to(DEV), m.make_cache(batch_size=B))[:, -1].float().cpu()
    monkeypatch.setattr(ops, "_EXT", real)
    return (got - ref).abs().max().item(), ref.abs().max().item(), spy


_dense_err = {}


def _dense_route_error(monkeypatch):
    if "err" not in _dense_err:
        _dense_err["err"] = _gpu_prefill("forced_dense", monkeypatch)[0]
    return _dense_err["err"]


@pytest.mark.parametrize("mode", ("no_dq_cache", "dq_cache_0gb",
                                  "forced_packed"))
def test_prefill_runs_packed(mode, monkeypatch):
    cfg = get_preset(PRESET)
    n_moe = cfg.num_hidden_layers - 1
    dense_err = _dense_route_error(monkeypatch)
    err, scale, spy = _gpu_prefill(mode, monkeypatch)
    print(f"{mode}: err {err:.3e} (dense route {dense_err:.3e}) "
          f"scale {scale:.3f}")
    assert spy.count("moe_fp8f16_gateup_wide") == n_moe, spy.calls
    assert spy.count("moe_fp8f16_down_wide") == n_moe, spy.calls
    assert spy.count("moe_scatter_rows") == 0
    assert spy.count("moe_gather_reduce") == 0
    assert ("fp8_block_dequant", 3) not in spy.calls
    assert not any(n in ("moe_fp8f16_gateup", "moe_fp8f16_gateup_acc",
                         "moe_fp8f16_down") for n, _ in spy.calls)
    assert err <= 6e-2 + 1e-2 * scale, (err, scale)


@pytest.mark.parametrize("mode", ("default", "forced_dense"))
def test_prefill_keeps_dense_route(mode, monkeypatch):
    """Budget to spare (or the dense route forced): the batched-GEMM route
    as before, no wide call."""
    cfg = get_preset(PRESET)
    n_moe = cfg.num_hidden_layers - 1
    err, scale, spy = _gpu_prefill(mode, monkeypatch)
    print(f"{mode}: err {err:.3e} scale {scale:.3f}")
    assert spy.count("moe_scatter_rows") == n_moe, spy.calls
    assert spy.count("moe_gather_reduce") == n_moe, spy.calls
    assert spy.count("moe_fp8f16_gateup_wide") == 0
    assert spy.count("moe_fp8f16_down_wide") == 0
    assert err <= 6e-2 + 1e-2 * scale, (err, scale)


def test_unknown_value_raises(monkeypatch):
    for name in ENVS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MLXS_AMD_FP8_PREFILL", "fast")
    sd, cfg, ids, _ = _cpu_prefill()
    m = _fp8_model(sd, cfg).to(DEV)
    with torch.no_grad(), pytest.raises(ValueError,
                                        match="MLXS_AMD_FP8_PREFILL"):
        m(ids.to(DEV), m.make_cache(batch_size=B))
