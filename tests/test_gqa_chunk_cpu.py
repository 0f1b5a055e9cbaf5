"""ops.gqa_chunk_route's truth table, and ops.gqa_chunk / ops.gqa_chunk_fp8 on
CPU tensors."""
import types

import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref


@pytest.fixture
def stub_ext(monkeypatch):
    stub = types.SimpleNamespace(
        gqa_chunk_shape_ok=lambda g, dk, dv: 1 <= g <= 16 and dk == dv
        and dk in (64, 128))
    monkeypatch.setattr(ops, "hip_ext", lambda: stub)


# (G, D, batch, hkv, T, S)
LLAMA8 = (4, 128, 1, 8, 16, 4112)


@pytest.mark.parametrize("env,shape,want", [
    ("0", LLAMA8, False),
    ("1", LLAMA8, True),
    ("1", (1, 64, 64, 2, 2, 3), True),                  # any served shape
    ("1", (4, 128, 1, 8, 16, 16), False),               # S == T: cold prefill
    ("1", (4, 256, 1, 8, 16, 4112), False),             # no instantiation
    ("1", (17, 128, 1, 8, 16, 4112), False),
    ("1", LLAMA8 + (True,), False),                     # device position
    (None, LLAMA8, True),
    (None, (8, 64, 8, 4, 64, 576), True),
    (None, (7, 128, 1, 4, 4, 516), True),
    (None, (7, 128, 1, 4, 4, 515), False),              # prefix 511
    (None, (4, 128, 1, 8, 65, 4161), False),            # T above it
    (None, (4, 128, 9, 8, 16, 4112), False),            # batch above it
    (None, (4, 64, 1, 4, 16, 4112), False),             # shape not measured
])
def test_route_truth_table(stub_ext, monkeypatch, env, shape, want):
    if env is None:
        monkeypatch.delenv("MLXS_AMD_GQA_CHUNK", raising=False)
    else:
        monkeypatch.setenv("MLXS_AMD_GQA_CHUNK", env)
    assert ops.gqa_chunk_route(*shape) is want


def test_route_rejects_other_values_and_needs_the_ext(stub_ext, monkeypatch):
    monkeypatch.setenv("MLXS_AMD_GQA_CHUNK", "yes")
    with pytest.raises(ValueError, match="MLXS_AMD_GQA_CHUNK"):
        ops.gqa_chunk_route(*LLAMA8)
    monkeypatch.setenv("MLXS_AMD_GQA_CHUNK", "1")
    monkeypatch.setattr(ops, "hip_ext", lambda: None)
    assert ops.gqa_chunk_route(*LLAMA8) is False


@pytest.mark.parametrize("T", (1, 3, 7))
def test_cpu_ops_are_the_reference_over_the_prefix(T):
    B, Hq, Hkv, D, S, cap = 2, 6, 2, 64, 7, 9
    g = torch.Generator().manual_seed(T)
    q = torch.randn(B, T, Hq, D, generator=g).bfloat16().transpose(1, 2)
    k = torch.randn(B, Hkv, cap, D, generator=g).bfloat16()
    v = torch.randn(B, Hkv, cap, D, generator=g).bfloat16()
    want = ref.attention(q, k[:, :, :S], v[:, :, :S], 0.25,
                         causal_offset=S - T)
    got = ops.gqa_chunk(q, k[:, :, :S], v[:, :, :S], 0.25)
    assert got.shape == (B, Hq, T, D)
    torch.testing.assert_close(got, want)
    (k8, ks), (v8, vs) = ref.kv_fp8_quantize(k), ref.kv_fp8_quantize(v)
    kd = ref.kv_fp8_dequantize(k8[:, :, :S], ks[:, :, :S])
    vd = ref.kv_fp8_dequantize(v8[:, :, :S], vs[:, :, :S])
    got8 = ops.gqa_chunk_fp8(q, k8, ks, v8, vs, 0.25, S)
    torch.testing.assert_close(
        got8, ref.attention(q, kd, vd, 0.25, causal_offset=S - T))
