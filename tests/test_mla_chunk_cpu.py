"""The absorbed chunk route's predicate, and ops.mla_chunk on CPU tensors."""
import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.models.deepseek_v2 import MLA_CHUNK_MAX_T, mla_chunk_route
from mlx_sharding_amd.ops import reference as ref

ON = dict(native=True, graph_pos=None, offset=20, T=5, served=True,
          enabled=True)


@pytest.mark.parametrize("change,taken", [
    ({}, True),
    ({"T": 2}, True),
    ({"T": MLA_CHUNK_MAX_T}, True),
    ({"T": 1}, False),                      # decode keeps its own kernels
    ({"offset": 0}, False),                 # cold prompt: expanded prefill
    ({"T": MLA_CHUNK_MAX_T + 1}, False),
    ({"served": False}, False),             # e.g. a 4-head debug model
    ({"enabled": False}, False),            # MLXS_AMD_NO_MLA_CHUNK=1
    ({"graph_pos": torch.zeros(1, dtype=torch.int32)}, False),
    ({"native": False}, False),             # CPU / MLXS_AMD_FORCE_TORCH
])
def test_route_predicate(change, taken):
    assert mla_chunk_route(**{**ON, **change}) is taken


def test_switch_and_unserved_heads(monkeypatch):
    monkeypatch.delenv("MLXS_AMD_NO_MLA_CHUNK", raising=False)
    assert ops.mla_chunk_enabled()
    monkeypatch.setenv("MLXS_AMD_NO_MLA_CHUNK", "1")
    assert not ops.mla_chunk_enabled()
    assert not ops.mla_chunk_shape_ok(4, 64, 16)


@pytest.mark.parametrize("P,T", [(0, 3), (9, 4)])
def test_cpu_mla_chunk_is_per_token_attention(P, T):
    B, Hq, rank, rope = 2, 4, 16, 8
    g = torch.Generator().manual_seed(P + T)
    q_nope = torch.randn(B, T, Hq, rank, generator=g)
    q_rope = torch.randn(B, T, Hq, rope, generator=g)
    kv = torch.randn(B, 1, P + T, rank + rope, generator=g)
    got = ops.mla_chunk(q_nope, q_rope, kv, rank, 0.25)
    assert got.shape == (B, T, Hq, rank)
    for t in range(T):  # token t over its own prefix, no mask involved
        q = torch.cat([q_nope[:, t], q_rope[:, t]], dim=-1).unsqueeze(2)
        k = kv[:, :, :P + t + 1]
        want = ref.attention(q, k, k[..., :rank], 0.25, causal_offset=P + t)
        torch.testing.assert_close(got[:, t], want[:, :, 0])
