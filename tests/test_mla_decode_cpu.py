"""ops.mla_decode on CPU tensors is ops.attention on the concatenated q."""
import pytest
import torch

from mlx_sharding_amd import ops


@pytest.mark.parametrize("pos", (None, [4], [0, 6, 3]),
                         ids=("host", "shared", "ragged"))
def test_cpu_mla_decode_is_attention_on_cat_q(pos):
    B, Hq, rank, rope, S = 3, 4, 16, 8, 7
    g = torch.Generator().manual_seed(3)
    q_nope = torch.randn(Hq, B, rank, generator=g).transpose(0, 1)
    q_rope = torch.randn(B, Hq, rope, generator=g)
    kv = torch.randn(B, 1, S, rank + rope, generator=g)
    p = None if pos is None else torch.tensor(pos, dtype=torch.int32)
    got = ops.mla_decode(q_nope, q_rope, kv, rank, 0.25, p)
    q = torch.cat([q_nope, q_rope], dim=-1).unsqueeze(2)
    want = ops.attention(q, kv, kv[..., :rank], 0.25, causal_offset=S - 1,
                         pos_dev=p)
    assert got.shape == (Hq, B, rank)
    torch.testing.assert_close(got, want[:, :, 0].transpose(0, 1))
    if pos is not None and len(pos) == B:
        # row 0 attends over its own single key: the V row itself
        torch.testing.assert_close(got[:, 0], kv[0, 0, :1, :rank].expand(Hq, -1))
