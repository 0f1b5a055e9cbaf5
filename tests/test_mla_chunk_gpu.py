"""The MFMA absorbed-MLA chunk kernel (mla_chunk.hip) against the fp32
reference: T new tokens attending causally over the compressed cache."""
import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 1024
# (prefix P, new tokens T): pure causal; odd; limits 15..18 straddle a tile
# edge inside one block; 80 rows at 16 heads (partial last block); limits
# 255..258 straddle the 256-key slice edge (an empty partial); several slices
CHUNKS = ((0, 2), (1, 3), (14, 4), (30, 5), (254, 4), (700, 7))
SHAPES = [(16, 576, 512), (128, 576, 512), (32, 80, 64), (16, 80, 64)]
ext = ops.hip_ext


def _case(Hq, Dk, Dv, B, P, T):
    """Seeded CPU inputs (a different q per token and head) and the fp32
    reference [B, T, Hq, Dv] on the bf16 inputs."""
    g = torch.Generator().manual_seed(Hq * 11 + Dk + B + 7 * P + T)
    q = torch.randn(B, Hq, T, Dk, generator=g).to(torch.bfloat16)
    kbuf = (torch.randn(B, 1, CAP, Dk, generator=g) * 0.5).to(torch.bfloat16)
    k = kbuf[:, :, :P + T].float()
    want = ref.attention(q.float(), k, k[..., :Dv].contiguous(), Dk ** -0.5,
                         causal_offset=P).transpose(1, 2)
    return q, kbuf, want


@pytest.mark.parametrize("P,T", CHUNKS)
@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("Hq,Dk,Dv", SHAPES)
def test_mla_chunk_matches_reference(Hq, Dk, Dv, B, P, T):
    assert ext().mla_chunk_shape_ok(Hq, Dk, Dv)
    S = P + T
    if P == 254:
        assert ext().mla_chunk_nsplit(B, T * Hq, S) > 1
    q_c, kbuf, want = _case(Hq, Dk, Dv, B, P, T)
    q = q_c.to(DEV)
    # q_nope as the model passes it: a permuted view of the head-major bmm
    # result [Hq, B*T, Dv]
    q_abs = q[..., :Dv].permute(1, 0, 2, 3).reshape(Hq, B * T, Dv).contiguous()
    qn = q_abs.view(Hq, B, T, Dv).permute(1, 2, 0, 3)
    qr = q[..., Dv:].transpose(1, 2).contiguous()
    k = kbuf.to(DEV).clone()
    k[:, :, S:] = float("nan")  # rows the kernel must not use
    got = ops.mla_chunk(qn, qr, k[:, :, :S], Dv, Dk ** -0.5)
    assert got.shape == (B, T, Hq, Dv) and got.is_contiguous()
    got = got.float().cpu()
    assert torch.isfinite(got).all()
    for b in range(B):
        v = kbuf[b, 0, :S, :Dv].float()
        bound = 2.0 ** -7 * v.abs().max().item()
        err = (got[b] - want[b]).abs().max().item()
        print(f"b={b} P={P} T={T}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (b, err, bound)
        if P == 0:  # token 0 sees one key: the V row itself, bit for bit
            assert torch.equal(got[b, 0], v[0].expand_as(got[b, 0]))


def test_mla_chunk_binding_limits():
    def call(Hq=32, Hkv=1, dtype=torch.bfloat16, T=3, S=8):
        qn = torch.zeros(2, T, Hq, 64, device=DEV, dtype=dtype)
        qr = torch.zeros(2, T, Hq, 16, device=DEV, dtype=dtype)
        kv = torch.zeros(2, Hkv, S, 80, device=DEV, dtype=dtype)
        return ext().mla_chunk(qn, qr, kv, 64, 0.1)

    assert call().shape == (2, 3, 32, 64)
    with pytest.raises(RuntimeError, match="Hkv"):
        call(Hkv=2)
    with pytest.raises(RuntimeError, match="bf16"):
        call(dtype=torch.float16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        call(Hq=48)
    with pytest.raises(RuntimeError, match="new tokens"):
        call(T=9)
    torch.cuda.synchronize()
