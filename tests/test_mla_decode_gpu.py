"""The MFMA absorbed-MLA decode kernel (mla_decode.hip) against the fp32
reference, at every head count and both row geometries it serves."""
import functools

import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 1024
# one key, both sides of a tile edge, several split-S slices, odd tail
LENGTHS = (1, 31, 32, 33, 257, 700)
SHAPES = [(32, 576, 512), (64, 576, 512), (128, 576, 512), (32, 80, 64)]
ext = ops.hip_ext


@functools.lru_cache(maxsize=None)
def _case(Hq, Dk, Dv, B):
    """Seeded CPU inputs (a different q per head) and, per length, the fp32
    reference [B, Hq, Dv] on the bf16 inputs."""
    g = torch.Generator().manual_seed(Hq * 11 + Dk + B)
    q = torch.randn(B, Hq, 1, Dk, generator=g).to(torch.bfloat16)
    kbuf = (torch.randn(B, 1, CAP, Dk, generator=g) * 0.5).to(torch.bfloat16)
    scale = Dk ** -0.5
    want = {}
    for L in LENGTHS:
        k = kbuf[:, :, :L].float()
        want[L] = ref.attention(q.float(), k, k[..., :Dv].contiguous(), scale,
                                causal_offset=L - 1)[:, :, 0]
    return q, kbuf, scale, want


def _views(q, Dv):
    """q as the model passes it: the transposed head-major bmm result
    [Hq, B, Dv] and a separate rope tensor [B, Hq, rope]."""
    q_abs = q[:, :, 0, :Dv].permute(1, 0, 2).contiguous()
    return q_abs.transpose(0, 1), q[:, :, 0, Dv:].contiguous()


def _poisoned(kbuf, lens):
    """Device copy of the cache, NaN in every row a batch row must not use."""
    k = kbuf.to(DEV).clone()
    for b, L in enumerate(lens):
        k[b, :, L:] = float("nan")
    return k


def _check(got, want, kbuf, lens):
    got = got.permute(1, 0, 2).float().cpu()                  # [B, Hq, Dv]
    assert torch.isfinite(got).all()
    Dv = got.shape[-1]
    for b, L in enumerate(lens):
        v = kbuf[b, 0, :L, :Dv].float()
        bound = 2.0 ** -7 * v.abs().max().item()
        err = (got[b] - want[L][b]).abs().max().item()
        print(f"b={b} L={L}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (b, L, err, bound)
        if L == 1:  # softmax over one key: the V row itself, bit for bit
            assert torch.equal(got[b], v.expand_as(got[b]))


@pytest.mark.parametrize("mode", ("host", "shared", "ragged"))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("Hq,Dk,Dv", SHAPES)
def test_mla_decode_matches_reference(Hq, Dk, Dv, B, mode):
    assert ext().mla_decode_shape_ok(Hq, Dk, Dv)
    q_c, kbuf, scale, want = _case(Hq, Dk, Dv, B)
    qn, qr = _views(q_c.to(DEV), Dv)
    if mode == "ragged":
        rows = [(LENGTHS * 2)[i:i + B] for i in range(0, len(LENGTHS), B)]
    else:
        rows = [(L,) * B for L in LENGTHS]
    if mode != "host":  # capacity slices: every length runs the combiner
        assert ext().mla_decode_nsplit(B, Hq, CAP) > 1
    for lens in rows:
        k, pos = _poisoned(kbuf, lens), None
        if mode == "host":
            k = k[:, :, :lens[0]]
        else:
            pos = torch.tensor([L - 1 for L in lens][:B if mode == "ragged"
                                                     else 1],
                               dtype=torch.int32, device=DEV)
        got = ops.mla_decode(qn, qr, k, Dv, scale, pos)
        assert got.shape == (Hq, B, Dv) and got.is_contiguous()
        _check(got, want, kbuf, lens)


def test_mla_decode_graph_replays_match_eager():
    Hq, Dk, Dv, B = 64, 576, 512, 3
    q_c, kbuf, scale, _ = _case(Hq, Dk, Dv, B)
    qn, qr = _views(q_c.to(DEV), Dv)
    k = kbuf.to(DEV)
    pos = torch.tensor([0, 32, 699], dtype=torch.int32, device=DEV)
    ops.mla_decode(qn, qr, k, Dv, scale, pos)  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.mla_decode(qn, qr, k, Dv, scale, pos)
    for p in ([0, 32, 699], [256, 5, 31]):
        pos.copy_(torch.tensor(p, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.mla_decode(qn, qr, k, Dv, scale, pos)
        assert torch.equal(out, eager), p


def test_mla_decode_binding_limits():
    def call(Hq=32, Hkv=1, dtype=torch.bfloat16, npos=None, B=2):
        qn = torch.zeros(B, Hq, 64, device=DEV, dtype=dtype)
        qr = torch.zeros(B, Hq, 16, device=DEV, dtype=dtype)
        kv = torch.zeros(B, Hkv, 8, 80, device=DEV, dtype=dtype)
        pos = None if npos is None else torch.zeros(npos, dtype=torch.int32,
                                                    device=DEV)
        return ext().mla_decode(qn, qr, kv, 64, 0.1, pos)

    assert call().shape == (32, 2, 64)
    with pytest.raises(RuntimeError, match="Hkv"):
        call(Hkv=2)
    with pytest.raises(RuntimeError, match="bf16"):
        call(dtype=torch.float16)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        call(Hq=48)
    with pytest.raises(RuntimeError, match="pos must hold"):
        call(npos=3)
    torch.cuda.synchronize()
