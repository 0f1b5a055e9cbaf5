"""The 16-head MFMA absorbed-MLA decode kernel against the fp32 reference.
At (80, 64) wave 3 has no QK k-step and each wave owns one column tile."""
import functools

import pytest
import torch

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV, CAP, Hq = "cuda", 1024, 16
# one key, both sides of a tile edge, several split-S slices, odd tail
LENGTHS = (1, 31, 32, 33, 257, 700)
ext = ops.hip_ext


@functools.lru_cache(maxsize=None)
def _case(Dk, Dv, B):
    """Seeded inputs, the model's q views, fp32 reference per length."""
    g = torch.Generator().manual_seed(Dk + B)
    q = torch.randn(B, Hq, 1, Dk, generator=g).to(torch.bfloat16)
    kbuf = (torch.randn(B, 1, CAP, Dk, generator=g) * 0.5).to(torch.bfloat16)
    scale = Dk ** -0.5
    want = {}
    for L in LENGTHS:
        k = kbuf[:, :, :L].float()
        want[L] = ref.attention(q.float(), k, k[..., :Dv].contiguous(), scale,
                                causal_offset=L - 1)[:, :, 0]
    qd = q.to(DEV)
    qn = qd[:, :, 0, :Dv].permute(1, 0, 2).contiguous().transpose(0, 1)
    return qn, qd[:, :, 0, Dv:].contiguous(), kbuf, scale, want


def _check(got, want, kbuf, lens):
    got = got.permute(1, 0, 2).float().cpu()                  # [B, Hq, Dv]
    assert torch.isfinite(got).all()
    for b, L in enumerate(lens):
        v = kbuf[b, 0, :L, :got.shape[-1]].float()
        bound = 2.0 ** -7 * v.abs().max().item()
        err = (got[b] - want[L][b]).abs().max().item()
        print(f"b={b} L={L}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (b, L, err, bound)
        if L == 1:  # softmax over one key: the V row itself, bit for bit
            assert torch.equal(got[b], v.expand_as(got[b]))


@pytest.mark.parametrize("mode", ("host", "shared", "ragged"))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("Dk,Dv", ((576, 512), (80, 64)))
def test_mla_decode16_matches_reference(Dk, Dv, B, mode):
    qn, qr, kbuf, scale, want = _case(Dk, Dv, B)
    if mode == "ragged":
        rows = [(LENGTHS * 2)[i:i + B] for i in range(0, len(LENGTHS), B)]
    else:
        rows = [(L,) * B for L in LENGTHS]
    if mode != "host":  # capacity slices: every length runs the combiner
        assert ext().mla_decode_nsplit(B, Hq, CAP) > 1
    for lens in rows:
        k, pos = kbuf.to(DEV).clone(), None
        for b, L in enumerate(lens):  # NaN in every row a batch row must not use
            k[b, :, L:] = float("nan")
        if mode == "host":
            k = k[:, :, :lens[0]]
        else:
            pos = torch.tensor([L - 1 for L in lens], dtype=torch.int32,
                               device=DEV)[:B if mode == "ragged" else 1]
        got = ops.mla_decode(qn, qr, k, Dv, scale, pos)
        assert got.shape == (Hq, B, Dv) and got.is_contiguous()
        _check(got, want, kbuf, lens)


def test_mla_decode16_graph_replays_match_eager():
    qn, qr, kbuf, scale, _ = _case(576, 512, 3)
    k = kbuf.to(DEV)
    pos = torch.tensor([0, 32, 699], dtype=torch.int32, device=DEV)
    ops.mla_decode(qn, qr, k, 512, scale, pos)  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.mla_decode(qn, qr, k, 512, scale, pos)
    for p in ([0, 32, 699], [256, 5, 31]):
        pos.copy_(torch.tensor(p, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.mla_decode(qn, qr, k, 512, scale, pos)), p
