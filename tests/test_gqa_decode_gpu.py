"""gqa_decode (the MFMA GQA flash-decode kernel) against the fp64 reference:
the probe cases of attn_cases.py whose shape it serves, shapes those cases
lack, graph capture and the binding's limits.  Cache rows at or beyond a
row's length are NaN in K and V.

The bound: P rounded to bf16 costs at most 2**-9 * max|V|, the bf16 output
another 2**-9 * max|V|, so a correct kernel stays under 2**-8 * max|V| and
attn_cases.BOUND allows 2**-7 * max|V| (the prefill argument of the
attn_cases docstring)."""
import pytest
import torch

import attn_cases as ac
from mlx_sharding_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ext = ops.hip_ext

RUNS = [r for r in ac.decode_runs()
        if not r[0].alias and ext() is not None
        and ext().gqa_decode_shape_ok(r[0].Hq // r[0].Hkv, r[0].Dk, r[0].Dv)]


def _poisoned(buf, lens):
    """Device copy of a cache with NaN in every row past each length."""
    d = buf.to(DEV).clone()
    for b, L in enumerate(lens):
        d[b, :, L:] = float("nan")
    return d


def _check(label, got, want, bound):
    got = got.float().cpu()
    assert torch.isfinite(got).all(), label
    ratio = ac.worst_ratio(got, want, bound)
    print(f"{label}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, (label, ratio)


def test_probe_selection():
    assert RUNS
    assert any(c.softcap > 0 for c, *_ in RUNS)
    assert any(c.window > 0 for c, *_ in RUNS)


@pytest.mark.parametrize(
    "run", RUNS, ids=[f"{c.name}-{mode}-{'_'.join(map(str, lens[:3]))}"
                      for c, mode, lens, _, _ in RUNS])
def test_gqa_decode_probes(run):
    c, mode, lens, _, _ = run
    q, kbuf, vbuf, scale = ac.decode_inputs(c.name, lens)
    want, _, bound = ac.decode_reference(c, lens)
    k, v = _poisoned(kbuf, lens), _poisoned(vbuf, lens)
    pos = None
    if mode == "host":
        k, v = k[:, :, :lens[0]], v[:, :, :lens[0]]
    else:
        n = c.B if mode == "ragged" else 1
        pos = torch.tensor([L - 1 for L in lens[:n]], dtype=torch.int32,
                           device=DEV)
    got = ext().gqa_decode(q.to(DEV), k, v, scale, c.softcap, c.window, pos)
    assert got.shape == (c.B, c.Hq, 1, c.Dv)
    got = got[:, :, 0]
    _check(f"gqa_decode {c.name} {mode} {lens[:3]}", got, want, bound)
    for b, L in enumerate(lens):
        if L == 1 or c.window == 1:  # one key: that V row, bit for bit
            row = vbuf[b, :, L - 1].repeat_interleave(c.Hq // c.Hkv, 0)
            assert torch.equal(got[b].cpu(), row), (c.name, mode, b, L)


@pytest.mark.parametrize("G,Hkv,Dk,Dv", [(16, 2, 128, 128), (2, 2, 256, 256),
                                         (12, 1, 64, 64), (8, 2, 128, 128)])
def test_gqa_decode_shapes(G, Hkv, Dk, Dv):
    """Head -> column map, k-step count and column tiling at shapes the
    probe cases lack."""
    B, cap, lens = 3, 512, (1, 33, 300)
    g = torch.Generator().manual_seed(G * 1000 + Dk)
    q = torch.randn(B, G * Hkv, 1, Dk, generator=g).to(ac.BF16)
    kbuf = torch.randn(B, Hkv, cap, Dk, generator=g).to(ac.BF16)
    vbuf = (torch.rand(B, Hkv, cap, Dv, generator=g) * 4 - 2).to(ac.BF16)
    scale = Dk ** -0.5
    pos = torch.tensor([L - 1 for L in lens], dtype=torch.int32, device=DEV)
    got = ext().gqa_decode(q.to(DEV), _poisoned(kbuf, lens),
                           _poisoned(vbuf, lens), scale, 0.0, 0, pos)[:, :, 0]
    for b, L in enumerate(lens):
        kb, vb = kbuf[b:b + 1, :, :L], vbuf[b:b + 1, :, :L]
        want, _ = ac.reference(q[b:b + 1], kb, vb, scale, [L - 1])
        _check(f"gqa_decode G{G} {Dk}x{Dv} L{L}", got[b:b + 1], want[:, :, 0],
               ac.bounds(vb, [L - 1], 1, 0))
    assert torch.equal(got[0].cpu(), vbuf[0, :, 0].repeat_interleave(G, 0))


def test_gqa_decode_graph_replay():
    """A captured ragged launch reads the positions at replay."""
    B, Hkv, G, D, cap = 3, 2, 4, 128, 1024
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, G * Hkv, 1, D, generator=g).to(ac.BF16).to(DEV)
    k = torch.randn(B, Hkv, cap, D, generator=g).to(ac.BF16).to(DEV)
    v = torch.randn(B, Hkv, cap, D, generator=g).to(ac.BF16).to(DEV)
    pos = torch.tensor([0, 254, 600], dtype=torch.int32, device=DEV)
    args = (q, k, v, D ** -0.5, 0.0, 0)
    ext().gqa_decode(*args, pos)  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext().gqa_decode(*args, pos)
    for new in ([257, 1023, 31], [512, 0, 700]):
        pos.copy_(torch.tensor(new, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ext().gqa_decode(*args, pos)), new


def test_gqa_decode_binding_limits():
    def bf(*shape):
        return torch.zeros(*shape, device=DEV, dtype=torch.bfloat16)

    with pytest.raises(RuntimeError, match="1 to 16 heads"):        # G = 17
        ext().gqa_decode(bf(1, 17, 1, 64), bf(1, 1, 8, 64), bf(1, 1, 8, 64),
                         0.1, 0.0, 0, None)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ext().gqa_decode(bf(1, 2, 1, 192), bf(1, 1, 8, 192), bf(1, 1, 8, 128),
                         0.1, 0.0, 0, None)
    kv = bf(1, 1, 8, 128)
    with pytest.raises(RuntimeError, match="not aliased"):  # V = K[..., :64]
        ext().gqa_decode(bf(1, 2, 1, 128), kv, kv[..., :64], 0.1, 0.0, 0,
                         None)
    with pytest.raises(RuntimeError, match="must be bf16"):
        ext().gqa_decode(bf(1, 2, 1, 64).half(), bf(1, 1, 8, 64).half(),
                         bf(1, 1, 8, 64).half(), 0.1, 0.0, 0, None)
    torch.cuda.synchronize()
