"""gqa_chunk.hip on the GPU: T new tokens over a cached prefix against fp64
attention on the bf16 inputs, bf16 and FP8 caches.

Inputs are seeded on the CPU: q = randn + 1 in the [B, T, Hq, D]-transposed
view the model passes, K = 0.5 * randn, V uniform in [-2, 2], capacity 1024
with NaN in the rows at or past S.  Hot keys: the rows at keys 255 and 256
and each token's own last key P + t get HOT / sqrt(D) added to every element
(about +HOT on their score for every query row), so that dropping one, or
admitting one too many, shows at slice and tile edges too.  Checked once on
the CPU for these shapes at HOT = 12 (6 left a 700-key prefix most of the
mass): the hot keys a row attends hold 0.88 or more of its softmax mass.  The
K noise (score sigma 0.7, whatever HOT is) spreads it unevenly over the up to
12 hot keys of a row, so 1/16 for every key in every row is out of reach;
every hot key has a row where it carries 0.029 or more (0.047 without G = 1),
and a key of that share whose V row is 1 away from the output in some column
moves it by twice the bound.  The bound is attn_cases.BOUND * max|V| per
(batch row, kv head), 0.016; a token that attends a single key (P = 0, t = 0)
must return the V row bit for bit."""
import functools

import pytest
import torch

import attn_cases as ac
from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV, ext, CAP, HOT = "cuda", ops.hip_ext, 1024, 12.0
SHAPES = ((8, 2, 128), (14, 2, 128), (16, 2, 64), (2, 2, 128), (32, 2, 64))
CHUNKS = ((0, 2), (1, 3), (14, 4), (30, 5), (254, 4), (700, 7), (20, 10))


@functools.lru_cache(maxsize=None)
def _inputs(Hq, Hkv, D, B, P, T):
    g = torch.Generator().manual_seed(Hq * 1009 + D * 31 + B * 7 + P * 13 + T)
    S = P + T
    q = (torch.randn(B, T, Hq, D, generator=g) + 1.0).to(ac.BF16)
    k = 0.5 * torch.randn(B, Hkv, CAP, D, generator=g)
    hot = [j for j in (255, 256) if j < S] + list(range(P, S))
    k[:, :, hot] += HOT / D ** 0.5
    v = torch.rand(B, Hkv, CAP, D, generator=g) * 4 - 2
    return q, k.to(ac.BF16), v.to(ac.BF16), S


def _want(q, k, v, S, T):
    want = ac.reference(q.transpose(1, 2), k[:, :, :S], v[:, :, :S],
                        q.shape[-1] ** -0.5, [S - T] * q.shape[0])[0]
    return want, ac.bounds(v[:, :, :S], [S - T] * q.shape[0], T, 0)


def _check(got, want, bound, v_first, P, tag):
    B, Hq, T, D = got.shape
    ratio = ac.worst_ratio(got.cpu(), want, bound)
    print(f"{tag}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    if P == 0:       # token 0 attends key 0 alone: its V row, bit for bit
        Hkv = v_first.shape[1]
        assert torch.equal(got[:, :, 0].cpu().view(B, Hkv, -1, D),
                           v_first[:, :, None].expand(B, Hkv, Hq // Hkv, D))


@pytest.mark.parametrize("P,T", CHUNKS)
@pytest.mark.parametrize("B", (1, 2))
@pytest.mark.parametrize("Hq,Hkv,D", SHAPES)
def test_chunk_against_fp64(Hq, Hkv, D, B, P, T):
    q, k, v, S = _inputs(Hq, Hkv, D, B, P, T)
    want, bound = _want(q, k, v, S, T)
    if P in (254, 700):
        blocks = B * Hkv * -(-T * (Hq // Hkv) // 64)
        assert ext().gqa_chunk_nsplit(blocks, S) > 1
    kb, vb = k.clone(), v.clone()
    kb[:, :, S:], vb[:, :, S:] = float("nan"), float("nan")
    got = ops.gqa_chunk(q.to(DEV).transpose(1, 2), kb.to(DEV)[:, :, :S],
                        vb.to(DEV)[:, :, :S], D ** -0.5)
    assert got.shape == (B, Hq, T, D)
    _check(got, want, bound, v[:, :, 0], P, f"G={Hq // Hkv} D={D} P={P} T={T}")


@pytest.mark.parametrize("P,T", ((0, 2), (30, 5), (254, 4), (700, 7), (20, 10)))
@pytest.mark.parametrize("Hq,Hkv,D", ((14, 2, 128), (16, 2, 64)))
def test_fp8_chunk_against_fp64_and_the_bf16_kernel(Hq, Hkv, D, P, T):
    B = 2
    q, k, v, S = _inputs(Hq, Hkv, D, B, P, T)
    k8, ks = ops.kv_fp8_quantize(k.to(DEV))
    v8, vs = ops.kv_fp8_quantize(v.to(DEV))
    kd, vd = (ref.kv_fp8_dequantize(c.cpu(), s.cpu())
              for c, s in ((k8, ks), (v8, vs)))
    want, bound = _want(q, kd, vd, S, T)
    for c, s in ((k8, ks), (v8, vs)):
        c[:, :, S:], s[:, :, S:] = 0x7F, float("nan")
    qd = q.to(DEV).transpose(1, 2)
    got = ops.gqa_chunk_fp8(qd, k8, ks, v8, vs, D ** -0.5, S)
    _check(got, want, bound, vd[:, :, 0], P, f"fp8 D={D} P={P} T={T}")
    twin = ops.gqa_chunk(qd, ext().kv_fp8_dequant(k8, ks, S),
                         ext().kv_fp8_dequant(v8, vs, S), D ** -0.5)
    assert torch.equal(got, twin)


def test_binding_limits():
    z = functools.partial(torch.zeros, device=DEV)

    def call(Hq=2, Hkv=1, T=2, S=8, D=64, Dv=None, qdt=ac.BF16, qoff=0,
             krow=None, bpad=0):
        q = z(Hq * T * D + qoff, dtype=qdt)[qoff:].view(1, T, Hq, D)
        k = z(2, Hkv, 8, krow or D, dtype=ac.BF16)[..., :D]
        v = z(2, Hkv, 8, Dv or D, dtype=ac.BF16)
        if bpad:
            k = z(2 * k[0].numel() + bpad, dtype=ac.BF16).as_strided(
                k.shape, (k.stride(0) + bpad,) + k.stride()[1:])
            q = torch.cat([q, q])
        nb = q.shape[0]
        ext().gqa_chunk(q.transpose(1, 2), k[:nb, :, :S], v[:nb, :, :S], 0.1)

    for kw, msg in ((dict(qdt=torch.float16), "must be bf16"),
                    (dict(D=256), "unsupported shape"),
                    (dict(Dv=128), "unsupported shape"),
                    (dict(Hq=17), "1 to 16 heads"),
                    (dict(Hq=3, Hkv=2), "divisible by Hkv"),
                    (dict(T=0), "must be among"),
                    (dict(T=9), "must be among"),
                    (dict(krow=128), "K/V rows must be contiguous"),
                    (dict(qoff=4), "q rows must be contiguous and 16-byte"),
                    (dict(bpad=8), "whole number of rows")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    k8, sc = z(1, 1, 8, 64, dtype=torch.uint8), z(1, 1, 8)
    with pytest.raises(RuntimeError, match="must be among"):
        ext().gqa_chunk_fp8(z(1, 2, 3, 64, dtype=ac.BF16), k8, sc, k8, sc, 0.1, 2)
    torch.cuda.synchronize()
