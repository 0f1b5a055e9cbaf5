"""kv_fp8.hip on the GPU: the quantizing append and the dequantizer bit for
bit against ops.reference, and gqa_decode_fp8 against fp64 attention.

The decode oracle is attn_cases.reference in fp64 over the DEQUANTIZED cache
(quantization error is not the kernel's) and the bound stays
attn_cases.BOUND * max|V_deq|: widening e4m3 to bf16 is exact, the K scale is
one fp32 multiply on an fp32 score, and vs being a power of two,
bf16(p * vs) = bf16(p) * vs: P carries exactly the bf16 kernel's rounding.
Inputs are built in the storage format with scales that differ between
neighbouring keys and between K and V; rows at or past a row's length hold
the NaN code 0x7F with a NaN scale."""
import functools

import pytest
import torch

import attn_cases as ac
from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV, ext = "cuda", ops.hip_ext


def _codes(g, *shape):
    c = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.where((c & 0x7F) == 0x7F, c - 1, c)    # no NaN codes


@pytest.mark.parametrize("table", ("shared", "per_row"))
@pytest.mark.parametrize("mode", ("host", "dev1", "devB"))
@pytest.mark.parametrize("T", (1, 5))
@pytest.mark.parametrize("D", (64, 128))
def test_append_matches_reference_bit_for_bit(D, T, mode, table):
    B, H, cap = 3, 2, 32
    g = torch.Generator().manual_seed(D + T)
    k = (torch.randn(B, T, H, D, generator=g) * 5).to(ac.BF16).to(DEV)
    v = (torch.randn(B, T, H, D, generator=g) * 0.01).to(ac.BF16).to(DEV)
    v[0, 0, 0] = 0                                      # an all-zero row
    ang = torch.rand(*((B,) if table == "per_row" else ()), T, D // 2,
                     generator=g) * 6.28
    cos, sin = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
    starts = {"host": [9] * B, "dev1": [9] * B, "devB": [0, 27, 13]}[mode]
    pos = None if mode == "host" else torch.tensor(
        starts[:1] if mode == "dev1" else starts, dtype=torch.int32, device=DEV)
    want_k8 = torch.full((B, H, cap, D), 0x55, dtype=torch.uint8)
    want_ks = torch.full((B, H, cap), 7.0)
    want_v8, want_vs = want_k8.clone(), want_ks.clone()
    k8, ks, v8, vs = (t.to(DEV) for t in (want_k8, want_ks, want_v8, want_vs))
    ext().rope_append_kv_fp8(k, v, cos, sin, k8, ks, v8, vs, pos=pos,
                             pos0=starts[0])
    kq = ref.kv_fp8_quantize(ops.apply_rope(k, cos, sin).cpu())
    vq = ref.kv_fp8_quantize(v.cpu())
    for b, p in enumerate(starts):
        want_k8[b, :, p:p + T] = kq[0][b].transpose(0, 1)
        want_ks[b, :, p:p + T] = kq[1][b].transpose(0, 1)
        want_v8[b, :, p:p + T] = vq[0][b].transpose(0, 1)
        want_vs[b, :, p:p + T] = vq[1][b].transpose(0, 1)
    assert torch.equal(ks.cpu(), want_ks) and torch.equal(vs.cpu(), want_vs)
    assert torch.equal(k8.cpu(), want_k8) and torch.equal(v8.cpu(), want_v8)


@pytest.mark.parametrize("S", (1, 300))
@pytest.mark.parametrize("D", (64, 128))
def test_dequant_kernel_bit_for_bit(D, S):
    g = torch.Generator().manual_seed(S)
    buf = _codes(g, 2, 3, 320, D)
    sc = 2.0 ** torch.randint(-100, 121, (2, 3, 320), generator=g).float()
    buf[:, :, S:], sc[:, :, S:] = 0x7F, float("nan")
    got = ext().kv_fp8_dequant(buf.to(DEV), sc.to(DEV), S)
    assert torch.equal(got.cpu(), ref.kv_fp8_dequantize(buf[:, :, :S],
                                                        sc[:, :, :S]))


@functools.lru_cache(maxsize=2)
def _decode_inputs(D, G, Hkv, cap, lens):
    B = len(lens)
    g = torch.Generator().manual_seed(D * 131 + G * 7 + cap)
    q = (torch.randn(B, G * Hkv, 1, D, generator=g) / 4).to(ac.BF16)
    k8, v8 = _codes(g, B, Hkv, cap, D), _codes(g, B, Hkv, cap, D)
    i = torch.arange(cap)
    ks = (2.0 ** ((3 * i) % 7 - 3)).float().expand(B, Hkv, cap).clone()
    vs = (2.0 ** ((5 * i) % 7 - 3)).float().expand(B, Hkv, cap).clone()
    want, bound = [], []
    for b, L in enumerate(lens):
        kd = ref.kv_fp8_dequantize(k8[b:b + 1, :, :L], ks[b:b + 1, :, :L])
        vd = ref.kv_fp8_dequantize(v8[b:b + 1, :, :L], vs[b:b + 1, :, :L])
        want.append(ac.reference(q[b:b + 1], kd, vd, D ** -0.5, [L - 1])[0])
        bound.append(ac.bounds(vd, [L - 1], 1, 0))
        for t in (k8, v8):
            t[b, :, L:] = 0x7F
        for t in (ks, vs):
            t[b, :, L:] = float("nan")
    v_first = ref.kv_fp8_dequantize(v8[:, :, 0], vs[:, :, 0])   # [B, Hkv, D]
    return q, k8, ks, v8, vs, torch.cat(want), torch.cat(bound), v_first


RUNS = {  # mode: (capacity, lengths)
    "ragged": (512, (1, 33, 300)),      # one key, one tile + 1, past a slice
    "ragged4k": (4096, (1, 257, 4000)),  # 8 slices of 512, some empty
    "host": (512, (300, 300, 300)),
    "shared": (512, (300, 300, 300)),
}


@pytest.mark.parametrize("mode", RUNS)
@pytest.mark.parametrize("G,Hkv", ((1, 2), (4, 2), (7, 1), (16, 1)))
@pytest.mark.parametrize("D", (64, 128))
def test_decode_against_fp64(D, G, Hkv, mode):
    cap, lens = RUNS[mode]
    q, k8, ks, v8, vs, want, bound, v_first = _decode_inputs(D, G, Hkv, cap, lens)
    pos = {"host": None, "shared": torch.tensor([lens[0] - 1]),
           }.get(mode, torch.tensor([L - 1 for L in lens]))
    got = ops.gqa_decode_fp8(
        q.to(DEV), k8.to(DEV), ks.to(DEV), v8.to(DEV), vs.to(DEV), D ** -0.5,
        pos=None if pos is None else pos.to(DEV, torch.int32),
        length=lens[0] if pos is None else None).cpu()
    ratio = ac.worst_ratio(got, want, bound)
    print(f"D={D} G={G} {mode}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    for b, L in enumerate(lens):
        if L == 1:    # one key: the dequantized V row, bit for bit
            assert torch.equal(got[b, :, 0].view(Hkv, G, D),
                               v_first[b][:, None].expand(Hkv, G, D))


def test_decode_graph_replay():
    D, G, Hkv, cap = 128, 4, 2, 1024
    q, k8, ks, v8, vs = (t.to(DEV) for t in _decode_inputs(
        D, G, Hkv, cap, (cap,) * 3)[:5])
    pos = torch.tensor([0, 254, 600], dtype=torch.int32, device=DEV)
    args = (q, k8, ks, v8, vs, D ** -0.5)
    ext().gqa_decode_fp8(*args, pos)  # warm up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext().gqa_decode_fp8(*args, pos)
    for new in ([257, 1023, 31], [512, 0, 700]):
        pos.copy_(torch.tensor(new, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ext().gqa_decode_fp8(*args, pos)), new


def test_binding_limits():
    def call(Hq=2, D=64, qdt=ac.BF16, sdt=torch.float32):
        z = functools.partial(torch.zeros, device=DEV)
        k8 = z(1, 1, 8, D, dtype=torch.uint8)
        sc = z(1, 1, 8, dtype=sdt)
        ext().gqa_decode_fp8(z(1, Hq, 1, D, dtype=qdt), k8, sc, k8, sc, 0.1)

    for kw, msg in ((dict(Hq=17), "1 to 16 heads"),
                    (dict(D=256), "unsupported shape"),
                    (dict(sdt=torch.float16), "scales must be fp32"),
                    (dict(qdt=torch.float16), "must be bf16")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
