"""Fused T == 1 decode glue: every new launch against the unfused op
sequence it replaces (torch.equal — same arithmetic, same rounding
points), and the whole model against MLXS_AMD_NO_DECODE_FUSE=1.
"""

import copy

import pytest
import torch

import quant_cases as qc
from mlx_sharding_amd import ops

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DEV = "cuda"


def ext():
    e = ops.hip_ext()
    assert e is not None, "HIP extension not built"
    return e


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0, dtype=BF16):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).to(dtype).to(DEV)


# --------------------------------------------------------------------------
# mla_decode_prep
# --------------------------------------------------------------------------

PREP_SHAPES = [(1, 4, 16, 8, 32), (3, 4, 16, 8, 32), (2, 16, 128, 64, 512)]
SCAP = 12


def _prep_inputs(B, nh, nope, rope, rank, layout):
    D = nope + rope
    if layout == "contiguous":
        qh = _randn(B, 1, nh, D, seed=1)
        ckv = _randn(B, 1, rank + rope, seed=2)
        return qh, ckv
    # one wider buffer, as the fused q|kv_a projection lays it out; "odd"
    # pads the row so the views lose the kernel's vector alignment
    pad = 2 if layout == "split_odd" else 0
    buf = _randn(B, 1, nh * D + rank + rope + pad, seed=3)
    qh = buf[..., : nh * D].view(B, 1, nh, D)
    ckv = buf[..., nh * D: nh * D + rank + rope]
    assert not ckv.is_contiguous() or B == 1
    return qh, ckv


def _positions(B, mode):
    """(pos tensor or None, pos0, per-row positions)."""
    if mode == "host":
        return None, 7, [7] * B
    if mode == "shared":
        return torch.tensor([7], dtype=torch.int32, device=DEV), 0, [7] * B
    rows = [3, 9, 0][:B]
    assert len(set(rows)) == B
    return torch.tensor(rows, dtype=torch.int32, device=DEV), 0, rows


@pytest.mark.parametrize("mode", ("host", "shared", "per_row"))
@pytest.mark.parametrize("layout", ("contiguous", "split", "split_odd"))
@pytest.mark.parametrize("B,nh,nope,rope,rank", PREP_SHAPES)
def test_mla_decode_prep_matches_unfused(B, nh, nope, rope, rank, layout, mode):
    qh, ckv = _prep_inputs(B, nh, nope, rope, rank, layout)
    w = _randn(rank, seed=4).abs() + 0.5
    eps = 1e-6
    pos, pos0, rows = _positions(B, mode)
    half = rope // 2
    ang = torch.rand(SCAP, half, generator=_gen(5)) * 6.28
    cos_t, sin_t = ang.cos().to(DEV), ang.sin().to(DEV)
    idx = torch.tensor(rows, device=DEV)
    if mode == "per_row":
        cos, sin = cos_t[idx].unsqueeze(1), sin_t[idx].unsqueeze(1)  # [B,1,half]
    else:
        cos, sin = cos_t[idx[:1]], sin_t[idx[:1]]                    # [1,half]
    init = _randn(B, 1, SCAP, rank + rope, seed=6)

    # today's sequence
    q_pe_ref = ext().apply_rope(qh[..., nope:], cos, sin, True)
    c_kv = ext().rms_norm(ckv[..., :rank], w, eps, 0.0)
    k_pe = ext().apply_rope(ckv[..., rank:].reshape(B, 1, 1, rope), cos, sin,
                            True).view(B, 1, rope)
    kc_ref = init.clone()
    vc_ref = torch.empty(B, 1, SCAP, 0, dtype=BF16, device=DEV)
    ext().mla_append_kv(c_kv.reshape(B, 1, 1, rank), k_pe, kc_ref, vc_ref,
                        pos=pos, pos0=pos0)

    kc = init.clone()
    q_pe, q_nope = ext().mla_decode_prep(qh, ckv, w, eps, 0.0, cos, sin, kc,
                                         rope, pos=pos, pos0=pos0)
    assert q_pe.shape == (B, nh, rope) and q_nope.shape == (nh, B, nope)
    assert torch.equal(q_pe, q_pe_ref.view(B, nh, rope))
    assert torch.equal(q_nope, qh[:, 0, :, :nope].transpose(0, 1))
    assert torch.equal(kc, kc_ref)
    touched = torch.zeros(B, SCAP, dtype=torch.bool, device=DEV)
    touched[torch.arange(B, device=DEV), idx] = True
    assert torch.equal(kc[:, 0][~touched], init[:, 0][~touched])
    assert not torch.equal(kc[:, 0][touched], init[:, 0][touched])


def test_mla_decode_prep_rounding_many_draws():
    """The shapes above hold a few thousand elements each.  A product pair
    such as x2*c + x1*s can be contracted into an fma around either
    product; the two forms differ in the last fp32 bit and move a bf16
    result about once in 1e5 elements, so equality is also checked on
    4096 rows x 4 draws: 0.5M k_pe pairs, 8M q_pe pairs, 8M c_kv values."""
    B, nh, nope, rope, rank = 4096, 16, 128, 64, 512
    D, half, scap = nope + rope, rope // 2, 2
    w = _randn(rank, seed=4).abs() + 0.5
    vc = torch.empty(B, 1, scap, 0, dtype=BF16, device=DEV)
    for draw in range(4):
        buf = _randn(B, 1, nh * D + rank + rope, seed=100 + draw)
        qh = buf[..., : nh * D].view(B, 1, nh, D)
        ckv = buf[..., nh * D:]
        ang = torch.rand(B, 1, half, generator=_gen(200 + draw)) * 6.28
        cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
        q_pe_ref = ext().apply_rope(qh[..., nope:], cos, sin, True)
        c_kv = ext().rms_norm(ckv[..., :rank], w, 1e-6, 0.0)
        k_pe = ext().apply_rope(ckv[..., rank:].reshape(B, 1, 1, rope), cos,
                                sin, True).view(B, 1, rope)
        kc_ref = torch.zeros(B, 1, scap, rank + rope, dtype=BF16, device=DEV)
        ext().mla_append_kv(c_kv.reshape(B, 1, 1, rank), k_pe, kc_ref, vc,
                            pos0=1)
        kc = torch.zeros_like(kc_ref)
        q_pe, _ = ext().mla_decode_prep(qh, ckv, w, 1e-6, 0.0, cos, sin, kc,
                                        rope, pos0=1)
        bad_q = int((q_pe != q_pe_ref.view(B, nh, rope)).sum())
        bad_c = int((kc[..., :rank] != kc_ref[..., :rank]).sum())
        bad_k = int((kc[..., rank:] != kc_ref[..., rank:]).sum())
        assert (bad_q, bad_c, bad_k) == (0, 0, 0), \
            "draw %d: %d q_pe, %d c_kv, %d k_pe elements differ" % (
                draw, bad_q, bad_c, bad_k)


def test_mla_decode_prep_rejects_position_past_capacity():
    qh, ckv = _prep_inputs(1, 4, 16, 8, 32, "contiguous")
    cs = torch.zeros(1, 4, device=DEV)
    kc = torch.zeros(1, 1, SCAP, 40, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError, match="capacity"):
        ext().mla_decode_prep(qh, ckv, _randn(32, seed=4), 1e-6, 0.0, cs, cs,
                              kc, 8, pos0=SCAP)


# --------------------------------------------------------------------------
# attn_decode: two q sources, strided output
# --------------------------------------------------------------------------

# (B, G, Dn, Dr): G = 4 / Dv = 32 and the absorbed V2-Lite G = 16 / Dv = 512
ATTN_SHAPES = [(3, 4, 32, 8), (2, 16, 512, 64)]
ATTN_SCAP = 600   # > 2 * 256 keys: device-position calls split S three ways


@pytest.mark.parametrize("mode", ("host_one_slice", "host_split", "shared",
                                  "per_row"))
@pytest.mark.parametrize("B,G,Dn,Dr", ATTN_SHAPES)
def test_attn_decode_split_matches_contiguous(B, G, Dn, Dr, mode):
    Dk, Dv = Dn + Dr, Dn
    kbuf = _randn(B, 1, ATTN_SCAP, Dk, seed=11, scale=0.5)
    q_abs = _randn(G, B, Dn, seed=12)            # W_UK bmm result layout
    q_pe = _randn(B, G, Dr, seed=13)
    scale = Dk ** -0.5
    pos = None
    k = kbuf
    if mode == "host_one_slice":
        k = kbuf[:, :, :5]
    elif mode == "host_split":
        k = kbuf[:, :, :300]                     # two 256-key slices
    elif mode == "shared":
        pos = torch.tensor([4], dtype=torch.int32, device=DEV)   # S = 5
    else:
        pos = torch.tensor([4, 299, 130][:B], dtype=torch.int32, device=DEV)
    v = k[..., :Dv]
    qf = torch.cat([q_abs.permute(1, 0, 2), q_pe], dim=-1).unsqueeze(2)
    want = ext().attn_decode(qf.contiguous(), k, v, scale, 0.0, 0, pos)
    got = ext().attn_decode_split(q_abs.transpose(0, 1), q_pe, k, v, scale,
                                  0.0, 0, pos)
    assert got.shape == (G, B, Dv) and got.is_contiguous()
    assert torch.equal(got.permute(1, 0, 2), want[:, :, 0])
    assert want.float().abs().max() > 0


# --------------------------------------------------------------------------
# rms_norm_residual fp16 output
# --------------------------------------------------------------------------

def test_rms_norm_residual_f16_output_equals_cast():
    rows, H = 5, 256
    x = _randn(rows, 1, H, seed=21)
    r = _randn(rows, 1, H, seed=22)
    # weights spread over 1e-7 .. 1e6: y runs past both ends of fp16's range
    w = (10.0 ** torch.linspace(-7, 6, H)).to(BF16).to(DEV)
    y, h, y16 = ext().rms_norm_residual(x, r, w, 1e-6, 0.0, True)
    y2, h2 = ext().rms_norm_residual(x, r, w, 1e-6, 0.0)
    assert torch.equal(y, y2) and torch.equal(h, h2)
    assert y16.dtype == F16 and y16.shape == y.shape
    yf = y.float().abs()
    assert (yf > 65504).any() and ((yf < 2.0 ** -14) & (yf > 0)).any()
    assert torch.equal(y16, y.to(F16))
    # through ops: the copy is where _to_f16_cached looks for it
    yo, ho = ops.rms_norm_residual(x, r, w, 1e-6, 0.0, want_f16=True)
    assert torch.equal(yo, y) and torch.equal(ho, h)
    assert ops._to_f16_cached(yo) is yo._mlxs_f16
    assert torch.equal(yo._mlxs_f16, y.to(F16))


# --------------------------------------------------------------------------
# moe_finalize
# --------------------------------------------------------------------------

@pytest.mark.parametrize("with_shared", (False, True))
@pytest.mark.parametrize("H", (64, 2048))
@pytest.mark.parametrize("N", (1, 5, 64))
def test_moe_finalize_equals_three_step(N, H, with_shared):
    acc = _randn(N, H, seed=31, scale=3.0, dtype=F32)
    h = _randn(N, 1, H, seed=32)
    shared = _randn(N, H, seed=33) if with_shared else None
    y = acc.to(BF16)
    if with_shared:
        y = y + shared
    want = h + y.reshape(N, 1, H)
    got = ops.moe_finalize(acc, shared, h)
    assert got.shape == h.shape and got.dtype == BF16
    assert torch.equal(got, want)


# --------------------------------------------------------------------------
# accumulator cleared by the gate+up launch
# --------------------------------------------------------------------------

# one token, one active expert, padded slots on both sides; 71 output
# columns: 71 floats is no multiple of the 4-float clearing vector
PLAN_ONE = dict(N=1, plan=[(1, []), (2, [0]), (0, [])])
ZERO_FILL = [(qc.PLAN16, qc.MOE_OUT), (PLAN_ONE, 71)]


def _poison(n_floats):
    """Leave 1e30 in the blocks the caching allocator hands out next."""
    junk = [torch.full((n_floats,), 1e30, dtype=F32, device=DEV)
            for _ in range(8)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("plan_d,Hout", ZERO_FILL, ids=("plan16", "one_token"))
def test_gateup_clears_down_accumulator(plan_d, Hout):
    bits, gs = 4, 64
    H, I = qc.MOE_F16_DIMS[gs][1], qc.MOE_F16_DIMS[gs][0]   # 256, 320
    N = plan_d["N"]
    subs_cpu, live = qc.build_subranges(plan_d["plan"])
    subs = tuple(t.to(DEV) for t in subs_cpu)
    P = subs[3].numel()
    gate, up = qc.gateup_expert_weights("a", qc.N_EXPERTS, qc.MOE_OUT, H, gs,
                                        bits)
    x = qc.gateup_x(N, H, 0).to(F16).to(DEV)
    want_h = qc.gateup_expected("a", gate[3], up[3], plan_d, H, 0, F16).to(F16)
    q, sc, bi, W64 = qc.exact_expert_weights(qc.N_EXPERTS, Hout, I, gs, bits)
    hd = qc.down_h(plan_d, I)
    want = qc.down_expected(W64, hd, plan_d).to(F32)
    dq = ops.repack_w4(qc.pack(q, bits), bits).to(DEV)
    gq = ops.repack_w4(qc.pack(gate[0], bits), bits).to(DEV)
    uq = ops.repack_w4(qc.pack(up[0], bits), bits).to(DEV)
    dev = lambda t: t.to(DEV)  # noqa: E731

    _poison(N * Hout)
    hh, acc = ext().moe_w4f16_gateup_acc(
        x, gq, uq, dev(gate[1]), dev(gate[2]), dev(up[1]), dev(up[2]),
        *subs[:4], P, gs, bits, N, Hout)
    assert acc.shape == (N, Hout) and acc.dtype == F32
    assert not acc.any(), "gate+up left part of the accumulator uncleared"
    assert torch.equal(hh.cpu()[live], want_h[live])
    out = ext().moe_w4f16_down(hd.to(F16).to(DEV), dq, dev(sc), dev(bi),
                               *subs, N, gs, bits, acc)
    assert out.data_ptr() == acc.data_ptr()
    assert torch.equal(out.cpu(), want)


# --------------------------------------------------------------------------
# model level: fused vs MLXS_AMD_NO_DECODE_FUSE=1
# --------------------------------------------------------------------------

def _quant_tiny_deepseek(cfg):
    from conftest import init_model
    from mlx_sharding_amd.config import QuantConfig
    from mlx_sharding_amd.models import get_model_class
    from mlx_sharding_amd.models.base import Linear
    from mlx_sharding_amd.models.deepseek_v2 import _StackedLinear
    from mlx_sharding_amd.ops import reference as ref

    qcfg = QuantConfig(32, 4)
    cls = get_model_class("deepseek_v2")
    m = init_model(cls, cfg, cfg.shard(0, cfg.num_hidden_layers), seed=21,
                   quant_for=lambda p: qcfg)
    g = _gen(9)
    for mod in m.modules():
        if isinstance(mod, Linear) and mod.quant is not None:
            w = torch.randn(mod.out_features, mod.in_features, generator=g) * 0.05
            mod.weight.data, mod.scales.data, mod.biases.data = \
                ref.quantize(w.bfloat16(), 32, 4)
        elif isinstance(mod, _StackedLinear) and mod.quantc is not None:
            E, O = mod.weight.shape[0], mod.weight.shape[1]
            IN = mod.scales.shape[2] * 32
            parts = [ref.quantize((torch.randn(O, IN, generator=g) * 0.05)
                                  .bfloat16(), 32, 4) for _ in range(E)]
            mod.weight.data = torch.stack([p[0] for p in parts])
            mod.scales.data = torch.stack([p[1] for p in parts])
            mod.biases.data = torch.stack([p[2] for p in parts])
    return m.to(DEV)


@pytest.mark.parametrize("graph_pos", (False, True), ids=("eager", "graph_pos"))
def test_model_decode_fused_matches_unfused(tiny_deepseek_config, monkeypatch,
                                            graph_pos):
    """Four decode steps.  The attention block passes through no atomics:
    replayed on the unfused path from the same inputs and cache state it
    must be bit-equal.  The MoE accumulates with fp32 atomics in an order
    that varies run to run, so whole-model logits are held to the
    tolerance of the GPU-vs-reference model test (test_hip_kernels._close
    with atol 6e-2: 6e-2 + 1e-2 * max|ref|)."""
    monkeypatch.delenv("MLXS_AMD_NO_DECODE_FUSE", raising=False)
    m = _quant_tiny_deepseek(tiny_deepseek_config)
    assert m._use_absorbed()
    B, T, steps = 3, 5, 4
    ids = torch.randint(0, 128, (B, T), generator=_gen(3)).to(DEV)
    layers = list(m.model.layers.values())
    rec = []   # per step: [(x, cos, sin, out)] per layer

    def pre_hook(mod, args):
        rec[-1].append([a for a in args[:3]])

    def post_hook(mod, args, out):
        rec[-1][-1].append(out)

    def advance(caches, pos):
        if graph_pos:
            for c in caches:
                c.graph_pos = pos

    with torch.no_grad():
        cache_f = m.make_cache(batch_size=B)
        logits = m(ids, cache_f)
        cache_replay = copy.deepcopy(cache_f)
        cache_u = copy.deepcopy(cache_f)
        toks = [logits[:, -1].argmax(-1)]

        hooks = []
        for layer in layers:
            hooks.append(layer.self_attn.register_forward_pre_hook(pre_hook))
            hooks.append(layer.self_attn.register_forward_hook(post_hook))
        fused = []
        for s in range(steps):
            rec.append([])
            advance(cache_f, torch.tensor([T + s], dtype=torch.int32,
                                          device=DEV))
            out = m(toks[-1][:, None], cache_f)
            fused.append(out[:, -1].float())
            toks.append(out[:, -1].argmax(-1))
        for h in hooks:
            h.remove()

        monkeypatch.setenv("MLXS_AMD_NO_DECODE_FUSE", "1")
        assert not ops.decode_fuse_enabled()
        unfused = []
        for s in range(steps):
            pos = torch.tensor([T + s], dtype=torch.int32, device=DEV)
            advance(cache_replay, pos)
            advance(cache_u, pos)
            for j, layer in enumerate(layers):
                x, cos, sin, want = rec[s][j]
                got = layer.self_attn(x, cos, sin, cache_replay[j])
                assert torch.equal(got, want), (s, j)
            out = m(toks[s][:, None], cache_u)   # teacher-forced tokens
            unfused.append(out[:, -1].float())
    for j in range(len(layers)):
        assert torch.equal(cache_replay[j]._k[:, :, :T + steps],
                           cache_f[j]._k[:, :, :T + steps])
    for s in range(steps):
        a, b = fused[s], unfused[s]
        err = (a - b).abs().max().item()
        scale = b.abs().max().item()
        assert err <= 6e-2 + 1e-2 * scale, (s, err, scale)
