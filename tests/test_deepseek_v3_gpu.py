"""GPU tests for DeepSeek-V3: the fused gate in sigmoid mode, absorbed MLA
decode beyond 16 heads, and the debug-deepseek-v3 model against the CPU."""

import functools

import pytest
import torch

import moe_gate_v3_cases as gc
from conftest import init_model
from mlx_sharding_amd.config import ModelConfig
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.ops import reference as ref
from mlx_sharding_amd.utils.presets import get_preset

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ext():
    from mlx_sharding_amd import ops
    e = ops.hip_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _close(a, b, atol, rtol=1e-2):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= atol + rtol * scale, f"max err {err} (scale {scale})"


# --------------------------------------------------------------------------
# fused gate, sigmoid mode
# --------------------------------------------------------------------------

def _gate(case, logits, bias, **kw):
    """Fused op in sigmoid mode; all outputs as CPU lists."""
    from mlx_sharding_amd import ops
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case
    outs = ops.moe_gate_subranges(
        logits.to(DEV), K, routed_scaling_factor=scaling, norm_topk_prob=norm,
        max_tok=max_tok, n_group=n_group, topk_group=topk_group,
        scoring="sigmoid", e_bias=None if bias is None else bias.to(DEV), **kw)
    torch.cuda.synchronize()
    return [o.cpu().tolist() for o in outs]


def _pair_map(outs):
    """(expert, token) -> weight from the sub-range arrays."""
    sub_e, sub_off, sub_cnt, sorted_tok, sorted_wt = outs
    got = {}
    for s in range(len(sub_e)):
        for j in range(sub_cnt[s]):
            p = sub_off[s] + j
            key = (sub_e[s], sorted_tok[p])
            assert key not in got, f"pair {key} emitted twice"
            got[key] = sorted_wt[p]
    return got


def _host_subranges(idx, E, max_tok):
    """The sub-range arrays rebuilt on the host from the chosen experts:
    (sub_expert, sub_off, sub_cnt, {expert: set of tokens})."""
    N, K = idx.shape
    toks = {e: set() for e in range(E)}
    for n in range(N):
        for e in idx[n].tolist():
            toks[e].add(n)
    S = E + (N * K) // max_tok
    sub_e, sub_off, sub_cnt = [], [], []
    start = 0
    for e in range(E):
        cnt = len(toks[e])
        for j in range(0, cnt, max_tok):
            sub_e.append(e)
            sub_off.append(start + j)
            sub_cnt.append(min(max_tok, cnt - j))
        start += cnt
    pad = S - len(sub_e)
    return sub_e + [0] * pad, sub_off + [0] * pad, sub_cnt + [0] * pad, toks


@pytest.mark.parametrize("entry", gc.ALL_INPUTS, ids=gc.ALL_IDS)
def test_sigmoid_gate_matches_reference(entry):
    """Exact expert sets (the inputs hold no near tie), sub-range arrays
    equal to a host rebuild, weights within the softmax gate test's
    1e-4 * scaling."""
    case, logits, bias = gc.case_inputs(*entry)
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case
    outs = _gate(case, logits, bias)
    sub_e, sub_off, sub_cnt, sorted_tok, sorted_wt = outs

    w_ref, idx_ref = ref.moe_gate(logits.float(), K, n_group, topk_group,
                                  scaling, norm, scoring="sigmoid",
                                  e_bias=bias)
    want_e, want_off, want_cnt, toks = _host_subranges(idx_ref, E, max_tok)
    assert len(sorted_tok) == len(sorted_wt) == N * K
    assert sub_e == want_e
    assert sub_off == want_off
    assert sub_cnt == want_cnt
    start = 0
    for e in range(E):
        run = sorted_tok[start:start + len(toks[e])]
        assert len(run) == len(set(run)) and set(run) == toks[e], f"expert {e}"
        start += len(toks[e])

    expect = {(int(idx_ref[n, k]), n): float(w_ref[n, k])
              for n in range(N) for k in range(K)}
    got = _pair_map(outs)
    assert set(got) == set(expect), "selected (expert, token) set differs"
    worst = max(abs(got[k] - expect[k]) for k in expect)
    print(f"max |w - w_ref| = {worst:.3e} (bound {1e-4 * scaling:.1e})")
    assert worst <= 1e-4 * scaling


def test_sigmoid_gate_missing_bias_equals_zero_bias():
    case, logits, bias = gc.case_inputs(gc.ZERO_BIAS_ENTRY, True)
    assert not bias.any()
    assert _pair_map(_gate(case, logits, None)) == \
        _pair_map(_gate(case, logits, bias))


def test_sigmoid_gate_under_graph_capture():
    from mlx_sharding_amd import ops
    case, logits, bias = gc.case_inputs(2)
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case
    eager = _pair_map(_gate(case, logits, bias))
    lg = logits.to(DEV)
    bg = bias.to(DEV)

    def call():
        return ops.moe_gate_subranges(
            lg, K, routed_scaling_factor=scaling, norm_topk_prob=norm,
            max_tok=max_tok, n_group=n_group, topk_group=topk_group,
            scoring="sigmoid", e_bias=bg)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = call()
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _pair_map([o.cpu().tolist() for o in outs]) == eager
    # new inputs in the captured buffers, replayed
    lg.copy_(logits.flip(0).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = _pair_map([o.cpu().tolist() for o in outs])
    assert replayed == _pair_map(_gate(case, logits.flip(0), bias))
    assert replayed != eager


def test_softmax_mode_through_keyword_defaults():
    from mlx_sharding_amd import ops
    from moe_gate_cases import GRID, make_logits
    case = GRID[1]
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case
    logits = make_logits(N, E).to(DEV)
    pos = ops.moe_gate_subranges(logits, K, scaling, norm, max_tok, n_group,
                                 topk_group)
    kw = ops.moe_gate_subranges(logits, K, scaling, norm, max_tok, n_group,
                                topk_group, scoring="softmax", e_bias=None)
    torch.cuda.synchronize()
    a, b = ([o.cpu().tolist() for o in outs] for outs in (pos, kw))
    assert a[:3] == b[:3]
    assert _pair_map(a) == _pair_map(b)


def test_sigmoid_gate_limit_checks():
    from mlx_sharding_amd import ops

    def call(E, n_group, topk_group, bias=None, scoring="sigmoid", K=2):
        logits = torch.zeros(4, E, dtype=torch.bfloat16, device=DEV)
        return ops.moe_gate_subranges(logits, K, max_tok=16, n_group=n_group,
                                      topk_group=topk_group, scoring=scoring,
                                      e_bias=bias)

    with pytest.raises(RuntimeError, match="E/n_group >= 2"):
        call(32, 32, 4)
    with pytest.raises(RuntimeError, match="scoring"):
        call(64, 1, 1, scoring="tanh")
    with pytest.raises(RuntimeError, match="e_bias"):
        call(64, 1, 1, torch.zeros(64, device=DEV), scoring="softmax")
    with pytest.raises(RuntimeError, match="e_bias"):
        call(64, 1, 1, torch.zeros(63, device=DEV))
    with pytest.raises(RuntimeError, match="e_bias"):
        call(64, 1, 1, torch.zeros(64, device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="e_bias"):
        call(64, 1, 1, torch.zeros(64))
    with pytest.raises(RuntimeError, match="e_bias"):
        call(64, 1, 1, torch.zeros(128, device=DEV)[::2])
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# absorbed MLA decode beyond 16 heads
# --------------------------------------------------------------------------

ATTN_CAP = 1024
ATTN_LENGTHS = (1, 257, 700)   # one key, a tile edge, several split-S slices
# (Hq, Dk, Dv): the V3 row shape at 32 and 128 heads, and the small-rank
# rows of debug-deepseek-v3 (Dv <= 256 takes the one-column-per-thread kernel)
ATTN_SHAPES = [(32, 576, 512), (128, 576, 512), (32, 80, 64)]


@functools.lru_cache(maxsize=None)
def _attn_case(Hq, Dk, Dv, B):
    """Seeded CPU inputs and, per length, the fp32 reference [B, Hq, Dv].
    Every head has its own random q."""
    g = torch.Generator().manual_seed(Hq * 7 + B)
    q = torch.randn(B, Hq, 1, Dk, generator=g).to(torch.bfloat16)
    kbuf = (torch.randn(B, 1, ATTN_CAP, Dk, generator=g) * 0.5).to(
        torch.bfloat16)
    scale = Dk ** -0.5
    want = {}
    for L in ATTN_LENGTHS:
        k = kbuf[:, :, :L].float()
        want[L] = ref.attention(q.float(), k, k[..., :Dv].contiguous(), scale,
                                causal_offset=L - 1)[:, :, 0]
    return q, kbuf, scale, want


def _both_entry_points(q, k, Dv, scale, pos):
    """attn_decode and the two-source head-major attn_decode_split, both as
    [B, Hq, Dv]."""
    Dr = 64 if q.shape[-1] == 576 else 16
    v = k[..., :Dv]
    one = ext().attn_decode(q, k, v, scale, 0.0, 0, pos)[:, :, 0]
    q_nope = q[:, :, 0, :-Dr].permute(1, 0, 2).contiguous()   # [Hq, B, Dn]
    q_rope = q[:, :, 0, -Dr:].contiguous()                    # [B, Hq, Dr]
    two = ext().attn_decode_split(q_nope.transpose(0, 1), q_rope, k, v, scale,
                                  0.0, 0, pos)
    assert two.shape == (q.shape[1], q.shape[0], Dv) and two.is_contiguous()
    return one, two.permute(1, 0, 2)


@pytest.mark.parametrize("mode", ("host", "shared", "ragged"))
@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("Hq,Dk,Dv", ATTN_SHAPES)
def test_attn_decode_many_heads(Hq, Dk, Dv, B, mode):
    assert ext().attn_decode_shape_ok(Hq, Dv)
    q_c, kbuf_c, scale, want = _attn_case(Hq, Dk, Dv, B)
    q, kbuf = q_c.to(DEV), kbuf_c.to(DEV)
    if mode == "ragged":
        lens = ATTN_LENGTHS[:B]
        pos = torch.tensor([L - 1 for L in lens], dtype=torch.int32,
                           device=DEV)
        expect = torch.stack([want[L][b] for b, L in enumerate(lens)])
        for got in _both_entry_points(q, kbuf, Dv, scale, pos):
            _close(got, expect, atol=3e-2)
        return
    for L in ATTN_LENGTHS:
        if mode == "host":
            k, pos = kbuf[:, :, :L], None
        else:
            k = kbuf
            pos = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
        for got in _both_entry_points(q, k, Dv, scale, pos):
            _close(got, want[L], atol=3e-2)


# --------------------------------------------------------------------------
# model
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _cpu_model_run():
    """debug-deepseek-v3 on the CPU: prefill + 8 greedy decode steps.
    Returns (state dict, prompt ids, greedy tokens, logits rows)."""
    cfg = get_preset("debug-deepseek-v3")
    m = init_model(get_model_class("deepseek_v3"), cfg,
                   cfg.shard(0, cfg.num_hidden_layers), seed=13)
    ids = torch.randint(0, cfg.vocab_size, (2, 7),
                        generator=torch.Generator().manual_seed(2))
    cache = m.make_cache(batch_size=2)
    rows, toks = [], []
    with torch.no_grad():
        h = m(ids, cache)
        for _ in range(8):
            rows.append(h[:, -1].float())
            toks.append(h[:, -1].argmax(-1))
            h = m(toks[-1][:, None], cache)
        rows.append(h[:, -1].float())
    return m.state_dict(), ids, toks, rows


@pytest.mark.parametrize("fuse", (True, False), ids=("fused", "no_decode_fuse"))
def test_debug_v3_gpu_matches_cpu(fuse, monkeypatch):
    """Compressed one-head cache, and teacher-forced prefill + 8 decode
    steps within the fused-decode model test's 6e-2 + 1e-2 * max|ref| of
    the CPU model."""
    from mlx_sharding_amd import ops
    if fuse:
        monkeypatch.delenv("MLXS_AMD_NO_DECODE_FUSE", raising=False)
    else:
        monkeypatch.setenv("MLXS_AMD_NO_DECODE_FUSE", "1")
    assert ops.decode_fuse_enabled() == fuse
    sd, ids, toks, rows = _cpu_model_run()
    cfg = get_preset("debug-deepseek-v3")
    m = get_model_class("deepseek_v3")(cfg, cfg.shard(0, cfg.num_hidden_layers))
    m.load_weights(sd)
    m = m.to(DEV).eval()
    assert m._use_absorbed()
    cache = m.make_cache(batch_size=2)
    assert all(c.n_kv_heads == 1 for c in cache)
    assert m.cache_specs()[0] == (1, 64 + 16, 0)

    calls = []
    real = ops.moe_gate_subranges

    def spy(*args, **kwargs):
        calls.append((kwargs.get("scoring"), kwargs.get("n_group"),
                      kwargs.get("topk_group"),
                      kwargs["e_bias"].dtype, kwargs["e_bias"].is_cuda))
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, "moe_gate_subranges", spy)
    got = []
    with torch.no_grad():
        h = m(ids.to(DEV), cache)
        for t in toks:
            got.append(h[:, -1].float().cpu())
            h = m(t[:, None].to(DEV), cache)
        got.append(h[:, -1].float().cpu())
    n_moe = cfg.num_hidden_layers - 1
    assert len(calls) == 9 * n_moe, "fused gate not taken on every MoE layer"
    assert all(c == ("sigmoid", 8, 3, torch.float32, True) for c in calls)
    for step, (a, b) in enumerate(zip(got, rows)):
        err = (a - b).abs().max().item()
        scale = b.abs().max().item()
        print(f"step {step}: err {err:.3e} scale {scale:.3f}")
        assert err <= 6e-2 + 1e-2 * scale, (step, err, scale)


def test_128_head_v2_keeps_expanded_cache_v3_takes_compressed():
    raw = {
        "model_type": "deepseek_v2", "hidden_size": 64, "num_hidden_layers": 1,
        "intermediate_size": 64, "num_attention_heads": 128,
        "vocab_size": 64, "rms_norm_eps": 1e-6, "rope_theta": 10000.0,
        "q_lora_rank": 32, "kv_lora_rank": 512, "qk_nope_head_dim": 16,
        "qk_rope_head_dim": 64, "v_head_dim": 16,
    }
    cfg = ModelConfig.from_dict(raw)
    with torch.device(DEV):
        v2 = get_model_class("deepseek_v2")(cfg, cfg.shard(0, 1))
    assert not v2._use_absorbed()
    assert v2.cache_specs() == [(128, 16 + 64, 16)]
    cfg3 = ModelConfig.from_dict(dict(raw, model_type="deepseek_v3"))
    with torch.device(DEV):
        v3 = get_model_class("deepseek_v3")(cfg3, cfg3.shard(0, 1))
    assert v3._use_absorbed()
    assert v3.cache_specs() == [(1, 512 + 64, 0)]
