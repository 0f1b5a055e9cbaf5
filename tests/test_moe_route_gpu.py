"""GPU tests of the fused prefill routing (moe_route.hip): the three
kernels against reference.moe_gate and make_expert_subranges on tie-free
inputs, reproducibility and graph capture, the binding's limits, and the
model dispatch in front of both prefill expert routes.  The kernels take 64
tokens per block."""

import pytest
import torch

from moe_gate_cases import make_logits
from moe_gate_v3_cases import MIN_GAP, make_bias, min_gap
from test_moe_route_cpu import check_sort_fields

from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

# (N, E, n_group, topk_group, K, norm, scaling, max_tok, scoring, seeds)
# sigmoid seeds are (logits seed, bias seed), searched on the CPU for
# min_gap >= MIN_GAP; the softmax rows are tie-free by construction
CASES = [
    (129, 64, 1, 1, 6, False, 1.0, 16, "softmax", None),   # one past decode
    (333, 160, 8, 3, 6, False, 16.0, 64, "softmax", None),  # V2: E tail, 5
                                                 # full blocks + a partial one
    (333, 256, 8, 4, 8, True, 2.5, 64, "sigmoid", (0, 29)),  # V3 shape
    (333, 96, 8, 3, 4, True, 2.5, 16, "sigmoid", (0, 0)),   # R = 2 with tail
    (129, 256, 8, 4, 8, True, 2.5, 16, "sigmoid", (0, 2)),  # 1-token block
    (1000, 256, 8, 4, 8, True, 2.5, 64, "softmax", None),   # 16 blocks, R = 4
    (1, 64, 1, 1, 6, False, 1.0, 16, "softmax", None),      # single token
    # row 0 of make_logits(1, 160) 333 times: K experts of 333 pairs each,
    # the rest empty, every run crossing all six blocks
    (333, 160, 8, 3, 6, False, 16.0, 64, "skew", None),
]
IDS = ["N%d-E%d-%s" % (c[0], c[1], c[8]) for c in CASES]


def _inputs(case):
    """(logits bf16 [N, E], e_bias or None, scoring) on the CPU."""
    N, E, scoring, seeds = case[0], case[1], case[8], case[9]
    if scoring == "skew":
        return make_logits(1, E).repeat(N, 1), None, "softmax"
    if scoring == "softmax":
        return make_logits(N, E), None, scoring
    logits, bias = make_logits(N, E, seeds[0]), make_bias(E, seeds[1])
    gap = min_gap(case, logits, bias)  # a condition on the inputs
    assert gap >= MIN_GAP, f"near tie in the inputs: {gap:.3e}"
    return logits, bias, scoring


def _route(case, logits, bias, scoring, wt_bf16=False):
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case[:8]
    r = ops.moe_route(logits.cuda(), K, n_group, topk_group, scaling, norm,
                      max_tok, scoring=scoring, wt_bf16=wt_bf16,
                      e_bias=None if bias is None else bias.cuda())
    torch.cuda.synchronize()
    return ref.MoeRoute(*(f.cpu() for f in r[:-1]), r.max_tok)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_route_matches_reference(case):
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case[:8]
    logits, bias, scoring = _inputs(case)
    r = _route(case, logits, bias, scoring)
    w_ref, idx_ref = ref.moe_gate(logits.float(), K, n_group, topk_group,
                                  scaling, norm, scoring=scoring, e_bias=bias)
    assert torch.equal(r.indices.long(), idx_ref), "picks or their order"
    worst = (r.weights - w_ref).abs().max().item()
    print(f"max |w - w_ref| = {worst:.3e} (bound {1e-4 * scaling:.1e})")
    assert worst <= 1e-4 * scaling
    # the sort of the kernel's own picks, integers exact, weights bit-equal
    check_sort_fields(r, r.indices, r.weights, E)
    if case[8] == "sigmoid" and N == 333 and E == 256:
        rb = _route(case, logits, bias, scoring, wt_bf16=True)
        assert torch.equal(rb.weights, r.weights.to(torch.bfloat16).float())
        assert torch.equal(rb.indices, r.indices)
        check_sort_fields(rb, rb.indices, rb.weights, E)


def test_route_reproducible_and_capturable():
    """Two eager calls agree bit for bit in every field, and so does a
    captured graph replayed twice onto refreshed logits."""
    case = CASES[1]
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case[:8]
    batches = [make_logits(N, E, seed).cuda() for seed in (0, 1, 2)]

    def call(lg):
        return ops.moe_route(lg, K, n_group, topk_group, scaling, norm,
                             max_tok)

    eager = [call(lg) for lg in batches]
    again = call(batches[0])
    for a, b in zip(eager[0][:-1], again[:-1]):
        assert torch.equal(a, b)
    static = batches[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(static)  # warm up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(static)
    for lg, want in zip(batches[1:], eager[1:]):
        static.copy_(lg)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(out._fields, out[:-1], want[:-1]):
            assert torch.equal(a, b), name


def test_route_limit_checks():
    """Outside the kernels' limits the binding raises before any launch."""
    def call(E, K, n_group, topk_group, N=200, **kw):
        logits = torch.zeros(N, E, dtype=torch.bfloat16, device="cuda")
        return ops.moe_route(logits, K, n_group, topk_group, **kw)

    for match, args, kw in (("E<=256", (257, 6, 1, 1), {}),
                            ("K<=8", (64, 9, 1, 1), {}),
                            ("n_group", (160, 6, 7, 3), {}),
                            ("topk_group", (160, 6, 8, 9), {}),
                            ("E/n_group", (64, 8, 16, 1), {}),
                            ("E/n_group >= 2", (32, 4, 32, 8),
                             {"scoring": "sigmoid"}),
                            ("max_tok", (64, 6, 1, 1), {"max_tok": 0}),
                            ("1<=N", (64, 6, 1, 1), {"N": 0})):
        with pytest.raises(RuntimeError, match=match):
            call(*args, **kw)
    torch.cuda.synchronize()


def _count_calls(monkeypatch, name):
    calls = []
    real = getattr(ops, name)

    def spy(*a, **k):
        calls.append(a[0].shape)
        return real(*a, **k)

    monkeypatch.setattr(ops, name, spy)
    return calls


@pytest.mark.parametrize("preset", ["debug-deepseek-grouped",
                                    "debug-deepseek-v3"])
def test_model_prefill_takes_fused_route(preset, monkeypatch):
    """A 140-token prefill: one ops.moe_route call per MoE layer and no
    torch gate; with MLXS_AMD_NO_FUSED_ROUTE=1 the torch route as before,
    and the two agree."""
    from mlx_sharding_amd.parallel.rccl import build_stage_model
    from mlx_sharding_amd.utils.presets import get_preset

    cfg = get_preset(preset)
    dev = torch.device("cuda", 0)
    model = build_stage_model(cfg, 0, 1, dev, seed=17)
    torch.manual_seed(4)
    ids = torch.randint(0, cfg.vocab_size, (2, 70), device=dev)
    routes = _count_calls(monkeypatch, "moe_route")
    gates = _count_calls(monkeypatch, "moe_gate")
    n_moe = cfg.num_hidden_layers - 1  # first_k_dense_replace = 1

    def prefill():
        with torch.no_grad():
            return model(ids, model.make_cache(batch_size=2))[:, -1].float()

    monkeypatch.delenv("MLXS_AMD_NO_FUSED_ROUTE", raising=False)
    fused = prefill()
    assert len(routes) == n_moe and len(gates) == 0, (routes, gates)
    assert all(s[0] == 140 for s in routes)
    monkeypatch.setenv("MLXS_AMD_NO_FUSED_ROUTE", "1")
    torch_route = prefill()
    assert len(routes) == n_moe and len(gates) == n_moe, (routes, gates)
    cos = torch.nn.functional.cosine_similarity(
        fused.flatten(), torch_route.flatten(), dim=0).item()
    print(f"{preset}: fused vs torch route cos={cos:.6f}")
    assert cos > 0.999


def test_fp8_packed_prefill_runs_no_torch_sort(monkeypatch):
    """debug-deepseek-v3-fp8 on the packed route: the wide kernels take the
    route's sub-ranges, nothing is sorted or scattered in torch."""
    from test_fp8_prefill_model_gpu import _gpu_prefill
    from mlx_sharding_amd.utils.presets import get_preset

    monkeypatch.delenv("MLXS_AMD_NO_FUSED_ROUTE", raising=False)
    sorts = _count_calls(monkeypatch, "make_expert_subranges")
    err, scale, spy = _gpu_prefill("forced_packed", monkeypatch)
    n_moe = get_preset("debug-deepseek-v3-fp8").num_hidden_layers - 1
    print(f"fp8 packed behind the fused route: err {err:.3e} scale {scale:.3f}")
    assert spy.count("moe_route") == n_moe, spy.calls
    assert spy.count("moe_fp8f16_gateup_wide") == n_moe
    assert spy.count("moe_fp8f16_down_wide") == n_moe
    assert spy.count("moe_scatter_rows") == 0 and len(sorts) == 0
    assert err <= 6e-2 + 1e-2 * scale, (err, scale)
