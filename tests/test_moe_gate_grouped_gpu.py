"""GPU tests for fused group-limited MoE gating (E <= 256): the kernel
against reference.moe_gate on tie-free inputs, the binding's limit checks,
and the model / graphed-serving paths behind the new dispatch."""

import os

import pytest
import torch

from moe_gate_cases import GRID, GRID_IDS, make_logits

from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _run(case, n_group=None, topk_group=None):
    """Fused op on the case's logits; all outputs as CPU lists."""
    from mlx_sharding_amd import ops
    N, E, ng, tg, K, norm, scaling, max_tok = case
    logits = make_logits(N, E).cuda()
    outs = ops.moe_gate_subranges(
        logits, K, routed_scaling_factor=scaling, norm_topk_prob=norm,
        max_tok=max_tok, n_group=ng if n_group is None else n_group,
        topk_group=tg if topk_group is None else topk_group)
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


@pytest.mark.parametrize("case", GRID, ids=GRID_IDS)
def test_grouped_gate_matches_reference(case):
    N, E, n_group, topk_group, K, norm, scaling, max_tok = case
    outs = _run(case)
    sub_e, sub_off, sub_cnt, sorted_tok, sorted_wt = outs
    P = N * K

    # ---- structure of the sub-range arrays ----
    S = E + P // max_tok
    assert len(sub_e) == len(sub_off) == len(sub_cnt) == S
    assert len(sorted_tok) == len(sorted_wt) == P
    assert all(0 <= c <= max_tok for c in sub_cnt)
    assert sum(sub_cnt) == P
    live = sum(1 for c in sub_cnt if c > 0)
    assert all(c > 0 for c in sub_cnt[:live]), "live slots must come first"
    assert all(c == 0 for c in sub_cnt[live:])
    # experts in order, each expert's slots contiguous, offsets advancing
    # by max_tok from the expert's start; the starts tile [0, P) in order
    assert sub_e[:live] == sorted(sub_e[:live])
    nxt = 0
    s = 0
    while s < live:
        e = sub_e[s]
        assert 0 <= e < E
        start = sub_off[s]
        assert start == nxt, "expert runs must be back to back in order"
        j = 0
        toks = []
        while s < live and sub_e[s] == e:
            assert sub_off[s] == start + j * max_tok
            if s + 1 < live and sub_e[s + 1] == e:
                assert sub_cnt[s] == max_tok, "only the last slot is partial"
            toks += sorted_tok[sub_off[s]:sub_off[s] + sub_cnt[s]]
            nxt = sub_off[s] + sub_cnt[s]
            j += 1
            s += 1
        assert len(set(toks)) == len(toks), "token twice in one expert run"
        assert all(0 <= t < N for t in toks)
    assert nxt == P

    # ---- selection and weights vs the reference on the same values ----
    w_ref, idx_ref = ref.moe_gate(make_logits(N, E).float(), K, n_group,
                                  topk_group, scaling, norm)
    expect = {(int(idx_ref[n, k]), n): float(w_ref[n, k])
              for n in range(N) for k in range(K)}
    got = _pair_map(outs)
    assert set(got) == set(expect), "selected (expert, token) set differs"
    worst = max(abs(got[k] - expect[k]) for k in expect)
    print(f"max |w - w_ref| = {worst:.3e} (bound {1e-4 * scaling:.1e})")
    assert worst <= 1e-4 * scaling


def test_all_groups_kept_equals_ungrouped_kernel():
    """topk_group == n_group masks nothing: same pairs and bit-identical
    weights as the n_group=1 launch on the same input."""
    case = GRID[-1]
    assert case[2] == case[3] == 16
    assert _pair_map(_run(case)) == _pair_map(_run(case, 1, 1))


def test_grouped_gate_limit_checks():
    """Outside the kernel's limits the binding raises before any launch."""
    from mlx_sharding_amd import ops

    def call(E, K, n_group, topk_group, N=4):
        logits = torch.zeros(N, E, dtype=torch.bfloat16, device="cuda")
        return ops.moe_gate_subranges(logits, K, max_tok=16, n_group=n_group,
                                      topk_group=topk_group)

    with pytest.raises(RuntimeError, match="E<=256"):
        call(257, 6, 1, 1)
    with pytest.raises(RuntimeError, match="n_group"):
        call(160, 6, 7, 3)
    with pytest.raises(RuntimeError, match="topk_group"):
        call(160, 6, 8, 9)
    with pytest.raises(RuntimeError, match="topk_group"):
        call(160, 6, 8, 0)
    with pytest.raises(RuntimeError, match="n_group"):
        call(256, 6, 64, 8)
    with pytest.raises(RuntimeError, match=r"E/n_group"):
        call(64, 8, 16, 1)       # 1 * 4 < 8
    with pytest.raises(RuntimeError, match="N<=128"):
        call(64, 6, 1, 1, N=129)
    torch.cuda.synchronize()


@pytest.mark.parametrize("quant", [False, True], ids=["bf16", "w4g64"])
def test_grouped_model_native_vs_eager(quant, monkeypatch):
    """Teacher-forced prefill + 2 decode steps of debug-deepseek-grouped:
    the HIP path (fused grouped gate in front of the MFMA expert kernels)
    tracks MLXS_AMD_FORCE_TORCH eager, and really takes the fused gate."""
    from mlx_sharding_amd import ops
    from mlx_sharding_amd.parallel.rccl import build_stage_model
    from mlx_sharding_amd.utils.presets import get_preset

    cfg = get_preset("debug-deepseek-grouped", quant=quant, group_size=64,
                     bits=4)
    dev = torch.device("cuda", 0)
    model = build_stage_model(cfg, 0, 1, dev, seed=17)
    torch.manual_seed(4)
    ids = torch.randint(0, cfg.vocab_size, (2, 9), device=dev)

    calls = []
    real = ops.moe_gate_subranges

    def spy(*args, **kwargs):
        calls.append((args[0].shape[1], kwargs.get("n_group"),
                      kwargs.get("topk_group")))
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, "moe_gate_subranges", spy)

    def chain(force):
        os.environ.pop("MLXS_AMD_FORCE_TORCH", None)
        if force:
            os.environ["MLXS_AMD_FORCE_TORCH"] = "1"
        cache = model.make_cache(batch_size=2)
        outs = []
        with torch.no_grad():
            h = model(ids, cache)
            outs.append(h[:, -1, :].float())
            t = h[:, -1, :].argmax(-1, keepdim=True)
            for _ in range(2):
                h = model(t, cache)
                outs.append(h[:, -1, :].float())
        return outs

    try:
        a = chain(False)
        n_native = len(calls)
        b = chain(True)
    finally:
        os.environ.pop("MLXS_AMD_FORCE_TORCH", None)
    n_moe = cfg.num_hidden_layers - 1  # first_k_dense_replace = 1
    assert n_native == 3 * n_moe, "fused gate not taken on every MoE layer"
    assert len(calls) == n_native, "eager run must not use the fused gate"
    assert all(c == (96, 8, 3) for c in calls), calls[:3]
    for i, (x, y) in enumerate(zip(a, b)):
        cos = torch.nn.functional.cosine_similarity(
            x.flatten(), y.flatten(), dim=0).item()
        print(f"step {i}: cos={cos:.6f}")
        assert cos > 0.999, f"step {i}: native/eager diverge (cos={cos})"


def test_grouped_serving_graph_matches_eager():
    """Graphed B=1 decode engages for a group-limited model (the fused
    gate has no host sync), re-arms, and matches eager greedy tokens."""
    from mlx_sharding_amd.parallel.engine import SamplingParams
    from mlx_sharding_amd.parallel.rccl import PipelineWorker, build_stage_model
    from mlx_sharding_amd.parallel.rccl_serve import RcclPipeline
    from mlx_sharding_amd.utils.presets import get_preset

    cfg = get_preset("debug-deepseek-grouped")
    dev = torch.device("cuda", 0)
    model = build_stage_model(cfg, 0, 1, dev, seed=5)
    pipe = RcclPipeline(PipelineWorker(model, 0, 1, dev))
    ids = torch.tensor([[5, 9, 2, 17, 3, 8]], dtype=torch.long)

    def gen_tokens(p, n):
        toks = []
        for tid, _ in p.generate_step(ids, SamplingParams(max_tokens=n)):
            toks.append(tid)
            if len(toks) >= n:
                break
        return toks

    t1 = gen_tokens(pipe, 6)
    assert pipe._graph is not None, "graph path did not engage"
    g1 = pipe._graph
    t2 = gen_tokens(pipe, 6)
    assert pipe._graph is g1, "graph was rebuilt instead of re-armed"
    assert t1 == t2, "graphed generations not reproducible"

    os.environ["MLXS_AMD_SERVE_GRAPH"] = "0"
    try:
        pipe2 = RcclPipeline(PipelineWorker(model, 0, 1, dev))
        t_eager = gen_tokens(pipe2, 6)
    finally:
        os.environ.pop("MLXS_AMD_SERVE_GRAPH", None)
    assert t1 == t_eager, f"graphed {t1} != eager {t_eager}"
