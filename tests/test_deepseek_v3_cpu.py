"""DeepSeek-V3 on the CPU path: the sigmoid gate formula, an independent
fp32 reference (transformers' DeepseekV3ForCausalLM), pipeline parity,
checkpoint key handling, config errors and continuous batching."""

import json
import threading

import pytest
import torch

import moe_gate_v3_cases as gc
from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.config import ModelConfig
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.ops import reference as ref
from mlx_sharding_amd.utils.presets import get_preset

JOIN_S = 60  # bound for thread joins; nothing here waits it out


# -- 1. gate formula -----------------------------------------------------------

def _gate_by_hand(logits, bias, n_group, topk_group, K, norm, scaling):
    """DeepSeek-V3's noaux_tc rule, written out; sets of experts per row
    and an {expert: weight} map per row."""
    s = torch.sigmoid(logits.float())
    c = s + bias
    N, E = s.shape
    sets, weights = [], []
    for n in range(N):
        allowed = set(range(E))
        if n_group > 1:
            gsz = E // n_group
            score = []
            for g in range(n_group):
                top2 = sorted(c[n, g * gsz:(g + 1) * gsz].tolist())[-2:]
                score.append(torch.tensor(top2[0], dtype=torch.float32)
                             + torch.tensor(top2[1], dtype=torch.float32))
            keep = sorted(range(n_group), key=lambda g: -float(score[g]))
            allowed = {e for g in keep[:topk_group]
                       for e in range(g * gsz, (g + 1) * gsz)}
        chosen = sorted(allowed, key=lambda e: -float(c[n, e]))[:K]
        w = s[n, chosen]
        if norm:
            w = w / (w.sum() + 1e-20)
        w = w * scaling
        sets.append(set(chosen))
        weights.append(dict(zip(chosen, w.tolist())))
    return sets, weights


@pytest.mark.parametrize("entry", gc.ALL_INPUTS, ids=gc.ALL_IDS)
def test_sigmoid_gate_formula(entry):
    case, logits, bias = gc.case_inputs(*entry)
    N, E, n_group, topk_group, K, norm, scaling, _ = case
    w, idx = ops.moe_gate(logits, K, n_group, topk_group, scaling, norm,
                          scoring="sigmoid", e_bias=bias)
    assert w.dtype == torch.float32 and w.shape == idx.shape == (N, K)
    sets, weights = _gate_by_hand(logits, bias, n_group, topk_group, K, norm,
                                  scaling)
    if not entry[1]:
        c = torch.sigmoid(logits.float()) + bias
        assert (c < -1.0).any(), "no biased score below the softmax sentinel"
    for n in range(N):
        assert set(idx[n].tolist()) == sets[n], f"row {n}"
        for k in range(K):
            want = weights[n][int(idx[n, k])]
            # same fp32 values, summed in another order
            assert abs(float(w[n, k]) - want) <= 4e-7 * scaling, (n, k)


def test_sigmoid_gate_missing_bias_is_zero():
    case, logits, _ = gc.case_inputs(gc.ZERO_BIAS_ENTRY, True)
    N, E, n_group, topk_group, K, norm, scaling, _ = case
    a = ops.moe_gate(logits, K, n_group, topk_group, scaling, norm,
                     scoring="sigmoid")
    b = ops.moe_gate(logits, K, n_group, topk_group, scaling, norm,
                     scoring="sigmoid", e_bias=torch.zeros(E))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_sigmoid_gate_rejects_one_wide_groups():
    with pytest.raises(ValueError, match="n_group"):
        ops.moe_gate(torch.zeros(2, 8), 2, 8, 4, scoring="sigmoid")
    with pytest.raises(ValueError, match="scoring"):
        ops.moe_gate(torch.zeros(2, 8), 2, scoring="tanh")


def _softmax_gate_as_before(router_logits, top_k, n_group, topk_group,
                            scaling, norm):
    """The softmax gate as it stood before the scoring keyword."""
    scores = torch.softmax(router_logits.float(), dim=-1)
    N, E = scores.shape
    if n_group > 1:
        gscores = scores.reshape(N, n_group, E // n_group)
        top_groups = torch.topk(gscores.max(dim=-1).values, k=topk_group,
                                dim=-1).indices
        gmask = torch.zeros(N, n_group, dtype=torch.bool)
        gmask.scatter_(1, top_groups, True)
        mask = gmask[:, :, None].expand(N, n_group, E // n_group).reshape(N, E)
        scores = scores.masked_fill(~mask, 0.0)
    weights, indices = torch.topk(scores, k=top_k, dim=-1)
    if norm:
        weights = weights / (weights.sum(-1, keepdim=True) + 1e-20)
    return weights * scaling, indices


@pytest.mark.parametrize("case", gc.GRID, ids=gc.GRID_IDS)
def test_softmax_default_unchanged(case):
    N, E, n_group, topk_group, K, norm, scaling, _ = case
    logits = gc.make_logits(N, E)
    old = _softmax_gate_as_before(logits, K, n_group, topk_group, scaling,
                                  norm)
    for fn in (ops.moe_gate, ref.moe_gate):
        pos = fn(logits, K, n_group, topk_group, scaling, norm)
        kw = fn(logits, K, n_group, topk_group, scaling, norm,
                scoring="softmax", e_bias=None)
        for got in (pos, kw):
            assert torch.equal(got[0], old[0]) and torch.equal(got[1], old[1])


# -- 2. independent reference ----------------------------------------------------

_HF_SHAPES = dict(
    vocab_size=128, hidden_size=64, intermediate_size=128,
    moe_intermediate_size=32, num_hidden_layers=3, num_attention_heads=4,
    n_shared_experts=1, n_routed_experts=16, routed_scaling_factor=2.5,
    kv_lora_rank=32, q_lora_rank=24, qk_rope_head_dim=8, v_head_dim=16,
    qk_nope_head_dim=16, n_group=4, topk_group=2, num_experts_per_tok=4,
    first_k_dense_replace=1, norm_topk_prob=True, rms_norm_eps=1e-6)
_YARN = {"factor": 4.0, "beta_fast": 32, "beta_slow": 1, "mscale": 1.0,
         "mscale_all_dim": 1.0, "original_max_position_embeddings": 16}

# max |logit difference| measured against transformers 5.15 on the CPU over
# the prompt and 8 decode steps (logits reach 1.13 in magnitude)
_HF_MEASURED = {"plain": 4.5e-7, "yarn": 7.2e-7}


def _hf_state_to_project_keys(state):
    """transformers' fused expert tensors -> per-expert checkpoint keys
    (`mlp.experts.gate_up_proj` [E, 2I, H] is gate then up)."""
    out = {}
    for k, v in state.items():
        if k.endswith("mlp.experts.gate_up_proj"):
            pre = k[:-len("gate_up_proj")]
            inter = v.shape[1] // 2
            for e in range(v.shape[0]):
                out[f"{pre}{e}.gate_proj.weight"] = v[e, :inter].clone()
                out[f"{pre}{e}.up_proj.weight"] = v[e, inter:].clone()
        elif k.endswith("mlp.experts.down_proj"):
            pre = k[:-len("down_proj")]
            for e in range(v.shape[0]):
                out[f"{pre}{e}.down_proj.weight"] = v[e].clone()
        else:
            out[k] = v.clone()
    return out


@pytest.mark.parametrize("rope", ["plain", "yarn"])
def test_logits_match_transformers_fp32(rope):
    """Prompt of 10 tokens, then 8 greedy steps through the KV cache, fp32
    on both sides: the greedy tokens are equal and the logits differ by
    summation order only.  Measured max |difference|: 4.5e-7 (plain rope)
    and 7.2e-7 (YaRN factor 4, mscale = mscale_all_dim = 1.0) at a logit
    magnitude of 1.13; the bound is 10x the measured value, and far under
    the 1e-3 relative level at which a convention error would show."""
    transformers = pytest.importorskip("transformers")
    kw = {}
    raw = dict(_HF_SHAPES, model_type="deepseek_v3", rope_theta=10000.0,
               topk_method="noaux_tc", scoring_func="sigmoid",
               moe_layer_freq=1)
    if rope == "yarn":
        kw["rope_parameters"] = dict(_YARN, rope_type="yarn",
                                     rope_theta=10000.0)
        raw["rope_scaling"] = dict(_YARN, type="yarn")
    hcfg = transformers.DeepseekV3Config(
        num_key_value_heads=4, max_position_embeddings=64,
        tie_word_embeddings=False, attn_implementation="eager",
        **_HF_SHAPES, **kw)
    hf = transformers.DeepseekV3ForCausalLM(hcfg).float().eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in hf.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            if name.endswith("norm.weight"):
                p.add_(1.0)
        n_bias = 0
        for name, b in list(hf.named_buffers()) + list(hf.named_parameters()):
            if name.endswith("e_score_correction_bias"):
                b.copy_(torch.rand(b.shape, generator=g) * 2 - 1.5)
                n_bias += 1
    assert n_bias == 2
    assert all(p.abs().sum() > 0 for n, p in hf.named_parameters()
               if n.endswith("mlp.gate.weight"))

    cfg = ModelConfig.from_dict(raw)
    model = get_model_class("deepseek_v3")(cfg, cfg.shard(0, 3)).float().eval()
    missing, unexpected = model.load_weights(
        _hf_state_to_project_keys(hf.state_dict()))
    assert not missing and not unexpected

    ids = torch.randint(0, 128, (1, 10),
                        generator=torch.Generator().manual_seed(1))
    cache = model.make_cache(batch_size=1)
    worst = peak = 0.0
    with torch.no_grad():
        out = hf(ids, use_cache=True)
        a, b = out.logits[:, -1], model(ids, cache)[:, -1]
        for step in range(9):
            worst = max(worst, (a - b).abs().max().item())
            peak = max(peak, a.abs().max().item())
            ta, tb = a.argmax(-1), b.argmax(-1)
            assert ta.item() == tb.item(), f"greedy token differs at {step}"
            if step == 8:
                break
            out = hf(ta[:, None], past_key_values=out.past_key_values,
                     use_cache=True)
            a, b = out.logits[:, -1], model(tb[:, None], cache)[:, -1]
    print(f"{rope}: max |logit diff| = {worst:.3e}, max |logit| = {peak:.3f}")
    assert worst <= 1e-3 * peak, "convention error, not noise"
    assert worst <= 10 * _HF_MEASURED[rope]


# -- 3. pipeline parity ----------------------------------------------------------

def _save_checkpoint(model, cfg, path, extra=None):
    from safetensors.torch import save_file
    path.mkdir()
    sd = {k: v.clone() for k, v in model.state_dict().items()
          if "rope_inv_freq" not in k}
    sd.update(extra or {})
    save_file(sd, str(path / "model.safetensors"))
    with open(path / "config.json", "w") as f:
        json.dump(cfg.raw, f)
    return path


@pytest.fixture(scope="module")
def debug_v3_checkpoint(tmp_path_factory):
    cfg = get_preset("debug-deepseek-v3")
    model = init_model(get_model_class("deepseek_v3"), cfg,
                       cfg.shard(0, cfg.num_hidden_layers), seed=21)
    return _save_checkpoint(model, cfg,
                            tmp_path_factory.mktemp("v3") / "dense")


def _greedy_chain(stages, ids, n_decode=6):
    caches = [st.make_cache() for st in stages]
    toks = []
    x = ids
    with torch.no_grad():
        for _ in range(n_decode + 1):
            h = x
            for st, c in zip(stages, caches):
                h = st(h, c)
            x = h[:, -1, :].argmax(-1, keepdim=True)
            toks.append(int(x))
    return toks


@pytest.mark.parametrize("quant", [False, True], ids=["dense", "w4g32"])
def test_pp_parity_debug_v3(debug_v3_checkpoint, quant, tmp_path):
    """PP=1, PP=2 (cut between the dense layer and the MoE layers) and
    PP=3 emit the same greedy tokens."""
    from mlx_sharding_amd.utils.loading import load_model
    cfg = get_preset("debug-deepseek-v3")
    n = cfg.num_hidden_layers
    assert cfg["first_k_dense_replace"] == 1
    ids = torch.randint(0, cfg.vocab_size, (1, 6),
                        generator=torch.Generator().manual_seed(3))
    src = debug_v3_checkpoint
    runs = []
    for splits in ([(0, n)], [(0, 1), (1, n)], [(0, 1), (1, 5), (5, n)]):
        if quant and len(splits) == 1:
            # PP=1 quantizes on load; its weights, saved, are the
            # pre-quantized checkpoint the sharded runs load
            stages = [load_model(src, 0, n, quantize=(4, 32))[0]]
            src = _save_checkpoint(stages[0], stages[0].config,
                                   tmp_path / "w4")
        else:
            stages = [load_model(src, s, e)[0] for s, e in splits]
        if quant:
            moe = stages[-1].model.layers[str(n - 1)].mlp
            assert moe.switch_mlp.quant is not None
            assert moe.e_score_correction_bias.dtype == torch.float32
        runs.append(_greedy_chain(stages, ids))
    assert runs[0] == runs[1] == runs[2], runs


def test_q_lora_projections_fuse_for_v3_only(debug_v3_checkpoint):
    from mlx_sharding_amd.utils.loading import load_model
    m, _ = load_model(debug_v3_checkpoint, 0, 2)
    assert all(l.self_attn._fused_qkv is not None
               for l in m.model.layers.values())
    v2 = get_preset("debug-deepseek")
    v2.raw["q_lora_rank"] = 48
    m2 = init_model(get_model_class("deepseek_v2"), v2, v2.shard(0, 2))
    from mlx_sharding_amd.models.fuse import fuse_model
    fuse_model(m2)
    assert all(l.self_attn._fused_qkv is None
               for l in m2.model.layers.values())


# -- 4. splitter and checkpoint keys ---------------------------------------------

def test_splitter_round_trip_keeps_bias_and_drops_extras(tmp_path):
    from safetensors.torch import load_file
    from mlx_sharding_amd.utils.loading import load_model, save_sharded_weights

    cfg = get_preset("debug-deepseek-v3")
    n = cfg.num_hidden_layers
    full = init_model(get_model_class("deepseek_v3"), cfg, cfg.shard(0, n),
                      seed=4)
    # what a published checkpoint carries besides the model proper: the
    # recomputed rotary buffer and a multi-token-prediction layer
    extra = {
        "model.layers.2.self_attn.rotary_emb.inv_freq": torch.ones(8),
        f"model.layers.{n}.embed_tokens.weight": torch.ones(4, 4),
        f"model.layers.{n}.mlp.gate.e_score_correction_bias": torch.ones(96),
        f"model.layers.{n}.eh_proj.weight": torch.ones(4, 8),
    }
    src = _save_checkpoint(full, cfg, tmp_path / "src", extra)
    bias_key = "model.layers.{}.mlp.gate.e_score_correction_bias"

    cut = 3
    for s, e in ((0, cut), (cut, n)):
        out = tmp_path / f"shard_{s}_{e}"
        kept = load_file(str(save_sharded_weights(src, out, s, e)))
        assert not any(int(k.split(".")[2]) >= n for k in kept
                       if k.startswith("model.layers."))
        for i in range(n):
            has = bias_key.format(i) in kept
            assert has == (s <= i < e and i >= 1), (s, e, i)
        stage, _ = load_model(out)     # strict: no unexpected key survives
        assert not any("inv_freq" in k for k in stage.state_dict()
                       if "rope_inv_freq" not in k)
        for i in range(max(s, 1), e):
            got = stage.model.layers[str(i)].mlp.e_score_correction_bias
            want = full.model.layers[str(i)].mlp.e_score_correction_bias
            assert got.dtype == torch.float32 and torch.equal(got, want)

    # a model dtype on load must not round the bias
    stage, _ = load_model(src, cut, n, dtype=torch.bfloat16)
    got = stage.model.layers[str(cut)].mlp.e_score_correction_bias
    assert got.dtype == torch.float32
    assert torch.equal(got,
                       full.model.layers[str(cut)].mlp.e_score_correction_bias)


def test_embed_q_checkpoint_is_refused(tmp_path):
    from mlx_sharding_amd.utils.loading import load_model
    cfg = get_preset("debug-deepseek-v3")
    full = init_model(get_model_class("deepseek_v3"), cfg, cfg.shard(0, 2))
    src = _save_checkpoint(full, cfg, tmp_path / "src", {
        "model.layers.0.self_attn.embed_q.weight": torch.ones(4, 4),
        "model.layers.0.self_attn.unembed_out.weight": torch.ones(4, 4)})
    with pytest.raises(ValueError, match="embed_q/unembed_out"):
        load_model(src, 0, 2)


# -- 5. config errors --------------------------------------------------------------

@pytest.mark.parametrize("field,value", [
    ("scoring_func", "softmax"), ("topk_method", "group_limited_greedy"),
    ("topk_method", "greedy")])
def test_unknown_router_config_raises(field, value):
    cfg = get_preset("debug-deepseek-v3")
    cfg.raw[field] = value
    with pytest.raises(ValueError, match=value):
        get_model_class("deepseek_v3")(cfg, cfg.shard(0, 2))


def test_v3_router_defaults():
    from mlx_sharding_amd.models.deepseek_v3 import DeepseekV3MoE
    raw = {"model_type": "deepseek_v3", "hidden_size": 32,
           "num_hidden_layers": 2, "moe_intermediate_size": 16}
    with torch.device("meta"):
        moe = DeepseekV3MoE(ModelConfig.from_dict(raw), lambda p: None,
                            "model.layers.1.mlp")
    assert (moe.n_experts, moe.top_k, moe.n_group, moe.topk_group) == (
        256, 8, 8, 4)
    assert moe.norm_topk_prob and moe.routed_scaling_factor == 2.5
    assert moe._gate_groups() == (8, 4) and moe._fused_gate_ok(64)
    assert moe._gate_kwargs()["scoring"] == "sigmoid"


def test_registry_and_presets():
    from mlx_sharding_amd.models.deepseek_v3 import DeepseekV3StageModel
    assert get_model_class("deepseek_v3") is DeepseekV3StageModel
    v3 = get_preset("deepseek-v3").raw
    assert (v3["hidden_size"], v3["num_hidden_layers"],
            v3["num_attention_heads"]) == (7168, 61, 128)
    assert (v3["q_lora_rank"], v3["kv_lora_rank"]) == (1536, 512)
    assert (v3["n_routed_experts"], v3["moe_intermediate_size"],
            v3["first_k_dense_replace"]) == (256, 2048, 3)
    dbg = get_preset("debug-deepseek-v3").raw
    assert (dbg["n_routed_experts"], dbg["n_group"], dbg["topk_group"],
            dbg["num_experts_per_tok"], dbg["num_attention_heads"]) == (
        96, 8, 3, 4, 32)


# -- 6. continuous batching --------------------------------------------------------

def test_scheduler_matches_sequential_generation():
    from mlx_sharding_amd.parallel.batching import BatchScheduler
    from mlx_sharding_amd.parallel.engine import SamplingParams, generate_step

    cfg = get_preset("debug-deepseek-v3")
    model = init_model(get_model_class("deepseek_v3"), cfg,
                       cfg.shard(0, cfg.num_hidden_layers), seed=9)
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
               for n in (3, 8, 5)]
    budgets = (7, 5, 6)

    want = []
    for p, n in zip(prompts, budgets):
        gen = generate_step(torch.tensor([p]), model,
                            model.make_cache(batch_size=1))
        want.append([next(gen)[0] for _ in range(n)])

    sched = BatchScheduler(model, max_batch=3, capacity=32)
    got = {}
    started = [threading.Event() for _ in prompts]
    try:
        def worker(i):
            def run():
                # staggered: request i joins once request i-1 is decoding
                if i:
                    assert started[i - 1].wait(JOIN_S)
                out = []
                for tid, _ in sched.submit(
                        prompts[i], SamplingParams(max_tokens=budgets[i])):
                    out.append(tid)
                    started[i].set()
                got[i] = out
                started[i].set()
            return run

        ths = [threading.Thread(target=worker(i)) for i in range(3)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(JOIN_S)
        assert not any(t.is_alive() for t in ths), "a request stream hung"
    finally:
        sched.close()
    for i in range(3):
        assert got[i] == want[i], f"request {i}"
