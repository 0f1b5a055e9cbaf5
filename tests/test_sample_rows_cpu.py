"""ops.sample_rows on the CPU: the torch reference against the fp64
specification of sample_cases.py, the margins of the cases against a
worst-order fp32 evaluation, negative controls, the scheduler's
eligibility rule and the equality of the edits with BatchScheduler._emit's
per-row tensors."""

import numpy as np
import pytest
import torch

import sample_cases as sc
from mlx_sharding_amd import ops
from mlx_sharding_amd.ops import reference as ref
from mlx_sharding_amd.parallel import batching
from mlx_sharding_amd.parallel.engine import SamplingParams

f32 = np.float32
ALL = sc.cases() + sc.dyadic_cases()
IDS = [c["name"] for c in ALL]


def _run_ref(case):
    a = sc.torch_args(case)
    ops.sample_rows(**a)          # CPU tensors: the reference
    return a


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_reference_equals_fp64_spec(case):
    a = _run_ref(case)
    assert a["ids_out"].tolist() == case["want_ids"].tolist()
    assert np.array_equal(a["logits"].numpy(), case["want_logits"])
    assert np.abs(a["lse_out"].numpy() - case["want_lse"]).max() <= 2e-4
    for b, keep in enumerate(case["want_keep"]):
        if keep is None or float(case["top_p"][b]) >= 1.0:
            continue
        p = torch.softmax(a["logits"][b] / a["temperature"][b], dim=-1)
        got = ref.nucleus_keep(p, float(case["top_p"][b])).numpy()
        assert np.array_equal(got, keep), (case["name"], b)


def test_reference_accepts_a_column_of_ids():
    case = sc.cases()[2]
    a = sc.torch_args(case)
    a["ids_out"] = a["ids_out"].view(-1, 1)
    ops.sample_rows(**a)
    assert a["ids_out"].view(-1).tolist() == case["want_ids"].tolist()


def _sequential_fp32_ids(case):
    """The specification evaluated in fp32 with strictly sequential sums
    (np.cumsum accumulates left to right): the worst summation order."""
    logits = case["want_logits"]
    ids = case["ids_init"].copy()
    for b in range(len(ids)):
        if not case["active"][b]:
            continue
        x, T = logits[b], f32(case["temperature"][b])
        if T <= 0:
            ids[b] = int(np.argmax(x))
            continue
        e = np.exp((x - x.max()) / T).astype(f32)
        p = (e / np.cumsum(e, dtype=f32)[-1]).astype(f32)
        keep = np.ones(len(p), dtype=bool)
        if case["top_p"][b] < 1.0:
            order = np.argsort(-p, kind="stable")
            sp = p[order]
            excl = np.cumsum(sp, dtype=f32) - sp
            # a tie class shares the exclusive sum of its first member
            first = np.concatenate([[True], sp[1:] != sp[:-1]])
            above = excl[np.maximum.accumulate(
                np.where(first, np.arange(len(sp)), 0))]
            keep[order] = above < case["top_p"][b]
            keep[p == sp[0]] = True
        cdf = np.cumsum(np.where(keep, p, f32(0)), dtype=f32)
        hit = np.nonzero(keep & (cdf > f32(case["u"][b]) * cdf[-1]))[0]
        ids[b] = hit[0] if len(hit) else np.nonzero(keep)[0][-1]
    return ids


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_sequential_fp32_picks_the_same_ids(case):
    assert _sequential_fp32_ids(case).tolist() == case["want_ids"].tolist()


def test_kept_set_is_top_p_samples_on_tie_free_rows():
    rng = np.random.default_rng(3)
    for V, T, scale in ((63, 1.0, 2), (1000, 0.5, 3), (4099, 1.7, 5)):
        x = sc.normal_row(V, T, scale, rng)
        assert len(np.unique(x)) == V
        top_p = float(sc.design_top_p(x, T, "mid", sel=V))
        lg = torch.from_numpy(x)[None]
        # ref.top_p_sample's own kept set, in vocabulary order
        probs = torch.softmax(lg.float() / T, dim=-1)
        sp, si = torch.sort(probs, descending=True, dim=-1)
        keep_sorted = torch.cumsum(sp, dim=-1) - sp < top_p
        keep_sorted[..., 0] = True
        want = torch.zeros(V, dtype=torch.bool)
        want[si[0]] = keep_sorted[0]
        assert torch.equal(ref.nucleus_keep(probs[0], top_p), want)
        assert np.array_equal(sc.keep_set(sc.softmax64(x, T), top_p),
                              want.numpy())


def test_stratified_draws_follow_the_distribution():
    """u_k = (k + 0.5) / N over a 63-token row: token i is picked
    N * p_i / Z times, within 1."""
    N, V, T = 4096, 63, 1.0
    x = sc.normal_row(V, T, 2, np.random.default_rng(9))
    # a mid-gap top_p that keeps several tokens and drops several
    top_p = next(tp for tp in (float(sc.design_top_p(x, T, "mid", sel=s))
                               for s in range(V))
                 if 8 <= sc.keep_set(sc.softmax64(x, T), tp).sum() < V - 8)
    logits = torch.from_numpy(x)[None].repeat(N, 1).contiguous()
    ids = torch.zeros(N, dtype=torch.int64)
    ops.sample_rows(logits, torch.full((N,), T), torch.full((N,), top_p),
                    (torch.arange(N, dtype=torch.float64) + 0.5).div(N)
                    .float(), torch.ones(N, dtype=torch.int32), ids,
                    torch.zeros(N))
    p = sc.softmax64(x, T)
    keep = sc.keep_set(p, float(f32(top_p)))
    assert 1 < keep.sum() < V
    want = N * np.where(keep, p, 0.0) / p[keep].sum()
    got = np.bincount(ids.numpy(), minlength=V)
    assert np.abs(got - want).max() <= 1.0, np.abs(got - want).max()
    assert got[~keep].sum() == 0


# -- negative controls: each wrong reading of the spec fails the cases --------

def _mismatches(cases, **controls):
    bad = []
    for case in cases:
        logits, ids, _, _ = sc.spec_case(case, **controls)
        if (ids.tolist() != case["want_ids"].tolist()
                or not np.array_equal(logits, case["want_logits"])):
            bad.append(case["name"])
    return bad


def test_control_nucleus_ignored_fails():
    assert len(_mismatches(sc.cases(), ignore_nucleus=True)) >= 5


def test_control_pick_with_ge_fails():
    # only an exact hit of u * Z on a CDF step tells > from >=: the margin
    # of the designed cases rules that out, the dyadic cases are built on it
    assert _mismatches(sc.cases(), pick_ge=True) == []
    assert _mismatches(sc.dyadic_cases(), pick_ge=True) == \
        [c["name"] for c in sc.dyadic_cases()]


def test_control_penalty_per_occurrence_fails():
    assert _mismatches(sc.cases(), per_occurrence=True) == ["edits-V1000"]


# -- scheduler ------------------------------------------------------------------

def _sampled(**kw):
    flags = dict(on_gpu=True, native=True, disabled=False)
    flags.update({k: kw.pop(k) for k in list(kw) if k in flags})
    return batching.device_sampled(SamplingParams(**kw), **flags)


def test_eligibility_truth_table():
    assert _sampled(temperature=1.0)
    assert _sampled(temperature=0.8, top_p=0.9)
    # not plain greedy: temperature 0 with an edit
    assert _sampled(temperature=0.0, logit_bias={3: 1.0})
    assert _sampled(temperature=0.0, repetition_penalty=1.2)
    assert not _sampled(temperature=0.0)
    assert not _sampled(temperature=0.0, repetition_penalty=1.0)
    assert not _sampled(temperature=1.0, seed=0)
    assert not _sampled(temperature=1.0, on_gpu=False)
    assert not _sampled(temperature=1.0, native=False)
    assert not _sampled(temperature=1.0, disabled=True)
    bias = {k: 0.5 for k in range(33)}
    assert not _sampled(temperature=1.0, logit_bias=bias)
    bias.pop(32)
    assert _sampled(temperature=1.0, logit_bias=bias)
    assert _sampled(temperature=1.0, repetition_penalty=1.1,
                    repetition_context_size=64)
    assert not _sampled(temperature=1.0, repetition_penalty=1.1,
                        repetition_context_size=65)
    # size 0 penalizes the whole context
    assert not _sampled(temperature=1.0, repetition_penalty=1.1,
                        repetition_context_size=0)
    # without a penalty the window does not matter
    assert _sampled(temperature=1.0, repetition_context_size=4096)
    assert _sampled(temperature=1.0, repetition_penalty=1.0,
                    repetition_context_size=0)


def test_env_switch(monkeypatch):
    monkeypatch.delenv("MLXS_AMD_NO_FUSED_SAMPLE", raising=False)
    assert not batching.fused_sample_disabled()
    monkeypatch.setenv("MLXS_AMD_NO_FUSED_SAMPLE", "1")
    assert batching.fused_sample_disabled()


def test_cpu_scheduler_has_no_row_sampler():
    import ragged_cases as rc
    sched = batching.BatchScheduler(rc.build_model("llama"), max_batch=2,
                                    capacity=16)
    try:
        assert sched._sampler is None
        out = list(sched.submit([1, 2, 3], SamplingParams(
            temperature=0.8, top_p=0.9, max_tokens=3)))
        assert len(out) == 3
    finally:
        sched.close()


def test_edits_equal_emits_tensors_bit_for_bit():
    """Step 1 against the tensors BatchScheduler._emit builds for a
    request: logit_bias, then ops.apply_repetition_penalty over the
    window."""
    torch.manual_seed(4)
    V = 257
    bias = {5: 2.5, 200: -1.25, 17: 0.3}
    window = [9, 200, 9, 31, 256, 200]
    pen = 1.3
    base = torch.randn(1, V) * 3
    # _emit's sequence
    lg = base.clone()
    lg[0, torch.tensor(list(bias.keys()))] += torch.tensor(
        list(bias.values()), dtype=lg.dtype)
    lg = ops.apply_repetition_penalty(lg, torch.tensor(window), pen)
    # sample_rows
    NB, W = ops.SAMPLE_ROWS_MAX_BIAS, ops.SAMPLE_ROWS_MAX_WINDOW
    bi = torch.full((1, NB), -1, dtype=torch.int32)
    bv = torch.zeros(1, NB)
    bi[0, :3] = torch.tensor(list(bias.keys()), dtype=torch.int32)
    bv[0, :3] = torch.tensor(list(bias.values()))
    pi = torch.full((1, W), -1, dtype=torch.int32)
    pi[0, :len(window)] = torch.tensor(window, dtype=torch.int32)
    got = base.clone()
    ids, lse = torch.zeros(1, dtype=torch.int64), torch.zeros(1)
    ops.sample_rows(got, torch.zeros(1), torch.ones(1), torch.zeros(1),
                    torch.ones(1, dtype=torch.int32), ids, lse, bi, bv, pi,
                    torch.tensor([pen]))
    assert torch.equal(got, lg)
    assert not torch.equal(got, base)
    assert ids.item() == lg.argmax().item()
    assert abs(lse.item() - torch.logsumexp(lg, -1).item()) < 1e-5
