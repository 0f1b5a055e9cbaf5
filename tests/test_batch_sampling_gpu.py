"""The batched sampler inside BatchScheduler on the GPU: which requests
it serves (a spy on the extension's sample_rows records every launch and
its active rows), that it follows the nucleus rule on the logprobs it
yields, and that greedy and seeded requests keep their own paths.

debug-llama (V = 1024), max_batch = 3."""

import threading

import numpy as np
import pytest
import torch

import ragged_cases as rc
from mlx_sharding_amd import ops
from mlx_sharding_amd.parallel.batching import BatchScheduler
from mlx_sharding_amd.parallel.engine import SamplingParams

pytestmark = pytest.mark.gpu

N_TOK = 6
SLACK = 2e-3   # sample_cases.MARGIN: 16 x the worst fp32 CDF error


class _Spy:
    """The HIP extension with every sample_rows launch recorded as the
    list of its active flags."""

    def __init__(self, real):
        self._real, self.launches = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "sample_rows":
            return fn

        def wrapped(*a, **k):
            self.launches.append(a[4].tolist())
            return fn(*a, **k)
        return wrapped


@pytest.fixture(scope="module")
def model():
    return rc.build_model("debug-llama", "cuda")


@pytest.fixture
def spy(monkeypatch):
    monkeypatch.delenv("MLXS_AMD_NO_FUSED_SAMPLE", raising=False)
    monkeypatch.delenv("MLXS_AMD_FORCE_TORCH", raising=False)
    real = ops.hip_ext()
    assert real is not None, "HIP extension must be built on a GPU box"
    s = _Spy(real)
    monkeypatch.setattr(ops, "_EXT", s)
    return s


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (n,), generator=g).tolist()


def _stream(sched, prompt, **params):
    """(token ids, fp64 logprobs [n, V]) of one request."""
    out = list(sched.submit(prompt, SamplingParams(max_tokens=N_TOK,
                                                   **params)))
    return ([t for t, _ in out],
            np.stack([lp.double().cpu().numpy() for _, lp in out]))


def _top_gap(lp):
    top2 = np.sort(lp, axis=-1)[:, -2:]
    return (top2[:, 1] - top2[:, 0]).min()


def test_tiny_top_p_is_greedy(model, spy):
    sched = BatchScheduler(model, max_batch=3, capacity=64)
    try:
        # the first seeded prompt whose greedy run has no tie for the
        # top-1 (bf16 logits over 1024 tokens do tie now and then)
        for seed in range(16):
            prompt = _prompt(7, seed)
            greedy, lp = _stream(sched, prompt)
            if _top_gap(lp) > 0:
                break
        else:
            pytest.fail("no prompt with a tie-free greedy run")
        assert spy.launches == []      # plain greedy launches nothing new
        got, lp = _stream(sched, prompt, temperature=0.8, top_p=1e-6)
        assert _top_gap(lp) > 0
        assert got == greedy
        # the admission at B = 1, then one launch per decode step
        assert len(spy.launches) == N_TOK
        assert spy.launches[0] == [1]
        assert all(sum(a) == 1 and len(a) == 3 for a in spy.launches[1:])
    finally:
        sched.close()


def _nucleus_ok(tid, lp, temperature, top_p):
    z = lp / temperature
    p = np.exp(z - z.max())
    p /= p.sum()
    return p[p > p[tid]].sum() < top_p + SLACK


def test_sampled_rows_beside_a_greedy_one(model, spy):
    sched = BatchScheduler(model, max_batch=3, capacity=64)
    try:
        g_prompt = _prompt(5, 100)
        alone, _ = _stream(sched, g_prompt)
        got = {}

        def run(key, prompt, **params):
            def fn():
                got[key] = _stream(sched, prompt, **params)
            return threading.Thread(target=fn)

        ths = [run("s0", _prompt(4, 101), temperature=0.8, top_p=0.9),
               run("g", g_prompt),
               run("s1", _prompt(9, 102), temperature=0.8, top_p=0.9)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(60)
        assert not any(t.is_alive() for t in ths), "a request stream hung"
        assert got["g"][0] == alone
        for key in ("s0", "s1"):
            toks, lps = got[key]
            assert len(toks) == N_TOK
            for tid, lp in zip(toks, lps):
                assert abs(np.exp(lp).sum() - 1.0) <= 1e-4
                assert _nucleus_ok(tid, lp, 0.8, 0.9), (key, tid)
        # never a greedy row among the active ones: at most the two
        assert spy.launches and all(sum(a) <= 2 for a in spy.launches)
    finally:
        sched.close()


def test_seeded_request_keeps_the_cpu_generator(model, spy, monkeypatch):
    """A seeded request draws what generate_step's sampling line draws.
    generate_step itself cannot be the reference on a GPU model: it hands
    its CPU generator to multinomial over GPU logits, which raises (the
    scheduler moves the row to the CPU first).  So its line
    ``ops.sample(logits, temperature, top_p, gen)`` is replayed here with
    a fresh generator of the same seed over the logprobs yielded with
    every token, and the stream is compared with the per-row path the
    env switch restores."""
    params = dict(temperature=0.8, top_p=0.9, seed=1234)
    prompt = _prompt(6, 42)
    sched = BatchScheduler(model, max_batch=3, capacity=64)
    try:
        got, lps = _stream(sched, prompt, **params)
        assert spy.launches == []
        gen = torch.Generator(device="cpu").manual_seed(params["seed"])
        want = [int(ops.sample(torch.from_numpy(lp)[None].float(), 0.8, 0.9,
                               gen).item()) for lp in lps]
        assert got == want
        monkeypatch.setenv("MLXS_AMD_NO_FUSED_SAMPLE", "1")
        assert _stream(sched, prompt, **params)[0] == got
        assert spy.launches == []
    finally:
        sched.close()


def test_env_switch_keeps_the_per_row_path(model, spy, monkeypatch):
    monkeypatch.setenv("MLXS_AMD_NO_FUSED_SAMPLE", "1")
    sched = BatchScheduler(model, max_batch=3, capacity=64)
    try:
        toks, lps = _stream(sched, _prompt(5, 7), temperature=0.8, top_p=0.9)
        assert len(toks) == N_TOK
        assert spy.launches == []
    finally:
        sched.close()
