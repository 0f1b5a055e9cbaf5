"""Continuous batching on the CPU path: ragged batched decode through
the models, the slot scheduler, and the API server with --max-batch."""

import http.client
import json
import threading
import time

import pytest
import torch

import ragged_cases as rc
from mlx_sharding_amd.parallel.batching import BatchScheduler
from mlx_sharding_amd.parallel.engine import SamplingParams, generate_step
from mlx_sharding_amd.utils import metrics

JOIN_S = 60  # generous bound for joins; nothing here waits it out


# -- 1. model-level parity ---------------------------------------------------

@pytest.mark.parametrize("name", ["llama", "gemma2", "debug-deepseek"])
def test_ragged_decode_rows_bit_equal_solo(name):
    model = rc.build_model(name)
    prompts, forced = rc.sequences(model.config.vocab_size)
    got = rc.ragged_run(model, prompts, forced)
    for i, (prompt, f) in enumerate(zip(prompts, forced)):
        want = rc.solo_run(model, prompt, f)
        assert len(got[i]) == len(want) == 1 + rc.N_STEPS
        for step, (a, b) in enumerate(zip(got[i], want)):
            assert torch.equal(a, b), (
                f"{name} seq {i} step {step}: max diff "
                f"{(a - b).abs().max().item()}")


def test_slot_view_shares_pool_rows_and_has_fixed_capacity():
    from mlx_sharding_amd.ops.kvcache import KVCache
    pool = KVCache(2, 8, 8, dtype=torch.float32, batch_size=3)
    pool.allocate(16, 3)
    assert pool.capacity == 16
    view = pool.slot(1)
    k = torch.randn(1, 2, 5, 8)
    view.update(k, k * 2)
    assert view.offset == 5 and view.capacity == 16
    assert torch.equal(pool.keys_buffer()[1, :, :5], k[0])
    assert pool.keys_buffer()[0].abs().sum() == 0
    assert pool.keys_buffer()[2].abs().sum() == 0
    assert view.keys_buffer().is_contiguous()
    with pytest.raises(ValueError):
        view.update(torch.randn(1, 2, 12, 8), torch.randn(1, 2, 12, 8))
    with pytest.raises(IndexError):
        pool.slot(3)


def test_rope_for_per_sequence_tables():
    model = rc.build_model("llama")
    cache = model.make_cache(batch_size=3)
    for c in cache:
        c.allocate(16, 3)
        c.graph_pos = torch.tensor([0, 5, 9], dtype=torch.int32)
    cos, sin, off = model.rope_for(cache[0], 1, torch.device("cpu"))
    table_cos, table_sin = model._rope_tables(torch.device("cpu"), 16)
    assert cos.shape == sin.shape == (3, 1, table_cos.shape[1]) and off == 0
    assert torch.equal(cos[:, 0], table_cos[[0, 5, 9]])
    assert torch.equal(sin[:, 0], table_sin[[0, 5, 9]])


# -- scheduler helpers -------------------------------------------------------

@pytest.fixture(scope="module")
def llama():
    return rc.build_model("llama")


def _alone(model, prompt, params, n):
    out = []
    gen = generate_step(torch.tensor([prompt]), model,
                        model.make_cache(batch_size=1), params=params)
    for tid, _ in gen:
        out.append(tid)
        if len(out) >= n:
            break
    return out


def _prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 128, (n,), generator=g).tolist()


def _run_threads(fns):
    ths = [threading.Thread(target=f) for f in fns]
    for t in ths:
        t.start()
    for t in ths:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in ths), "a request stream hung"


# -- 2. scheduler parity -----------------------------------------------------

def test_scheduler_streams_equal_single_generation(llama):
    sched = BatchScheduler(llama, max_batch=2, capacity=64)
    try:
        lengths = (2, 4, 7, 9, 11)
        budgets = (3, 5, 6, 8, 9)
        prompts = [_prompt(n, 100 + n) for n in lengths]
        got = {}

        def worker(i):
            def run():
                time.sleep(0.005 * i)  # staggered arrivals
                sp = SamplingParams(max_tokens=budgets[i])
                got[i] = [t for t, _ in sched.submit(prompts[i], sp)]
            return run

        steps0 = metrics.batching_metrics()["decode_steps"].value
        _run_threads([worker(i) for i in range(5)])
        for i in range(5):
            want = _alone(llama, prompts[i], SamplingParams(), budgets[i])
            assert got[i] == want, f"request {i}"
        # five requests over two slots: some queued and slots were reused
        assert metrics.batching_metrics()["decode_steps"].value > steps0
    finally:
        sched.close()


def test_scheduler_logprobs_match_single_generation(llama):
    sched = BatchScheduler(llama, max_batch=2, capacity=64)
    try:
        p = _prompt(5, 7)
        got = list(sched.submit(p, SamplingParams(max_tokens=3)))
        gen = generate_step(torch.tensor([p]), llama,
                            llama.make_cache(batch_size=1))
        for (tid, lp), (wtid, wlp) in zip(got, gen):
            assert tid == wtid
            assert lp.shape == wlp.shape
            assert torch.equal(lp, wlp)
    finally:
        sched.close()


# -- 3. sampling ---------------------------------------------------------------

@pytest.mark.parametrize("params", [
    dict(temperature=0.8, top_p=0.9, seed=1234),
    dict(temperature=0.0, repetition_penalty=1.3, repetition_context_size=4,
         logit_bias={5: 4.0, 17: -3.0}),
    dict(temperature=0.7, seed=5, repetition_penalty=1.2,
         logit_bias={9: 2.5}),
])
def test_sampled_request_same_alone_and_in_a_shared_batch(llama, params):
    n = 8
    p = _prompt(6, 42)
    want = _alone(llama, p, SamplingParams(**params), n)
    sched = BatchScheduler(llama, max_batch=3, capacity=64)
    try:
        alone = [t for t, _ in sched.submit(
            p, SamplingParams(max_tokens=n, **params))]
        got = {}

        def sampled():
            got["s"] = [t for t, _ in sched.submit(
                p, SamplingParams(max_tokens=n, **params))]

        def greedy(i):
            def run():
                got[i] = [t for t, _ in sched.submit(
                    _prompt(3 + 4 * i, i), SamplingParams(max_tokens=10))]
            return run

        _run_threads([greedy(0), sampled, greedy(1)])
        assert alone == want
        assert got["s"] == want
        for i in (0, 1):
            assert got[i] == _alone(llama, _prompt(3 + 4 * i, i),
                                    SamplingParams(), 10)
    finally:
        sched.close()


# -- 4. lifecycle --------------------------------------------------------------

def test_closing_a_stream_frees_its_slot(llama):
    sched = BatchScheduler(llama, max_batch=1, capacity=64)
    try:
        first = sched.submit(_prompt(4, 1), SamplingParams())  # no budget
        assert len([next(first) for _ in range(3)]) == 3
        queued = sched.submit(_prompt(5, 2), SamplingParams(max_tokens=4))
        out = {}

        def consume():
            out["q"] = [t for t, _ in queued]

        th = threading.Thread(target=consume)
        th.start()
        first.close()
        th.join(JOIN_S)
        assert not th.is_alive(), "queued request never got the slot"
        assert out["q"] == _alone(llama, _prompt(5, 2), SamplingParams(), 4)
    finally:
        sched.close()


def test_capacity_stop_never_writes_past_the_slot(llama):
    cap = 16
    sched = BatchScheduler(llama, max_batch=2, capacity=cap)
    try:
        p = _prompt(10, 3)
        toks = [t for t, _ in sched.submit(p, SamplingParams(max_tokens=50))]
        # first token from the prefill, then one per append at rows
        # 10..14; at position capacity-1 the stream ends with no further
        # append
        assert len(toks) == cap - 1 - len(p) + 1
        assert toks == _alone(llama, p, SamplingParams(), len(toks))
        for c in sched.caches:
            assert c.capacity == cap and c.keys_buffer().shape[2] == cap
            # the last row was never appended to (pool starts zeroed)
            assert c.keys_buffer()[:, :, cap - 1].abs().sum() == 0
        # a slot view cannot grow: writing at index >= capacity raises
        view = sched.caches[0].slot(0)
        view.offset = cap
        k = torch.zeros(1, view.n_kv_heads, 1, view.k_head_dim,
                        dtype=view.dtype)
        with pytest.raises(ValueError):
            view.update(k, k)
    finally:
        sched.close()


def test_prompt_longer_than_capacity_rejected(llama):
    sched = BatchScheduler(llama, max_batch=2, capacity=16)
    try:
        with pytest.raises(ValueError):
            sched.submit(_prompt(16, 0), SamplingParams())
        # capacity - 1 prompt tokens still fit: one token, then full
        assert len(list(sched.submit(_prompt(15, 0), SamplingParams()))) == 1
    finally:
        sched.close()


def test_max_batch_limits(llama):
    for bad in (0, 65):
        with pytest.raises(ValueError):
            BatchScheduler(llama, max_batch=bad, capacity=16)


def test_forward_error_reaches_every_waiter():
    class Boom(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner
            self.config = inner.config
            self.shard = inner.shard

        def make_cache(self, **kw):
            return self.inner.make_cache(**kw)

        def forward(self, x, cache):
            raise RuntimeError("boom")

    sched = BatchScheduler(Boom(rc.build_model("llama")), max_batch=2,
                           capacity=32)
    errors = {}

    def waiter(i):
        def run():
            try:
                list(sched.submit(_prompt(3 + i, i),
                                  SamplingParams(max_tokens=4)))
            except RuntimeError as e:
                errors[i] = str(e)
        return run

    _run_threads([waiter(i) for i in range(4)])
    assert sorted(errors) == [0, 1, 2, 3]
    assert all("boom" in m for m in errors.values())
    # and a request submitted after the failure is told, not left hanging
    with pytest.raises(RuntimeError, match="boom"):
        list(sched.submit(_prompt(3, 9), SamplingParams(max_tokens=2)))


# -- 5. API --------------------------------------------------------------------

def _make_ckpt(tmp):
    """The tiny llama checkpoint + word-level tokenizer of
    test_openai_api.py's fixture."""
    from safetensors.torch import save_file
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace

    from mlx_sharding_amd.config import ModelConfig
    from mlx_sharding_amd.models import get_model_class

    ckpt = tmp / "ckpt"
    ckpt.mkdir()
    vocab = {"<unk>": 0, "<eos>": 1, "hello": 2, "world": 3, "STOPWORD": 4}
    vocab.update({f"tok{i}": 5 + i for i in range(123)})
    tok = Tokenizer(WordLevel(vocab, unk_token="<unk>"))
    tok.pre_tokenizer = Whitespace()
    tok.save(str(ckpt / "tokenizer.json"))
    with open(ckpt / "tokenizer_config.json", "w") as f:
        json.dump({"tokenizer_class": "PreTrainedTokenizerFast",
                   "eos_token": "<eos>", "unk_token": "<unk>"}, f)
    cfg_raw = {
        "model_type": "llama", "hidden_size": 64, "num_hidden_layers": 2,
        "intermediate_size": 128, "num_attention_heads": 4,
        "num_key_value_heads": 2, "vocab_size": 128,
        "rms_norm_eps": 1e-5, "rope_theta": 10000.0,
    }
    with open(ckpt / "config.json", "w") as f:
        json.dump(cfg_raw, f)
    cfg = ModelConfig.from_dict(cfg_raw)
    torch.manual_seed(0)
    m = get_model_class("llama")(cfg, cfg.shard(0, 2))
    for p in m.parameters():
        p.data = p.data.float().normal_(0, 0.05).to(p.dtype)
    sd = {k: v for k, v in m.state_dict().items() if "rope_inv_freq" not in k}
    save_file(sd, str(ckpt / "model.safetensors"))
    return ckpt


def _serve(ckpt, **extra):
    from mlx_sharding_amd.server import openai_api

    class Args:
        model = str(ckpt)
        llm_shard_addresses = ""
        start_layer = None
        end_layer = None

    args = Args()
    for k, v in extra.items():
        setattr(args, k, v)
    provider = openai_api.ModelProvider(args)
    server = openai_api.run("127.0.0.1", 0, provider)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    return server, provider


@pytest.fixture(scope="module")
def servers(tmp_path_factory, monkeypatch_module):
    monkeypatch_module.setenv("MLXS_AMD_SERVE_CAPACITY", "64")
    ckpt = _make_ckpt(tmp_path_factory.mktemp("batch_api"))
    # both servers load on the CPU wherever the suite runs: text equality
    # between a B=1 and a batched server holds on the CPU path only (on
    # the GPU, M=1 and M=3 take different GEMM kernels)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "is_available", lambda: False)
        seq, seq_provider = _serve(ckpt)
        bat, bat_provider = _serve(ckpt, max_batch=3)
    yield (seq.server_address[1], bat.server_address[1], seq_provider,
           bat_provider, ckpt)
    seq.shutdown()
    bat.shutdown()
    bat_provider._scheduler.close()


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _post(port, body):
    conn = http.client.HTTPConnection("127.0.0.1", port, timeout=JOIN_S)
    conn.request("POST", "/v1/completions", json.dumps(body),
                 {"Content-Type": "application/json"})
    resp = conn.getresponse()
    data = resp.read()
    conn.close()
    return resp.status, data


def _text(status, data, stream):
    assert status == 200, data
    if not stream:
        return json.loads(data)["choices"][0]["text"]
    frames = [f for f in data.decode().split("\n\n") if f.startswith("data: ")]
    assert frames[-1] == "data: [DONE]"
    chunks = [json.loads(f[6:]) for f in frames[:-1]]
    assert chunks[-1]["choices"][0]["finish_reason"] in ("length", "stop")
    return "".join(c["choices"][0]["text"] for c in chunks)


PROMPTS = ["hello world", "tok1 tok2 tok3", "world tok7",
           "tok9 tok10 tok11 tok12 tok13", "hello", "tok40 tok41 world tok2"]


def _body(i):
    return {"prompt": PROMPTS[i], "max_tokens": 4 + i, "temperature": 0,
            "stream": i == 2}


def test_default_server_builds_no_scheduler(servers):
    _, _, seq_provider, bat_provider, _ = servers
    assert not hasattr(seq_provider, "generate")
    assert seq_provider._scheduler is None
    assert bat_provider._scheduler is not None
    assert bat_provider._scheduler.max_batch == 3


def test_concurrent_batched_completions_match_sequential_server(servers):
    seq_port, bat_port = servers[0], servers[1]
    want = [_text(*_post(seq_port, _body(i)), stream=(i == 2))
            for i in range(6)]
    got = {}

    def client(i):
        def run():
            got[i] = _text(*_post(bat_port, _body(i)), stream=(i == 2))
        return run

    _run_threads([client(i) for i in range(6)])
    assert [got[i] for i in range(6)] == want

    conn = http.client.HTTPConnection("127.0.0.1", bat_port, timeout=JOIN_S)
    conn.request("GET", "/metrics")
    text = conn.getresponse().read().decode()
    conn.close()
    for series in ("mlxs_batch_active_slots", "mlxs_batch_queued_requests",
                   "mlxs_batch_decode_steps_total"):
        assert series in text


def test_batched_server_rejects_prompt_longer_than_a_slot(servers):
    bat_port = servers[1]
    status, data = _post(bat_port, {"prompt": " ".join(["hello"] * 64),
                                    "max_tokens": 2, "temperature": 0})
    assert status == 400, data
    assert "capacity" in json.loads(data)["error"]


def test_batched_server_reports_length_at_capacity(servers):
    bat_port = servers[1]
    status, data = _post(bat_port, {"prompt": " ".join(["tok3"] * 60),
                                    "max_tokens": 50, "temperature": 0})
    assert status == 200, data
    r = json.loads(data)
    assert r["choices"][0]["finish_reason"] in ("length", "stop")
    assert r["usage"]["completion_tokens"] <= 64 - 1 - 60 + 1


def test_max_batch_with_shard_addresses_fails_at_startup(servers):
    from mlx_sharding_amd.server import openai_api

    class Args:
        model = None
        llm_shard_addresses = "127.0.0.1:1"
        start_layer = None
        end_layer = None
        max_batch = 2

    with pytest.raises(ValueError, match="llm-shard-addresses"):
        openai_api.ModelProvider(Args())
    with pytest.raises(SystemExit):
        openai_api.main(["--max-batch", "2", "--llm-shard-addresses",
                         "127.0.0.1:1"])


def test_max_batch_out_of_range_fails_at_startup():
    from mlx_sharding_amd.server import openai_api

    class Args:
        model = None
        llm_shard_addresses = ""
        start_layer = None
        end_layer = None
        max_batch = 65

    with pytest.raises(ValueError, match="max-batch"):
        openai_api.ModelProvider(Args())


def test_rccl_provider_batches_single_stage_only(llama):
    from types import SimpleNamespace

    from mlx_sharding_amd.parallel.rccl_serve import RcclModelProvider

    def pipeline(world):
        return SimpleNamespace(
            worker=SimpleNamespace(model=llama, world=world),
            device=torch.device("cpu"))

    with pytest.raises(ValueError, match="single-stage"):
        RcclModelProvider(SimpleNamespace(max_batch=2), pipeline(2), None)
    plain = RcclModelProvider(SimpleNamespace(), pipeline(2), None)
    assert plain._scheduler is None
    prov = RcclModelProvider(SimpleNamespace(max_batch=2), pipeline(1), None)
    try:
        p = _prompt(4, 8)
        got = [t for t, _ in prov.generate(p, SamplingParams(max_tokens=5))]
        assert got == _alone(llama, p, SamplingParams(), 5)
        with pytest.raises(ValueError):
            prov.check_prompt(10 ** 6)
    finally:
        prov._scheduler.close()
