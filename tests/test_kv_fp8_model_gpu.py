"""debug-llama-gqa (G = 4, head dim 64) with MLXS_AMD_KV_DTYPE=fp8: the GPU
model against the CPU model (the same storage format, by the reference), alone
and through BatchScheduler.  Tolerance: test_gqa_decode_model_gpu.py's rule."""
import functools
import threading

import pytest
import torch

from conftest import init_model
from mlx_sharding_amd import ops
from mlx_sharding_amd.models import get_model_class
from mlx_sharding_amd.parallel.batching import BatchScheduler
from mlx_sharding_amd.parallel.engine import SamplingParams
from mlx_sharding_amd.utils.presets import get_preset

pytestmark = pytest.mark.gpu
DEV, STEPS = "cuda", 12
SPIED = ("rope_append_kv_fp8", "gqa_decode_fp8", "kv_fp8_dequant",
         "rope_append_kv", "gqa_decode", "attn_decode")


@pytest.fixture
def fp8(monkeypatch):
    monkeypatch.setenv("MLXS_AMD_KV_DTYPE", "fp8")
    calls = {n: 0 for n in SPIED}
    for n in SPIED:
        def spy(*a, _n=n, _f=getattr(ops.hip_ext(), n), **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops.hip_ext(), n, spy)
    return calls


def _close(a, b):
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    return err <= 6e-2 + 1e-2 * scale


def _run(m, ids, toks, dev):
    cache = m.make_cache(batch_size=ids.shape[0])
    assert all(c.fp8 for c in cache)
    rows = []
    with torch.no_grad():
        for t in [ids] + toks:
            rows.append(m(t.to(dev), cache)[:, -1].float().cpu())
    return rows


@functools.lru_cache(maxsize=None)
def _models():
    cfg = get_preset("debug-llama-gqa")
    cls, shard = get_model_class(cfg.model_type), cfg.shard(0, cfg.num_hidden_layers)
    cpu = init_model(cls, cfg, shard, seed=13)
    gpu = cls(cfg, shard)
    gpu.load_weights(cpu.state_dict())
    return cfg, cpu, gpu.to(DEV).eval()


def test_fp8_cache_decodes_through_the_fp8_kernels(fp8):
    cfg, cpu, gpu = _models()
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, cfg.vocab_size, (2, 7), generator=g)
    toks = [torch.randint(0, cfg.vocab_size, (2, 1), generator=g)
            for _ in range(STEPS)]
    want, got = _run(cpu, ids, toks, "cpu"), _run(gpu, ids, toks, DEV)
    L = cfg.num_hidden_layers
    assert fp8["rope_append_kv_fp8"] == (STEPS + 1) * L
    assert fp8["gqa_decode_fp8"] == STEPS * L
    assert fp8["kv_fp8_dequant"] == 2 * L           # the prefill's K and V
    assert not (fp8["rope_append_kv"] or fp8["gqa_decode"] or fp8["attn_decode"])
    assert all(_close(a, b) for a, b in zip(got, want))


def test_fp8_cache_under_the_batch_scheduler(fp8):
    cfg, cpu, gpu = _models()
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist()
               for n in (4, 11)]
    sched = BatchScheduler(gpu, max_batch=2, capacity=64)
    got = {}

    def run(i):
        got[i] = list(sched.submit(prompts[i], SamplingParams(max_tokens=6)))

    try:
        ths = [threading.Thread(target=run, args=(i,)) for i in (0, 1)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(60)
        assert not any(t.is_alive() for t in ths), "a request stream hung"
        assert sched.graphed and all(c.fp8 for c in sched.caches)
    finally:
        sched.close()
    assert fp8["gqa_decode_fp8"] and not (fp8["gqa_decode"] or fp8["attn_decode"])
    for i in (0, 1):      # each stream against the CPU model on its own tokens
        toks = [torch.tensor([[t]]) for t, _ in got[i]]
        want = _run(cpu, torch.tensor([prompts[i]]), toks[:-1], "cpu")
        assert len(got[i]) == len(want) == 6 and all(
            _close(lp.float().cpu().view(-1), torch.log_softmax(row[0], -1))
            for (_, lp), row in zip(got[i], want))
