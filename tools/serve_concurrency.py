"""Measure continuous-batching serving throughput on GPU: N concurrent
request streams against one BatchScheduler (no HTTP), seeded prompt ids.

    python tools/serve_concurrency.py deepseek-v2-lite --streams 8

``--max-batch`` defaults to the stream count; ``--temperature`` and
``--top-p`` make every stream a sampled (unseeded) request.  Prints
aggregate tok/s (all generated tokens over the wall time of the whole
wave), per-stream decode tok/s and the p50 time to first token."""
import argparse
import pathlib
import statistics
import sys
import threading
import time

sys.path.insert(0, str(pathlib.Path(__file__).parent.parent))
import torch

from mlx_sharding_amd.parallel.batching import BatchScheduler
from mlx_sharding_amd.parallel.engine import SamplingParams
from mlx_sharding_amd.parallel.rccl import build_stage_model
from mlx_sharding_amd.utils.presets import get_preset

ap = argparse.ArgumentParser()
ap.add_argument("preset", nargs="?", default="deepseek-v2-lite")
ap.add_argument("--streams", type=int, default=8)
ap.add_argument("--max-batch", type=int, default=0)
ap.add_argument("--prompt-len", type=int, default=128)
ap.add_argument("--tokens", type=int, default=200)
ap.add_argument("--capacity", type=int, default=1024)
ap.add_argument("--temperature", type=float, default=0.0,
                help="sampling temperature of every stream (0: greedy)")
ap.add_argument("--top-p", type=float, default=1.0)
args = ap.parse_args()
max_batch = args.max_batch or args.streams

config = get_preset(args.preset, quant="deepseek" in args.preset)
qc = config.quantization
dev = torch.device("cuda", 0)
model = build_stage_model(config, 0, 1, dev,
                          quant_for=(lambda p: qc) if qc else None)
sched = BatchScheduler(model, max_batch, args.capacity, dev)
g = torch.Generator().manual_seed(0)
prompts = [torch.randint(0, config.vocab_size, (args.prompt_len,),
                         generator=g).tolist() for _ in range(args.streams)]


def wave(n_tok):
    res = [None] * args.streams

    def run(i):
        t0 = time.perf_counter()
        t_first, n = t0, 0
        for _ in sched.submit(prompts[i], SamplingParams(
                max_tokens=n_tok, temperature=args.temperature,
                top_p=args.top_p)):
            if n == 0:
                t_first = time.perf_counter()
            n += 1
        res[i] = (n, t_first - t0, time.perf_counter() - t_first)

    ths = [threading.Thread(target=run, args=(i,))
           for i in range(args.streams)]
    t0 = time.perf_counter()
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    return res, time.perf_counter() - t0


wave(16)  # warm-up generation (graph captured at scheduler start)
res, wall = wave(args.tokens)
total = sum(n for n, _, _ in res)
per = [(n - 1) / d for n, _, d in res if n > 1]
ttft = statistics.median(t for _, t, _ in res)
print(f"{args.preset}: streams={args.streams} max_batch={max_batch} "
      f"temperature={args.temperature} top_p={args.top_p} "
      f"aggregate {total / wall:.1f} tok/s, per-stream decode "
      f"{statistics.mean(per):.1f} tok/s (min {min(per):.1f}), "
      f"p50 TTFT {ttft * 1000:.1f} ms, {total} tokens in {wall:.2f} s "
      f"({'graph' if sched.graphed else 'eager'})", flush=True)
sched.close()
