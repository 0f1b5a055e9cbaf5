"""`mlx-sharding-rccl-serve`: OpenAI API over an in-node RCCL pipeline.

Launch with one rank per GPU:
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 -m mlx_sharding_amd.cli.rccl_serve \
        --model /path/to/checkpoint --port 8080
"""

from __future__ import annotations

import argparse

from . import quantize_choice, quantize_request


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--model", type=str, required=True)
    p.add_argument("--host", type=str, default="127.0.0.1")
    p.add_argument("--port", type=int, default=8080)
    p.add_argument("--quantize", type=quantize_choice, default=None,
                   metavar="{4,8,fp8}",
                   help="quantize a dense checkpoint to w4a16/w8a16 (or fp8: FP8 "
                        "128x128 blocks) at load "
                        "(the fast path on MI355X)")
    p.add_argument("--quantize-group-size", type=int, default=64)
    from ..parallel.batching import MAX_BATCH_LIMIT, env_max_batch
    p.add_argument("--max-batch", type=int, default=env_max_batch(),
                   help="continuous batching: decode up to N concurrent "
                        "requests in one batched step (default "
                        "MLXS_MAX_BATCH or 1 = off; world size 1 only)")
    args = p.parse_args(argv)
    if not 1 <= args.max_batch <= MAX_BATCH_LIMIT:
        p.error(f"--max-batch must be in [1, {MAX_BATCH_LIMIT}]")

    from transformers import AutoTokenizer

    from ..config import ModelConfig
    from ..parallel.rccl import PipelineWorker, init_distributed, split_layers
    from ..parallel.rccl_serve import (RcclModelProvider, RcclPipeline)
    from ..server.openai_api import run
    from ..utils.loading import load_model

    rank, world, device = init_distributed()
    if args.max_batch > 1 and world > 1:
        raise SystemExit("--max-batch > 1 batches on one single-stage "
                         "model; launch rccl-serve with one rank")
    cfg = ModelConfig.load(args.model)
    s, e = split_layers(cfg.num_hidden_layers, world)[rank]
    q = quantize_request(args.quantize, args.quantize_group_size)
    model, _ = load_model(args.model, s, e, device=str(device), quantize=q)
    worker = PipelineWorker(model, rank, world, device)
    pipeline = RcclPipeline(worker)

    if rank == 0:
        tokenizer = AutoTokenizer.from_pretrained(args.model)
        provider = RcclModelProvider(args, pipeline, tokenizer)
        server = run(args.host, args.port, provider)
        print(f"RCCL pipeline API on {args.host}:{server.server_address[1]} "
              f"(pp{world})", flush=True)
        try:
            server.serve_forever()
        finally:
            pipeline.shutdown()
    else:
        pipeline.worker_loop()


if __name__ == "__main__":
    main()
