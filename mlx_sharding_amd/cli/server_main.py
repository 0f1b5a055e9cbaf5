"""`mlx-sharding-server` CLI — parity with /root/reference/shard/main.py:4-14."""

from __future__ import annotations

import argparse

import torch

from . import quantize_choice, quantize_request


def main():
    p = argparse.ArgumentParser(description="Start a pipeline shard server")
    p.add_argument("--model", type=str, required=True,
                   help="model checkpoint directory (full or pre-sharded)")
    p.add_argument("-s", "--start-layer", type=int, default=None)
    p.add_argument("-e", "--end-layer", type=int, default=None)
    p.add_argument("--port", type=int, default=0,
                   help="listen port (0 = auto-assign and print)")
    p.add_argument("--device", type=str,
                   default="cuda" if torch.cuda.is_available() else "cpu")
    p.add_argument("--quantize", type=quantize_choice, default=None,
                   metavar="{4,8,fp8}",
                   help="quantize a dense checkpoint to w4a16/w8a16 (or fp8: FP8 "
                        "128x128 blocks) at load")
    p.add_argument("--quantize-group-size", type=int, default=64)
    args = p.parse_args()

    from ..server.shard_server import serve
    q = quantize_request(args.quantize, args.quantize_group_size)
    serve(args.model, args.start_layer, args.end_layer, port=args.port,
          device=args.device, quantize=q)


if __name__ == "__main__":
    main()
