#!/usr/bin/env python3
"""Per-kernel timing microbench (within-probe A/B, guide §5.4 rule 24).

Times the hand-written kernels at DeepSeek-Coder-V2-Lite decode shapes
with hipEvent brackets.  Run on a GPU box:
    python tools/bench_kernels.py [--iters 50]
"""

import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).parent.parent))

import torch


def timeit(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1000  # us


def bench_grouped_gate(ops, ref, iters, dev="cuda"):
    """Fused group-limited gating at DeepSeek-V2's routing shape vs the
    torch sequence it replaces (ref.moe_gate + make_expert_subranges),
    same process, same timer."""
    N, E, K, n_group, topk_group = 64, 160, 6, 8, 3
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(N, E, generator=g).to(torch.bfloat16).to(dev)

    def fused():
        return ops.moe_gate_subranges(logits, K, 16.0, False, max_tok=16,
                                      n_group=n_group, topk_group=topk_group)

    def torch_path():
        w, idx = ref.moe_gate(logits, K, n_group, topk_group, 16.0, False)
        return ops.make_expert_subranges(idx, w, E, max_tok=16)

    t_fused = timeit(fused, iters)
    t_torch = timeit(torch_path, iters)
    print(f"moe_gate_subranges E=160 grouped  fused {t_fused:8.1f} us   "
          f"torch gate+subranges {t_torch:8.1f} us   "
          f"({t_torch / t_fused:.1f}x)")


def _repeat(fn, iters, repeats=5):
    """(median, min, max) us over `repeats` timed windows."""
    ts = sorted(timeit(fn, iters, warmup=20) for _ in range(repeats))
    return ts[len(ts) // 2], ts[0], ts[-1]


def bench_v3(ops, ext, dev="cuda"):
    """DeepSeek-V3 shapes: the fused gate at E=256 in softmax
    group-limited mode vs sigmoid mode (alternated, same process), and
    128-head absorbed decode attention at B=64."""
    N, E, K, n_group, topk_group = 64, 256, 8, 8, 4
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(N, E, generator=g).to(torch.bfloat16).to(dev)
    bias = (torch.rand(E, generator=g) * 2.0 - 1.5).to(dev)

    def softmax():
        return ops.moe_gate_subranges(logits, K, 2.5, True, max_tok=16,
                                      n_group=n_group, topk_group=topk_group)

    def sigmoid():
        return ops.moe_gate_subranges(logits, K, 2.5, True, max_tok=16,
                                      n_group=n_group, topk_group=topk_group,
                                      scoring="sigmoid", e_bias=bias)

    for rnd in range(2):  # alternate the two modes
        for name, fn in (("softmax", softmax), ("sigmoid", sigmoid)):
            med, lo, hi = _repeat(fn, 3000)
            print(f"moe_gate_subranges N=64 E=256 g8/4 k=8 {name:8s} "
                  f"round {rnd}: median {med:7.2f} us  "
                  f"min {lo:7.2f}  max {hi:7.2f}")

    B, Hq, Dk, Dv = 64, 128, 576, 512
    q = torch.randn(B, Hq, 1, Dk, dtype=torch.bfloat16, device=dev)
    for S in (512, 4096):
        kbuf = torch.randn(B, 1, S, Dk, dtype=torch.bfloat16, device=dev)
        v = kbuf[..., :Dv]
        med, lo, hi = _repeat(
            lambda: ext.attn_decode(q, kbuf, v, Dk ** -0.5, 0.0, 0, None), 200)
        kv_bytes = B * S * Dk * 2
        print(f"attn_decode/abs Hq=128 B=64 S={S:5d}: median {med:8.1f} us  "
              f"min {lo:8.1f}  max {hi:8.1f}  "
              f"~{kv_bytes / (med / 1e6) / 1e12:.2f} TB/s of one K pass")


def bench_fp8(ops, ext, dev="cuda", E=64, windows=3):
    """FP8 block-quantized kernels against the 8-bit affine (gs 128)
    fp16-dequant kernels, which stream the same weight bytes: DeepSeek-V3
    decode shapes (H=7168, I=2048, 64 tokens x top-8 over E experts) and
    an o_proj-class GEMV.  Same process, alternating, `windows` timed
    windows each; prints median and min-max us and achieved weight
    bytes/s."""
    H, I, N, K = 7168, 2048, 64, 8
    g = torch.Generator(device=dev).manual_seed(3)

    def rand8(*shape):
        return (torch.randn(*shape, device=dev, generator=g) * 64.0) \
            .clamp_(-448, 448).to(torch.float8_e4m3fn)

    def randq(*shape):
        return torch.randint(0, 2 ** 31 - 1, shape, device=dev,
                             dtype=torch.int32, generator=g)

    def sb(*shape):
        return torch.rand(*shape, device=dev, generator=g) \
            .to(torch.bfloat16) * 0.01

    logits = torch.randn(N, E, device=dev, generator=g).to(torch.bfloat16)
    subs = ops.moe_gate_subranges(logits, K, max_tok=16)
    s_e, s_off, s_cnt, s_tok, s_wt = subs
    P = N * K
    x16 = (torch.randn(N, H, device=dev, generator=g) * 0.1).to(torch.float16)
    hh = (torch.randn(P, I, device=dev, generator=g) * 0.1).to(torch.float16)
    active = int((torch.bincount(s_e[s_cnt > 0].long(), minlength=E) > 0).sum())

    # fp8 operands
    g8, u8, d8 = rand8(E, I, H), rand8(E, I, H), rand8(E, H, I)
    gs8 = torch.full((E, I // 128, H // 128), 3e-4, device=dev)
    ds8 = torch.full((E, H // 128, I // 128), 3e-4, device=dev)
    # 8-bit affine operands, group size 128 (repacked once)
    gq, uq, dq = (ops.repack_w4(randq(E, I, H // 4), 8),
                  ops.repack_w4(randq(E, I, H // 4), 8),
                  ops.repack_w4(randq(E, H, I // 4), 8))
    gsc, gbi = sb(E, I, H // 128), sb(E, I, H // 128)
    dsc, dbi = sb(E, H, I // 128), sb(E, H, I // 128)

    cases = {
        "gateup": (
            lambda: ext.moe_fp8f16_gateup(x16, g8, u8, gs8, gs8, s_e, s_off,
                                          s_cnt, s_tok, P),
            lambda: ext.moe_w4f16_gateup(x16, gq, uq, gsc, gbi, gsc, gbi, s_e,
                                         s_off, s_cnt, s_tok, P, 128, 8),
            active * 2 * I * H),
        "down": (
            lambda: ext.moe_fp8f16_down(hh, d8, ds8, s_e, s_off, s_cnt, s_tok,
                                        s_wt, N),
            lambda: ext.moe_w4f16_down(hh, dq, dsc, dbi, s_e, s_off, s_cnt,
                                       s_tok, s_wt, N, 128, 8),
            active * H * I),
    }
    O, KK = 7168, 16384  # o_proj of a 128-head V3 layer
    w8, ws = rand8(O, KK), torch.full((O // 128, KK // 128), 3e-4, device=dev)
    wq = ops.repack_w4(randq(O, KK // 4), 8)
    wsc, wbi = sb(O, KK // 128), sb(O, KK // 128)
    xg = (torch.randn(N, KK, device=dev, generator=g) * 0.1).to(torch.float16)
    cases["gemv o_proj M=64"] = (
        lambda: ext.fp8f16_gemv(xg, w8, ws),
        lambda: ext.w4f16_gemv(xg, wq, wsc, wbi, 128, 8), O * KK)
    x1 = xg[:1].contiguous()
    cases["gemv o_proj M=1"] = (
        lambda: ext.fp8f16_gemv(x1, w8, ws),
        lambda: ext.w4f16_gemv(x1, wq, wsc, wbi, 128, 8), O * KK)

    print(f"fp8 vs w8-affine(gs128): H={H} I={I} N={N} top-{K} E={E} "
          f"({active} experts active)")
    for name, (f8, w8a, nbytes) in cases.items():
        ts = {"fp8": [], "w8": []}
        for _ in range(windows):  # alternate the two paths
            ts["fp8"].append(timeit(f8, 30, warmup=5))
            ts["w8"].append(timeit(w8a, 30, warmup=5))
        for k, v in ts.items():
            v.sort()
            med = v[len(v) // 2]
            print(f"  {name:18s} {k:4s} median {med:8.1f} us  "
                  f"min {v[0]:8.1f}  max {v[-1]:8.1f}  "
                  f"{nbytes / (med / 1e6) / 1e12:5.2f} TB/s "
                  f"({nbytes / (v[-1] / 1e6) / 1e12:.2f}-"
                  f"{nbytes / (v[0] / 1e6) / 1e12:.2f})")


def bench_fp8_prefill(ops, ext, dev="cuda", windows=3, iters=3):
    """One DeepSeek-V3 MoE layer (E=256, H=7168, I=2048, top-8, seeded
    random routing) prefilled from FP8 experts at N=4096 and N=512 tokens:
    the packed wide-tile route against the dequant-per-call route
    (MLXS_AMD_FP8_PREFILL=dense with the dq-cache off).  Same process,
    alternating, `windows` timed windows of `iters` calls each after one
    warm-up call; prints median and min-max ms and the peak-memory growth
    of one call per route, then each wide kernel alone with its achieved
    weight bytes/s (every activated expert's matrices counted once) and
    FLOP/s, both computed from shapes."""
    import os
    E, H, I, K = 256, 7168, 2048, 8
    TM = ext.moe_fp8f16_wide_tile()
    g = torch.Generator(device=dev).manual_seed(3)

    def rand8(*shape):
        b = torch.randint(0, 256, shape, device=dev, dtype=torch.uint8,
                          generator=g)
        b[(b & 0x7F) == 0x7F] = 0x38  # no NaN codes
        return b.view(torch.float8_e4m3fn)

    def scales(*shape):
        return torch.rand(*shape, device=dev, generator=g) * 2e-4 + 1e-4

    gate = (rand8(E, I, H), scales(E, I // 128, H // 128))
    up = (rand8(E, I, H), scales(E, I // 128, H // 128))
    down = (rand8(E, H, I), scales(E, H // 128, I // 128))
    env = {"packed": {"MLXS_AMD_FP8_PREFILL": "packed"},
           "dense": {"MLXS_AMD_FP8_PREFILL": "dense",
                     "MLXS_AMD_NO_DQ_CACHE": "1"}}

    def run(route, x, w, idx):
        for k in ("MLXS_AMD_FP8_PREFILL", "MLXS_AMD_NO_DQ_CACHE"):
            os.environ.pop(k, None)
        os.environ.update(env[route])
        # a fresh tensor object: the packed route pays its fp16 cast
        return ops.grouped_expert_mlp_fp8(x.view_as(x), gate, up, down, w, idx)

    print(f"fp8 prefill, one V3 MoE layer: E={E} H={H} I={I} top-{K}, "
          f"wide tile TM={TM}")
    for N in (4096, 512):
        x = (torch.randn(N, H, device=dev, generator=g) * 0.1) \
            .to(torch.bfloat16)
        idx = torch.rand(N, E, device=dev, generator=g).topk(K, dim=-1).indices
        w = torch.rand(N, K, device=dev, generator=g).to(torch.bfloat16)
        ts, mem, outs = {"packed": [], "dense": []}, {}, {}
        for route in ts:  # warm-up, and the memory of one call
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            outs[route] = run(route, x, w, idx).float()
            torch.cuda.synchronize()
            mem[route] = torch.cuda.max_memory_allocated() - base
        diff = float((outs["packed"] - outs["dense"]).abs().max())
        scale = float(outs["dense"].abs().max())
        for _ in range(windows):  # alternate the two routes
            for route in ts:
                ts[route].append(timeit(lambda: run(route, x, w, idx), iters,
                                        warmup=0) / 1000)
        print(f"  N={N}: max |packed - dense| {diff:.3e} at scale {scale:.3e}")
        for route, v in ts.items():
            v.sort()
            print(f"  N={N:5d} {route:6s} median {v[len(v) // 2]:8.2f} ms  "
                  f"min {v[0]:8.2f}  max {v[-1]:8.2f}  "
                  f"peak memory +{mem[route] / 2 ** 30:6.2f} GiB")
        # the two wide kernels alone
        subs = ops.make_expert_subranges(idx, w, E, max_tok=TM)[:5]
        s_e, s_off, s_cnt, s_tok, s_wt = subs
        P = N * K
        active = int((torch.bincount(idx.reshape(-1), minlength=E) > 0).sum())
        tiles = int((s_cnt > 0).sum())
        x16 = x.to(torch.float16)
        hh = ext.moe_fp8f16_gateup_wide(x16, gate[0], up[0], gate[1], up[1],
                                        s_e, s_off, s_cnt, s_tok, P)
        kernels = {
            "gateup_wide": (
                lambda: ext.moe_fp8f16_gateup_wide(
                    x16, gate[0], up[0], gate[1], up[1], s_e, s_off, s_cnt,
                    s_tok, P),
                active * 2 * I * H, 2.0 * P * 2 * I * H),
            "down_wide": (
                lambda: ext.moe_fp8f16_down_wide(
                    hh, down[0], down[1], s_e, s_off, s_cnt, s_tok, s_wt, N),
                active * H * I, 2.0 * P * H * I),
        }
        print(f"  N={N}: {active} experts active, {tiles} tiles of <= {TM} "
              f"tokens")
        for name, (fn, nbytes, flops) in kernels.items():
            v = sorted(timeit(fn, iters, warmup=1) for _ in range(windows))
            med = v[len(v) // 2]
            print(f"  N={N:5d} {name:12s} median {med / 1000:8.2f} ms  "
                  f"min {v[0] / 1000:8.2f}  max {v[-1] / 1000:8.2f}  "
                  f"{nbytes / (med / 1e6) / 1e12:5.2f} TB/s of weights  "
                  f"{flops / (med / 1e6) / 1e12:6.1f} TFLOP/s")
        del x16, hh, outs
    for k in ("MLXS_AMD_FP8_PREFILL", "MLXS_AMD_NO_DQ_CACHE"):
        os.environ.pop(k, None)


def bench_sample(ops, dev="cuda", windows=3, iters=20):
    """Batched sampling at DeepSeek-V3's vocabulary (V = 129 280), B in
    {1, 16, 64}, temperature 0.8, top_p in {1.0, 0.9}: one sample_rows
    launch (with its uniform_ and the step's one readback of the ids)
    against the per-row path of BatchScheduler._emit (row clone,
    logsumexp, ops.sample, .item() per row).  Same process, alternating,
    `windows` timed windows of `iters` steps after a warm-up; prints
    median and min-max us per step."""
    V, T = 129280, 0.8
    g = torch.Generator(device=dev).manual_seed(5)
    print(f"batched sampling, V={V}, temperature {T}: us per decode step")
    for B in (1, 16, 64):
        logits = torch.randn(B, V, device=dev, generator=g) * 3
        temperature = torch.full((B,), T, device=dev)
        u = torch.zeros(B, device=dev)
        active = torch.ones(B, dtype=torch.int32, device=dev)
        tok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        lse = torch.zeros(B, device=dev)
        for tp in (1.0, 0.9):
            top_p = torch.full((B,), tp, device=dev)

            def kernel():
                u.uniform_()
                ops.sample_rows(logits, temperature, top_p, u, active, tok,
                                lse)
                return tok.view(-1).tolist()

            def per_row():
                out = []
                for b in range(B):
                    lg = logits[b: b + 1].clone()
                    lp = lg - torch.logsumexp(lg, dim=-1, keepdim=True)
                    out.append(int(ops.sample(lg, T, tp).item()))
                return out, lp

            ts = {"kernel": [], "per-row": []}
            fns = {"kernel": kernel, "per-row": per_row}
            for fn in fns.values():
                timeit(fn, 3, warmup=2)
            for _ in range(windows):  # alternate the two paths
                for name, fn in fns.items():
                    ts[name].append(timeit(fn, iters, warmup=0))
            for name, v in ts.items():
                v.sort()
                print(f"  B={B:2d} top_p={tp:.1f} {name:8s} median "
                      f"{v[len(v) // 2]:9.1f} us  min {v[0]:9.1f}  "
                      f"max {v[-1]:9.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sample", action="store_true",
                    help="only the batched sampling comparison: the "
                         "sample_rows kernel vs the per-row torch path")
    ap.add_argument("--fp8-prefill", action="store_true",
                    help="only the FP8 MoE prefill comparison: packed "
                         "wide-tile route vs dequant per call")
    ap.add_argument("--fp8-only", action="store_true",
                    help="only the FP8-block vs 8-bit-affine comparison")
    ap.add_argument("--gate-only", action="store_true",
                    help="only the grouped-gating fused-vs-torch line")
    ap.add_argument("--v3-only", action="store_true",
                    help="only the DeepSeek-V3 gate and 128-head attention "
                         "lines")
    args = ap.parse_args()
    from mlx_sharding_amd import ops
    from mlx_sharding_amd.ops import reference as ref
    ext = ops.hip_ext()
    assert ext is not None
    dev = "cuda"
    torch.manual_seed(0)

    if args.sample:
        bench_sample(ops, dev)
        return
    if args.gate_only:
        bench_grouped_gate(ops, ref, args.iters, dev)
        return
    if args.v3_only:
        bench_v3(ops, ext, dev)
        return
    if args.fp8_only:
        bench_fp8(ops, ext, dev)
        return
    if args.fp8_prefill:
        bench_fp8_prefill(ops, ext, dev)
        return

    E, H, I, N, K = 64, 2048, 1408, 64, 6
    x = torch.randn(N, H, dtype=torch.bfloat16, device=dev)
    gw = torch.randn(E, I, H, dtype=torch.bfloat16, device=dev) * 0.03
    uw = torch.randn(E, I, H, dtype=torch.bfloat16, device=dev) * 0.03
    dw = torch.randn(E, H, I, dtype=torch.bfloat16, device=dev) * 0.03
    logits = torch.randn(N, E, dtype=torch.bfloat16, device=dev)

    subs = ops.moe_gate_subranges(logits, K, max_tok=4)
    sub_e, sub_off, sub_cnt, sorted_tok, sorted_wt = subs
    P = N * K
    h = ext.moe_gateup_grouped(x, gw, uw, sub_e, sub_off, sub_cnt, sorted_tok,
                               P, 4)

    t = timeit(lambda: ext.moe_gateup_grouped(x, gw, uw, sub_e, sub_off,
                                              sub_cnt, sorted_tok, P, 4),
               args.iters)
    bw = 64 * (2 * I * H * 2) / (t / 1e6) / 1e12
    print(f"moe_gateup_grouped      {t:8.1f} us   ~{bw:.2f} TB/s wt")

    t = timeit(lambda: ext.moe_down_grouped(h, dw, sub_e, sub_off, sub_cnt,
                                            sorted_tok, sorted_wt, N, 4),
               args.iters)
    bw = 64 * (H * I * 2) / (t / 1e6) / 1e12
    print(f"moe_down_grouped        {t:8.1f} us   ~{bw:.2f} TB/s wt")

    subs16 = ops.moe_gate_subranges(logits, K, max_tok=16)
    s16_e, s16_off, s16_cnt, s16_tok, s16_wt = subs16
    t = timeit(lambda: ext.moe_gateup_grouped(x, gw, uw, s16_e, s16_off,
                                              s16_cnt, s16_tok, P, 16),
               args.iters)
    bw = 64 * (2 * I * H * 2) / (t / 1e6) / 1e12
    print(f"moe_gateup_mfma16       {t:8.1f} us   ~{bw:.2f} TB/s wt")
    t = timeit(lambda: ext.moe_down_grouped(h, dw, s16_e, s16_off, s16_cnt,
                                            s16_tok, s16_wt, N, 16),
               args.iters)
    bw = 64 * (H * I * 2) / (t / 1e6) / 1e12
    print(f"moe_down_mfma16         {t:8.1f} us   ~{bw:.2f} TB/s wt")

    t = timeit(lambda: ops.moe_gate_subranges(logits, K), args.iters)
    print(f"moe_gate_subranges      {t:8.1f} us")
    bench_grouped_gate(ops, ref, args.iters, dev)

    # w4 variants
    wq = torch.randint(0, 2**31 - 1, (E, I, H // 8), device=dev, dtype=torch.int32)
    sc = torch.rand(E, I, H // 64, dtype=torch.bfloat16, device=dev) * 0.01
    bi = torch.rand(E, I, H // 64, dtype=torch.bfloat16, device=dev) * 0.01
    subs32 = ops.moe_gate_subranges(logits, K, max_tok=32)
    s32_e, s32_off, s32_cnt, s32_tok, _ = subs32
    t = timeit(lambda: ext.moe_w4_mfma(x, wq, sc, bi, s32_e, s32_off,
                                       s32_cnt, s32_tok, P, 64, 4), args.iters)
    bw = 64 * (I * H // 2) / (t / 1e6) / 1e12
    print(f"moe_w4_mfma             {t:8.1f} us   ~{bw:.2f} TB/s wt")

    # round-2 fp16-dequant kernels (the production quant decode path)
    x16 = x.to(torch.float16)
    uq2 = torch.randint(0, 2**31 - 1, (E, I, H // 8), device=dev,
                        dtype=torch.int32)
    dq2 = torch.randint(0, 2**31 - 1, (E, H, I // 8), device=dev,
                        dtype=torch.int32)
    dsc = torch.rand(E, H, I // 64, dtype=torch.bfloat16, device=dev) * 0.01
    dbi = torch.rand(E, H, I // 64, dtype=torch.bfloat16, device=dev) * 0.01
    usc = sc.clone(); ubi = bi.clone()
    gq = ops.repack_w4(wq, 4); uq = ops.repack_w4(uq2, 4)
    dq = ops.repack_w4(dq2, 4)
    hh16 = ext.moe_w4f16_gateup(x16, gq, uq, sc, bi, usc, ubi, s16_e, s16_off,
                                s16_cnt, s16_tok, P, 64, 4)
    t = timeit(lambda: ext.moe_w4f16_gateup(x16, gq, uq, sc, bi, usc, ubi,
                                            s16_e, s16_off, s16_cnt, s16_tok,
                                            P, 64, 4), args.iters)
    bw = 64 * (2 * I * H // 2) / (t / 1e6) / 1e12
    print(f"moe_w4f16_gateup        {t:8.1f} us   ~{bw:.2f} TB/s wt(packed)")
    t = timeit(lambda: ext.moe_w4f16_down(hh16, dq, dsc, dbi, s16_e, s16_off,
                                          s16_cnt, s16_tok, s16_wt, N, 64, 4),
               args.iters)
    bw = 64 * (H * I // 2) / (t / 1e6) / 1e12
    print(f"moe_w4f16_down          {t:8.1f} us   ~{bw:.2f} TB/s wt(packed)")

    for (O, HH, name) in [(3648, 2048, "qkv"), (102400, 2048, "lm_head"),
                          (5632, 2048, "sh_gateup"), (2048, 2816, "sh_down")]:
        wq2 = torch.randint(0, 2**31 - 1, (O, HH // 8), device=dev, dtype=torch.int32)
        sc2 = torch.rand(O, HH // 64, dtype=torch.bfloat16, device=dev) * 0.01
        bi2 = torch.rand(O, HH // 64, dtype=torch.bfloat16, device=dev) * 0.01
        x2 = torch.randn(N, HH, dtype=torch.bfloat16, device=dev)
        t = timeit(lambda: ext.w4a16_gemv(x2, wq2, sc2, bi2, 64, 4), args.iters)
        bw = (O * HH // 2) / (t / 1e6) / 1e12
        print(f"w4a16_gemv {name:10s}  {t:8.1f} us   ~{bw:.2f} TB/s wt")
        rp2 = ops.repack_w4(wq2, 4)
        x216 = x2.to(torch.float16)
        t = timeit(lambda: ext.w4f16_gemv(x216, rp2, sc2, bi2, 64, 4),
                   args.iters)
        bw = O * HH // 2 / (t / 1e6) / 1e12
        print(f"w4f16_gemv {name:10s}  {t:8.1f} us   ~{bw:.2f} TB/s wt")

    # attention decode, MLA shape
    for S in (512, 2048):
        B, Hq, Dk, Dv = 32, 16, 192, 128
        Scap = ((S + 1023) // 1024) * 1024
        q = torch.randn(B, Hq, 1, Dk, dtype=torch.bfloat16, device=dev)
        kb = torch.randn(B, Hq, Scap, Dk, dtype=torch.bfloat16, device=dev)
        vb = torch.randn(B, Hq, Scap, Dv, dtype=torch.bfloat16, device=dev)
        kv_, vv_ = kb[:, :, :S], vb[:, :, :S]
        t = timeit(lambda: ext.attn_decode(q, kv_, vv_, 0.1, 0.0, 0, None),
                   args.iters)
        bw = B * Hq * S * (Dk + Dv) * 2 / (t / 1e6) / 1e12
        print(f"attn_decode S={S:5d}     {t:8.1f} us   ~{bw:.2f} TB/s kv")

    # attention decode, absorbed-MLA shape (compressed cache, V in K rows)
    for S in (512, 2048):
        B, Hq, Dk, Dv = 64, 16, 576, 512
        Scap = ((S + 1023) // 1024) * 1024
        q = torch.randn(B, Hq, 1, Dk, dtype=torch.bfloat16, device=dev)
        kb = torch.randn(B, 1, Scap, Dk, dtype=torch.bfloat16, device=dev)
        kv_ = kb[:, :, :S]
        vv_ = kv_[..., :Dv]
        t = timeit(lambda: ext.attn_decode(q, kv_, vv_, 0.04, 0.0, 0, None),
                   args.iters)
        bw = B * S * Dk * 2 / (t / 1e6) / 1e12
        print(f"attn_decode/abs S={S:5d} {t:8.1f} us   ~{bw:.2f} TB/s kv")

    # attention prefill, MLA shape
    B, Hq, T, Dk, Dv = 32, 16, 512, 192, 128
    q = torch.randn(B, Hq, T, Dk, dtype=torch.bfloat16, device=dev) * 0.3
    kb = torch.randn(B, Hq, 1024, Dk, dtype=torch.bfloat16, device=dev) * 0.3
    vb = torch.randn(B, Hq, 1024, Dv, dtype=torch.bfloat16, device=dev) * 0.3
    kv_, vv_ = kb[:, :, :T], vb[:, :, :T]
    t = timeit(lambda: ext.attn_prefill(q, kv_, vv_, 0.072, 0.0, 0, 0),
               iters=10)
    fl = 2 * B * Hq * T * T * (Dk + Dv) / 2  # causal ~half
    print(f"attn_prefill T=512      {t:8.1f} us   ~{fl/(t/1e6)/1e12:.1f} TF")

    # rmsnorm
    xr = torch.randn(N, H, dtype=torch.bfloat16, device=dev)
    wr = torch.randn(H, dtype=torch.bfloat16, device=dev)
    t = timeit(lambda: ext.rms_norm(xr, wr, 1e-6, 0.0), args.iters)
    print(f"rms_norm [32,2048]      {t:8.1f} us")


if __name__ == "__main__":
    main()
