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


def bench_moe_route(ops, ref, dev="cuda", iters=200):
    """The fused prefill routing (ops.moe_route, three launches) against the
    torch sequences it replaces: ref.moe_gate on the GPU + the bf16 weight
    cast, followed by make_expert_subranges (the packed route's prologue) or
    by the sort section of _moe_prefill_gemm without its host sync (the
    batched-GEMM route's).  The three alternate in one process after
    warm-up, two rounds; median of five windows of `iters` calls between
    device events, with min-max."""
    shapes = [(E, K, ng, tg, sc, N) for (E, K, ng, tg, sc) in
              ((64, 6, 1, 1, "softmax"), (256, 8, 8, 4, "sigmoid"))
              for N in (512, 4096, 32768)]
    g = torch.Generator().manual_seed(1)
    for E, K, n_group, topk_group, scoring, N in shapes:
        logits = torch.randn(N, E, generator=g).to(torch.bfloat16).to(dev)
        kw = {}
        if scoring == "sigmoid":
            kw = {"scoring": "sigmoid",
                  "e_bias": (torch.rand(E, generator=g) * 2.0 - 1.5).to(dev)}
        norm, scaling, max_tok = scoring == "sigmoid", 2.5, 64

        def fused():
            return ops.moe_route(logits, K, n_group, topk_group, scaling,
                                 norm, max_tok, wt_bf16=True, **kw)

        def gate():
            w, idx = ref.moe_gate(logits.float(), K, n_group, topk_group,
                                  scaling, norm, **kw)
            return w.to(torch.bfloat16), idx

        def torch_subranges():
            w, idx = gate()
            return ops.make_expert_subranges(idx, w, E, max_tok=max_tok)

        def torch_gemm_sort():
            # _moe_prefill_gemm up to its scatter, cap fixed (no host sync)
            w, idx = gate()
            cap = N
            flat_e = idx.reshape(-1).long()
            order = torch.argsort(flat_e, stable=True)
            sorted_e = flat_e[order]
            tok = torch.arange(N, device=dev).repeat_interleave(K)[order]
            counts = torch.zeros(E, dtype=torch.long, device=dev)
            counts.scatter_add_(0, sorted_e, torch.ones_like(sorted_e))
            start = torch.cumsum(counts, 0) - counts
            dst = sorted_e * cap + torch.arange(N * K, device=dev) \
                - start[sorted_e]
            inv = torch.empty_like(order)
            inv[order] = torch.arange(N * K, device=dev)
            return (tok.to(torch.int32), dst.to(torch.int32),
                    dst[inv].view(N, K).to(torch.int32), w.float())

        for rnd in range(2):
            for name, fn in (("fused", fused),
                             ("torch+subranges", torch_subranges),
                             ("torch+gemm-sort", torch_gemm_sort)):
                med, lo, hi = _repeat(fn, iters)
                print(f"moe_route N={N:5d} E={E:3d} k={K} {scoring:7s} "
                      f"{name:15s} round {rnd}: median {med:8.1f} us  "
                      f"min {lo:8.1f}  max {hi:8.1f}", flush=True)


# vendor-published MI355X peaks, for the share-of-bound column
_PEAK_HBM = 8.0e12        # B/s
_PEAK_BF16 = 2.5e15       # dense bf16 matrix FLOP/s


def bench_mla(ops, ext, dev="cuda", iters=200):
    """Absorbed MLA decode, Dk=576, Dv=512: the head-group attn_decode_split
    kernel and the MFMA mla_decode kernel, alternated in one process after
    warm-up.  Rows are (B, Hq, S, mode, L): "host" passes S on the host,
    "device" passes an int32 [B] position L - 1 over a capacity-S buffer.
    128 heads at B=64, S=512/4096, both modes; 16 heads at B=64,
    S=512/1024/2048/4096, both modes, and at B=1, S=1024/4096, device, all
    with L = S; and the serving case, 16 heads under a device position with
    L far below a 4096-key capacity (L=256/512/1024 at B=1/16/64).  Median
    of five windows between device events (min-max).  The bound is the
    larger of the one-pass bytes of the L live KV rows over peak HBM
    bandwidth and the QK+PV FLOPs over peak bf16."""
    Dk, Dv = 576, 512
    scale = Dk ** -0.5
    rows = [(64, 128, S, m, S) for S in (512, 4096) for m in ("host", "device")]
    rows += [(64, 16, S, m, S) for S in (512, 1024, 2048, 4096)
             for m in ("host", "device")]
    rows += [(1, 16, S, "device", S) for S in (1024, 4096)]
    rows += [(B, 16, 4096, "device", L) for B in (1, 16, 64)
             for L in (256, 512, 1024)]
    for B, Hq, S, mode, L in rows:
        q_abs = torch.randn(Hq, B, Dv, dtype=torch.bfloat16, device=dev)
        q_pe = torch.randn(B, Hq, Dk - Dv, dtype=torch.bfloat16, device=dev)
        qn = q_abs.transpose(0, 1)
        kv = torch.randn(B, 1, S, Dk, dtype=torch.bfloat16, device=dev) * 0.5
        v = kv[..., :Dv]
        nbytes = B * L * Dk * 2
        flops = 2 * B * Hq * L * (Dk + Dv)
        t_mem, t_mma = nbytes / _PEAK_HBM * 1e6, flops / _PEAK_BF16 * 1e6
        bound, which = max((t_mem, "HBM"), (t_mma, "MFMA"))
        pos = None if mode == "host" else torch.full(
            (B,), L - 1, dtype=torch.int32, device=dev)
        fns = (("attn_decode_split", lambda: ext.attn_decode_split(
                    qn, q_pe, kv, v, scale, 0.0, 0, pos)),
               ("mla_decode", lambda: ext.mla_decode(
                    qn, q_pe, kv, Dv, scale, pos)))
        diff = (fns[0][1]().float() - fns[1][1]().float()).abs().max()
        tag = f"B={B:2d} Hq={Hq:3d} S={S:5d} {mode:6s} L={L:5d}"
        print(f"{tag}: max |old - new| = {diff.item():.3e}, "
              f"mla_decode_nsplit = {ext.mla_decode_nsplit(B, Hq, S)}")
        for rnd in range(2):  # alternate the two kernels
            for name, fn in fns:
                med, lo, hi = _repeat(fn, iters)
                print(f"{name:18s} {tag} round {rnd}: median {med:8.1f} us  "
                      f"min {lo:8.1f}  max {hi:8.1f}  "
                      f"bound {bound:5.2f} us ({which}) "
                      f"-> {100 * bound / med:5.1f}%", flush=True)


def _window_us(fn, window_s):
    """us per call over one timed window of about window_s seconds."""
    return timeit(fn, max(10, int(window_s * 1e6 / timeit(fn, 10, 5))), 0)


def bench_gqa_decode(ext, dev="cuda", window_s=0.25, batches=(1, 16, 64),
                     lengths=(512, 2048, 4096, 8192)):
    """GQA decode attention: the scalar attn_decode kernel and the MFMA
    gqa_decode kernel, alternated in one process on the same tensors after
    warm-up, two rounds of one window each.  Shapes (Hq, Hkv, D): llama-3-70b
    (64, 8, 128), llama-3-8b (32, 8, 128), qwen2-7b (28, 4, 128), tinyllama
    (32, 4, 64), gemma-2-9b (16, 8, 256) with softcap 50 / window 4096 and
    without a window.  "host" passes a view of L keys; "device" an int32 [B]
    position L - 1 over the whole capacity (the largest length).  TB/s is
    B*Hkv*L*(Dk+Dv)*2 bytes (of the keys inside the window) over the faster
    round."""
    shapes = [(64, 8, 128, 0.0, 0), (32, 8, 128, 0.0, 0), (28, 4, 128, 0.0, 0),
              (32, 4, 64, 0.0, 0), (16, 8, 256, 50.0, 4096),
              (16, 8, 256, 50.0, 0)]
    cap, bmax = max(lengths), max(batches)
    print("Hq Hkv D cap window B L mode: attn_decode us (r0 r1) TB/s | "
          "gqa_decode us (r0 r1) TB/s | old/new (min..max over rounds)")
    for Hq, Hkv, D, softcap, window in shapes:
        scale = D ** -0.5
        qb = torch.randn(bmax, Hq, 1, D, dtype=torch.bfloat16, device=dev)
        kb = torch.randn(bmax, Hkv, cap, D, dtype=torch.bfloat16, device=dev)
        vb = torch.randn(bmax, Hkv, cap, D, dtype=torch.bfloat16, device=dev)
        for B in batches:
            for L in lengths:
                for mode in ("host", "device"):
                    q = qb[:B]
                    if mode == "host":
                        k, v, pos = kb[:B, :, :L], vb[:B, :, :L], None
                    else:
                        k, v = kb[:B], vb[:B]
                        pos = torch.full((B,), L - 1, dtype=torch.int32,
                                         device=dev)
                    a = (q, k, v, scale, softcap, window, pos)
                    fns = (lambda: ext.attn_decode(*a),
                           lambda: ext.gqa_decode(*a))
                    diff = (fns[0]().float() - fns[1]().float()).abs().max()
                    t = [[_window_us(fn, window_s) for fn in fns]
                         for _ in range(2)]  # alternate the two kernels
                    old, new = (t[0][0], t[1][0]), (t[0][1], t[1][1])
                    live = min(L, window) if window else L
                    tb = B * Hkv * live * 2 * D * 2 / 1e6
                    print(f"{Hq:2d} {Hkv} {D:3d} cap{softcap:g} w{window:<4d} "
                          f"B={B:2d} L={L:4d} {mode:6s}: "
                          f"{old[0]:7.1f} {old[1]:7.1f} {tb / min(old):5.2f} | "
                          f"{new[0]:7.1f} {new[1]:7.1f} {tb / min(new):5.2f} | "
                          f"{min(old) / max(new):5.2f}..{max(old) / min(new):5.2f}"
                          f"  diff {diff.item():.1e}", flush=True)


def bench_gqa_decode_fp8(ops, ext, dev="cuda", window_s=0.25,
                         batches=(1, 16, 64), lengths=(512, 4096, 16384)):
    """Decode attention over the FP8 KV cache (gqa_decode_fp8) against the
    bf16 path ops.attention routes the same shape to, alternated in one
    process after warm-up, two rounds of one window each.  Shapes (Hq, Hkv,
    D): llama-3-8b (32, 8, 128), llama-3-70b (64, 8, 128), tinyllama (32, 4,
    64).  "host" passes the length L; "device" an int32 [B] position L - 1
    over the whole capacity (the largest length).  TB/s is the KV bytes the
    kernel has to read (B*Hkv*L*2*D elements of 2 or 1 bytes, plus 8 bytes of
    scales per key for FP8) over the faster round."""
    shapes = [(32, 8, 128), (64, 8, 128), (32, 4, 64)]
    cap, bmax = max(lengths), max(batches)
    print("Hq Hkv D B L mode: bf16 us (r0 r1) TB/s | fp8 us (r0 r1) TB/s | "
          "bf16/fp8 (min..max over rounds)")
    for Hq, Hkv, D in shapes:
        scale = D ** -0.5
        qb = torch.randn(bmax, Hq, 1, D, dtype=torch.bfloat16, device=dev)
        kb = torch.randn(bmax, Hkv, cap, D, dtype=torch.bfloat16, device=dev)
        vb = torch.randn(bmax, Hkv, cap, D, dtype=torch.bfloat16, device=dev)
        for B in batches:
            q = qb[:B]
            k8, ks = ops.kv_fp8_quantize(kb[:B])
            v8, vs = ops.kv_fp8_quantize(vb[:B])
            for L in lengths:
                for mode in ("host", "device"):
                    if mode == "host":
                        k, v, pos, n = kb[:B, :, :L], vb[:B, :, :L], None, L
                    else:
                        k, v, n = kb[:B], vb[:B], -1
                        pos = torch.full((B,), L - 1, dtype=torch.int32,
                                         device=dev)
                    fns = (lambda: ops.attention(q, k, v, scale, pos_dev=pos),
                           lambda: ext.gqa_decode_fp8(q, k8, ks, v8, vs, scale,
                                                      pos, n))
                    diff = (fns[0]().float() - fns[1]().float()).abs().max()
                    t = [[_window_us(fn, window_s) for fn in fns]
                         for _ in range(2)]  # alternate the two kernels
                    old, new = (t[0][0], t[1][0]), (t[0][1], t[1][1])
                    tb16 = B * Hkv * L * 2 * D * 2 / 1e6
                    tb8 = B * Hkv * L * (2 * D + 8) / 1e6
                    print(f"{Hq:2d} {Hkv} {D:3d} B={B:2d} L={L:5d} {mode:6s}: "
                          f"{old[0]:7.1f} {old[1]:7.1f} {tb16 / min(old):5.2f} | "
                          f"{new[0]:7.1f} {new[1]:7.1f} {tb8 / min(new):5.2f} | "
                          f"{min(old) / max(new):5.2f}..{max(old) / min(new):5.2f}"
                          f"  diff {diff.item():.1e}", flush=True)


def bench_gqa_chunk(ops, ext, dev="cuda", window_s=0.12, rounds=3,
                    chunks=(4, 16, 64), prefixes=(512, 4096, 32768),
                    batches=(1, 8)):
    """T new tokens over a cached prefix: gqa_chunk / gqa_chunk_fp8 against
    what the same call runs without them (attn_prefill on the bf16 cache;
    kv_fp8_dequant of K and V + attn_prefill on the FP8 cache), the four
    paths alternated in one process on the same tensors after warm-up,
    `rounds` rounds of one window each.  Shapes (Hq, Hkv, D): llama-3-8b
    (32, 8, 128), llama-3-70b (64, 8, 128), qwen2-7b (28, 4, 128), tinyllama
    (32, 4, 64).  Per path: median us and (max - min) / median over the
    rounds; old/new is min(old) / max(new) .. max(old) / min(new)."""
    shapes = [(32, 8, 128), (64, 8, 128), (28, 4, 128), (32, 4, 64)]
    cap, bmax, tmax = max(prefixes) + max(chunks), max(batches), max(chunks)
    print("Hq Hkv D B T prefix: prefill us spread | chunk us spread old/new "
          "|| dequant+prefill us spread | chunk_fp8 us spread old/new",
          flush=True)
    worst = 0.0
    for Hq, Hkv, D in shapes:
        scale = D ** -0.5
        qb = torch.randn(bmax, tmax, Hq, D, dtype=torch.bfloat16, device=dev)
        kb = torch.randn(bmax, Hkv, cap, D, dtype=torch.bfloat16, device=dev)
        vb = torch.randn(bmax, Hkv, cap, D, dtype=torch.bfloat16, device=dev)
        k8b, ksb = ops.kv_fp8_quantize(kb)
        v8b, vsb = ops.kv_fp8_quantize(vb)
        for B in batches:
            k8, ks, v8, vs = (t[:B].contiguous() for t in (k8b, ksb, v8b, vsb))
            for T in chunks:
                q = qb[:B, :T].transpose(1, 2)
                for P in prefixes:
                    S = P + T
                    k, v = kb[:B, :, :S], vb[:B, :, :S]

                    def old8():
                        return ext.attn_prefill(
                            q, ext.kv_fp8_dequant(k8, ks, S),
                            ext.kv_fp8_dequant(v8, vs, S), scale, 0.0, 0, P)

                    fns = (lambda: ext.attn_prefill(q, k, v, scale, 0.0, 0, P),
                           lambda: ext.gqa_chunk(q, k, v, scale), old8,
                           lambda: ext.gqa_chunk_fp8(q, k8, ks, v8, vs, scale,
                                                     S))
                    d16 = (fns[0]().float() - fns[1]().float()).abs().max()
                    d8 = (fns[2]().float() - fns[3]().float()).abs().max()
                    t = [[_window_us(fn, window_s) for fn in fns]
                         for _ in range(rounds)]  # alternate the paths
                    cols = [sorted(r[i] for r in t) for i in range(4)]
                    med = [c[len(c) // 2] for c in cols]
                    spr = [(c[-1] - c[0]) / m for c, m in zip(cols, med)]
                    worst = max(worst, *spr)
                    line = f"{Hq:2d} {Hkv} {D:3d} B={B} T={T:2d} P={P:5d}:"
                    for o, n in ((0, 1), (2, 3)):
                        line += (f" {med[o]:8.1f} {100 * spr[o]:4.1f}% |"
                                 f" {med[n]:8.1f} {100 * spr[n]:4.1f}%"
                                 f" {cols[o][0] / cols[n][-1]:5.2f}.."
                                 f"{cols[o][-1] / cols[n][0]:5.2f} |")
                    print(line + f" diff {d16.item():.1e} {d8.item():.1e}",
                          flush=True)
    print(f"largest (max - min) / median over the rounds: {100 * worst:.1f}%",
          flush=True)


def bench_mla_chunk(ops, ext, dev="cuda", iters=200):
    """One layer's attention section for T new tokens over a cached prefix
    of a V2-Lite / V3 geometry (rows 576 / 512, nope 128, vd 128), B=1, two
    ways alternated in one process after warm-up: the expanded path
    (kv_b_proj over all S rows, mla_append_kv into per-head K/V temporaries,
    attn_prefill) and the absorbed path (W_UK bmm, mla_chunk, W_UV bmm).
    Median of five windows between device events (min-max).  The bound of
    the absorbed path is the larger of one pass over the KV rows plus the
    two absorb weights over peak HBM bandwidth and its FLOPs over peak
    bf16."""
    B, rank, rope, nope, vd = 1, 512, 64, 128, 128
    scale = (nope + rope) ** -0.5
    for nh in (16, 128):
        w = (torch.randn(nh * (nope + vd), rank, device=dev) * rank ** -0.5
             ).to(torch.bfloat16)
        w3 = w.view(nh, nope + vd, rank)
        w_uk = w3[:, :nope].contiguous()
        w_uv = w3[:, nope:].transpose(1, 2).contiguous()
        for S in (1024, 4096):
            kv = (torch.randn(B, 1, S, rank + rope, device=dev) * 0.5
                  ).to(torch.bfloat16)
            for T in (8, 32, 64):
                q_nope = torch.randn(B, T, nh, nope, dtype=torch.bfloat16,
                                     device=dev)
                q_pe = torch.randn(B, T, nh, rope, dtype=torch.bfloat16,
                                   device=dev)

                def expanded():
                    kvh = torch.nn.functional.linear(
                        kv[:, 0, :, :rank], w).view(B, S, nh, nope + vd)
                    k = kvh.new_empty(B, nh, S, nope + rope)
                    v = kvh.new_empty(B, nh, S, vd)
                    ext.mla_append_kv(kvh, kv[:, 0, :, rank:], k, v, pos0=0)
                    qf = torch.cat([q_nope, q_pe], dim=-1).transpose(1, 2)
                    o = ops.attention(qf, k, v, scale, causal_offset=S - T)
                    return o.transpose(1, 2).reshape(B, T, -1)

                def absorbed():
                    qn = q_nope.permute(2, 0, 1, 3).reshape(nh, B * T, nope)
                    q_abs = torch.bmm(qn, w_uk)
                    o = ext.mla_chunk(
                        q_abs.view(nh, B, T, rank).permute(1, 2, 0, 3), q_pe,
                        kv, rank, scale)
                    ov = torch.bmm(o.view(B * T, nh, rank).transpose(0, 1),
                                   w_uv)
                    return ov.view(nh, B, T, vd).permute(1, 2, 0, 3).reshape(
                        B, T, -1)

                diff = (expanded().float() - absorbed().float()).abs().max()
                nbytes = B * S * (rank + rope) * 2 + 2 * w_uk.numel() * 2
                flops = (2 * B * T * nh * S * (2 * rank + rope)
                         + 2 * B * T * nh * rank * (nope + vd))
                t_mem = nbytes / _PEAK_HBM * 1e6
                t_mma = flops / _PEAK_BF16 * 1e6
                bound, which = max((t_mem, "HBM"), (t_mma, "MFMA"))
                print(f"Hq={nh} S={S} T={T}: max |expanded - absorbed| = "
                      f"{diff.item():.3e}, mla_chunk_nsplit = "
                      f"{ext.mla_chunk_nsplit(B, T * nh, S)}, absorbed bound "
                      f"{bound:.2f} us ({which})")
                for rnd in range(2):  # alternate the two paths
                    for name, fn in (("expanded", expanded),
                                     ("absorbed", absorbed)):
                        med, lo, hi = _repeat(fn, iters)
                        print(f"{name:9s} Hq={nh:3d} S={S:5d} T={T:2d} round "
                              f"{rnd}: median {med:8.1f} us  min {lo:8.1f}  "
                              f"max {hi:8.1f}")


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


def bench_w4_prefill(ops, ext, dev="cuda", windows=3, iters=3):
    """One DeepSeek-V2-Lite MoE layer (E=64, H=2048, I=1408, top-6) and one
    DeepSeek-V3 layer (E=256, H=7168, I=2048, top-8), 4-bit gs 64 experts,
    seeded random routing, prefilled at N=512 and N=4096 tokens: the packed
    wide-tile route against the no-resident dense route
    (MLXS_AMD_W4_PREFILL=dense with the dq-cache off: dequantize every
    call), and for information the resident dense route (dq-cache on).
    Same process, alternating, `windows` timed windows of `iters` calls
    each after one warm-up call; prints median and min-max ms and the
    peak-memory growth of one call per route, then each wide kernel alone
    with its achieved packed-weight bytes/s (every activated expert's words
    counted once) and FLOP/s, both computed from shapes."""
    import os
    gs, bits = 64, 4
    TM = ext.moe_w4f16_wide_tile()
    g = torch.Generator(device=dev).manual_seed(3)
    keys = ("MLXS_AMD_W4_PREFILL", "MLXS_AMD_NO_DQ_CACHE")
    env = {"packed": {"MLXS_AMD_W4_PREFILL": "packed"},
           "dense": {"MLXS_AMD_W4_PREFILL": "dense",
                     "MLXS_AMD_NO_DQ_CACHE": "1"},
           "resident": {}}

    def trip(O, Kd):
        wq = torch.randint(-2 ** 31, 2 ** 31 - 1, (E, O, Kd * bits // 32),
                           device=dev, dtype=torch.int32, generator=g)
        sc = (torch.rand(E, O, Kd // gs, device=dev, generator=g) * 4e-3
              + 4e-3).to(torch.bfloat16)
        return wq, sc, (-7.5 * sc.float()).to(torch.bfloat16)

    for name, E, H, I, K in (("V2-Lite", 64, 2048, 1408, 6),
                             ("V3", 256, 7168, 2048, 8)):
        gate, up, down = trip(I, H), trip(I, H), trip(H, I)

        def run(route, x, w, idx):
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(env[route])
            # a fresh tensor object: the packed route pays its fp16 cast
            return ops.grouped_expert_mlp_quant(x.view_as(x), gate, up, down,
                                                w, idx, gs, bits)

        print(f"w4 prefill, one {name} MoE layer: E={E} H={H} I={I} top-{K}, "
              f"{bits}-bit gs {gs}, wide tile TM={TM}")
        for N in (512, 4096):
            x = (torch.randn(N, H, device=dev, generator=g) * 0.1) \
                .to(torch.bfloat16)
            idx = torch.rand(N, E, device=dev, generator=g) \
                .topk(K, dim=-1).indices
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
                    ts[route].append(timeit(lambda: run(route, x, w, idx),
                                            iters, warmup=0) / 1000)
            print(f"  N={N}: max |packed - dense| {diff:.3e} at scale "
                  f"{scale:.3e}")
            for route, v in ts.items():
                v.sort()
                print(f"  N={N:5d} {route:8s} median {v[len(v) // 2]:8.2f} ms"
                      f"  min {v[0]:8.2f}  max {v[-1]:8.2f}  "
                      f"peak memory +{mem[route] / 2 ** 30:6.2f} GiB")
            # the two wide kernels alone
            s_e, s_off, s_cnt, s_tok, s_wt = ops.make_expert_subranges(
                idx, w, E, max_tok=TM)[:5]
            P = N * K
            active = int((torch.bincount(idx.reshape(-1), minlength=E) > 0)
                         .sum())
            x16 = x.to(torch.float16)
            gq, uq, dq = (ops.repack_w4(t[0], bits) for t in (gate, up, down))
            gu = lambda: ext.moe_w4f16_gateup_wide(  # noqa: E731
                x16, gq, uq, gate[1], gate[2], up[1], up[2], s_e, s_off,
                s_cnt, s_tok, P, gs, bits)
            hh = gu()
            dn = lambda: ext.moe_w4f16_down_wide(  # noqa: E731
                hh, dq, down[1], down[2], s_e, s_off, s_cnt, s_tok, s_wt, N,
                gs, bits)
            print(f"  N={N}: {active} experts active, "
                  f"{int((s_cnt > 0).sum())} tiles of <= {TM} tokens")
            for kn, fn, elems in (("gateup_wide", gu, 2 * I * H),
                                  ("down_wide", dn, H * I)):
                v = sorted(timeit(fn, iters, warmup=1) for _ in range(windows))
                med = v[len(v) // 2]
                print(f"  N={N:5d} {kn:12s} median {med / 1000:8.2f} ms  "
                      f"min {v[0] / 1000:8.2f}  max {v[-1] / 1000:8.2f}  "
                      f"{active * elems * bits / 8 / (med / 1e6) / 1e12:5.2f}"
                      f" TB/s of weights  "
                      f"{2.0 * P * elems / (med / 1e6) / 1e12:6.1f} TFLOP/s")
            del x16, hh, outs
        # for information: the resident dense route (builds its copy once)
        for N in (512, 4096):
            x = (torch.randn(N, H, device=dev, generator=g) * 0.1) \
                .to(torch.bfloat16)
            idx = torch.rand(N, E, device=dev, generator=g) \
                .topk(K, dim=-1).indices
            w = torch.rand(N, K, device=dev, generator=g).to(torch.bfloat16)
            run("resident", x, w, idx)
            v = sorted(timeit(lambda: run("resident", x, w, idx), iters,
                              warmup=0) / 1000 for _ in range(windows))
            print(f"  N={N:5d} resident median {v[len(v) // 2]:8.2f} ms  "
                  f"min {v[0]:8.2f}  max {v[-1]:8.2f}")
        del gate, up, down
        torch.cuda.empty_cache()
    for k in keys:
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
    ap.add_argument("--w4-prefill", action="store_true",
                    help="only the w4 MoE prefill comparison: packed "
                         "wide-tile route vs dequant per call")
    ap.add_argument("--fp8-only", action="store_true",
                    help="only the FP8-block vs 8-bit-affine comparison")
    ap.add_argument("--gate-only", action="store_true",
                    help="only the grouped-gating fused-vs-torch line")
    ap.add_argument("--v3-only", action="store_true",
                    help="only the DeepSeek-V3 gate and 128-head attention "
                         "lines")
    ap.add_argument("--mla-only", action="store_true",
                    help="only the 128- and 16-head absorbed-MLA decode "
                         "comparison: attn_decode_split vs the MFMA "
                         "mla_decode kernels")
    ap.add_argument("--mla-chunk", action="store_true",
                    help="only the short-chunk-over-a-prefix comparison: "
                         "expanded prefill vs the absorbed mla_chunk path")
    ap.add_argument("--gqa-chunk", action="store_true",
                    help="only the chunk-over-a-prefix comparison for the "
                         "GQA models: attn_prefill (after kv_fp8_dequant for "
                         "the FP8 cache) vs gqa_chunk / gqa_chunk_fp8")
    ap.add_argument("--gqa-decode", action="store_true",
                    help="only the GQA decode comparison: the scalar "
                         "attn_decode kernel vs the MFMA gqa_decode kernel")
    ap.add_argument("--gqa-decode-fp8", action="store_true",
                    help="only the FP8 KV cache rows: gqa_decode_fp8 vs the "
                         "bf16 decode path of the same shape (lengths 512, "
                         "4096 and 16384)")
    ap.add_argument("--lengths", type=int, nargs="+",
                    default=[512, 2048, 4096, 8192],
                    help="key lengths of --gqa-decode; the largest is the "
                         "capacity of the device-position rows")
    ap.add_argument("--moe-route", action="store_true",
                    help="only the prefill routing comparison: the fused "
                         "moe_route kernels vs the torch gate + sort")
    args = ap.parse_args()
    from mlx_sharding_amd import ops
    from mlx_sharding_amd.ops import reference as ref
    ext = ops.hip_ext()
    assert ext is not None
    dev = "cuda"
    torch.manual_seed(0)

    if args.moe_route:
        bench_moe_route(ops, ref, dev)
        return
    if args.gqa_chunk:
        bench_gqa_chunk(ops, ext, dev)
        return
    if args.gqa_decode:
        bench_gqa_decode(ext, dev, lengths=tuple(args.lengths))
        return
    if args.gqa_decode_fp8:
        bench_gqa_decode_fp8(ops, ext, dev)
        return
    if args.mla_only:
        bench_mla(ops, ext, dev)
        return
    if args.mla_chunk:
        bench_mla_chunk(ops, ext, dev)
        return
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
    if args.w4_prefill:
        bench_w4_prefill(ops, ext, dev)
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
