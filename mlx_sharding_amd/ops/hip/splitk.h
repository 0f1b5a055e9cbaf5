// Shared split-K plumbing for the decode-regime (M <= 64) GEMM family.
//
// A split-K launcher runs "zero fp32 scratch, accumulate partials with
// atomics, convert to bf16".  Every such launcher goes through the two
// host entry points below (defined once, in splitk.hip) — in
// particular the scratch is zeroed by a KERNEL, never hipMemsetAsync:
// when gemm_kseg was written, a memset enqueued during hipGraph stream
// capture was not recorded into the graph and replays accumulated into
// stale partials (caught by test_gemm_kseg_under_graph_capture).  A
// kernel launch is always captured, whatever the runtime does with
// memset nodes.
#pragma once

#include "hip_common.h"

extern "C" {
void launch_f32_zero(float* p, long n, hipStream_t stream);
// dst: bf16 [n], round-to-nearest-even (f2bf)
void launch_f32_to_bf16(const float* src, void* dst, long n,
                        hipStream_t stream);
}

// One lane's share of a 16x16 MFMA C tile D[row = output, col = token]:
// 4 consecutive output rows o0..o0+3 of token t.  fp32 atomicAdd into
// yf when split-K is active (yf != null), else a bf16 store into y;
// both are [M, O] row-major.
__device__ __forceinline__ void store_c_tile_lane(short* __restrict__ y,
                                                  float* __restrict__ yf,
                                                  const float4v& acc, int t,
                                                  int M, int o0, int O) {
  if (t >= M) return;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int o = o0 + reg;
    if (o < O) {
      if (yf != nullptr)
        atomicAdd(yf + (long)t * O + o, acc[reg]);
      else
        y[(long)t * O + o] = (short)__bfloat16_as_ushort(f2bf(acc[reg]));
    }
  }
}
