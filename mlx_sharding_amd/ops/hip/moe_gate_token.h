// Limits and wave helpers shared by the fused MoE gates: the
// single-workgroup decode kernel (moe.hip: moe_gate_subranges_kernel) and
// the multi-block prefill route (moe_route.hip).
#pragma once

#include "hip_common.h"

#define GK_MAXK 8
#define GK_MAXE 256  // max experts (fixed-size LDS arrays)

// Wave argmax of (v, idx) pairs, ties to the lowest idx; every lane ends
// up with the winner.
__device__ __forceinline__ void gk_wave_argmax(float& best, int& bidx) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(best, off, WAVE);
    int oi = __shfl_xor(bidx, off, WAVE);
    if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
  }
}

// out[e] = sum_{j<e} ceil(cnt[j] / div) for e in [0, E], by ONE wave:
// lane l owns experts 4l..4l+3 (E <= 256), then a 6-step wave scan.
__device__ __forceinline__ void gk_wave_prefix(const int* cnt, int* out, int E,
                                               int div, int lane) {
  int c[4];
  int s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane * 4 + j;
    c[j] = (e < E) ? (cnt[e] + div - 1) / div : 0;
    s += c[j];
  }
  int inc = s;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int o = __shfl_up(inc, off, WAVE);
    if (lane >= off) inc += o;
  }
  int acc = inc - s;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane * 4 + j;
    if (e < E) out[e] = acc;
    acc += c[j];
  }
  if (lane == WAVE - 1) out[E] = inc;
}
