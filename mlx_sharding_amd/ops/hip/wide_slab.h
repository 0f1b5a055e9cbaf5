// The activation slab of the wide-tile MoE prefill kernels (fp8_prefill.hip,
// w4_prefill.hip): the TM x 128 fp16 activations of one k-block, gathered
// once per 4-wave block into LDS in full 256-byte rows (16 lanes per row)
// and read back as 16-byte MFMA fragments.  LDS image, in 16-byte slots:
//     slot(t, c) = c * TM + (t ^ swz(c)),   c = k / 8 in 0..15,
//     swz(c) = ((c & 3) << 1) | ((c >> 2) & 1)
// A fragment read has c = q * 4 + i (lane quarter q, MFMA i): the 16 lanes
// of a ds_read_b128 group hold two quarters q, q + 1 with complementary
// token sets ({0-3, 12-15} and {4-11}); TM * 16 bytes is a multiple of
// the 256-byte bank row, swz differs between the two only in bit 0 and both
// sets are closed under that, so the group covers 16 distinct slots.  A
// gather write has 8 consecutive lanes on one token and c = 0..7 (or
// 8..15), where swz takes 8 distinct values: no bank is hit twice.
#pragma once

#include "hip_common.h"
#include "w4f16_dequant.h"  // f16x8

#define WS_KB 128  // k-block: elements of the reduction dimension per slab

__device__ __forceinline__ int ws_swz(int c) {
  return ((c & 3) << 1) | ((c >> 2) & 1);
}

// Gather side: thread tid of a 256-thread block owns chunk c = tid & 15 of
// rows j * 16 + tid / 16, j = 0 .. TM / 16 - 1.
template <int TM>
struct WideStage {
  static constexpr int MZ = TM / 16;
  f16x8 v[MZ];
  __device__ __forceinline__ void load(const _Float16* (&rowp)[MZ], int kb,
                                       int c) {
#pragma unroll
    for (int j = 0; j < MZ; ++j)
      v[j] = *reinterpret_cast<const f16x8*>(rowp[j] + kb * WS_KB + c * 8);
  }
  __device__ __forceinline__ void store(f16x8* buf, int r, int c) const {
    const int sw = ws_swz(c);
#pragma unroll
    for (int j = 0; j < MZ; ++j) buf[c * TM + ((j * 16 + r) ^ sw)] = v[j];
  }
};
