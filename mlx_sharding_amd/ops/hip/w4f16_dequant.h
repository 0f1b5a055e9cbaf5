// fp16 magic-number dequant of repacked w4/w8 words (ops.repack_w4),
// shared by the fp16-dequant MFMA kernels (moe_w4f16.hip, gemm_kseg.hip).
// Scheme (derivation in the moe_w4f16.hip header): OR 0x6400 makes each
// nibble/byte the exact fp16 1024+q, a pk_add recenters to the exact
// q-8 (q-128 for w8), and one pk_fma applies (s, b + 8s).
#pragma once

#include "hip_common.h"

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

union f16pack {
  unsigned int u;
  f16x2 h;
};

// dequant one repacked u32 (8 x 4-bit) into 4 fp16 pairs
template <int BITS>
__device__ __forceinline__ void dq8(unsigned int w, f16x2 s2, f16x2 b2,
                                    f16x8* out) {
  f16x2* op = reinterpret_cast<f16x2*>(out);
  if (BITS == 4) {
    const f16x2 c = {(_Float16)(-1032.0f), (_Float16)(-1032.0f)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f16pack p;
      p.u = ((w >> (4 * j)) & 0x000F000Fu) | 0x64006400u;  // v_and_or_b32
      f16x2 v = p.h + c;          // exact small int q-8
      op[j] = v * s2 + b2;        // v_pk_fma_f16
    }
  }
}

// w8: two repacked u32s -> 4 fp16 pairs
__device__ __forceinline__ void dq8_w8(unsigned int w0, unsigned int w1,
                                       f16x2 s2, f16x2 b2, f16x8* out) {
  const f16x2 c = {(_Float16)(-1152.0f), (_Float16)(-1152.0f)};
  f16x2* op = reinterpret_cast<f16x2*>(out);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    f16pack p;
    p.u = ((w0 >> (8 * j)) & 0x00FF00FFu) | 0x64006400u;
    op[j] = (p.h + c) * s2 + b2;
    p.u = ((w1 >> (8 * j)) & 0x00FF00FFu) | 0x64006400u;
    op[2 + j] = (p.h + c) * s2 + b2;
  }
}

__device__ __forceinline__ f16x2 splat2(float v) {
  const _Float16 h = (_Float16)v;
  return (f16x2){h, h};
}
