// Shared pieces of the FP8 block-quantized W8A16 kernels (fp8_block.hip,
// fp8_prefill.hip): block geometry, the per-lane weight share of a
// k-block and the fp32 scale fold.  The arithmetic contract is in the
// header of fp8_block.hip.
#pragma once

#include "hip_common.h"
#include "fp8_dequant.h"

#define F8_WAVES 4
#define F8_BLOCK (F8_WAVES * WAVE)
#define F8_KB 128  // scale-block edge

__device__ __forceinline__ float4v f8_zero4() { return float4v{0, 0, 0, 0}; }

// acc += s * b
__device__ __forceinline__ void f8_fold(float4v& acc, float s,
                                        const float4v& b) {
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] += s * b[r];
}

// One lane's share of a weight k-block: 32 contiguous bytes.
struct F8Lane {
  uint4 lo, hi;
  __device__ __forceinline__ void load(const unsigned char* p) {
    lo = *reinterpret_cast<const uint4*>(p);
    hi = *reinterpret_cast<const uint4*>(p + 16);
  }
  // A fragment of MFMA i (bytes i*8 .. i*8+7)
  __device__ __forceinline__ f16x8 frag(int i) const {
    switch (i) {
      case 0: return fp8x8_to_f16(lo.x, lo.y);
      case 1: return fp8x8_to_f16(lo.z, lo.w);
      case 2: return fp8x8_to_f16(hi.x, hi.y);
      default: return fp8x8_to_f16(hi.z, hi.w);
    }
  }
};
