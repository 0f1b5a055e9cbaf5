// OCP e4m3 (float8_e4m3fn) -> fp16 conversion for the W8A16 block-scaled
// kernels (fp8_block.hip).  All 254 finite e4m3 codes are fp16 values
// (4 significant bits, exponents 2^-9 .. 2^8), so the widening is exact;
// gfx950 does it in hardware, two weights per instruction
// (v_cvt_scalef32_pk_f16_fp8).  The instruction's scale operand is held
// at 1.0: the checkpoint's fp32 block scale is applied to the fp32
// block accumulator instead (see fp8_block.hip), never folded in here.
#pragma once

#include "hip_common.h"
#include "w4f16_dequant.h"  // f16x2 / f16x8

typedef __fp16 fp8cvt_h2 __attribute__((ext_vector_type(2)));

// two fp8 bytes (the low or high half of w) -> two fp16, byte order kept
__device__ __forceinline__ f16x2 fp8x2_to_f16(unsigned int w, bool hi) {
  const fp8cvt_h2 r =
      hi ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true)
         : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false);
  return __builtin_bit_cast(f16x2, r);
}

// 8 fp8 bytes in memory order (w0 = bytes 0..3, w1 = bytes 4..7) -> one
// f16x8 MFMA fragment in natural k order
__device__ __forceinline__ f16x8 fp8x8_to_f16(unsigned int w0,
                                              unsigned int w1) {
  f16x8 out;
  f16x2* op = reinterpret_cast<f16x2*>(&out);
  op[0] = fp8x2_to_f16(w0, false);
  op[1] = fp8x2_to_f16(w0, true);
  op[2] = fp8x2_to_f16(w1, false);
  op[3] = fp8x2_to_f16(w1, true);
  return out;
}

// one fp8 byte -> fp32 (exact)
__device__ __forceinline__ float fp8_to_f32(unsigned char b) {
  return __builtin_amdgcn_cvt_f32_fp8((int)b, 0);
}
