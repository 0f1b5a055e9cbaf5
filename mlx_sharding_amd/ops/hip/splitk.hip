// Split-K scratch zeroing and fp32 -> bf16 convert (see splitk.h).

#include "splitk.h"

__global__ void splitk_zero_kernel(float* __restrict__ p, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.0f;
}

__global__ void splitk_to_bf16_kernel(const float* __restrict__ src,
                                      short* __restrict__ dst, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (short)__bfloat16_as_ushort(f2bf(src[i]));
}

extern "C" void launch_f32_zero(float* p, long n, hipStream_t stream) {
  splitk_zero_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       stream>>>(p, n);
}

extern "C" void launch_f32_to_bf16(const float* src, void* dst, long n,
                                   hipStream_t stream) {
  splitk_to_bf16_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                          stream>>>(src, (short*)dst, n);
}
