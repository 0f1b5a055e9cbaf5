// FP8 block-quantized weights (DeepSeek-V3/R1 checkpoints), W8A16:
// e4m3 weights [.., O, K] with one fp32 scale per 128x128 block
// (weight_scale_inv [.., ceil(O/128), K/128]), fp16 activations, fp32
// accumulation.  W[o, k] = float(w8[o, k]) * scale[o / 128, k / 128].
//
// Dequant is the hardware e4m3 -> fp16 widening (fp8_dequant.h), exact
// for every finite code and 4 VALU per 8 weights.  The block scale is
// NOT applied to the weights: a 16-row wave tile starts at a multiple of
// 16, so it lies inside one 128-row block and the scale of a (tile,
// k-block) is wave-uniform — one scalar load.  Each 128-wide k-block is
// accumulated from zero (4 MFMAs of k = 32) and folded into the running
// fp32 accumulator as acc += s * block_acc, so the fp32 scale is applied
// in fp32, once per 128 products.
//
// Lane-to-k map inside a k-block (the batch_kk_d shape of the w4f16
// GEMV): lane quarter q = lane >> 4 owns k = kb*128 + q*32 + i*8 + j for
// MFMA i = 0..3, element j = 0..7 — 32 contiguous weight bytes per lane
// (two 16-byte loads) and no MFMA that mixes two k-blocks.  A and B use
// the same map, so the k-permutation inside the dot product is
// consistent.
//
// Preconditions (checked by the bindings): K % 128 == 0, contiguous
// tensors, fp32 scales of the shape above; O is arbitrary (rows are
// clamped for loads, stores are guarded).

#include "hip_common.h"
#include "splitk.h"
#include "fp8_block.h"  // F8_* geometry, F8Lane, f8_fold

// ---------------------------------------------------------------------------
// Dequant to bf16: w8 [R, K] (R = E*O rows), scales [E, RB, KB], any O, K.
// One thread per 8 consecutive k (K % 8 == 0) or per element.
// ---------------------------------------------------------------------------
__global__ void fp8_block_dequant_kernel(const unsigned char* __restrict__ w,
                                         const float* __restrict__ sc,
                                         short* __restrict__ out, long R,
                                         int O, int K, int vec) {
  const int RB = (O + F8_KB - 1) / F8_KB, KB = (K + F8_KB - 1) / F8_KB;
  const long per_row = vec ? K / 8 : K;
  const long n = R * per_row;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (long)gridDim.x * blockDim.x) {
    const long r = t / per_row;
    const int c = (int)(t - r * per_row);
    const long e = r / O;
    const int o = (int)(r - e * O);
    const float* srow = sc + (e * RB + o / F8_KB) * KB;
    if (vec) {
      const int k = c * 8;  // 8 | 128: one scale block
      const float s = srow[k / F8_KB];
      const uint2 v = *reinterpret_cast<const uint2*>(w + r * K + k);
      const unsigned int wd[2] = {v.x, v.y};
      short8v o8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = fp8_to_f32((unsigned char)(wd[j / 4] >> (8 * (j & 3))));
        o8[j] = (short)__bfloat16_as_ushort(f2bf(f * s));
      }
      *reinterpret_cast<short8v*>(out + r * K + k) = o8;
    } else {
      const float f = fp8_to_f32(w[r * K + c]);
      out[r * K + c] = (short)__bfloat16_as_ushort(f2bf(f * srow[c / F8_KB]));
    }
  }
}

extern "C" void launch_fp8_block_dequant(const void* w, const float* sc,
                                         void* out, long R, int O, int K,
                                         hipStream_t stream) {
  const int vec = K % 8 == 0;
  const long n = R * (vec ? K / 8 : K);
  if (n <= 0) return;
  long blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  fp8_block_dequant_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(
      (const unsigned char*)w, sc, (short*)out, R, O, K, vec);
}

// ---------------------------------------------------------------------------
// Dense GEMV, M <= 64: y[M, O] = x[M, K] @ W[O, K]^T, bf16 out.
// LDS-free like w4f16_gemv_kernel: B fragments from the L2-resident fp16
// token rows, MZ = ceil(M/16) token groups share each A fragment,
// split-K over grid.y on k-block boundaries (fp32 atomics into yf).
// MZ == 1 walks two k-blocks per iteration so two MFMA chains are in
// flight; MZ >= 2 has one chain per token group.
// ---------------------------------------------------------------------------
template <int MZ, int KU>
__device__ __forceinline__ void f8_gemv_kblocks(
    const unsigned char* wrow, const float* srow,
    const _Float16* (&xrow)[MZ], int kb, int q, float4v (&acc)[MZ]) {
  F8Lane wl[KU];
  f16x8 bv[KU][MZ][4];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const int k0 = (kb + u) * F8_KB + q * 32;
    wl[u].load(wrow + k0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int z = 0; z < MZ; ++z)
        bv[u][z][i] = *reinterpret_cast<const f16x8*>(xrow[z] + k0 + i * 8);
  }
  float4v bacc[KU][MZ];
#pragma unroll
  for (int u = 0; u < KU; ++u)
#pragma unroll
    for (int z = 0; z < MZ; ++z) bacc[u][z] = f8_zero4();
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const f16x8 af = wl[u].frag(i);
#pragma unroll
      for (int z = 0; z < MZ; ++z)
        bacc[u][z] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
            af, bv[u][z][i], bacc[u][z], 0, 0, 0);
    }
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const float s = srow[kb + u];
#pragma unroll
    for (int z = 0; z < MZ; ++z) f8_fold(acc[z], s, bacc[u][z]);
  }
}

template <int MZ>
__global__ __launch_bounds__(F8_BLOCK) void fp8f16_gemv_kernel(
    const _Float16* __restrict__ x,        // [M, K] fp16
    const unsigned char* __restrict__ w,   // [O, K] e4m3
    const float* __restrict__ sc,          // [ceil(O/128), K/128]
    short* __restrict__ y,                 // [M, O] bf16
    float* __restrict__ yf,                // split-K fp32 partials or null
    int M, int O, int K) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int row0 = (blockIdx.x * F8_WAVES + wid) * 16;
  if (row0 >= O) return;
  const int nkb = K / F8_KB;
  const int wr = min(row0 + (lane & 15), O - 1);
  const unsigned char* wrow = w + (long)wr * K;
  const int rb = __builtin_amdgcn_readfirstlane(row0 / F8_KB);
  const float* srow = sc + (long)rb * nkb;
  const _Float16* xrow[MZ];
#pragma unroll
  for (int z = 0; z < MZ; ++z)
    xrow[z] = x + (long)min(z * 16 + (lane & 15), M - 1) * K;

  float4v acc[MZ];
#pragma unroll
  for (int z = 0; z < MZ; ++z) acc[z] = f8_zero4();

  // k-blocks of this split
  const int nbps = (nkb + gridDim.y - 1) / gridDim.y;
  const int kb_lo = blockIdx.y * nbps;
  const int kb_hi = min(nkb, kb_lo + nbps);
  const int q = lane >> 4;
  constexpr int KU = MZ == 1 ? 2 : 1;

  int kb = kb_lo;
  for (; kb + KU <= kb_hi; kb += KU)
    f8_gemv_kblocks<MZ, KU>(wrow, srow, xrow, kb, q, acc);
  if (KU > 1 && kb < kb_hi)
    f8_gemv_kblocks<MZ, 1>(wrow, srow, xrow, kb, q, acc);

#pragma unroll
  for (int z = 0; z < MZ; ++z)
    store_c_tile_lane(y, yf, acc[z], z * 16 + (lane & 15), M,
                      row0 + (lane >> 4) * 4, O);
}

extern "C" int fp8f16_gemv_nsplit(int M, int O, int K) {
  (void)M;
  const int gx = (O + F8_WAVES * 16 - 1) / (F8_WAVES * 16);
  const int nkb = K / F8_KB;
  int nk = 256 / (gx > 0 ? gx : 1);
  if (nk > nkb) nk = nkb;
  if (nk < 1) nk = 1;
  return nk;
}

extern "C" void launch_fp8f16_gemv(const void* x, const void* w,
                                   const float* sc, void* y, float* yf,
                                   int nk, int M, int O, int K,
                                   hipStream_t stream) {
  if (nk > 1) launch_f32_zero(yf, (long)M * O, stream);
  const int gx = (O + F8_WAVES * 16 - 1) / (F8_WAVES * 16);
  const int mz = (M + 15) / 16;
  dim3 grid((unsigned)gx, (unsigned)nk);
  float* yfp = nk > 1 ? yf : nullptr;
#define F8GV_CASE(Z)                                                     \
  case Z:                                                                \
    fp8f16_gemv_kernel<Z><<<grid, dim3(F8_BLOCK), 0, stream>>>(          \
        (const _Float16*)x, (const unsigned char*)w, sc, (short*)y, yfp, \
        M, O, K);                                                        \
    break;
  switch (mz) {
    F8GV_CASE(1)
    F8GV_CASE(2)
    F8GV_CASE(3)
    F8GV_CASE(4)
    default:
      break;
  }
#undef F8GV_CASE
  if (nk > 1) launch_f32_to_bf16(yf, y, (long)M * O, stream);
}

// ---------------------------------------------------------------------------
// Fused gate+up+SiLU over 16-token sub-ranges (the moe_w4f16_gateup
// contract; a longer sub-range is walked in 16-token tiles).
//   x:  [N, H] fp16;  gw/uw: [E, I, H] e4m3;  gs/us: [E, ceil(I/128), H/128]
//   h:  [P, I] fp16 out
// grid = (ceil(I/64), S).  Gate and up are the two independent MFMA
// chains.  clear: optional fp32 [clear_n] buffer zeroed by this launch
// (the down kernel's accumulator): every block clears a grid-stride
// share BEFORE any early exit, so the whole buffer is covered whatever
// the grid size and however many sub-range slots are padding.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(F8_BLOCK) void moe_fp8f16_gateup_kernel(
    const _Float16* __restrict__ x, const unsigned char* __restrict__ gw,
    const unsigned char* __restrict__ uw, const float* __restrict__ gsc,
    const float* __restrict__ usc, _Float16* __restrict__ h,
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    int H, int I, float* __restrict__ clear, long clear_n) {
  if (clear) {
    const long nthr = (long)gridDim.x * gridDim.y * F8_BLOCK;
    const long t0 =
        ((long)blockIdx.y * gridDim.x + blockIdx.x) * F8_BLOCK + threadIdx.x;
    const long n4 = clear_n / 4;  // allocation is 16-byte aligned
    for (long i = t0; i < n4; i += nthr)
      reinterpret_cast<float4v*>(clear)[i] = float4v{0, 0, 0, 0};
    for (long i = n4 * 4 + t0; i < clear_n; i += nthr) clear[i] = 0.0f;
  }
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;

  const int row0 = (blockIdx.x * F8_WAVES + wid) * 16;
  if (row0 >= I) return;
  const int wr = min(row0 + (lane & 15), I - 1);
  const long ebase = (long)e * I;
  const unsigned char* grow = gw + (ebase + wr) * H;
  const unsigned char* urow = uw + (ebase + wr) * H;
  const int nkb = H / F8_KB;
  const int nrb = (I + F8_KB - 1) / F8_KB;
  const int rb = __builtin_amdgcn_readfirstlane(row0 / F8_KB);
  const float* gsr = gsc + ((long)e * nrb + rb) * nkb;
  const float* usr = usc + ((long)e * nrb + rb) * nkb;
  const int q = lane >> 4;
  const int tok = lane & 15;
  // a sub-range longer than one 16-token tile is walked tile by tile
  for (int c0 = 0; c0 < cnt; c0 += 16) {
  const int cc = min(16, cnt - c0);
  const _Float16* xrow =
      x + (long)sorted_tok[p0 + c0 + min(tok, cc - 1)] * H;

  float4v gacc = f8_zero4(), uacc = f8_zero4();
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * F8_KB + q * 32;
    F8Lane gl, ul;
    gl.load(grow + k0);
    ul.load(urow + k0);
    f16x8 bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      bv[i] = *reinterpret_cast<const f16x8*>(xrow + k0 + i * 8);
    float4v gb = f8_zero4(), ub = f8_zero4();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gb = __builtin_amdgcn_mfma_f32_16x16x32_f16(gl.frag(i), bv[i], gb, 0, 0,
                                                  0);
      ub = __builtin_amdgcn_mfma_f32_16x16x32_f16(ul.frag(i), bv[i], ub, 0, 0,
                                                  0);
    }
    f8_fold(gacc, gsr[kb], gb);
    f8_fold(uacc, usr[kb], ub);
  }

  if (tok < cc) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int o = row0 + (lane >> 4) * 4 + reg;
      if (o < I) {
        const float g = gacc[reg], u = uacc[reg];
        const float a = g / (1.0f + __expf(-g));  // silu
        h[(long)(p0 + c0 + tok) * I + o] = (_Float16)(a * u);
      }
    }
  }
  }  // 16-token tiles
}

// ---------------------------------------------------------------------------
// Down-proj + weighted atomic scatter (fp32 out).
//   hh: [P, I] fp16 (gate-up output);  dw: [E, H, I] e4m3;
//   dsc: [E, ceil(H/128), I/128]
// Two k-blocks per iteration give the two independent MFMA chains.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(F8_BLOCK) void moe_fp8f16_down_kernel(
    const _Float16* __restrict__ hh, const unsigned char* __restrict__ dw,
    const float* __restrict__ dsc, float* __restrict__ out,
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    const float* __restrict__ sorted_wt, int I, int H) {
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;

  const int row0 = (blockIdx.x * F8_WAVES + wid) * 16;
  if (row0 >= H) return;
  const int wr = min(row0 + (lane & 15), H - 1);
  const unsigned char* drow = dw + ((long)e * H + wr) * I;
  const int nkb = I / F8_KB;
  const int nrb = (H + F8_KB - 1) / F8_KB;
  const int rb = __builtin_amdgcn_readfirstlane(row0 / F8_KB);
  const float* dsr = dsc + ((long)e * nrb + rb) * nkb;
  const int q = lane >> 4;
  const int tok = lane & 15;
  // a sub-range longer than one 16-token tile is walked tile by tile
  for (int c0 = 0; c0 < cnt; c0 += 16) {
  const int cc = min(16, cnt - c0);
  const _Float16* hrow = hh + (long)(p0 + c0 + min(tok, cc - 1)) * I;

  float4v acc = f8_zero4();
  int kb = 0;
  for (; kb + 2 <= nkb; kb += 2) {
    const int k0 = kb * F8_KB + q * 32;
    F8Lane d0, d1;
    d0.load(drow + k0);
    d1.load(drow + k0 + F8_KB);
    f16x8 bv0[4], bv1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bv0[i] = *reinterpret_cast<const f16x8*>(hrow + k0 + i * 8);
      bv1[i] = *reinterpret_cast<const f16x8*>(hrow + k0 + F8_KB + i * 8);
    }
    float4v b0 = f8_zero4(), b1 = f8_zero4();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      b0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d0.frag(i), bv0[i], b0, 0,
                                                  0, 0);
      b1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d1.frag(i), bv1[i], b1, 0,
                                                  0, 0);
    }
    f8_fold(acc, dsr[kb], b0);
    f8_fold(acc, dsr[kb + 1], b1);
  }
  if (kb < nkb) {  // odd k-block count: the last one alone
    const int k0 = kb * F8_KB + q * 32;
    F8Lane d0;
    d0.load(drow + k0);
    float4v b0 = f8_zero4();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f16x8 bvv = *reinterpret_cast<const f16x8*>(hrow + k0 + i * 8);
      b0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(d0.frag(i), bvv, b0, 0, 0,
                                                  0);
    }
    f8_fold(acc, dsr[kb], b0);
  }

  if (tok < cc) {
    const float wt = sorted_wt[p0 + c0 + tok];
    const long trow = (long)sorted_tok[p0 + c0 + tok] * H;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int o = row0 + (lane >> 4) * 4 + reg;
      if (o < H) atomicAdd(out + trow + o, wt * acc[reg]);
    }
  }
  }  // 16-token tiles
}

extern "C" void launch_moe_fp8f16_gateup(
    const void* x, const void* gw, const void* uw, const float* gsc,
    const float* usc, void* h, const int* sub_expert, const int* sub_off,
    const int* sub_cnt, const int* sorted_tok, int S, int H, int I,
    float* clear, long clear_n, hipStream_t stream) {
  const int gx = (I + F8_WAVES * 16 - 1) / (F8_WAVES * 16);
  moe_fp8f16_gateup_kernel<<<dim3(gx, S), dim3(F8_BLOCK), 0, stream>>>(
      (const _Float16*)x, (const unsigned char*)gw, (const unsigned char*)uw,
      gsc, usc, (_Float16*)h, sub_expert, sub_off, sub_cnt, sorted_tok, H, I,
      clear, clear_n);
}

extern "C" void launch_moe_fp8f16_down(
    const void* hh, const void* dw, const float* dsc, float* out,
    const int* sub_expert, const int* sub_off, const int* sub_cnt,
    const int* sorted_tok, const float* sorted_wt, int S, int I, int H,
    hipStream_t stream) {
  const int gx = (H + F8_WAVES * 16 - 1) / (F8_WAVES * 16);
  moe_fp8f16_down_kernel<<<dim3(gx, S), dim3(F8_BLOCK), 0, stream>>>(
      (const _Float16*)hh, (const unsigned char*)dw, dsc, out, sub_expert,
      sub_off, sub_cnt, sorted_tok, sorted_wt, I, H);
}
