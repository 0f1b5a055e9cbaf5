// Prefill-regime siblings of the packed FP8 MoE kernels of fp8_block.hip:
// the same sub-range contract and the same arithmetic (hardware e4m3 ->
// fp16 widening with scale 1.0, fp16 MFMA, every 128-wide k-block
// accumulated from zero and folded in as acc += s * block_acc with the
// wave-uniform fp32 block scale, the same lane-quarter k map for both
// operands), built for sub-ranges of F8W_TM tokens instead of 16.
//
// One block of 4 waves owns 64 weight rows x F8W_TM tokens.  Each wave
// streams its own 16 weight rows straight to registers (they are not
// shared) and keeps every weight fragment for all MZ = F8W_TM / 16 token
// column tiles, so an expert's weights are read once per F8W_TM tokens.
//
// The activations ARE shared by the four waves: the F8W_TM x 128 fp16 slab
// of a k-block is gathered once per block into LDS in full 256-byte
// rows (16 lanes per row), double-buffered, one barrier per k-block, and
// read back as 16-byte B fragments.  LDS image, in 16-byte slots:
//     slot(t, c) = c * F8W_TM + (t ^ swz(c)),   c = k / 8 in 0..15,
//     swz(c) = ((c & 3) << 1) | ((c >> 2) & 1)
// A fragment read has c = q * 4 + i (lane quarter q, MFMA i): the 16 lanes
// of a ds_read_b128 group hold two quarters q, q + 1 with complementary
// token sets ({0-3, 12-15} and {4-11}); F8W_TM * 16 bytes is a multiple of
// the 256-byte bank row, swz differs between the two only in bit 0 and both
// sets are closed under that, so the group covers 16 distinct slots.  A
// gather write has 8 consecutive lanes on one token and c = 0..7 (or
// 8..15), where swz takes 8 distinct values: no bank is hit twice.
//
// Token rows past cnt are clamped for loads and masked for stores; token
// column tiles wholly past cnt skip their MFMAs.  There are barriers
// inside the k loop, so no wave may leave early: the cnt == 0 exit is
// block-uniform and sits before the first barrier, and a wave whose 16
// rows lie past the last weight row stays in the loop on clamped (in
// bounds) rows and only skips its stores.
//
// Preconditions (checked by the bindings): K % 128 == 0, contiguous
// tensors; O is arbitrary.

#include "hip_common.h"
#include "fp8_block.h"

#ifndef F8W_TM
#define F8W_TM 64  // tokens per tile (docs/PERFORMANCE.md, "FP8 prefill")
#endif
#define F8W_MZ (F8W_TM / 16)
#define F8W_SLAB (16 * F8W_TM)  // 16-byte slots per buffer
static_assert(F8W_TM >= 64 && F8W_TM % 16 == 0, "tile is whole 16-token MFMAs");

__device__ __forceinline__ int f8w_swz(int c) {
  return ((c & 3) << 1) | ((c >> 2) & 1);
}

// Gather side: thread tid owns chunk c = tid & 15 of rows j * 16 + tid / 16.
struct F8WStage {
  f16x8 v[F8W_MZ];
  __device__ __forceinline__ void load(const _Float16* (&rowp)[F8W_MZ],
                                       int kb, int c) {
#pragma unroll
    for (int j = 0; j < F8W_MZ; ++j)
      v[j] = *reinterpret_cast<const f16x8*>(rowp[j] + kb * F8_KB + c * 8);
  }
  __device__ __forceinline__ void store(f16x8* buf, int r, int c) const {
    const int sw = f8w_swz(c);
#pragma unroll
    for (int j = 0; j < F8W_MZ; ++j)
      buf[c * F8W_TM + ((j * 16 + r) ^ sw)] = v[j];
  }
};

// The k loop of one tile: NW weight matrices (gate and up, or down alone)
// against the shared slab.  acc[w][z] is the 16 x 16 tile of matrix w and
// token column tile z.  XA: the activations are the MFMA's first operand
// (the accumulator then has tokens down the registers and weight rows
// across the lanes).  Ends on a barrier, so the caller may refill buffer 0
// at once.
template <int NW, bool XA>
__device__ __forceinline__ void f8w_tile(
    f16x8* slab, const _Float16* (&rowp)[F8W_MZ],
    const unsigned char* (&wrow)[NW], const float* (&srow)[NW],
    int nkb, int nz, float4v (&acc)[NW][F8W_MZ]) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int q = lane >> 4, tok = lane & 15;
  const int sr = threadIdx.x >> 4, scn = threadIdx.x & 15;

  F8WStage st;
  F8Lane wl[NW];
  st.load(rowp, 0, scn);
#pragma unroll
  for (int w = 0; w < NW; ++w) wl[w].load(wrow[w] + q * 32);
  st.store(slab, sr, scn);
  __syncthreads();

  for (int kb = 0; kb < nkb; ++kb) {
    const f16x8* cur = slab + (kb & 1) * F8W_SLAB;
    const bool more = kb + 1 < nkb;  // block-uniform
    F8Lane wn[NW];
    if (more) {
      st.load(rowp, kb + 1, scn);
#pragma unroll
      for (int w = 0; w < NW; ++w)
        wn[w].load(wrow[w] + (kb + 1) * F8_KB + q * 32);
    }
    float4v bacc[NW][F8W_MZ];
#pragma unroll
    for (int w = 0; w < NW; ++w)
#pragma unroll
      for (int z = 0; z < F8W_MZ; ++z) bacc[w][z] = f8_zero4();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f16x8 wf[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) wf[w] = wl[w].frag(i);
      const int c = q * 4 + i;
      const f16x8* col = cur + c * F8W_TM;
      const int sw = f8w_swz(c);
#pragma unroll
      for (int z = 0; z < F8W_MZ; ++z) {
        if (z < nz) {  // wave-uniform
          const f16x8 xf = col[(z * 16 + tok) ^ sw];
#pragma unroll
          for (int w = 0; w < NW; ++w)
            bacc[w][z] =
                XA ? __builtin_amdgcn_mfma_f32_16x16x32_f16(xf, wf[w],
                                                            bacc[w][z], 0, 0, 0)
                   : __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[w], xf,
                                                            bacc[w][z], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float s = srow[w][kb];
#pragma unroll
      for (int z = 0; z < F8W_MZ; ++z)
        if (z < nz) f8_fold(acc[w][z], s, bacc[w][z]);
    }
    if (more) {
      // the other buffer was last read before the previous barrier
      st.store(slab + ((kb + 1) & 1) * F8W_SLAB, sr, scn);
#pragma unroll
      for (int w = 0; w < NW; ++w) wl[w] = wn[w];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Fused gate+up+SiLU over F8W_TM-token sub-ranges.
//   x:  [N, H] fp16;  gw/uw: [E, I, H] e4m3;  gsc/usc: [E, ceil(I/128), H/128]
//   h:  [P, I] fp16 out
// grid = (ceil(I/64), S).  Weights are the MFMA's first operand and the
// epilogue is moe_fp8f16_gateup_kernel's: the two kernels agree bit for bit.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(F8_BLOCK) void moe_fp8f16_gateup_wide_kernel(
    const _Float16* __restrict__ x, const unsigned char* __restrict__ gw,
    const unsigned char* __restrict__ uw, const float* __restrict__ gsc,
    const float* __restrict__ usc, _Float16* __restrict__ h,
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    int H, int I) {
  __shared__ f16x8 slab[2 * F8W_SLAB];
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot: the whole block, before any barrier
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int q = lane >> 4, tok = lane & 15;

  const int row0 = (blockIdx.x * F8_WAVES + wid) * 16;
  const int wr = min(row0 + tok, I - 1);
  const long ebase = (long)e * I;
  const unsigned char* wrow[2] = {gw + (ebase + wr) * H,
                                        uw + (ebase + wr) * H};
  const int nkb = H / F8_KB;
  const int nrb = (I + F8_KB - 1) / F8_KB;
  const int rb = __builtin_amdgcn_readfirstlane(min(row0, I - 1) / F8_KB);
  const float* srow[2] = {gsc + ((long)e * nrb + rb) * nkb,
                                usc + ((long)e * nrb + rb) * nkb};
  const int sr = threadIdx.x >> 4;

  for (int c0 = 0; c0 < cnt; c0 += F8W_TM) {
    const int cc = min(F8W_TM, cnt - c0);
    const int nz = (cc + 15) >> 4;
    const _Float16* rowp[F8W_MZ];
#pragma unroll
    for (int j = 0; j < F8W_MZ; ++j)
      rowp[j] = x + (long)sorted_tok[p0 + c0 + min(j * 16 + sr, cc - 1)] * H;

    float4v acc[2][F8W_MZ];
#pragma unroll
    for (int z = 0; z < F8W_MZ; ++z) acc[0][z] = acc[1][z] = f8_zero4();
    f8w_tile<2, false>(slab, rowp, wrow, srow, nkb, nz, acc);

    // the 16-token kernel's epilogue, expression for expression, so that
    // the compiler lowers silu(g) * u -> fp16 the same way in both
#pragma unroll
    for (int z = 0; z < F8W_MZ; ++z) {
      const int t = z * 16 + tok;
      if (t < cc) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int o = row0 + q * 4 + reg;
          if (o < I) {
            const float g = acc[0][z][reg], u = acc[1][z][reg];
            const float a = g / (1.0f + __expf(-g));  // silu
            h[(long)(p0 + c0 + t) * I + o] = (_Float16)(a * u);
          }
        }
      }
    }
  }  // F8W_TM-token tiles
}

// ---------------------------------------------------------------------------
// Down-proj + weighted atomic scatter (fp32 out).
//   hh: [P, I] fp16 (gate-up output);  dw: [E, H, I] e4m3;
//   dsc: [E, ceil(H/128), I/128];  out: [N, H] fp32, zeroed by the caller
// grid = (ceil(H/64), S).  The activations are the MFMA's first operand,
// so a lane ends with one output column of 4 tokens and an atomic
// wave-instruction covers 4 token rows x 16 consecutive floats (64-byte
// segments) instead of 16 rows x 4 scattered dwords.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(F8_BLOCK) void moe_fp8f16_down_wide_kernel(
    const _Float16* __restrict__ hh, const unsigned char* __restrict__ dw,
    const float* __restrict__ dsc, float* __restrict__ out,
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    const float* __restrict__ sorted_wt, int I, int H) {
  __shared__ f16x8 slab[2 * F8W_SLAB];
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot: the whole block, before any barrier
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int q = lane >> 4, col = lane & 15;

  const int row0 = (blockIdx.x * F8_WAVES + wid) * 16;
  const int wr = min(row0 + col, H - 1);
  const unsigned char* wrow[1] = {dw + ((long)e * H + wr) * I};
  const int nkb = I / F8_KB;
  const int nrb = (H + F8_KB - 1) / F8_KB;
  const int rb = __builtin_amdgcn_readfirstlane(min(row0, H - 1) / F8_KB);
  const float* srow[1] = {dsc + ((long)e * nrb + rb) * nkb};
  const int sr = threadIdx.x >> 4;

  for (int c0 = 0; c0 < cnt; c0 += F8W_TM) {
    const int cc = min(F8W_TM, cnt - c0);
    const int nz = (cc + 15) >> 4;
    const _Float16* rowp[F8W_MZ];
#pragma unroll
    for (int j = 0; j < F8W_MZ; ++j)
      rowp[j] = hh + (long)(p0 + c0 + min(j * 16 + sr, cc - 1)) * I;

    float4v acc[1][F8W_MZ];
#pragma unroll
    for (int z = 0; z < F8W_MZ; ++z) acc[0][z] = f8_zero4();
    f8w_tile<1, true>(slab, rowp, wrow, srow, nkb, nz, acc);

    const int o = row0 + col;
    if (o < H) {
#pragma unroll
      for (int z = 0; z < F8W_MZ; ++z) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int t = z * 16 + q * 4 + reg;
          if (t < cc) {
            const int p = p0 + c0 + t;
            atomicAdd(out + (long)sorted_tok[p] * H + o,
                      sorted_wt[p] * acc[0][z][reg]);
          }
        }
      }
    }
  }  // F8W_TM-token tiles
}

extern "C" int moe_fp8f16_wide_tile() { return F8W_TM; }

extern "C" void launch_moe_fp8f16_gateup_wide(
    const void* x, const void* gw, const void* uw, const float* gsc,
    const float* usc, void* h, const int* sub_expert, const int* sub_off,
    const int* sub_cnt, const int* sorted_tok, int S, int H, int I,
    hipStream_t stream) {
  const int gx = (I + F8_WAVES * 16 - 1) / (F8_WAVES * 16);
  moe_fp8f16_gateup_wide_kernel<<<dim3(gx, S), dim3(F8_BLOCK), 0, stream>>>(
      (const _Float16*)x, (const unsigned char*)gw, (const unsigned char*)uw,
      gsc, usc, (_Float16*)h, sub_expert, sub_off, sub_cnt, sorted_tok, H, I);
}

extern "C" void launch_moe_fp8f16_down_wide(
    const void* hh, const void* dw, const float* dsc, float* out,
    const int* sub_expert, const int* sub_off, const int* sub_cnt,
    const int* sorted_tok, const float* sorted_wt, int S, int I, int H,
    hipStream_t stream) {
  const int gx = (H + F8_WAVES * 16 - 1) / (F8_WAVES * 16);
  moe_fp8f16_down_wide_kernel<<<dim3(gx, S), dim3(F8_BLOCK), 0, stream>>>(
      (const _Float16*)hh, (const unsigned char*)dw, dsc, out, sub_expert,
      sub_off, sub_cnt, sorted_tok, sorted_wt, I, H);
}
