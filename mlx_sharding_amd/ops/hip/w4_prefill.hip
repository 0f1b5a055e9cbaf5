// Prefill-regime siblings of the fp16-dequant w4/w8 MoE kernels of
// moe_w4f16.hip: the same sub-range contract and the same weight
// arithmetic (repacked words of ops.repack_w4, OR 0x6400, pk_add recenter,
// one pk_fma with (s, b + off * s): dq8 / dq8_w8 of w4f16_dequant.h, so the
// fp16 weight values are bit-identical), built for sub-ranges of W4W_TM
// tokens instead of 16.  The work split is fp8_prefill.hip's.
//
// One block of 4 waves owns 64 weight rows x W4W_TM tokens.  Each wave
// streams its own 16 weight rows straight to registers and keeps every
// dequantized fragment of a k-block for all MZ = W4W_TM / 16 token column
// tiles: the ~64 dequant VALU ops of a lane and k-block are paid once per
// W4W_TM tokens instead of once per 16, and an expert's packed weights are
// read once per W4W_TM tokens.
//
// A k-block is 128 elements.  Lane quarter q owns
//     k = kb * 128 + q * 32 + i * 8,  i = 0..3 (one MFMA each),
// for both operands.  A lane's 32 weights of a k-block are 4 (w4) or 8 (w8)
// consecutive repacked words: one or two 16-byte loads.  GS >= 32 and the
// run is 32-aligned, so it lies in exactly one quant group: one bf16 scale
// and one bf16 bias per lane, matrix and k-block, prefetched together with
// the next k-block's words.  The scale lives in the fragment, so the
// accumulators run straight through the k loop.
//
// The activations are shared by the four waves through the double-buffered
// LDS slab of wide_slab.h, one barrier per k-block.
//
// Token rows past cnt are clamped for loads and masked for stores; token
// column tiles wholly past cnt skip their MFMAs.  There are barriers
// inside the k loop, so no wave may leave early: the cnt == 0 exit is
// block-uniform and sits before the first barrier, and a wave whose 16
// rows lie past the last weight row stays in the loop on clamped (in
// bounds) rows and only skips its stores.
//
// Preconditions (checked by the bindings): K % 128 == 0, GS in
// {32, 64, 128}, bits in {4, 8}, contiguous 16-byte aligned tensors; the
// number of output rows is arbitrary.

#include "hip_common.h"
#include "splitk.h"
#include "w4f16_dequant.h"
#include "wide_slab.h"

#ifndef W4W_TM
#define W4W_TM 64  // tokens per tile (docs/PERFORMANCE.md, "w4 prefill")
#endif
#define W4W_MZ (W4W_TM / 16)
#define W4W_SLAB (16 * W4W_TM)  // 16-byte slots per buffer
#define W4W_WAVES 4
#define W4W_BLOCK (W4W_WAVES * WAVE)
static_assert(W4W_TM >= 64 && W4W_TM % 16 == 0, "tile is whole 16-token MFMAs");

// Built without the packed-fp32 VALU forms, as the MLA and route kernels are.
#if defined(__HIP_DEVICE_COMPILE__)
#define W4W_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define W4W_NO_PK_F32
#endif

// One lane's share of a weight k-block: 32 weights of one quant group.
template <int BITS, int GS>
struct W4WLane {
  uint4 lo, hi;  // hi: w8 only
  short s, b;
  __device__ __forceinline__ void load(const unsigned int* wrow,
                                       const short* srow, const short* brow,
                                       int kb, int q) {
    const int k0 = kb * WS_KB + q * 32;
    const unsigned int* p = wrow + k0 * BITS / 32;
    lo = *reinterpret_cast<const uint4*>(p);
    if (BITS == 8) hi = *reinterpret_cast<const uint4*>(p + 4);
    s = srow[k0 / GS];
    b = brow[k0 / GS];
  }
  // (s, b + off * s) as the 16-token kernels form them
  __device__ __forceinline__ void affine(f16x2& s2, f16x2& b2) const {
    constexpr float QOFF = BITS == 4 ? 8.0f : 128.0f;
    const float sf = bfbits2f(s);
    s2 = splat2(sf);
    b2 = splat2(bfbits2f(b) + QOFF * sf);
  }
  // weight fragment of MFMA i (elements i * 8 .. i * 8 + 7 of the run)
  __device__ __forceinline__ f16x8 frag(int i, f16x2 s2, f16x2 b2) const {
    f16x8 f;
    if (BITS == 4) {
      const unsigned int w = i == 0 ? lo.x : i == 1 ? lo.y : i == 2 ? lo.z : lo.w;
      dq8<4>(w, s2, b2, &f);
    } else {
      switch (i) {
        case 0: dq8_w8(lo.x, lo.y, s2, b2, &f); break;
        case 1: dq8_w8(lo.z, lo.w, s2, b2, &f); break;
        case 2: dq8_w8(hi.x, hi.y, s2, b2, &f); break;
        default: dq8_w8(hi.z, hi.w, s2, b2, &f); break;
      }
    }
    return f;
  }
};

// The k loop of one tile: NW weight matrices (gate and up, or down alone)
// against the shared slab.  acc[w][z] is the 16 x 16 tile of matrix w and
// token column tile z.  XA: the activations are the MFMA's first operand
// (the accumulator then has tokens down the registers and weight rows
// across the lanes).  Ends on a barrier, so the caller may refill buffer 0
// at once.
template <int NW, bool XA, int BITS, int GS>
__device__ __forceinline__ W4W_NO_PK_F32 void w4w_tile(
    f16x8* slab, const _Float16* (&rowp)[W4W_MZ],
    const unsigned int* (&wrow)[NW], const short* (&srow)[NW],
    const short* (&brow)[NW], int nkb, int nz,
    float4v (&acc)[NW][W4W_MZ]) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int q = lane >> 4, tok = lane & 15;
  const int sr = threadIdx.x >> 4, scn = threadIdx.x & 15;

  WideStage<W4W_TM> st;
  W4WLane<BITS, GS> wl[NW];
  st.load(rowp, 0, scn);
#pragma unroll
  for (int w = 0; w < NW; ++w) wl[w].load(wrow[w], srow[w], brow[w], 0, q);
  st.store(slab, sr, scn);
  __syncthreads();

  for (int kb = 0; kb < nkb; ++kb) {
    const f16x8* cur = slab + (kb & 1) * W4W_SLAB;
    const bool more = kb + 1 < nkb;  // block-uniform
    W4WLane<BITS, GS> wn[NW];
    if (more) {
      st.load(rowp, kb + 1, scn);
#pragma unroll
      for (int w = 0; w < NW; ++w)
        wn[w].load(wrow[w], srow[w], brow[w], kb + 1, q);
    }
    f16x2 s2[NW], b2[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) wl[w].affine(s2[w], b2[w]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f16x8 wf[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) wf[w] = wl[w].frag(i, s2[w], b2[w]);
      const int c = q * 4 + i;
      const f16x8* col = cur + c * W4W_TM;
      const int sw = ws_swz(c);
#pragma unroll
      for (int z = 0; z < W4W_MZ; ++z) {
        if (z < nz) {  // wave-uniform
          const f16x8 xf = col[(z * 16 + tok) ^ sw];
#pragma unroll
          for (int w = 0; w < NW; ++w)
            acc[w][z] =
                XA ? __builtin_amdgcn_mfma_f32_16x16x32_f16(xf, wf[w],
                                                            acc[w][z], 0, 0, 0)
                   : __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[w], xf,
                                                            acc[w][z], 0, 0, 0);
        }
      }
    }
    if (more) {
      // the other buffer was last read before the previous barrier
      st.store(slab + ((kb + 1) & 1) * W4W_SLAB, sr, scn);
#pragma unroll
      for (int w = 0; w < NW; ++w) wl[w] = wn[w];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Fused gate+up+SiLU over W4W_TM-token sub-ranges.
//   x:  [N, H] fp16;  gq/uq: [E, I, H*BITS/32] repacked u32
//   gsc/gbi/usc/ubi: [E, I, H/GS] bf16 scales/biases
//   h:  [P, I] fp16 out
// grid = (ceil(I/64), S).  Weights are the MFMA's first operand and the
// epilogue is moe_w4f16_gateup_kernel's.
// ---------------------------------------------------------------------------
template <int BITS, int GS>
__global__ __launch_bounds__(W4W_BLOCK) W4W_NO_PK_F32
void moe_w4f16_gateup_wide_kernel(
    const _Float16* __restrict__ x, const unsigned int* __restrict__ gq,
    const unsigned int* __restrict__ uq, const short* __restrict__ gsc,
    const short* __restrict__ gbi, const short* __restrict__ usc,
    const short* __restrict__ ubi, _Float16* __restrict__ h,
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    int H, int I) {
  __shared__ f16x8 slab[2 * W4W_SLAB];
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot: the whole block, before any barrier
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int q = lane >> 4, tok = lane & 15;

  const int row0 = (blockIdx.x * W4W_WAVES + wid) * 16;
  const long wr = (long)e * I + min(row0 + tok, I - 1);
  const int wpr = H * BITS / 32;  // packed words per row
  const int ngr = H / GS;
  const unsigned int* wrow[2] = {gq + wr * wpr, uq + wr * wpr};
  const short* srow[2] = {gsc + wr * ngr, usc + wr * ngr};
  const short* brow[2] = {gbi + wr * ngr, ubi + wr * ngr};
  const int nkb = H / WS_KB;
  const int sr = threadIdx.x >> 4;

  for (int c0 = 0; c0 < cnt; c0 += W4W_TM) {
    const int cc = min(W4W_TM, cnt - c0);
    const int nz = (cc + 15) >> 4;
    const _Float16* rowp[W4W_MZ];
#pragma unroll
    for (int j = 0; j < W4W_MZ; ++j)
      rowp[j] = x + (long)sorted_tok[p0 + c0 + min(j * 16 + sr, cc - 1)] * H;

    float4v acc[2][W4W_MZ];
#pragma unroll
    for (int z = 0; z < W4W_MZ; ++z)
      acc[0][z] = acc[1][z] = float4v{0, 0, 0, 0};
    w4w_tile<2, false, BITS, GS>(slab, rowp, wrow, srow, brow, nkb, nz, acc);

    // the 16-token kernel's epilogue, expression for expression
#pragma unroll
    for (int z = 0; z < W4W_MZ; ++z) {
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
  }  // W4W_TM-token tiles
}

// ---------------------------------------------------------------------------
// Down-proj + weighted atomic scatter (fp32 out).
//   hh: [P, I] fp16 (gate-up output);  dq: [E, H, I*BITS/32] repacked;
//   dsc/dbi: [E, H, I/GS] bf16;  out: [N, H] fp32, zeroed by the launcher
// grid = (ceil(H/64), S).  The activations are the MFMA's first operand,
// so a lane ends with one output column of 4 tokens and an atomic
// wave-instruction covers 4 token rows x 16 consecutive floats (64-byte
// segments) instead of 16 rows x 4 scattered dwords.
// ---------------------------------------------------------------------------
template <int BITS, int GS>
__global__ __launch_bounds__(W4W_BLOCK) W4W_NO_PK_F32
void moe_w4f16_down_wide_kernel(
    const _Float16* __restrict__ hh, const unsigned int* __restrict__ dq,
    const short* __restrict__ dsc, const short* __restrict__ dbi,
    float* __restrict__ out, const int* __restrict__ sub_expert,
    const int* __restrict__ sub_off, const int* __restrict__ sub_cnt,
    const int* __restrict__ sorted_tok, const float* __restrict__ sorted_wt,
    int I, int H) {
  __shared__ f16x8 slab[2 * W4W_SLAB];
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot: the whole block, before any barrier
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int q = lane >> 4, col = lane & 15;

  const int row0 = (blockIdx.x * W4W_WAVES + wid) * 16;
  const long wr = (long)e * H + min(row0 + col, H - 1);
  const int ngr = I / GS;
  const unsigned int* wrow[1] = {dq + wr * (I * BITS / 32)};
  const short* srow[1] = {dsc + wr * ngr};
  const short* brow[1] = {dbi + wr * ngr};
  const int nkb = I / WS_KB;
  const int sr = threadIdx.x >> 4;

  for (int c0 = 0; c0 < cnt; c0 += W4W_TM) {
    const int cc = min(W4W_TM, cnt - c0);
    const int nz = (cc + 15) >> 4;
    const _Float16* rowp[W4W_MZ];
#pragma unroll
    for (int j = 0; j < W4W_MZ; ++j)
      rowp[j] = hh + (long)(p0 + c0 + min(j * 16 + sr, cc - 1)) * I;

    float4v acc[1][W4W_MZ];
#pragma unroll
    for (int z = 0; z < W4W_MZ; ++z) acc[0][z] = float4v{0, 0, 0, 0};
    w4w_tile<1, true, BITS, GS>(slab, rowp, wrow, srow, brow, nkb, nz, acc);

    const int o = row0 + col;
    if (o < H) {
#pragma unroll
      for (int z = 0; z < W4W_MZ; ++z) {
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
  }  // W4W_TM-token tiles
}

extern "C" int moe_w4f16_wide_tile() { return W4W_TM; }

template <int BITS, int GS>
static void gateup_wide(const void* x, const void* gq, const void* uq,
                        const void* gsc, const void* gbi, const void* usc,
                        const void* ubi, void* h, const int* se, const int* so,
                        const int* sc, const int* st, int S, int H, int I,
                        hipStream_t stream) {
  const int gx = (I + W4W_WAVES * 16 - 1) / (W4W_WAVES * 16);
  moe_w4f16_gateup_wide_kernel<BITS, GS>
      <<<dim3(gx, S), dim3(W4W_BLOCK), 0, stream>>>(
          (const _Float16*)x, (const unsigned int*)gq,
          (const unsigned int*)uq, (const short*)gsc, (const short*)gbi,
          (const short*)usc, (const short*)ubi, (_Float16*)h, se, so, sc, st,
          H, I);
}

template <int BITS, int GS>
static void down_wide(const void* hh, const void* dq, const void* dsc,
                      const void* dbi, float* out, const int* se,
                      const int* so, const int* sc, const int* st,
                      const float* sw, int S, int I, int H,
                      hipStream_t stream) {
  const int gx = (H + W4W_WAVES * 16 - 1) / (W4W_WAVES * 16);
  moe_w4f16_down_wide_kernel<BITS, GS>
      <<<dim3(gx, S), dim3(W4W_BLOCK), 0, stream>>>(
          (const _Float16*)hh, (const unsigned int*)dq, (const short*)dsc,
          (const short*)dbi, out, se, so, sc, st, sw, I, H);
}

// bits in {4, 8} and gs in {32, 64, 128}: the bindings check
#define W4W_DISPATCH(FN, ...)                        \
  do {                                               \
    if (bits == 4) {                                 \
      if (gs == 32) FN<4, 32>(__VA_ARGS__);          \
      else if (gs == 64) FN<4, 64>(__VA_ARGS__);     \
      else FN<4, 128>(__VA_ARGS__);                  \
    } else {                                         \
      if (gs == 32) FN<8, 32>(__VA_ARGS__);          \
      else if (gs == 64) FN<8, 64>(__VA_ARGS__);     \
      else FN<8, 128>(__VA_ARGS__);                  \
    }                                                \
  } while (0)

extern "C" void launch_moe_w4f16_gateup_wide(
    const void* x, const void* gq, const void* uq, const void* gsc,
    const void* gbi, const void* usc, const void* ubi, void* h,
    const int* sub_expert, const int* sub_off, const int* sub_cnt,
    const int* sorted_tok, int S, int H, int I, int gs, int bits,
    hipStream_t stream) {
  W4W_DISPATCH(gateup_wide, x, gq, uq, gsc, gbi, usc, ubi, h, sub_expert,
               sub_off, sub_cnt, sorted_tok, S, H, I, stream);
}

// out: fp32 [N, H], uninitialised: zeroed here by a kernel (splitk.h), so
// the clear is part of any captured graph
extern "C" void launch_moe_w4f16_down_wide(
    const void* hh, const void* dq, const void* dsc, const void* dbi,
    float* out, long out_n, const int* sub_expert, const int* sub_off,
    const int* sub_cnt, const int* sorted_tok, const float* sorted_wt, int S,
    int I, int H, int gs, int bits, hipStream_t stream) {
  launch_f32_zero(out, out_n, stream);
  W4W_DISPATCH(down_wide, hh, dq, dsc, dbi, out, sub_expert, sub_off, sub_cnt,
               sorted_tok, sorted_wt, S, I, H, stream);
}
