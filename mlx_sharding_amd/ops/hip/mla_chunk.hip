// MFMA absorbed-MLA attention for a short chunk of T new tokens over the
// compressed cache: causal MQA (Hkv == 1) over rows [c_kv | k_pe]
// (Dk = rank + rope) whose first Dv = rank columns are V.
//
// Rows.  Queries are flattened to virtual rows r = t*Hq + h (R = T*Hq per
// batch row).  Hq % 16 == 0, so the 16 consecutive rows a wave owns are 16
// heads of ONE token t and the causal limit lim(t) = S - T + t + 1 (keys
// [0, lim)) is a wave-uniform scalar, not a per-lane mask.  That is what
// lets one kernel serve 16 heads as well as 32 / 64 / 128.
//
// Work split: a block is one batch row x one split-S key slice x 64
// consecutive virtual rows (NW = 4 waves; 4 tokens at 16 heads, half a
// token's heads at 128).  Grid (B, nsplit, ceil(R / 64)).  Each wave keeps
// its own running (m, l) and 16 x Dv fp32 accumulators, so the softmax has
// no cross-wave traffic.  When R is not a multiple of 64 the last block's
// surplus waves own no rows: they stage and hit every barrier, and skip
// the MFMAs and the stores.
//
// Data movement is mla_decode.hip's (see its header for the fragment maps
// and the bank arithmetic): a 16-key tile staged once per block as the
// row-major K image (stride DKP+8) and the register-transposed V^T image
// (stride 24), the next tile prefetched into registers after the barrier
// that publishes the current one, two barriers per tile;
// S^T = K . Q^T on mfma_f32_16x16x32_bf16 so a lane holds 4 consecutive
// keys of one row and P feeds mfma_f32_16x16x16_bf16 from the C registers.
// The tile body is interleaved with the per-wave causal tests here, so the
// file carries its own copy of it and mla_decode.hip is left as it is.
//
// Causality.  The block walks tiles up to the largest lim among its waves
// (the last wave that owns rows), clipped to the slice: hi_blk.  Keys at
// or past hi_blk are never loaded; both images hold zeros for them.  A
// wave's own end is hi_w = min(slice end, lim): it skips the MFMAs and the
// softmax of tiles starting at or past hi_w (so it never runs the softmax
// on a tile without a live key; tile start t0 < hi_w is itself live), and
// inside its boundary tile keys >= hi_w score -1e30 and get p = 0 exactly.
// Their staged rows are real cache rows below S, hence finite, and
// 0 x finite adds nothing.  No wave leaves the tile loop early: the
// barriers are block-wide.
//
// Split-S: S is a host value; slices are whole tiles of at least 256
// keys.  A wave whose lim <= the slice start writes the empty partial
// (m = -1e30, l = 0, o = 0).  Partials [B*R, nsplit, Dv] / [.., 2] feed
// attn_decode_combine_kernel with R virtual heads.

#include "hip_common.h"

#define MC_KT 16     // keys per tile
#define MC_VTS 24    // V^T row stride (elements)
#define MC_ROWS 64   // virtual rows per block (4 waves x 16)
#define MC_MIN_SLICE 256

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

// Built without the packed-fp32 VALU forms, as mla_decode_kernel is: the
// accumulator rescale must not be fused into them.
#if defined(__HIP_DEVICE_COMPILE__)
#define MC_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define MC_NO_PK_F32
#endif

template <int DK, int DV, int NW>
__global__ __launch_bounds__(NW * WAVE) MC_NO_PK_F32 void mla_chunk_kernel(
    const short* __restrict__ q_nope,  // [B, T, Hq, DV] via (q_bs, q_ts, q_hs)
    const short* __restrict__ q_rope,  // [B, T, Hq, DK-DV] via (qr_*)
    const short* __restrict__ kv,      // [B, Scap, DK]
    short* __restrict__ out,           // [B, T*Hq, DV]          (nsplit == 1)
    float* __restrict__ part_o,        // [B*T*Hq, NS, DV]       (nsplit > 1)
    float* __restrict__ part_ml,       // [B*T*Hq, NS, 2]
    int T, int Hq, int S, long Scap, float scale, long q_bs, long q_ts,
    long q_hs, long qr_bs, long qr_ts, long qr_hs) {
  constexpr int NT = NW * WAVE;
  constexpr int DKP = (DK + 31) / 32 * 32;
  constexpr int NKS = DKP / 32;
  constexpr int NDH = DV / 16;
  constexpr int KSTR = DKP + 8;
  constexpr int CPR = DKP / 8;          // 16-byte chunks per staged row
  constexpr int NITEMS = CPR * 4;       // (chunk, key quad) items per tile
  constexpr int NIT = (NITEMS + NT - 1) / NT;
  static_assert(NW * 16 == MC_ROWS, "a block is 64 virtual rows");
  static_assert(DK % 8 == 0 && DV % 16 == 0 && DV <= DK, "row geometry");

  const int b = blockIdx.x;
  const int split = blockIdx.y;
  const int nsplit = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int ln = lane & 15;
  const int lg = lane >> 4;
  const int R = T * Hq;                          // virtual rows, R % 16 == 0
  const int r0 = (blockIdx.z * NW + wid) * 16;   // this wave's first row
  const bool owns = r0 < R;
  const int tok = owns ? r0 / Hq : 0;
  const int h0 = r0 - tok * Hq;                  // first of its 16 heads
  // the last wave of the block that owns rows sees the most keys
  const int r_last = min(R, ((int)blockIdx.z + 1) * MC_ROWS) - 16;

  int lo = 0, hi = S;
  if (nsplit > 1) {
    const long per = max((long)MC_MIN_SLICE,
                         (((long)S + nsplit - 1) / nsplit + MC_KT - 1)
                             / MC_KT * MC_KT);
    lo = (int)min((long)S, per * split);
    hi = (int)min((long)S, per * (split + 1));
  }
  const int hi_blk = min(hi, S - T + r_last / Hq + 1);
  const int hi_w = owns ? min(hi, S - T + tok + 1) : lo;

  __shared__ __attribute__((aligned(16))) short k_lds[MC_KT * KSTR];
  __shared__ __attribute__((aligned(16))) short vt_lds[DV * MC_VTS];

  // ---- Q^T fragments (B operand): row r0 + ln, dims ks*32 + lg*8 .. ----
  bf16x8_t qf[NKS];
  {
    const long h = h0 + ln;
    const short* qn = q_nope + b * q_bs + tok * q_ts + h * q_hs;
    const short* qr = q_rope + b * qr_bs + tok * qr_ts + h * qr_hs;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int d = ks * 32 + lg * 8;
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (owns) {
        if (d < DV) v = *reinterpret_cast<const bf16x8_t*>(qn + d);
        else if (d < DK) v = *reinterpret_cast<const bf16x8_t*>(qr + d - DV);
      }
      qf[ks] = v;
    }
  }

  float m_run = -1e30f, l_run = 0.0f;   // row r0 + ln (replicated over lg)
  float4v oacc[NDH];
#pragma unroll
  for (int dh = 0; dh < NDH; ++dh) oacc[dh] = float4v{0, 0, 0, 0};

  const short* kvb = kv + (long)b * Scap * DK;
  short8v stg[NIT][4];
  // item = tid + it*NT -> chunk c = item >> 2, key quad kg = item & 3.
  // (A macro, not a lambda: the body must inline into the kernel so stg
  // stays in registers.)
#define MC_PREFETCH(T0)                                                      \
  _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                       \
    const int item = tid + it * NT;                                          \
    const int c = item >> 2, kg = item & 3;                                  \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                          \
      const int key = (T0) + kg * 4 + i;                                     \
      short8v v = {0, 0, 0, 0, 0, 0, 0, 0};                                  \
      if (item < NITEMS && c * 8 < DK && key < hi_blk)                       \
        v = *reinterpret_cast<const short8v*>(kvb + (long)key * DK + c * 8); \
      stg[it][i] = v;                                                        \
    }                                                                        \
  }

  if (lo < hi_blk) MC_PREFETCH(lo)
  for (int t0 = lo; t0 < hi_blk; t0 += MC_KT) {
    __syncthreads();  // every wave is done reading the previous tile
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int item = tid + it * NT;
      const int c = item >> 2, kg = item & 3;
      if (item < NITEMS) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<short8v*>(k_lds + (kg * 4 + i) * KSTR + c * 8) =
              stg[it][i];
        if (c * 8 < DV) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            *reinterpret_cast<short4v*>(vt_lds + (c * 8 + j) * MC_VTS +
                                        kg * 4) =
                short4v{stg[it][0][j], stg[it][1][j], stg[it][2][j],
                        stg[it][3][j]};
        }
      }
    }
    __syncthreads();  // tile published
    if (t0 + MC_KT < hi_blk) MC_PREFETCH(t0 + MC_KT)
    if (t0 >= hi_w) continue;  // wave-uniform: nothing here for this token

    // ---- S^T = K . Q^T: lane gets row ln, keys lg*4 + reg ----
    float4v c = {0, 0, 0, 0};
    {
      const short* kr = k_lds + ln * KSTR + lg * 8;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(kr + ks * 32);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], c, 0, 0, 0);
      }
    }
    // ---- online softmax for row ln over the tile's 16 keys ----
    float sc[4];
    float mx = -1e30f;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const bool live = t0 + lg * 4 + reg < hi_w;
      sc[reg] = live ? c[reg] * scale : -1e30f;
      mx = fmaxf(mx, sc[reg]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mnew = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - mnew);
    m_run = mnew;
    float ps = 0.0f;
    bf16x4_t pf;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      // dead keys must be exactly 0 (key t0 is live, so mnew is a real
      // score and a dead key's -1e30 never equals it)
      const float p = (sc[reg] <= -1e29f) ? 0.0f : __expf(sc[reg] - mnew);
      ps += p;
      pf[reg] = (__bf16)p;
    }
    ps += __shfl_xor(ps, 16, WAVE);
    ps += __shfl_xor(ps, 32, WAVE);
    l_run = l_run * alpha + ps;
    // O rows are rows lg*4 + reg: fetch their rescale factors
    float ar[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) ar[reg] = __shfl(alpha, lg * 4 + reg, WAVE);
    // ---- O = O*alpha + P . V ----
    const short* vr = vt_lds + ln * MC_VTS + lg * 4;
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) {
      bf16x4_t vf =
          *reinterpret_cast<const bf16x4_t*>(vr + dh * 16 * MC_VTS);
      float4v prev = oacc[dh];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) prev[reg] *= ar[reg];
      oacc[dh] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pf, vf, prev, 0, 0, 0);
    }
  }

#undef MC_PREFETCH

  // ---- epilogue: lane holds O[row r0 + lg*4 + reg][dh*16 + ln] ----
  if (!owns) return;
  const long vrow = (long)b * R + r0;  // [B, T, Hq] flattened
  if (nsplit == 1) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float rinv = 1.0f / __shfl(l_run, lg * 4 + reg, WAVE);
      short* orow = out + (vrow + lg * 4 + reg) * DV + ln;
#pragma unroll
      for (int dh = 0; dh < NDH; ++dh)
        reinterpret_cast<bf16*>(orow)[dh * 16] = f2bf(oacc[dh][reg] * rinv);
    }
    return;
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    float* prow = part_o + ((vrow + lg * 4 + reg) * nsplit + split) * DV + ln;
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) prow[dh * 16] = oacc[dh][reg];
  }
  if (lg == 0) {
    const long base = ((vrow + ln) * nsplit + split) * 2;
    part_ml[base + 0] = m_run;
    part_ml[base + 1] = l_run;
  }
}

extern "C" void launch_attn_decode_combine(const float* part_o,
                                           const float* part_ml, void* out,
                                           int nsplit, int B, int Hq, int Dv,
                                           long o_bs, long o_hs,
                                           hipStream_t stream);

extern "C" bool mla_chunk_supported_shape(int Hq, int Dk, int Dv) {
  if (Hq != 16 && Hq != 32 && Hq != 64 && Hq != 128) return false;
  return (Dk == 576 && Dv == 512) || (Dk == 80 && Dv == 64);
}

// Split-S factor, mla_decode_nsplit's rule with the row blocks in place of
// the head groups: one block per CU (B * ceil(rows / 64) * nsplit against
// 256 CUs), slices of at least 256 keys, at most 16 slices.
extern "C" int mla_chunk_nsplit(int B, long rows, long span) {
  const long blocks =
      std::max<long>(1, (long)B * ((rows + MC_ROWS - 1) / MC_ROWS));
  const long want = (256 + blocks - 1) / blocks;
  const long fit = std::max<long>(1, (span + MC_MIN_SLICE - 1) / MC_MIN_SLICE);
  return (int)std::min<long>(16, std::min(want, fit));
}

// out is [B, T, Hq, Dv] contiguous; part_o / part_ml are used when
// nsplit > 1.  The caller checked mla_chunk_supported_shape and T <= S.
extern "C" void launch_mla_chunk(const void* q_nope, const void* q_rope,
                                 const void* kv, void* out, float* part_o,
                                 float* part_ml, int nsplit, int B, int T,
                                 int Hq, int S, long Scap, int Dk, int Dv,
                                 float scale, long q_bs, long q_ts, long q_hs,
                                 long qr_bs, long qr_ts, long qr_hs,
                                 hipStream_t stream) {
  const int R = T * Hq;
  dim3 grid((unsigned)B, (unsigned)nsplit,
            (unsigned)((R + MC_ROWS - 1) / MC_ROWS));
#define MC_CASE(DKK, DVV)                                                   \
  mla_chunk_kernel<DKK, DVV, 4><<<grid, dim3(4 * WAVE), 0, stream>>>(       \
      (const short*)q_nope, (const short*)q_rope, (const short*)kv,         \
      (short*)out, part_o, part_ml, T, Hq, S, Scap, scale, q_bs, q_ts,      \
      q_hs, qr_bs, qr_ts, qr_hs)
  if (Dk == 576) MC_CASE(576, 512);
  else MC_CASE(80, 64);
#undef MC_CASE
  if (nsplit > 1)
    launch_attn_decode_combine(part_o, part_ml, out, nsplit, B, R, Dv,
                               (long)R * Dv, (long)Dv, stream);
}
