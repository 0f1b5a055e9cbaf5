// MFMA flash-decode (T = 1) for grouped-query attention: llama, qwen2 and
// gemma2 shapes, G = Hq/Hkv query heads (1..16, a runtime value) per KV
// head over a per-head K cache [B, Hkv, Scap, DK] and a separate V cache
// [B, Hkv, Scap, DV], (DK, DV) in {(64, 64), (128, 128), (256, 256)}.
// Softcap, sliding window and attn_decode_kernel's position contract
// (host length, or device position int32 [1] / [B], S_b = pos[b] + 1).
//
// Work split: a block serves one (batch row, kv head, split-S slice) and
// its 4 waves split the KEYS of the slice: wave w walks the 32-key tiles
// w, w+4, .. counted from the slice's first key.  Every wave keeps a private
// running (m, l) and a private 16 x DV fp32 accumulator whose 16 MFMA
// columns are the G heads, zero-padded above G.  Every K and V byte is
// consumed by exactly one wave, so nothing is staged for the block and the
// tile loop has no __syncthreads; the waves meet once, in the merge.
//
// Fragment maps (mla_decode.hip's):
//   mfma_f32_16x16x32_bf16: A(16x32) lane: row=l&15, k=(l>>4)*8+j
//                           B(32x16) lane: col=l&15, k=(l>>4)*8+j
//   C/D:                    lane: col=l&15, row=(l>>4)*4+reg
// with ln = l&15, lg = l>>4 below.
//
// QK^T is computed TRANSPOSED, S^T = K . Q^T, once per 16-key half-tile:
//   A = K rows   lane: key = half*16 + ln, dims ks*32 + lg*8 .. — one
//                16-byte load per k-step STRAIGHT FROM GLOBAL; a quarter
//                wave reads 64 contiguous bytes of each of 16 rows and two
//                k-steps complete a row's 128-byte line
//   B = Q^T      lane: head = ln, same dims — DK/32 register fragments
//                loaded once per block through q's (batch, head) strides,
//                zero for ln >= G
//   C = S^T      lane: head = ln, keys half*16 + lg*4 + reg
// so a lane holds 8 scores of ONE head per 32-key tile; the per-head max
// and sum are in-lane plus xor-16 / xor-32 shuffles.  Softcap is
// cap * tanh(s / cap) before the max.
//
// PV, O = P . V on the same 32-deep instruction.  The contraction order
// over keys is free, so k-slot lg*8 + j is DEFINED as
//   key lg*4 + j          of half-tile 0 for j <  4
//   key 16 + lg*4 + j - 4 of half-tile 1 for j >= 4
// and the two C tiles of a lane ARE its bf16 A fragment: no LDS round trip
// for P.
//   A = P        lane: head = ln, k-slots lg*8 + j          (registers)
//   B = V        lane: col = dh*16 + ln, k-slots lg*8 + j — one b128 LDS
//                read from the wave's transposed V image
//   C = O tile   lane: col = dh*16 + ln, head = lg*4 + reg
// (m, l) live in the lane whose ln is the head while O rows are heads
// lg*4 + reg, so the rescale factors are fetched with 4 lane shuffles.
//
// V staging.  Each wave loads its own 32 x DV V tile with 16-byte loads:
// item (8-column chunk c, key quad kq) = four loads, keys kq*4 .. +3; lane
// l owns kq = l&7 and chunks (l>>3) + 8*it, so one load instruction reads
// whole 128-byte lines of 8 rows.  The transpose happens in registers: the
// item becomes eight b64 writes (4 keys of one column) into the
// wave-private image [VC][GD_VS] bf16 at k-slot (kq&3)*8 + (kq>>2)*4,
// i.e. in the permuted key order above.  VC = min(DV, 128) columns are
// staged at a time (DV = 256 takes two passes over the same registers:
// four whole images would be 80 KB).  The image is private to the wave, LDS
// operations of one wave execute in order, and the compiler waits on the
// LDS counter before the MFMA consumes a read: no barrier.
//
// Bank conflicts, row stride GD_VS = 40 elements = 20 dwords = 4 * 5:
//   reads   a quarter wave (lg fixed, ln = 0..15) reads one b128 per lane at
//           dword 20*ln + 4*lg: 20*ln mod 64 takes 16 distinct multiples of
//           4 — conflict-free.
//   writes  a half wave holds 8 key quads x 4 chunks; a b64 write lands on
//           dword 160*c + 20*j + 4*(kq&3) + 2*(kq>>2).  The 8 key quads
//           cover 16 distinct dwords, but 160*c = 32*c mod 64 separates the
//           chunks only by parity: 2-way conflicts.  No stride that keeps
//           the b128 reads 16-byte aligned (a multiple of 4 dwords) avoids
//           that; at 2 x 8 KB of LDS writes per 16 KB of HBM traffic the
//           write phase is a few percent of a tile's memory time.
//
// Prefetch: the next tile's K fragments and V items are loaded into the
// same registers right after the QK MFMAs (K) and the V staging writes
// have consumed the current ones, ahead of the softmax and the PV MFMAs.
//
// Masking: keys at or past the slice end are never loaded — their K and V
// registers are zeros (0 x NaN inside an MFMA is NaN, so weight 0 alone is
// not enough), their scores are -1e30 and their p is exactly 0.  Tiles
// start at the window start, so no key before it is touched either.
//
// Merge: after the loop the waves publish (m, l) and, VC columns at a
// time, their accumulators to LDS (over the V images, after one barrier);
// every wave then combines a quarter of those columns in the fixed order
// w = 0..3 with exp(m_w - m*), where a wave without keys carries
// (-1e30, 0) and weighs nothing, and stores heads < G only.  No float
// atomics: results are bit-reproducible.
//
// Split-S: gridDim.y slices with attn_decode_kernel's bounds (fractions of
// the capacity under a device position, rounded up to 256 keys) and its
// partial layout; a slice past the row's S writes (m = -1e30, l = 0) and
// attn_decode_combine_kernel finishes nsplit > 1.

#include "hip_common.h"

#define GD_NW 4      // waves per block
#define GD_KT 32     // keys per wave tile
#define GD_VS 40     // V image row stride (elements)
#define GD_SLICE 256 // split-S granularity (attn_decode_kernel's tile)

template <int DK, int DV>
__global__ __launch_bounds__(GD_NW * WAVE) MD_NO_PK_F32 void gqa_decode_kernel(
    const short* __restrict__ q,       // [B, Hq, DK] via (q_bs, q_hs)
    const short* __restrict__ kcache,  // [B, Hkv, Scap, DK]
    const short* __restrict__ vcache,  // [B, Hkv, Scap, DV]
    short* __restrict__ out,           // [B, Hq, DV]            (nsplit == 1)
    float* __restrict__ part_o,        // [B*Hq, NS, DV]         (nsplit > 1)
    float* __restrict__ part_ml,       // [B*Hq, NS, 2]
    const int* __restrict__ s_ptr, int s_bstride, int Hkv, int G, int S,
    long Scap, float scale, float softcap, int window, long q_bs, long q_hs) {
  constexpr int NKS = DK / 32;            // QK k-steps
  constexpr int NDH = DV / 16;            // output column tiles
  constexpr int VC = DV < 128 ? DV : 128; // columns staged per pass
  constexpr int NPASS = DV / VC;
  constexpr int NDP = VC / 16;            // column tiles per pass
  constexpr int NIT = DV / 64;            // V items per lane
  constexpr int NIP = NIT / NPASS;        // .. per pass
  constexpr int CW = VC / GD_NW;          // merge columns per wave and pass
  static_assert(DK % 32 == 0 && DV % 64 == 0 && DV % VC == 0, "row geometry");
  // the merge buffer [4][16][VC] fp32 reuses the V images [4][VC][GD_VS] bf16
  static_assert(16 * 4 <= GD_VS * 2, "merge buffer fits the V images");

  const int b = blockIdx.x / Hkv;
  const int hk = blockIdx.x % Hkv;
  const int split = blockIdx.y;
  const int nsplit = gridDim.y;
  const int Hq = Hkv * G;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int ln = lane & 15;
  const int lg = lane >> 4;
  if (s_ptr) S = s_ptr[b * s_bstride] + 1;
  S = (int)min((long)S, Scap);  // loads stay inside the capacity buffer

  __shared__ __attribute__((aligned(16))) short vt_all[GD_NW * VC * GD_VS];
  __shared__ float ml_lds[GD_NW * 2 * 16];  // [wave][m | l][head]
  short* vt_lds = vt_all + wid * VC * GD_VS;

  // ---- Q^T fragments (B operand): head ln, dims ks*32 + lg*8 .. ----
  bf16x8_t qf[NKS];
  {
    const short* qh = q + b * q_bs + ((long)hk * G + ln) * q_hs + lg * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ln < G) v = *reinterpret_cast<const bf16x8_t*>(qh + ks * 32);
      qf[ks] = v;
    }
  }

  int lo = (window > 0 && S > window) ? (S - window) : 0;
  int hi = S;
  if (nsplit > 1) {
    const long spanc = s_ptr ? Scap : (long)S;
    const long per = ((spanc + nsplit - 1) / nsplit + GD_SLICE - 1)
                     / GD_SLICE * GD_SLICE;
    lo = (int)max((long)lo, per * split);
    hi = (int)min((long)S, per * (split + 1));
  }

  float m_run = -1e30f, l_run = 0.0f;   // head ln (replicated over lg)
  float4v oacc[NDH];
#pragma unroll
  for (int dh = 0; dh < NDH; ++dh) oacc[dh] = float4v{0, 0, 0, 0};

  const long rbase = ((long)b * Hkv + hk) * Scap;
  const short* kb = kcache + rbase * DK + lg * 8;
  const short* vb = vcache + rbase * DV + (lane >> 3) * 8;
  const int kq = lane & 7;
  bf16x8_t kf[2][NKS];
  short8v vs[NIT][4];

// K fragments and V items of the tile at T0; rows at or past hi are zeros
#define GD_LOAD_K(T0)                                                        \
  _Pragma("unroll") for (int hf = 0; hf < 2; ++hf) {                         \
    const int key = (T0) + hf * 16 + ln;                                     \
    _Pragma("unroll") for (int ks = 0; ks < NKS; ++ks) {                     \
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};                                 \
      if (key < hi)                                                          \
        v = *reinterpret_cast<const bf16x8_t*>(kb + (long)key * DK +         \
                                               ks * 32);                     \
      kf[hf][ks] = v;                                                        \
    }                                                                        \
  }
#define GD_LOAD_V(T0)                                                        \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                            \
    const int key = (T0) + kq * 4 + i;                                       \
    _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                     \
      short8v v = {0, 0, 0, 0, 0, 0, 0, 0};                                  \
      if (key < hi)                                                          \
        v = *reinterpret_cast<const short8v*>(vb + (long)key * DV +          \
                                              it * 64);                      \
      vs[it][i] = v;                                                         \
    }                                                                        \
  }
// items of pass P -> eight b64 columns each, at this key quad's k-slots
#define GD_STAGE_V(P)                                                        \
  _Pragma("unroll") for (int ii = 0; ii < NIP; ++ii) {                       \
    const int it = (P) * NIP + ii;                                           \
    short* col = vt_lds + (ii * 64 + (lane >> 3) * 8) * GD_VS +              \
                 (kq & 3) * 8 + (kq >> 2) * 4;                               \
    _Pragma("unroll") for (int j = 0; j < 8; ++j)                            \
      *reinterpret_cast<short4v*>(col + j * GD_VS) =                         \
          short4v{vs[it][0][j], vs[it][1][j], vs[it][2][j], vs[it][3][j]};   \
  }

  const int t_first = lo + wid * GD_KT;
  if (t_first < hi) {
    GD_LOAD_K(t_first)
    GD_LOAD_V(t_first)
  }
  for (int t0 = t_first; t0 < hi; t0 += GD_NW * GD_KT) {
    const int tn = t0 + GD_NW * GD_KT;
    // ---- S^T = K . Q^T per half-tile: head ln, keys hf*16 + lg*4 + reg ----
    float4v c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0][ks], qf[ks], c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[1][ks], qf[ks], c1, 0, 0, 0);
    }
    if (tn < hi) GD_LOAD_K(tn)
    GD_STAGE_V(0)
    __builtin_amdgcn_wave_barrier();
    if (NPASS == 1 && tn < hi) GD_LOAD_V(tn)

    // ---- online softmax of head ln over the tile's 32 keys ----
    float sc[8];
    float mx = -1e30f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int key = t0 + (j >> 2) * 16 + lg * 4 + (j & 3);
      float s = (j < 4 ? c0[j & 3] : c1[j & 3]) * scale;
      if (softcap > 0.0f) s = softcap * tanhf(s / softcap);
      sc[j] = key < hi ? s : -1e30f;
      mx = fmaxf(mx, sc[j]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mnew = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - mnew);
    m_run = mnew;
    float ps = 0.0f;
    bf16x8_t pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // dead keys are exactly 0 (a tile always has a live key, so mnew is
      // a real score)
      const float p = (sc[j] <= -1e29f) ? 0.0f : __expf(sc[j] - mnew);
      ps += p;
      pf[j] = (__bf16)p;
    }
    ps += __shfl_xor(ps, 16, WAVE);
    ps += __shfl_xor(ps, 32, WAVE);
    l_run = l_run * alpha + ps;
    // O rows are heads lg*4 + reg: fetch their rescale factors
    float ar[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) ar[reg] = __shfl(alpha, lg * 4 + reg, WAVE);

    // ---- O = O*alpha + P . V, VC columns per staged pass ----
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      if (p > 0) {
        GD_STAGE_V(p)
        __builtin_amdgcn_wave_barrier();
        if (p == NPASS - 1 && tn < hi) GD_LOAD_V(tn)
      }
      const short* vr = vt_lds + ln * GD_VS + lg * 8;
#pragma unroll
      for (int d = 0; d < NDP; ++d) {
        bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(vr + d * 16 * GD_VS);
        float4v prev = oacc[p * NDP + d];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) prev[reg] *= ar[reg];
        oacc[p * NDP + d] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, prev, 0, 0, 0);
      }
    }
  }
#undef GD_LOAD_K
#undef GD_LOAD_V
#undef GD_STAGE_V

  // ---- merge the 4 waves: lane holds O[head lg*4 + reg][dh*16 + ln] ----
  float* acc_lds = reinterpret_cast<float*>(vt_all);  // [wave][16][VC]
  if (lg == 0) {
    ml_lds[wid * 32 + ln] = m_run;
    ml_lds[wid * 32 + 16 + ln] = l_run;
  }
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    __syncthreads();  // V images (or the previous pass) are done with
#pragma unroll
    for (int d = 0; d < NDP; ++d)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        acc_lds[(wid * 16 + lg * 4 + reg) * VC + d * 16 + ln] =
            oacc[p * NDP + d][reg];
    __syncthreads();  // partials (and, at p == 0, m / l) published
    // wave wid combines columns [wid*CW, (wid+1)*CW) of this pass
    for (int idx = lane; idx < G * CW; idx += WAVE) {
      const int head = idx / CW;
      const int cl = wid * CW + idx % CW;
      float mstar = -1e30f;
#pragma unroll
      for (int w = 0; w < GD_NW; ++w) mstar = fmaxf(mstar, ml_lds[w * 32 + head]);
      float o = 0.0f, lsum = 0.0f;
#pragma unroll
      for (int w = 0; w < GD_NW; ++w) {
        const float f = __expf(ml_lds[w * 32 + head] - mstar);
        lsum += ml_lds[w * 32 + 16 + head] * f;
        o += acc_lds[(w * 16 + head) * VC + cl] * f;
      }
      const long h = (long)hk * G + head;
      const int col = p * VC + cl;
      if (nsplit == 1) {
        reinterpret_cast<bf16*>(out)[((long)b * Hq + h) * DV + col] =
            f2bf(o * (1.0f / lsum));
      } else {
        const long row = ((long)b * Hq + h) * nsplit + split;
        part_o[row * DV + col] = o;
        if (p == 0 && idx % CW == 0 && wid == 0) {
          part_ml[row * 2 + 0] = mstar;
          part_ml[row * 2 + 1] = lsum;
        }
      }
    }
  }
}

extern "C" void launch_attn_decode_combine(const float* part_o,
                                           const float* part_ml, void* out,
                                           int nsplit, int B, int Hq, int Dv,
                                           long o_bs, long o_hs,
                                           hipStream_t stream);

extern "C" bool gqa_decode_supported_shape(int G, int Dk, int Dv) {
  if (G < 1 || G > 16) return false;
  return Dk == Dv && (Dk == 64 || Dk == 128 || Dk == 256);
}

// out is [B, Hq, Dv], contiguous; part_o / part_ml are used when
// nsplit > 1.  The caller checked gqa_decode_supported_shape.
extern "C" void launch_gqa_decode(const void* q, const void* k, const void* v,
                                  void* out, float* part_o, float* part_ml,
                                  int nsplit, const int* s_ptr, int s_bstride,
                                  int B, int Hq, int Hkv, int S, long Scap,
                                  int Dk, float scale, float softcap,
                                  int window, long q_bs, long q_hs,
                                  hipStream_t stream) {
  dim3 grid((unsigned)(B * Hkv), (unsigned)nsplit, 1);
#define GD_CASE(D)                                                           \
  gqa_decode_kernel<D, D><<<grid, dim3(GD_NW * WAVE), 0, stream>>>(          \
      (const short*)q, (const short*)k, (const short*)v, (short*)out,        \
      part_o, part_ml, s_ptr, s_bstride, Hkv, Hq / Hkv, S, Scap, scale,      \
      softcap, window, q_bs, q_hs)
  if (Dk == 64) GD_CASE(64);
  else if (Dk == 128) GD_CASE(128);
  else GD_CASE(256);
#undef GD_CASE
  if (nsplit > 1)
    launch_attn_decode_combine(part_o, part_ml, out, nsplit, B, Hq, Dk,
                               (long)Hq * Dk, (long)Dk, stream);
}
