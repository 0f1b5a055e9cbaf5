// MFMA flash attention for a short chunk of T >= 1 new tokens over a long
// cached prefix, grouped-query models (llama, qwen2, tinyllama): G = Hq/Hkv
// query heads (1..16, a runtime value) per KV head over separate per-head
// caches [B, Hkv, Scap, D], D in {64, 128}, bf16 or FP8 (e4m3 bytes with a
// power-of-two fp32 scale per row, reference.kv_fp8_quantize's format).  The
// last T of the S cached rows are the new tokens; token t attends keys
// [0, S - T + t].  No softcap, no sliding window; S is a host value.
//
// Rows.  The queries of one (batch row, kv head) are flattened to virtual
// rows r = t*G + g, R = T*G of them, so the G heads x T tokens that share a
// KV head share every K/V read.  G need not divide 16 (qwen2: G = 7, a
// wave's 16 rows span three tokens), so the causal limit
// lim(r) = S - T + r/G + 1 (keys [0, lim)) is PER ROW.  With S^T = K . Q^T
// a lane's MFMA column is one virtual row: the limit is one integer per
// lane, computed once.
//
// Work split: a block is one (batch row, kv head) x one split-S key slice x
// 64 consecutive virtual rows; grid (B*Hkv, nsplit, ceil(R / 64)).  Each of
// the 4 waves owns 16 rows with a private running (m, l) and a 16 x D fp32
// accumulator, so the softmax has no cross-wave traffic.  Surplus waves of
// a partial last row group own no rows: they stage, hit every barrier, and
// skip the MFMAs and the stores.
//
// Fragment maps (mla_decode.hip's), ln = l&15, lg = l>>4:
//   mfma_f32_16x16x32_bf16: A(16x32) lane: row=ln, k=lg*8+j
//                           B(32x16) lane: col=ln, k=lg*8+j
//   C/D:                    lane: col=ln, row=lg*4+reg
// QK^T per 16-key half-tile hf, transposed:
//   A = K rows   lane: key hf*16 + ln, dims ks*32 + lg*8 ..  (b128, LDS)
//   B = Q^T      lane: row r0 + ln, same dims: D/32 register fragments read
//                once through q's (batch, head, token) strides
//   C = S^T      lane: row r0 + ln, keys hf*16 + lg*4 + reg
// PV on the same 32-deep instruction with gqa_decode.hip's k-slot order:
// k-slot lg*8 + j is key lg*4 + j of half 0 for j < 4 and key
// 16 + lg*4 + j - 4 of half 1 for j >= 4, so the two C tiles of a lane,
// rounded to bf16, ARE its A fragment; B = V^T is one b128 LDS read per
// 16 output columns; the O tile has rows lg*4 + reg, whose rescale factors
// come from the lanes that hold (m, l) by 4 shuffles.
//
// Data movement.  A 32-key K tile and V tile are staged ONCE per block and
// shared by the four waves.  Threads [0, D) stage K, threads [D, 2D) stage V
// (whole waves each; at D = 64 the upper two waves stage nothing), four
// 16-byte loads per thread (8-byte loads of the FP8 caches):
//   K  thread j: 8-dim chunk j % (D/8), rows j / (D/8) + 8*i.  One load
//      instruction reads 256 (D = 128) or 128 contiguous bytes of 4 or 8
//      rows.  Row-major image [32][D + 8] bf16, four b128 writes.
//   V  thread j: key quad j & 7 (keys 4*kq .. +3), chunk j >> 3; a load
//      instruction reads whole 128-byte lines of 8 rows.  The transpose
//      happens in registers: eight b64 writes (4 keys of one column) into
//      the image [D][40] bf16 at k-slot (kq&3)*8 + (kq>>2)*4.
// The next tile is prefetched into registers right after the barrier that
// publishes the current one, ahead of the MFMAs; two barriers per tile.
// FP8: the prefetch holds the raw bytes and the rows' scales; they are
// widened at the LDS write (v_cvt_pk_f32_fp8, times the scale, upper half:
// code * 2^e is exact in bf16) into the SAME images, so the staged bits are
// kv_fp8_dequant_kernel's and everything after the staging step is the same
// code: the FP8 output equals the bf16 kernel's on the dequantized buffers
// bit for bit.
//
// Bank conflicts (64 banks of 4 bytes; b128 traffic goes a quarter wave at a
// time).
//   K reads   row stride D + 8 elements = 68 (36) dwords = 4 * odd: the 16
//             rows of a quarter wave (lg fixed) start at 68*ln = 4*ln
//             (36*ln) mod 64, 16 distinct multiples of 4: conflict-free.
//   K writes  D = 128: a quarter wave writes the 16 chunks of one row, 64
//             consecutive dwords: conflict-free.  D = 64: two rows of 8
//             chunks, dwords 36*row + 4*c: only chunk 7 of the first and
//             chunk 0 of the second meet (36 + 28 = 64): one 2-way pair.
//   V reads   stride 40 elements = 20 dwords: dword 20*ln + 4*lg, 20*ln mod
//             64 takes 16 distinct multiples of 4: conflict-free.
//   V writes  gqa_decode.hip's map and its argument: a b64 write lands on
//             dword 160*c + 20*j + 4*(kq&3) + 2*(kq>>2); the 8 key quads
//             cover 16 distinct dwords and 160*c = 32*c mod 64 separates the
//             chunks only by parity: 2-way, on 8 KB per 16 KB tile.
//
// Causality.  The block walks tiles up to the largest limit among its rows,
// clipped to the slice: hi_blk.  Keys at or past hi_blk (hence at or past S)
// are never loaded; both images hold zeros for them (0 x NaN inside an MFMA
// is NaN, so weight 0 alone is not enough).  A wave skips the MFMAs and the
// softmax of tiles starting at or past the largest limit among ITS rows; it
// never leaves the loop, the barriers are block-wide.  Inside a tile a key
// at or past the lane's limit scores -1e30 and gets p = 0 exactly; the
// staged rows between a row's limit and hi_blk are real cache rows, finite,
// and 0 x finite adds nothing.  A row with no live key yet keeps
// (m = -1e30, l = 0): alpha = exp(0) = 1 on a zero accumulator.
//
// Split-S: slices are whole tiles of at least 256 keys.  A row whose limit
// is at or below the slice start ends with the empty partial
// (m = -1e30, l = 0, o = 0).  Virtual head t*Hq + hk*G + g, T*Hq per batch
// row, indexes attn_decode_kernel's partial layout, and its combiner writes
// the output [B, T, Hq, D] (head stride D).  nsplit == 1 writes bf16
// directly.  Fixed reduction order, no float atomics: bit-reproducible.

#include "hip_common.h"

#define GC_NW 4         // waves per block
#define GC_KT 32        // keys per tile
#define GC_VS 40        // V^T image row stride (elements)
#define GC_ROWS 64      // virtual rows per block (4 waves x 16)
#define GC_MIN_SLICE 256

typedef unsigned int gc_u32x2 __attribute__((ext_vector_type(2)));
typedef float gc_f2 __attribute__((ext_vector_type(2)));

// 8 e4m3 codes times the row's power-of-two scale -> 8 bf16 (exact)
__device__ __forceinline__ short8v gc_widen8(gc_u32x2 w, float sf) {
  short8v o;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const gc_f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false);
    const gc_f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
    o[d * 4 + 0] = (short)(__float_as_uint(lo[0] * sf) >> 16);
    o[d * 4 + 1] = (short)(__float_as_uint(lo[1] * sf) >> 16);
    o[d * 4 + 2] = (short)(__float_as_uint(hi[0] * sf) >> 16);
    o[d * 4 + 3] = (short)(__float_as_uint(hi[1] * sf) >> 16);
  }
  return o;
}

template <int D, bool FP8>
__global__ __launch_bounds__(GC_NW * WAVE) MD_NO_PK_F32 void gqa_chunk_kernel(
    const short* __restrict__ q,        // [B, Hq, T, D] via (q_bs, q_hs, q_ts)
    const void* __restrict__ kcache,    // [B, Hkv, Scap, D] bf16 or bytes
    const void* __restrict__ vcache,
    const float* __restrict__ kscale,   // [B, Hkv, Scap]          (FP8)
    const float* __restrict__ vscale,
    short* __restrict__ out,            // [B, T, Hq, D]           (nsplit == 1)
    float* __restrict__ part_o,         // [B*T*Hq, NS, D]         (nsplit > 1)
    float* __restrict__ part_ml,        // [B*T*Hq, NS, 2]
    int T, int Hkv, int G, int S, long Scap, float scale, long q_bs,
    long q_hs, long q_ts) {
  constexpr int NKS = D / 32;   // QK k-steps
  constexpr int NDH = D / 16;   // output column tiles
  constexpr int KSTR = D + 8;   // K image row stride (elements)
  constexpr int CPR = D / 8;    // 8-dim chunks per row
  static_assert(D == 64 || D == 128, "staging roles are whole waves");

  const int b = blockIdx.x / Hkv;
  const int hk = blockIdx.x % Hkv;
  const int split = blockIdx.y;
  const int nsplit = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int ln = lane & 15;
  const int lg = lane >> 4;
  const int Hq = Hkv * G;
  const int R = T * G;                                // virtual rows
  const int r0 = ((int)blockIdx.z * GC_NW + wid) * 16;  // wave's first row
  const bool owns = r0 < R;

  int lo = 0, hi = S;
  if (nsplit > 1) {
    const long per = max((long)GC_MIN_SLICE,
                         (((long)S + nsplit - 1) / nsplit + GC_KT - 1)
                             / GC_KT * GC_KT);
    lo = (int)min((long)S, per * split);
    hi = (int)min((long)S, per * (split + 1));
  }
  // lim(r) = lim0 + r / G; the last row of a block / wave sees the most keys
  const int lim0 = S - T + 1;
  const int hi_blk =
      min(hi, lim0 + (min(R, ((int)blockIdx.z + 1) * GC_ROWS) - 1) / G);
  const int hi_w = owns ? min(hi, lim0 + (min(R, r0 + 16) - 1) / G) : lo;
  // this lane's virtual row (its MFMA column in S^T)
  const int r = r0 + ln;
  const bool valid = r < R;
  const int tok = valid ? r / G : 0;
  const int g = valid ? r - tok * G : 0;
  const int lim = valid ? min(hi, lim0 + tok) : 0;

  __shared__ __attribute__((aligned(16))) short k_lds[GC_KT * KSTR];
  __shared__ __attribute__((aligned(16))) short vt_lds[D * GC_VS];

  // ---- Q^T fragments (B operand): row r0 + ln, dims ks*32 + lg*8 .. ----
  bf16x8_t qf[NKS];
  {
    const short* qp = q + b * q_bs + ((long)hk * G + g) * q_hs +
                      (long)tok * q_ts + lg * 8;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (valid) v = *reinterpret_cast<const bf16x8_t*>(qp + ks * 32);
      qf[ks] = v;
    }
  }

  float m_run = -1e30f, l_run = 0.0f;   // row r0 + ln (replicated over lg)
  float4v oacc[NDH];
#pragma unroll
  for (int dh = 0; dh < NDH; ++dh) oacc[dh] = float4v{0, 0, 0, 0};

  // ---- staging roles (wave-uniform: D is a multiple of 64) ----
  const bool is_k = tid < D;
  const bool stager = tid < 2 * D;
  const int j = is_k ? tid : tid - D;
  const int kq = j & 7;                          // V: key quad
  const int col8 = is_k ? j % CPR : j >> 3;      // 8-dim chunk
  const int row0 = is_k ? j / CPR : kq * 4;      // first tile row
  const int rstep = is_k ? 8 : 1;                // rows row0 + i*rstep
  const long rbase = ((long)b * Hkv + hk) * Scap;
  const void* src = is_k ? kcache : vcache;
  const float* ssrc = FP8 ? (is_k ? kscale : vscale) + rbase : nullptr;
  const long soff = rbase * D + col8 * 8;        // elements (bytes for FP8)

  short8v stg[4];      // bf16: the rows as loaded
  gc_u32x2 raw[4];     // FP8: their bytes ..
  float rsc[4];        // .. and scales
  // rows at or past hi_blk are zeros.  (A macro, not a lambda: the body must
  // inline into the kernel so the prefetch stays in registers.)
#define GC_PREFETCH(T0)                                                      \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                            \
    const int key = (T0) + row0 + i * rstep;                                 \
    const bool ld = stager && key < hi_blk;                                  \
    if constexpr (FP8) {                                                     \
      gc_u32x2 w = {0u, 0u};                                                 \
      float sf = 0.0f;                                                       \
      if (ld) {                                                              \
        w = *reinterpret_cast<const gc_u32x2*>(                              \
            (const unsigned char*)src + soff + (long)key * D);               \
        sf = ssrc[key];                                                      \
      }                                                                      \
      raw[i] = w;                                                            \
      rsc[i] = sf;                                                           \
    } else {                                                                 \
      short8v v = {0, 0, 0, 0, 0, 0, 0, 0};                                  \
      if (ld)                                                                \
        v = *reinterpret_cast<const short8v*>((const short*)src + soff +     \
                                              (long)key * D);                \
      stg[i] = v;                                                            \
    }                                                                        \
  }

  if (lo < hi_blk) GC_PREFETCH(lo)
  for (int t0 = lo; t0 < hi_blk; t0 += GC_KT) {
    __syncthreads();  // every wave is done reading the previous tile
    if (stager) {
      short8v w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (FP8) w[i] = gc_widen8(raw[i], rsc[i]);
        else w[i] = stg[i];
      }
      if (is_k) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<short8v*>(k_lds + (row0 + i * 8) * KSTR +
                                      col8 * 8) = w[i];
      } else {
        short* col = vt_lds + col8 * 8 * GC_VS + (kq & 3) * 8 + (kq >> 2) * 4;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          *reinterpret_cast<short4v*>(col + e * GC_VS) =
              short4v{w[0][e], w[1][e], w[2][e], w[3][e]};
      }
    }
    __syncthreads();  // tile published
    if (t0 + GC_KT < hi_blk) GC_PREFETCH(t0 + GC_KT)
    if (t0 >= hi_w) continue;  // wave-uniform: no row of this wave sees it

    // ---- S^T = K . Q^T per half-tile: row ln, keys hf*16 + lg*4 + reg ----
    float4v c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
    {
      const short* kr = k_lds + ln * KSTR + lg * 8;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const bf16x8_t k0 = *reinterpret_cast<const bf16x8_t*>(kr + ks * 32);
        const bf16x8_t k1 =
            *reinterpret_cast<const bf16x8_t*>(kr + 16 * KSTR + ks * 32);
        c0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf[ks], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf[ks], c1, 0, 0, 0);
      }
    }
    // ---- online softmax of row ln over the tile's 32 keys ----
    float sc[8];
    float mx = -1e30f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int key = t0 + (e >> 2) * 16 + lg * 4 + (e & 3);
      const float s = (e < 4 ? c0[e & 3] : c1[e & 3]) * scale;
      sc[e] = key < lim ? s : -1e30f;
      mx = fmaxf(mx, sc[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mnew = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - mnew);
    m_run = mnew;
    float ps = 0.0f;
    bf16x8_t pf;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      // dead keys are exactly 0, also while the row has no live key yet
      // (mnew is then -1e30 itself)
      const float p = (sc[e] <= -1e29f) ? 0.0f : __expf(sc[e] - mnew);
      ps += p;
      pf[e] = (__bf16)p;
    }
    ps += __shfl_xor(ps, 16, WAVE);
    ps += __shfl_xor(ps, 32, WAVE);
    l_run = l_run * alpha + ps;
    // O rows are rows lg*4 + reg: fetch their rescale factors
    float ar[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) ar[reg] = __shfl(alpha, lg * 4 + reg, WAVE);
    // ---- O = O*alpha + P . V ----
    const short* vr = vt_lds + ln * GC_VS + lg * 8;
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) {
      const bf16x8_t vf =
          *reinterpret_cast<const bf16x8_t*>(vr + dh * 16 * GC_VS);
      float4v prev = oacc[dh];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) prev[reg] *= ar[reg];
      oacc[dh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vf, prev, 0, 0, 0);
    }
  }
#undef GC_PREFETCH

  // ---- epilogue: lane holds O[row r0 + lg*4 + reg][dh*16 + ln] ----
  if (!owns) return;
  const long vh0 = (long)b * T * Hq + (long)hk * G;  // + t*Hq + g
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const float lr = __shfl(l_run, lg * 4 + reg, WAVE);
    const int rr = r0 + lg * 4 + reg;
    if (rr >= R) continue;
    const int tt = rr / G;
    const long vrow = vh0 + (long)tt * Hq + (rr - tt * G);
    if (nsplit == 1) {
      const float rinv = 1.0f / lr;
      short* orow = out + vrow * D + ln;
#pragma unroll
      for (int dh = 0; dh < NDH; ++dh)
        reinterpret_cast<bf16*>(orow)[dh * 16] = f2bf(oacc[dh][reg] * rinv);
    } else {
      float* prow = part_o + (vrow * nsplit + split) * D + ln;
#pragma unroll
      for (int dh = 0; dh < NDH; ++dh) prow[dh * 16] = oacc[dh][reg];
    }
  }
  if (nsplit > 1 && lg == 0 && valid) {
    const long base = ((vh0 + (long)tok * Hq + g) * nsplit + split) * 2;
    part_ml[base + 0] = m_run;
    part_ml[base + 1] = l_run;
  }
}

extern "C" void launch_attn_decode_combine(const float* part_o,
                                           const float* part_ml, void* out,
                                           int nsplit, int B, int Hq, int Dv,
                                           long o_bs, long o_hs,
                                           hipStream_t stream);

extern "C" bool gqa_chunk_supported_shape(int G, int Dk, int Dv) {
  if (G < 1 || G > 16) return false;
  return Dk == Dv && (Dk == 64 || Dk == 128);
}

// Split-S factor, mla_chunk_nsplit's rule: about one block per CU
// (blocks = B * Hkv * ceil(T*G / 64) without a split, against 256 CUs),
// slices of at least 256 keys, at most 16 slices.
extern "C" int gqa_chunk_nsplit(long blocks, long span) {
  blocks = std::max<long>(1, blocks);
  const long want = (256 + blocks - 1) / blocks;
  const long fit = std::max<long>(1, (span + GC_MIN_SLICE - 1) / GC_MIN_SLICE);
  return (int)std::min<long>(16, std::min(want, fit));
}

extern "C" long gqa_chunk_blocks(int B, int Hkv, int T, int G) {
  return (long)B * Hkv * (((long)T * G + GC_ROWS - 1) / GC_ROWS);
}

// out is [B, T, Hq, D] contiguous; part_o / part_ml are used when
// nsplit > 1; kscale / vscale select the FP8 instantiation.  The caller
// checked gqa_chunk_supported_shape and 1 <= T <= S <= Scap.
extern "C" void launch_gqa_chunk(const void* q, const void* k, const void* v,
                                 const float* kscale, const float* vscale,
                                 void* out, float* part_o, float* part_ml,
                                 int nsplit, int B, int T, int Hq, int Hkv,
                                 int S, long Scap, int D, float scale,
                                 long q_bs, long q_hs, long q_ts,
                                 hipStream_t stream) {
  const int G = Hq / Hkv;
  dim3 grid((unsigned)(B * Hkv), (unsigned)nsplit,
            (unsigned)((T * G + GC_ROWS - 1) / GC_ROWS));
#define GC_CASE(DD, F8)                                                      \
  gqa_chunk_kernel<DD, F8><<<grid, dim3(GC_NW * WAVE), 0, stream>>>(         \
      (const short*)q, k, v, kscale, vscale, (short*)out, part_o, part_ml,   \
      T, Hkv, G, S, Scap, scale, q_bs, q_hs, q_ts)
  if (kscale) {
    if (D == 64) GC_CASE(64, true); else GC_CASE(128, true);
  } else {
    if (D == 64) GC_CASE(64, false); else GC_CASE(128, false);
  }
#undef GC_CASE
  if (nsplit > 1)
    launch_attn_decode_combine(part_o, part_ml, out, nsplit, B, T * Hq, D,
                               (long)T * Hq * D, (long)D, stream);
}
