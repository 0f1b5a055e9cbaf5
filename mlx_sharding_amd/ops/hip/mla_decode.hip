// MFMA flash-decode for absorbed MLA (MQA over the compressed cache) at
// 32 / 64 / 128 query heads (mla_decode_kernel) and at 16 query heads
// (mla_decode16_kernel, second work split at the end of this comment).
//
// Cache rows are [c_kv | k_pe] (Dk = rank + rope); V is the first
// Dv = rank columns of the same rows, Hkv == 1.  q comes from two
// sources ([B, Hq, rank] and [B, Hq, rope] views with their own
// batch/head strides), the output is head-major [Hq, B, Dv].
//
// Work split: a block serves one batch row, one split-S key slice and
// up to 64 heads (gridDim.z head-groups: 2 at 128 heads, else 1).  It
// has NW = min(4, Hq/16) waves; each wave owns 16 heads for the whole
// slice with its own running (m, l) and 16 x Dv fp32 accumulators, so
// the softmax needs no cross-wave traffic.  The block stages each
// 16-key tile ONCE in LDS and every wave reads it from there: the K tile
// leaves HBM/L2 once per 64 heads instead of once per 8.
//
// Fragment maps (attn_prefill.hip's, plus the 16-deep instruction):
//   mfma_f32_16x16x32_bf16: A(16x32) lane: row=l&15, k=(l>>4)*8+j
//                           B(32x16) lane: col=l&15, k=(l>>4)*8+j
//   mfma_f32_16x16x16_bf16: A(16x16) lane: row=l&15, k=(l>>4)*4+j
//                           B(16x16) lane: col=l&15, k=(l>>4)*4+j
//   C/D (both):             lane: col=l&15, row=(l>>4)*4+reg
//
// QK^T is computed TRANSPOSED, S^T = K . Q^T:
//   A = K tile   lane: key = l&15, dims ks*32 + (l>>4)*8 ..  (one b128
//                LDS read from the row-major image)
//   B = Q^T      lane: head = l&15, same dims — NKS register fragments
//                loaded once per block from the two q sources (columns
//                past Dk are zero: Dk is padded to a multiple of 32)
//   C = S^T      lane: head = l&15, keys (l>>4)*4 + reg
// so a lane holds 4 consecutive keys of ONE head.  That is exactly the A
// layout of the 16-deep instruction, and P goes from the C registers to
// the PV A operand with no LDS round trip.  The per-head max / sum are
// 4 in-lane values plus xor-16 / xor-32 shuffles.
//
// PV, O = P . V with mfma_f32_16x16x16_bf16:
//   A = P        lane: head = l&15, keys (l>>4)*4 + j   (registers)
//   B = V        lane: col = dh*16 + (l&15), keys (l>>4)*4 + j — one b64
//                LDS read from a TRANSPOSED image of the V columns
//   C = O tile   lane: col = dh*16 + (l&15), head = (l>>4)*4 + reg
// O rows are heads (l>>4)*4+reg while (m, l) live in the lane whose
// l&15 is the head, so the per-tile rescale factor and the final 1/l
// are fetched with 4 lane shuffles.
//
// LDS per block (Dk=576: 43264 B, static, no launch attribute; the LDS
// would admit two blocks per CU, the ~400 registers of the 576/512
// instantiation hold it to one).  The tile is 16 keys, not 32: QK needs
// the rows row-major and PV needs the V columns key-contiguous, and two
// 32-key images (37 KB + 41 KB) do not fit 64 KB:
//   K image  [16][DKP + 8] bf16, row-major.  Stride DKP+8 elements =
//            4*(odd) dwords mod 64 banks: the 16 rows a quarter-wave
//            reads with one b128 each start at 16 distinct multiples of
//            4 dwords — conflict-free (584 -> 292 dwords = 36 mod 64).
//   V^T image [Dv][24] bf16.  Stride 24 elements = 12 dwords = 4*3: the
//            16 columns x 2 key-quads a half-wave reads with one b64 each
//            land on 32 distinct even dwords — conflict-free.
// Staging: a thread owns (8-column chunk c, key quad kg) items: four
// 16-byte global loads (keys kg*4..+3), four b128 writes into the K
// image and, for chunks inside Dv, eight b64 writes of 4 keys each into
// the V^T image (the transpose happens in registers).  The next tile's
// loads are issued into registers right after the barrier that
// publishes the current tile, ahead of its MFMAs; the only barriers are
// the two that hand a tile over (readers done / writers done).
//
// Masking: keys at or past the slice end are never loaded — their rows
// are staged as zeros in BOTH images (0 x NaN inside an MFMA is NaN, so
// weight 0 alone is not enough) and their scores are forced to -1e30.
//
// Split-S follows attn_decode_kernel's contract: device position(s)
// int32 [1] / [B] with stride 0/1; capacity-fraction slices under a
// device position; a slice past the row's S writes (m=-1e30, l=0);
// partials [B*Hq, nsplit, Dv] / [.., 2] feed attn_decode_combine_kernel.
//
// Second work split, 16 heads (mla_decode16_kernel, DeepSeek-V2-Lite).
// 16 heads are ONE MFMA tile: with a wave per 16 heads the block above
// would be a single wave staging the whole tile alone with ~400
// registers.  Here a block is still one batch row x one split-S slice,
// but its 4 waves share the 16 heads and split the feature dimensions.
// Tile images, staging, prefetch and masking are the ones above (the
// MD_PREFETCH / MD_STAGE macros), as is the softmax step (MD_SOFTMAX):
//   QK   split over the REDUCTION dimension: wave w holds the Q^T
//        fragments of k-steps w, w+4, .. of the NKS = DKP/32 (5/5/4/4 at
//        Dk = 576; 1/1/1/0 at Dk = 80, where wave 3 contributes zeros) and
//        accumulates a partial S^T tile from its own quarter of the K
//        image.  The four partial C tiles go to sp_lds[4][16][20] fp32
//        (head-major, a lane's 4 keys are one b128), and after one barrier
//        every wave adds them in the fixed order w = 0, 1, 2, 3: all
//        waves hold bit-identical scores, no float atomics.
//   softmax  runs redundantly in every wave on those identical scores, so
//        (m, l), the rescale factors and the bf16 P fragment are identical
//        in all waves and never cross waves.
//   PV   split over OUTPUT COLUMNS: wave w owns column tiles
//        [w*NDH/4, (w+1)*NDH/4) — 8 of 32 at Dv = 512, 1 of 4 at Dv = 64 —
//        reads only those V^T rows and keeps 8 (1) accumulators, not 32.
//   epilogue  each wave stores its columns; wave 0 writes (m, l).
// Each image is thus read from LDS once per tile across the block, and a
// wave needs 132 VGPR + 32 AGPR.  LDS is 43264 + 5120 = 48384 B: three
// blocks fit a CU's 160 KB and the registers allow three too, so one
// block's three barriers per tile (readers done / tile published /
// partials published) can be covered by other blocks' MFMAs;
// mla_decode_nsplit aims at two blocks per CU.  The tile stays 16 keys and
// single-buffered: a 32-key tile (78 KB) or a second LDS buffer (91 KB)
// would leave two or one block per CU.  One tile is prefetched into
// registers, as above: a second register set measured 1.5% at the cost
// of a block per CU (PERFORMANCE.md).

#include "hip_common.h"

#define MD_KT 16    // keys per tile
#define MD_VTS 24   // V^T row stride (elements)
#define MD_SPS 20   // partial-score row stride (floats), 16-head kernel

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));

// Tile staging, shared by both kernels.  The macros expect in scope: tid,
// NT, NIT, NITEMS, DK, DV, KSTR, kvb, hi, k_lds, vt_lds; STG is the prefetch
// register set, a `short8v [NIT][4]`.  item = tid + it*NT -> chunk
// c = item >> 2, key quad kg = item & 3.  (Macros, not lambdas: the bodies
// must inline into the kernel so stg stays in registers.)
#define MD_PREFETCH(STG, T0)                                                 \
  _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                       \
    const int item = tid + it * NT;                                          \
    const int c = item >> 2, kg = item & 3;                                  \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                          \
      const int key = (T0) + kg * 4 + i;                                     \
      short8v v = {0, 0, 0, 0, 0, 0, 0, 0};                                  \
      if (item < NITEMS && c * 8 < DK && key < hi)                           \
        v = *reinterpret_cast<const short8v*>(kvb + (long)key * DK + c * 8); \
      STG[it][i] = v;                                                        \
    }                                                                        \
  }
// stg -> four b128 rows of the K image and, inside Dv, eight b64 columns
// of the V^T image
#define MD_STAGE(STG)                                                        \
  _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                       \
    const int item = tid + it * NT;                                          \
    const int c = item >> 2, kg = item & 3;                                  \
    if (item < NITEMS) {                                                     \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                          \
        *reinterpret_cast<short8v*>(k_lds + (kg * 4 + i) * KSTR + c * 8) =   \
            STG[it][i];                                                      \
      if (c * 8 < DV) {                                                      \
        _Pragma("unroll") for (int j = 0; j < 8; ++j)                        \
          *reinterpret_cast<short4v*>(vt_lds + (c * 8 + j) * MD_VTS +        \
                                      kg * 4) =                              \
              short4v{STG[it][0][j], STG[it][1][j], STG[it][2][j],           \
                      STG[it][3][j]};                                        \
      }                                                                      \
    }                                                                        \
  }

// One online-softmax step of head l&15 over a tile's 16 keys, shared by
// both kernels (a macro so that it compiles exactly as when written
// inline).  C holds the raw scores of keys t0 + lg*4 + reg; keys at or past
// hi are dead.  Expects t0, lg, hi, scale, m_run, l_run in scope; declares
// the bf16 P fragment pf (the PV A operand) and ar[reg], the accumulator
// rescale factor of head lg*4 + reg (the O rows of this lane).
#define MD_SOFTMAX(C)                                                        \
  float sc[4];                                                               \
  float mx = -1e30f;                                                         \
  _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                      \
    const bool live = t0 + lg * 4 + reg < hi;                                \
    sc[reg] = live ? (C)[reg] * scale : -1e30f;                              \
    mx = fmaxf(mx, sc[reg]);                                                 \
  }                                                                          \
  mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));                                  \
  mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));                                  \
  const float mnew = fmaxf(m_run, mx);                                       \
  const float alpha = __expf(m_run - mnew);                                  \
  m_run = mnew;                                                              \
  float ps = 0.0f;                                                           \
  bf16x4_t pf;                                                               \
  _Pragma("unroll") for (int reg = 0; reg < 4; ++reg) {                      \
    /* dead keys must be exactly 0 (their sc equals mnew only if every */    \
    /* key so far is dead, which the loop bounds exclude) */                 \
    const float p = (sc[reg] <= -1e29f) ? 0.0f : __expf(sc[reg] - mnew);     \
    ps += p;                                                                 \
    pf[reg] = (__bf16)p;                                                     \
  }                                                                          \
  ps += __shfl_xor(ps, 16, WAVE);                                            \
  ps += __shfl_xor(ps, 32, WAVE);                                            \
  l_run = l_run * alpha + ps;                                                \
  /* O rows are heads lg*4 + reg: fetch their rescale factors */             \
  float ar[4];                                                               \
  _Pragma("unroll") for (int reg = 0; reg < 4; ++reg)                        \
    ar[reg] = __shfl(alpha, lg * 4 + reg, WAVE);

template <int DK, int DV, int NW>
__global__ __launch_bounds__(NW * WAVE) MD_NO_PK_F32 void mla_decode_kernel(
    const short* __restrict__ q_nope,  // [B, Hq, DV] via (q_bs, q_hs)
    const short* __restrict__ q_rope,  // [B, Hq, DK-DV] via (qr_bs, qr_hs)
    const short* __restrict__ kv,      // [B, Scap, DK]
    short* __restrict__ out,           // [Hq, B, DV]            (nsplit == 1)
    float* __restrict__ part_o,        // [B*Hq, NS, DV]         (nsplit > 1)
    float* __restrict__ part_ml,       // [B*Hq, NS, 2]
    const int* __restrict__ s_ptr, int s_bstride, int B, int Hq, int S,
    long Scap, float scale, long q_bs, long q_hs, long qr_bs, long qr_hs) {
  constexpr int NT = NW * WAVE;
  constexpr int DKP = (DK + 31) / 32 * 32;
  constexpr int NKS = DKP / 32;
  constexpr int NDH = DV / 16;
  constexpr int KSTR = DKP + 8;
  constexpr int CPR = DKP / 8;          // 16-byte chunks per staged row
  constexpr int NITEMS = CPR * 4;       // (chunk, key quad) items per tile
  constexpr int NIT = (NITEMS + NT - 1) / NT;
  static_assert(DK % 8 == 0 && DV % 16 == 0 && DV <= DK, "row geometry");

  const int b = blockIdx.x;
  const int split = blockIdx.y;
  const int nsplit = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int ln = lane & 15;
  const int lg = lane >> 4;
  const int h0 = (blockIdx.z * NW + wid) * 16;  // this wave's first head
  if (s_ptr) S = s_ptr[b * s_bstride] + 1;
  S = (int)min((long)S, Scap);  // loads stay inside the capacity buffer

  __shared__ __attribute__((aligned(16))) short k_lds[MD_KT * KSTR];
  __shared__ __attribute__((aligned(16))) short vt_lds[DV * MD_VTS];

  // ---- Q^T fragments (B operand): head h0 + ln, dims ks*32 + lg*8 .. ----
  bf16x8_t qf[NKS];
  {
    const long h = h0 + ln;
    const short* qn = q_nope + b * q_bs + h * q_hs;
    const short* qr = q_rope + b * qr_bs + h * qr_hs;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const int d = ks * 32 + lg * 8;
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (d < DV) v = *reinterpret_cast<const bf16x8_t*>(qn + d);
      else if (d < DK) v = *reinterpret_cast<const bf16x8_t*>(qr + d - DV);
      qf[ks] = v;
    }
  }

  int lo = 0, hi = S;
  if (nsplit > 1) {
    const long spanc = s_ptr ? Scap : (long)S;
    const long per = ((spanc + nsplit - 1) / nsplit + MD_KT - 1)
                     / MD_KT * MD_KT;
    lo = (int)min((long)S, per * split);
    hi = (int)min((long)S, per * (split + 1));
  }

  float m_run = -1e30f, l_run = 0.0f;   // head h0 + ln (replicated over lg)
  float4v oacc[NDH];
#pragma unroll
  for (int dh = 0; dh < NDH; ++dh) oacc[dh] = float4v{0, 0, 0, 0};

  const short* kvb = kv + (long)b * Scap * DK;
  short8v stg[NIT][4];

  if (lo < hi) MD_PREFETCH(stg, lo)
  for (int t0 = lo; t0 < hi; t0 += MD_KT) {
    __syncthreads();  // every wave is done reading the previous tile
    MD_STAGE(stg)
    __syncthreads();  // tile published
    if (t0 + MD_KT < hi) MD_PREFETCH(stg, t0 + MD_KT)

    // ---- S^T = K . Q^T: lane gets head ln, keys lg*4 + reg ----
    float4v c = {0, 0, 0, 0};
    {
      const short* kr = k_lds + ln * KSTR + lg * 8;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(kr + ks * 32);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], c, 0, 0, 0);
      }
    }
    // ---- online softmax for head ln over the tile's 16 keys ----
    MD_SOFTMAX(c)
    // ---- O = O*alpha + P . V ----
    const short* vr = vt_lds + ln * MD_VTS + lg * 4;
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) {
      bf16x4_t vf =
          *reinterpret_cast<const bf16x4_t*>(vr + dh * 16 * MD_VTS);
      float4v prev = oacc[dh];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) prev[reg] *= ar[reg];
      oacc[dh] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pf, vf, prev, 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds O[head h0 + lg*4 + reg][dh*16 + ln] ----
  if (nsplit == 1) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float rinv = 1.0f / __shfl(l_run, lg * 4 + reg, WAVE);
      short* orow = out + ((long)(h0 + lg * 4 + reg) * B + b) * DV + ln;
#pragma unroll
      for (int dh = 0; dh < NDH; ++dh)
        reinterpret_cast<bf16*>(orow)[dh * 16] = f2bf(oacc[dh][reg] * rinv);
    }
    return;
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    float* prow = part_o +
        (((long)b * Hq + h0 + lg * 4 + reg) * nsplit + split) * DV + ln;
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) prow[dh * 16] = oacc[dh][reg];
  }
  if (lg == 0) {
    const long base = (((long)b * Hq + h0 + ln) * nsplit + split) * 2;
    part_ml[base + 0] = m_run;
    part_ml[base + 1] = l_run;
  }
}

// The 16-head kernel (see the header): one block = one batch row x one
// split-S slice x all 16 heads; its 4 waves split the QK reduction
// dimension and the PV output columns instead of the heads.
template <int DK, int DV>
__global__ __launch_bounds__(4 * WAVE) MD_NO_PK_F32 void mla_decode16_kernel(
    const short* __restrict__ q_nope,  // [B, 16, DV] via (q_bs, q_hs)
    const short* __restrict__ q_rope,  // [B, 16, DK-DV] via (qr_bs, qr_hs)
    const short* __restrict__ kv,      // [B, Scap, DK]
    short* __restrict__ out,           // [16, B, DV]            (nsplit == 1)
    float* __restrict__ part_o,        // [B*16, NS, DV]         (nsplit > 1)
    float* __restrict__ part_ml,       // [B*16, NS, 2]
    const int* __restrict__ s_ptr, int s_bstride, int B, int S, long Scap,
    float scale, long q_bs, long q_hs, long qr_bs, long qr_hs) {
  constexpr int NW = 4;
  constexpr int HQ = 16;
  constexpr int NT = NW * WAVE;
  constexpr int DKP = (DK + 31) / 32 * 32;
  constexpr int NKS = DKP / 32;
  constexpr int NQ = (NKS + NW - 1) / NW;  // k-steps of wave 0 (the most)
  constexpr int NDH = DV / 16;
  constexpr int NDW = NDH / NW;            // column tiles per wave
  constexpr int KSTR = DKP + 8;
  constexpr int CPR = DKP / 8;
  constexpr int NITEMS = CPR * 4;
  constexpr int NIT = (NITEMS + NT - 1) / NT;
  static_assert(DK % 8 == 0 && DV % 16 == 0 && DV <= DK, "row geometry");
  static_assert(NDH % NW == 0, "column tiles split evenly over the waves");

  const int b = blockIdx.x;
  const int split = blockIdx.y;
  const int nsplit = gridDim.y;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int ln = lane & 15;
  const int lg = lane >> 4;
  if (s_ptr) S = s_ptr[b * s_bstride] + 1;
  S = (int)min((long)S, Scap);  // loads stay inside the capacity buffer

  __shared__ __attribute__((aligned(16))) short k_lds[MD_KT * KSTR];
  __shared__ __attribute__((aligned(16))) short vt_lds[DV * MD_VTS];
  // partial S^T tiles [wave][head][16 keys + pad]: a lane's 4 keys are one
  // b128
  __shared__ __attribute__((aligned(16))) float sp_lds[NW * 16 * MD_SPS];

  // ---- Q^T fragments of this wave's k-steps ks = wid + i*NW: head ln,
  // dims ks*32 + lg*8 .. (zero past Dk, which covers ks >= NKS) ----
  bf16x8_t qf[NQ];
  {
    const short* qn = q_nope + b * q_bs + ln * q_hs;
    const short* qr = q_rope + b * qr_bs + ln * qr_hs;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int d = (wid + i * NW) * 32 + lg * 8;
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (d < DV) v = *reinterpret_cast<const bf16x8_t*>(qn + d);
      else if (d < DK) v = *reinterpret_cast<const bf16x8_t*>(qr + d - DV);
      qf[i] = v;
    }
  }

  int lo = 0, hi = S;
  if (nsplit > 1) {
    const long spanc = s_ptr ? Scap : (long)S;
    const long per = ((spanc + nsplit - 1) / nsplit + MD_KT - 1)
                     / MD_KT * MD_KT;
    lo = (int)min((long)S, per * split);
    hi = (int)min((long)S, per * (split + 1));
  }

  // head ln, replicated over lg AND over the waves (identical scores)
  float m_run = -1e30f, l_run = 0.0f;
  float4v oacc[NDW];  // column tiles wid*NDW + j
#pragma unroll
  for (int j = 0; j < NDW; ++j) oacc[j] = float4v{0, 0, 0, 0};

  const short* kvb = kv + (long)b * Scap * DK;
  short8v stg[NIT][4];

  if (lo < hi) MD_PREFETCH(stg, lo)
  for (int t0 = lo; t0 < hi; t0 += MD_KT) {
    __syncthreads();  // every wave is done reading the previous tile
    MD_STAGE(stg)
    __syncthreads();  // tile published
    if (t0 + MD_KT < hi) MD_PREFETCH(stg, t0 + MD_KT)

    // ---- partial S^T = K . Q^T over this wave's k-steps ----
    float4v c = {0, 0, 0, 0};
    {
      const short* kr = k_lds + ln * KSTR + lg * 8;
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const int ks = wid + i * NW;
        if (ks < NKS) {  // wave-uniform
          bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(kr + ks * 32);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[i], c, 0, 0, 0);
        }
      }
    }
    *reinterpret_cast<float4v*>(sp_lds + (wid * 16 + ln) * MD_SPS + lg * 4) = c;
    // partials published.  The next tile's partials are written two
    // barriers after every wave has read these.
    __syncthreads();
    // fixed order w = 0, 1, 2, 3: every wave gets bit-identical scores
    c = *reinterpret_cast<const float4v*>(sp_lds + ln * MD_SPS + lg * 4);
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      const float4v pw = *reinterpret_cast<const float4v*>(
          sp_lds + (w * 16 + ln) * MD_SPS + lg * 4);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) c[reg] += pw[reg];
    }
    // ---- online softmax, redundantly in every wave ----
    MD_SOFTMAX(c)
    // ---- O = O*alpha + P . V over this wave's column tiles ----
    const short* vr = vt_lds + (wid * NDW * 16 + ln) * MD_VTS + lg * 4;
#pragma unroll
    for (int j = 0; j < NDW; ++j) {
      bf16x4_t vf = *reinterpret_cast<const bf16x4_t*>(vr + j * 16 * MD_VTS);
      float4v prev = oacc[j];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) prev[reg] *= ar[reg];
      oacc[j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pf, vf, prev, 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds O[head lg*4 + reg][(wid*NDW + j)*16 + ln] ----
  const int col = wid * NDW * 16 + ln;
  if (nsplit == 1) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float rinv = 1.0f / __shfl(l_run, lg * 4 + reg, WAVE);
      short* orow = out + ((long)(lg * 4 + reg) * B + b) * DV + col;
#pragma unroll
      for (int j = 0; j < NDW; ++j)
        reinterpret_cast<bf16*>(orow)[j * 16] = f2bf(oacc[j][reg] * rinv);
    }
    return;
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    float* prow = part_o +
        (((long)b * HQ + lg * 4 + reg) * nsplit + split) * DV + col;
#pragma unroll
    for (int j = 0; j < NDW; ++j) prow[j * 16] = oacc[j][reg];
  }
  if (wid == 0 && lg == 0) {
    const long base = (((long)b * HQ + ln) * nsplit + split) * 2;
    part_ml[base + 0] = m_run;
    part_ml[base + 1] = l_run;
  }
}

#undef MD_PREFETCH
#undef MD_STAGE
#undef MD_SOFTMAX

extern "C" void launch_attn_decode_combine(const float* part_o,
                                           const float* part_ml, void* out,
                                           int nsplit, int B, int Hq, int Dv,
                                           long o_bs, long o_hs,
                                           hipStream_t stream);

extern "C" bool mla_decode_supported_shape(int Hq, int Dk, int Dv) {
  if (Hq != 16 && Hq != 32 && Hq != 64 && Hq != 128) return false;
  return (Dk == 576 && Dv == 512) || (Dk == 80 && Dv == 64);
}

// Split-S factor: one block per CU (B * head-groups * nsplit against 256
// CUs), slices of at least 256 keys, at most 16 slices.  The 16-head
// kernel's blocks are B * nsplit and several fit a CU; its target is
// MD16_BLOCKS.
#define MD16_BLOCKS 512
extern "C" int mla_decode_nsplit(int B, int Hq, long span) {
  const long groups = Hq > 64 ? Hq / 64 : 1;
  const long blocks = std::max<long>(1, (long)B * groups);
  const long target = Hq == 16 ? MD16_BLOCKS : 256;
  const long want = (target + blocks - 1) / blocks;
  const long fit = std::max<long>(1, (span + 255) / 256);
  return (int)std::min<long>(16, std::min(want, fit));
}

// out is head-major [Hq, B, Dv]; part_o / part_ml are used when
// nsplit > 1.  The caller checked mla_decode_supported_shape.
extern "C" void launch_mla_decode(const void* q_nope, const void* q_rope,
                                  const void* kv, void* out, float* part_o,
                                  float* part_ml, int nsplit,
                                  const int* s_ptr, int s_bstride, int B,
                                  int Hq, int S, long Scap, int Dk, int Dv,
                                  float scale, long q_bs, long q_hs,
                                  long qr_bs, long qr_hs,
                                  hipStream_t stream) {
  if (Hq == 16) {
    dim3 grid16((unsigned)B, (unsigned)nsplit, 1);
#define MD16_CASE(DKK, DVV)                                                 \
  mla_decode16_kernel<DKK, DVV><<<grid16, dim3(4 * WAVE), 0, stream>>>(     \
      (const short*)q_nope, (const short*)q_rope, (const short*)kv,         \
      (short*)out, part_o, part_ml, s_ptr, s_bstride, B, S, Scap, scale,    \
      q_bs, q_hs, qr_bs, qr_hs)
    if (Dk == 576) MD16_CASE(576, 512);
    else MD16_CASE(80, 64);
#undef MD16_CASE
    if (nsplit > 1)
      launch_attn_decode_combine(part_o, part_ml, out, nsplit, B, Hq, Dv,
                                 (long)Dv, (long)B * Dv, stream);
    return;
  }
  const int nw = Hq >= 64 ? 4 : Hq / 16;
  dim3 grid((unsigned)B, (unsigned)nsplit, (unsigned)(Hq / (nw * 16)));
#define MD_CASE(DKK, DVV, NWW)                                              \
  mla_decode_kernel<DKK, DVV, NWW><<<grid, dim3(NWW * WAVE), 0, stream>>>(  \
      (const short*)q_nope, (const short*)q_rope, (const short*)kv,         \
      (short*)out, part_o, part_ml, s_ptr, s_bstride, B, Hq, S, Scap,       \
      scale, q_bs, q_hs, qr_bs, qr_hs)
  if (Dk == 576 && nw == 4) MD_CASE(576, 512, 4);
  else if (Dk == 576) MD_CASE(576, 512, 2);
  else if (nw == 4) MD_CASE(80, 64, 4);
  else MD_CASE(80, 64, 2);
#undef MD_CASE
  if (nsplit > 1)
    launch_attn_decode_combine(part_o, part_ml, out, nsplit, B, Hq, Dv,
                               (long)Dv, (long)B * Dv, stream);
}
