// FP8 (OCP e4m3) KV cache for the llama family: quantizing append, MFMA
// flash-decode over the byte caches, and the dequantizer T > 1 attention
// reads through.
//
// Storage format (ops/reference.py kv_fp8_quantize is the specification):
// K and V caches are [B, Hkv, Scap, D] bytes, each with an fp32 scale
// array [B, Hkv, Scap]: one power-of-two scale 2^e per (row, kv head,
// position), e the smallest integer with amax <= 448 * 2^e clamped to
// [-100, 120] (an all-zero row takes -100).  The byte is the
// round-to-nearest-even e4m3 code of x * 2^-e; x * 2^-e and code * 2^e are
// exact, so quantization is one deterministic rounding.
//
// ---------------------------------------------------------------------------
// gqa_decode_fp8_kernel<D>, D in {64, 128}: T = 1 flash-decode, G = Hq/Hkv
// query heads (1..16, a runtime value) per KV head, gqa_decode_kernel's
// position contract (host length, or device position int32 [1] / [B],
// S_b = pos[b] + 1), split-S bounds and partial layout.
//
// Work split: a block serves one (batch row, kv head, split-S slice); its 4
// waves split the KEYS of the slice in 64-key tiles (wave w walks tiles w,
// w+4, ..: a 256-key slice is one tile per wave).  Every wave keeps a
// private (m, l) and a private 16 x D fp32 accumulator whose 16 MFMA columns
// are the G heads, zero-padded above G.  Every K and V byte is consumed by
// exactly one wave: no block-wide staging, no __syncthreads in the tile
// loop; the waves meet once, in the merge.
//
// Fragment maps of mfma_f32_16x16x32_bf16, ln = l&15, lg = l>>4:
//   A(16x32) lane: row=ln, k=lg*8+j   B(32x16) lane: col=ln, k=lg*8+j
//   C/D:     lane: col=ln, row=lg*4+reg
// e4m3 -> bf16 is exact (4 significant bits into 8) and done in hardware,
// two values per v_cvt_scalef32_pk_bf16_fp8 at scale 1.0, so both products
// stay on the bf16 MFMA with fp32 accumulation.
//
// QK^T, transposed (S^T = K . Q^T), per 16-key sub-tile.  A 16-byte load of
// a one-byte row holds 16 dims = TWO k-steps of a lane, and the contraction
// order over dims is free, so k-slot lg*8 + j of k-step (c, h) is DEFINED as
//   dim c*64 + lg*16 + h*8 + j        c < D/64, h in {0, 1}
//   A = K rows  lane: key = sub*16 + ln; ONE 16-byte global load per c at
//               byte c*64 + lg*16 gives the fragments (c, 0) from its low
//               and (c, 1) from its high 8 bytes.  A wave instruction reads
//               64 contiguous bytes of each of 16 rows; the two c of D = 128
//               complete each row's 128-byte line.
//   B = Q^T     lane: head = ln, the same dims: D/32 register fragments
//               loaded once per block through q's (batch, head) strides
//               with the same permuted map, zero for ln >= G
//   C = S^T     lane: head = ln, keys sub*16 + lg*4 + reg
// so a lane holds 16 scores of ONE head per 64-key tile; the per-head max
// and sum are in-lane plus xor-16 / xor-32 shuffles.
//
// Scales.  The K scale of a key multiplies its score together with `scale`
// (one fp32 multiply).  The V scale folds into P before its bf16 rounding,
// pf = bf16(p * vs[key]); vs is a power of two, so this is bf16(p) * vs, the
// bf16 kernel's rounding of p exactly, while l sums the unscaled p.  A
// tile's 64 + 64 scales are two coalesced 4-byte loads (lane l: key t0 + l),
// prefetched with the tile, passed through 512 bytes of wave-private LDS and
// read back as four b128 broadcasts each (keys sub*16 + lg*4 .. +3).
//
// PV, O = P . V, two 32-deep k-steps u per tile.  The contraction order over
// keys is free: k-slot lg*8 + j of step u is DEFINED as
//   key (2u)*16     + lg*4 + j      for j <  4
//   key (2u + 1)*16 + lg*4 + j - 4  for j >= 4
// so the C tiles 2u and 2u+1 of a lane ARE its A fragment (no LDS round trip
// for P).
//   A = P       lane: head = ln, k-slots lg*8 + j             (registers)
//   B = V       lane: col = dh*16 + ln: ONE b128 LDS read holds the 16
//               bytes of both steps, widened after the read
//   C = O tile  lane: col = dh*16 + ln, head = lg*4 + reg
//
// V staging: the wave-private LDS image holds BYTES, transposed,
// image[col][key byte], key sub*16 + lg'*4 + r at byte lg'*16 + sub*4 + r.
// Each element is widened exactly once either way (64 conversions per lane
// and D = 128 tile), so bytes halve both the LDS writes and the LDS reads
// against a bf16 image and cost nothing extra.  A lane loads items of 4
// consecutive keys (quad kq = l>>2 = sub*4 + lg') x 16 columns (chunk
// (l&3) + 4*it) with four 16-byte loads, transposes each 4 x 4 byte block
// with 8 v_perm_b32, and writes one b32 (4 keys of one column) per column.
// The image is private to the wave and LDS operations of one wave execute
// in order: no barrier.
//
// Bank conflicts (64 banks of 4 bytes).  Column stride KF_VSB = 80 bytes =
// 20 dwords, plus KF_GPAD = 64 bytes = 16 dwords per 16-column group:
//   reads   a quarter wave (lg fixed, ln = 0..15, one column group) reads a
//           b128 per lane at dword 20*ln + 4*lg + const: 20*ln mod 64 takes
//           16 distinct multiples of 4: conflict-free.
//   writes  one instruction writes a fixed column offset of 4 chunks x 16
//           key quads at dword (chunk*16 + cc)*20 + chunk*16 + lg'*4 + sub.
//           chunk*320 = 0 mod 64, so WITHOUT the group pad the four chunks
//           would collide 4-way; with it the chunks sit 16 banks apart and
//           lg'*4 + sub fills each 16: 64 distinct banks, conflict-free.
//
// Prefetch: the next tile's K words are loaded right after the QK MFMAs
// have consumed the current ones, its V items and scales right after the
// staging writes, all ahead of the softmax and the PV MFMAs.
//
// Masking: keys at or past the slice end are never loaded: their K and V
// registers are zeros (0 x NaN inside an MFMA is NaN), their scales are 0,
// their scores -1e30 and their p exactly 0.  NaN codes (0x7F / 0xFF) or
// garbage scales past a row's length cannot reach the output.
//
// Merge and split-S: gqa_decode_kernel's.  The waves publish (m, l) and
// their accumulators to LDS (over the V images, after one barrier); every
// wave combines a quarter of the columns in the fixed order w = 0..3 and
// stores heads < G only.  No float atomics: bit-reproducible.  There is no
// fallback kernel: every G in 1..16 and every span from one key up runs
// here.

#include "fp8_dequant.h"

#define KF_NW 4      // waves per block
#define KF_KT 64     // keys per wave tile
#define KF_VSB 80    // V image column stride (bytes)
#define KF_GPAD 64   // V image pad per 16-column group (bytes)
#define KF_SLICE 256 // split-S granularity (attn_decode_kernel's tile)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float kf_f2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------
// quantization helpers
// ---------------------------------------------------------------------------

// smallest e with amax <= 448 * 2^e = 1.75 * 2^(e+8), clamped; amax >= 0.
// Integer arithmetic on the fp32 fields (zero and subnormals clamp to -100).
__device__ __forceinline__ int kv_fp8_exp(float amax) {
  const unsigned u = __float_as_uint(amax);
  const int e = (int)(u >> 23) - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return min(max(e, -100), 120);
}

__device__ __forceinline__ float kv_fp8_pow2(int e) {  // e in [-126, 127]
  return __uint_as_float((unsigned)(e + 127) << 23);
}

// four values times inv -> four e4m3 codes, memory order
__device__ __forceinline__ unsigned kv_fp8_pack4(const float* x, float inv) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, w, true);
  return (unsigned)w;
}

__device__ __forceinline__ float kf_round_bf16(float v) {
  return bf2f(f2bf(v));
}

// ---------------------------------------------------------------------------
// rope_append_kv_fp8_kernel: the FP8 twin of rope_append_kv_kernel.  One
// 16-lane group per new row: K rows [B, T, Hkv, D] are roped (half-split),
// rounded to bf16 as the bf16 kernel stores them, and quantized from that;
// V rows are quantized as they are.  Lane j of a group owns dims 4j .. 4j+3
// and D/2 + 4j .. +3 (D/8 lanes are active), the amax is a 16-lane xor
// reduction, and the bytes leave as two b32 stores per lane, the scale as
// one store of lane 0.  k == nullptr quantizes the rows of v alone
// (ops.kv_fp8_quantize).  Position as in rope_append_kv_kernel.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(WAVE) void rope_append_kv_fp8_kernel(
    const short* __restrict__ k, const short* __restrict__ v,
    const float* __restrict__ cost, const float* __restrict__ sint,
    unsigned char* __restrict__ kcache, float* __restrict__ kscale,
    unsigned char* __restrict__ vcache, float* __restrict__ vscale,
    const int* __restrict__ pos_ptr, int pos_bstride, int pos0, int B, int T,
    int Hkv, int D, long Scap, long k_rstride, long v_rstride,
    long cs_bstride) {
  const int j = threadIdx.x & 15;
  const long grp = (long)blockIdx.x * (WAVE / 16) + (threadIdx.x >> 4);
  const bool isk = k != nullptr && !(grp & 1);
  const long row = k != nullptr ? grp >> 1 : grp;  // (b, t, h)
  const int half = D / 2;
  const int h = (int)(row % Hkv);
  const int t = (int)((row / Hkv) % T);
  const long b = row / ((long)Hkv * T);
  const bool live = b < B && j < D / 8;

  float x[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // dims 4j .. +3, half + 4j .. +3
  long pos = 0;
  if (live) {
    pos = (long)(pos_ptr ? pos_ptr[b * pos_bstride] : pos0) + t;
    const short* src = isk ? k + (b * T + t) * k_rstride + (long)h * D
                           : v + (b * T + t) * v_rstride + (long)h * D;
    const short4v a = *reinterpret_cast<const short4v*>(src + 4 * j);
    const short4v c2 = *reinterpret_cast<const short4v*>(src + half + 4 * j);
    if (isk) {
      const long cs_off = b * cs_bstride + (long)t * half;
      const float* c = cost + cs_off;
      const float* s = sint + cs_off;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = 4 * j + i;
        const float x1 = bfbits2f(a[i]), x2 = bfbits2f(c2[i]);
        float o1 = x1 * c[p] - x2 * s[p];
        float o2 = x2 * c[p] + x1 * s[p];
        x[i] = kf_round_bf16(o1);
        x[4 + i] = kf_round_bf16(o2);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[i] = bfbits2f(a[i]);
        x[4 + i] = bfbits2f(c2[i]);
      }
    }
  }
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
#pragma unroll
  for (int off = 8; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, 16));
  const int e = kv_fp8_exp(amax);
  const float inv = kv_fp8_pow2(-e);
  if (live && pos >= 0 && pos < Scap) {  // never write outside the capacity
    const long r = (b * Hkv + h) * Scap + pos;
    unsigned char* dst = (isk ? kcache : vcache) + r * D;
    *reinterpret_cast<unsigned*>(dst + 4 * j) = kv_fp8_pack4(x, inv);
    *reinterpret_cast<unsigned*>(dst + half + 4 * j) = kv_fp8_pack4(x + 4, inv);
    if (j == 0) (isk ? kscale : vscale)[r] = kv_fp8_pow2(e);
  }
}

extern "C" void launch_rope_append_kv_fp8(
    const void* k, const void* v, const float* cost, const float* sint,
    void* kcache, float* kscale, void* vcache, float* vscale,
    const int* pos_ptr, int pos_bstride, int pos0, int B, int T, int Hkv,
    int D, long Scap, long k_rstride, long v_rstride, long cs_bstride,
    hipStream_t stream) {
  const long groups = (long)B * T * Hkv * (k ? 2 : 1);
  if (groups == 0) return;
  dim3 grid((unsigned)((groups + WAVE / 16 - 1) / (WAVE / 16)));
  rope_append_kv_fp8_kernel<<<grid, dim3(WAVE), 0, stream>>>(
      (const short*)k, (const short*)v, cost, sint, (unsigned char*)kcache,
      kscale, (unsigned char*)vcache, vscale, pos_ptr, pos_bstride, pos0, B,
      T, Hkv, D, Scap, k_rstride, v_rstride, cs_bstride);
}

// ---------------------------------------------------------------------------
// kv_fp8_dequant_kernel: rows [0, S) of a byte cache [BH, Scap, D] and its
// scales [BH, Scap] -> contiguous bf16 [BH, S, D].  One lane per 16 bytes:
// a 16-byte load, one scale per row, two 16-byte stores.  code * 2^e is
// exact in fp32 and has 4 significant bits, so its upper half IS the bf16.
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(256) void kv_fp8_dequant_kernel(
    const unsigned char* __restrict__ src, const float* __restrict__ scales,
    short* __restrict__ out, long nrows, int S, long Scap, int D) {
  const int cpr = D / 16;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nrows * cpr) return;
  const long r = idx / cpr;
  const int c = (int)(idx % cpr);
  const long srow = (r / S) * Scap + r % S;
  const u32x4 w = *reinterpret_cast<const u32x4*>(src + srow * D + c * 16);
  const float sf = scales[srow];
  short8v o[2];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const kf_f2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], false);
    const kf_f2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[d], true);
    const float f[4] = {lo[0] * sf, lo[1] * sf, hi[0] * sf, hi[1] * sf};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      o[d >> 1][(d & 1) * 4 + i] = (short)(__float_as_uint(f[i]) >> 16);
  }
  short8v* dst = reinterpret_cast<short8v*>(out + r * D + c * 16);
  dst[0] = o[0];
  dst[1] = o[1];
}

extern "C" void launch_kv_fp8_dequant(const void* src, const float* scales,
                                      void* out, long BH, int S, long Scap,
                                      int D, hipStream_t stream) {
  const long n = BH * S * (D / 16);
  if (n == 0) return;
  kv_fp8_dequant_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                          stream>>>((const unsigned char*)src, scales,
                                    (short*)out, BH * S, S, Scap, D);
}

// ---------------------------------------------------------------------------
// gqa_decode_fp8_kernel (design in the file header)
// ---------------------------------------------------------------------------

// 4 x 4 byte transpose: r[i] holds columns 0..3 of key i; returns, per
// column, the bytes of keys 0..3 in order.  v_perm_b32 selector bytes 0..3
// pick from the second operand, 4..7 from the first.
__device__ __forceinline__ void kf_transpose4(const unsigned r[4],
                                              unsigned o[4]) {
  const unsigned a_lo = __builtin_amdgcn_perm(r[1], r[0], 0x05010400u);
  const unsigned a_hi = __builtin_amdgcn_perm(r[1], r[0], 0x07030602u);
  const unsigned b_lo = __builtin_amdgcn_perm(r[3], r[2], 0x05010400u);
  const unsigned b_hi = __builtin_amdgcn_perm(r[3], r[2], 0x07030602u);
  o[0] = __builtin_amdgcn_perm(b_lo, a_lo, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(b_lo, a_lo, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(b_hi, a_hi, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(b_hi, a_hi, 0x07060302u);
}

template <int D>
__global__ __launch_bounds__(KF_NW * WAVE) MD_NO_PK_F32
void gqa_decode_fp8_kernel(
    const short* __restrict__ q,           // [B, Hq, D] via (q_bs, q_hs)
    const unsigned char* __restrict__ k8,  // [B, Hkv, Scap, D]
    const float* __restrict__ kscale,      // [B, Hkv, Scap]
    const unsigned char* __restrict__ v8,  // [B, Hkv, Scap, D]
    const float* __restrict__ vscale,      // [B, Hkv, Scap]
    short* __restrict__ out,               // [B, Hq, D]          (nsplit == 1)
    float* __restrict__ part_o,            // [B*Hq, NS, D]       (nsplit > 1)
    float* __restrict__ part_ml,           // [B*Hq, NS, 2]
    const int* __restrict__ s_ptr, int s_bstride, int Hkv, int G, int S,
    long Scap, float scale, long q_bs, long q_hs) {
  constexpr int NC = D / 64;         // 16-byte K loads per row and lane
  constexpr int NKS = D / 32;        // QK k-steps
  constexpr int NDH = D / 16;        // output column tiles
  constexpr int NIT = D / 64;        // V items per lane
  constexpr int NSUB = KF_KT / 16;   // 16-key sub-tiles
  constexpr int NPV = KF_KT / 32;    // PV k-steps
  constexpr int IMG = D * KF_VSB + NDH * KF_GPAD;  // image bytes per wave
  constexpr int CW = D / KF_NW;      // merge columns per wave
  static_assert(D == 64 || D == 128, "row geometry");
  static_assert(KF_KT == 64, "one scale per lane and tile");
  // the merge buffer [4][16][D] fp32 reuses the V images
  static_assert(16 * D * 4 <= IMG, "merge buffer fits the V images");

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

  __shared__ __attribute__((aligned(16))) unsigned char vt_all[KF_NW * IMG];
  __shared__ __attribute__((aligned(16))) float sc_all[KF_NW * 2 * KF_KT];
  __shared__ float ml_lds[KF_NW * 2 * 16];  // [wave][m | l][head]
  unsigned char* vt_lds = vt_all + wid * IMG;
  float* sc_lds = sc_all + wid * 2 * KF_KT;  // [k scales | v scales]

  // ---- Q^T fragments (B operand): head ln, dims c*64 + lg*16 + h*8 .. ----
  bf16x8_t qf[NKS];
  {
    const short* qh = q + b * q_bs + ((long)hk * G + ln) * q_hs + lg * 16;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      bf16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ln < G)
        v = *reinterpret_cast<const bf16x8_t*>(qh + (ks >> 1) * 64 +
                                               (ks & 1) * 8);
      qf[ks] = v;
    }
  }

  int lo = 0;
  int hi = S;
  if (nsplit > 1) {
    const long spanc = s_ptr ? Scap : (long)S;
    const long per = ((spanc + nsplit - 1) / nsplit + KF_SLICE - 1)
                     / KF_SLICE * KF_SLICE;
    lo = (int)min((long)S, per * split);
    hi = (int)min((long)S, per * (split + 1));
  }

  float m_run = -1e30f, l_run = 0.0f;   // head ln (replicated over lg)
  float4v oacc[NDH];
#pragma unroll
  for (int dh = 0; dh < NDH; ++dh) oacc[dh] = float4v{0, 0, 0, 0};

  const long rbase = ((long)b * Hkv + hk) * Scap;
  const unsigned char* kb = k8 + rbase * D + lg * 16;
  const unsigned char* vb = v8 + rbase * D + (lane & 3) * 16;
  const float* ksb = kscale + rbase;
  const float* vsb = vscale + rbase;
  const int kq = lane >> 2;  // key quad sub*4 + lg'
  u32x4 kraw[NSUB][NC];
  u32x4 vraw[NIT][4];
  float ksr = 0.0f, vsr = 0.0f;

// K words, V items and scales of the tile at T0; rows at or past hi are 0
#define KF_LOAD_K(T0)                                                        \
  _Pragma("unroll") for (int sub = 0; sub < NSUB; ++sub) {                   \
    const int key = (T0) + sub * 16 + ln;                                    \
    _Pragma("unroll") for (int c = 0; c < NC; ++c) {                         \
      u32x4 w = {0, 0, 0, 0};                                                \
      if (key < hi)                                                          \
        w = *reinterpret_cast<const u32x4*>(kb + (long)key * D + c * 64);    \
      kraw[sub][c] = w;                                                      \
    }                                                                        \
  }
#define KF_LOAD_V(T0)                                                        \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                            \
    const int key = (T0) + kq * 4 + i;                                       \
    _Pragma("unroll") for (int it = 0; it < NIT; ++it) {                     \
      u32x4 w = {0, 0, 0, 0};                                                \
      if (key < hi)                                                          \
        w = *reinterpret_cast<const u32x4*>(vb + (long)key * D + it * 64);   \
      vraw[it][i] = w;                                                       \
    }                                                                        \
  }                                                                          \
  {                                                                          \
    const int key = (T0) + lane;                                             \
    ksr = key < hi ? ksb[key] : 0.0f;                                        \
    vsr = key < hi ? vsb[key] : 0.0f;                                        \
  }

  const int t_first = lo + wid * KF_KT;
  if (t_first < hi) {
    KF_LOAD_K(t_first)
    KF_LOAD_V(t_first)
  }
  for (int t0 = t_first; t0 < hi; t0 += KF_NW * KF_KT) {
    const int tn = t0 + KF_NW * KF_KT;
    // ---- S^T = K . Q^T per sub-tile: head ln, keys sub*16 + lg*4 + reg ----
    float4v cs[NSUB];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      float4v acc = {0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const u32x4 w = kraw[sub][c];
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            fp8x8_to_bf16(w[0], w[1]), qf[2 * c], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            fp8x8_to_bf16(w[2], w[3]), qf[2 * c + 1], acc, 0, 0, 0);
      }
      cs[sub] = acc;
    }
    if (tn < hi) KF_LOAD_K(tn)

    // ---- stage V (transposed bytes) and the tile's scales ----
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int chunk = (lane & 3) + 4 * it;
      unsigned char* base = vt_lds + chunk * (16 * KF_VSB + KF_GPAD) +
                            (kq & 3) * 16 + (kq >> 2) * 4;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const unsigned r[4] = {vraw[it][0][d], vraw[it][1][d], vraw[it][2][d],
                               vraw[it][3][d]};
        unsigned o[4];
        kf_transpose4(r, o);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          *reinterpret_cast<unsigned*>(base + (d * 4 + cc) * KF_VSB) = o[cc];
      }
    }
    sc_lds[lane] = ksr;
    sc_lds[KF_KT + lane] = vsr;
    __builtin_amdgcn_wave_barrier();
    if (tn < hi) KF_LOAD_V(tn)

    // ---- online softmax of head ln over the tile's 64 keys ----
    float sc[4 * NSUB], vsl[4 * NSUB];
    float mx = -1e30f;
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      const float4v kk =
          *reinterpret_cast<const float4v*>(sc_lds + sub * 16 + lg * 4);
      const float4v vv =
          *reinterpret_cast<const float4v*>(sc_lds + KF_KT + sub * 16 + lg * 4);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int key = t0 + sub * 16 + lg * 4 + reg;
        const float s = cs[sub][reg] * (kk[reg] * scale);
        sc[sub * 4 + reg] = key < hi ? s : -1e30f;
        vsl[sub * 4 + reg] = vv[reg];
        mx = fmaxf(mx, sc[sub * 4 + reg]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mnew = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - mnew);
    m_run = mnew;
    float ps = 0.0f;
    bf16x8_t pf[NPV];
#pragma unroll
    for (int i = 0; i < 4 * NSUB; ++i) {
      // dead keys are exactly 0 (a tile always has a live key, so mnew is
      // a real score); k-slot j of step u is score u*8 + j
      const float p = (sc[i] <= -1e29f) ? 0.0f : __expf(sc[i] - mnew);
      ps += p;
      pf[i >> 3][i & 7] = (__bf16)(p * vsl[i]);
    }
    ps += __shfl_xor(ps, 16, WAVE);
    ps += __shfl_xor(ps, 32, WAVE);
    l_run = l_run * alpha + ps;
    // O rows are heads lg*4 + reg: fetch their rescale factors
    float ar[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) ar[reg] = __shfl(alpha, lg * 4 + reg, WAVE);

    // ---- O = O*alpha + P . V ----
    const unsigned char* vr = vt_lds + ln * KF_VSB + lg * 16;
#pragma unroll
    for (int dh = 0; dh < NDH; ++dh) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(
          vr + dh * (16 * KF_VSB + KF_GPAD));
      float4v prev = oacc[dh];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) prev[reg] *= ar[reg];
      prev = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pf[0], fp8x8_to_bf16(w[0], w[1]), prev, 0, 0, 0);
      oacc[dh] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          pf[1], fp8x8_to_bf16(w[2], w[3]), prev, 0, 0, 0);
    }
  }
#undef KF_LOAD_K
#undef KF_LOAD_V

  // ---- merge the 4 waves: lane holds O[head lg*4 + reg][dh*16 + ln] ----
  float* acc_lds = reinterpret_cast<float*>(vt_all);  // [wave][16][D]
  if (lg == 0) {
    ml_lds[wid * 32 + ln] = m_run;
    ml_lds[wid * 32 + 16 + ln] = l_run;
  }
  __syncthreads();  // the V images are done with
#pragma unroll
  for (int dh = 0; dh < NDH; ++dh)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      acc_lds[(wid * 16 + lg * 4 + reg) * D + dh * 16 + ln] = oacc[dh][reg];
  __syncthreads();  // partials and m / l published
  // wave wid combines columns [wid*CW, (wid+1)*CW)
  for (int idx = lane; idx < G * CW; idx += WAVE) {
    const int head = idx / CW;
    const int col = wid * CW + idx % CW;
    float mstar = -1e30f;
#pragma unroll
    for (int w = 0; w < KF_NW; ++w) mstar = fmaxf(mstar, ml_lds[w * 32 + head]);
    float o = 0.0f, lsum = 0.0f;
#pragma unroll
    for (int w = 0; w < KF_NW; ++w) {
      const float f = __expf(ml_lds[w * 32 + head] - mstar);
      lsum += ml_lds[w * 32 + 16 + head] * f;
      o += acc_lds[(w * 16 + head) * D + col] * f;
    }
    const long h = (long)hk * G + head;
    if (nsplit == 1) {
      reinterpret_cast<bf16*>(out)[((long)b * Hq + h) * D + col] =
          f2bf(o * (1.0f / lsum));
    } else {
      const long row = ((long)b * Hq + h) * nsplit + split;
      part_o[row * D + col] = o;
      if (idx % CW == 0 && wid == 0) {
        part_ml[row * 2 + 0] = mstar;
        part_ml[row * 2 + 1] = lsum;
      }
    }
  }
}

extern "C" void launch_attn_decode_combine(const float* part_o,
                                           const float* part_ml, void* out,
                                           int nsplit, int B, int Hq, int Dv,
                                           long o_bs, long o_hs,
                                           hipStream_t stream);

extern "C" bool gqa_decode_fp8_supported_shape(int G, int Dk, int Dv) {
  if (G < 1 || G > 16) return false;
  return Dk == Dv && (Dk == 64 || Dk == 128);
}

// out is [B, Hq, D], contiguous; part_o / part_ml are used when nsplit > 1.
// The caller checked gqa_decode_fp8_supported_shape.
extern "C" void launch_gqa_decode_fp8(
    const void* q, const void* k8, const float* kscale, const void* v8,
    const float* vscale, void* out, float* part_o, float* part_ml, int nsplit,
    const int* s_ptr, int s_bstride, int B, int Hq, int Hkv, int S, long Scap,
    int D, float scale, long q_bs, long q_hs, hipStream_t stream) {
  dim3 grid((unsigned)(B * Hkv), (unsigned)nsplit, 1);
#define KF_CASE(DD)                                                          \
  gqa_decode_fp8_kernel<DD><<<grid, dim3(KF_NW * WAVE), 0, stream>>>(        \
      (const short*)q, (const unsigned char*)k8, kscale,                     \
      (const unsigned char*)v8, vscale, (short*)out, part_o, part_ml, s_ptr, \
      s_bstride, Hkv, Hq / Hkv, S, Scap, scale, q_bs, q_hs)
  if (D == 64) KF_CASE(64);
  else KF_CASE(128);
#undef KF_CASE
  if (nsplit > 1)
    launch_attn_decode_combine(part_o, part_ml, out, nsplit, B, Hq, D,
                               (long)Hq * D, (long)D, stream);
}
