// Grouped (gather-style) expert MLP kernels for the stacked `switch_mlp`
// layout (/root/reference/shard/server/model/deepseek_v2.py:101-112).
//
// Decode regime: N tokens × top_k experts.  Tokens are sorted by expert
// on the host and split into sub-ranges of ≤ MG_TOK tokens; each block
// owns one (sub-range, output-row tile) and streams the expert's weight
// rows ONCE, applying each row to all MG_TOK staged tokens — expert
// weights are read per *expert sub-range*, not per (token, expert) pair
// (the naive gather re-read weights per pair: 96% of decode GPU time).
//
// x for the sub-range is staged in LDS (MG_TOK * H bf16); per-token dot
// accumulators are statically indexed (guide §5.4 rule 20).  Large-N
// (prefill) goes through per-expert hipBLASLt GEMMs from Python.

#include "hip_common.h"

#define MG_BLOCK 256
#define MG_WAVES (MG_BLOCK / WAVE)
#define MG_TOK 4

// ---------------------------------------------------------------------------
// bf16 experts: fused gate/up + SwiGLU.
// grid = (row_tiles, n_subranges)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(MG_BLOCK) void moe_gateup_grouped_kernel(
    const short* __restrict__ x,        // [N, H]
    const short* __restrict__ gate_w,   // [E, I, H]
    const short* __restrict__ up_w,     // [E, I, H]
    short* __restrict__ h,              // [P, I] (sorted pair order)
    const int* __restrict__ sub_expert, // [S]
    const int* __restrict__ sub_off,    // [S] first sorted-pair index
    const int* __restrict__ sub_cnt,    // [S] tokens in sub-range (<= MG_TOK)
    const int* __restrict__ sorted_tok, // [P]
    int H, int I) {
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  short* x_lds = reinterpret_cast<short*>(smem_raw);  // [MG_TOK][H]
#pragma unroll
  for (int t = 0; t < MG_TOK; ++t) {
    short4v* dst = reinterpret_cast<short4v*>(x_lds + t * H);
    if (t < cnt) {
      const short4v* src =
          reinterpret_cast<const short4v*>(x + (long)sorted_tok[p0 + t] * H);
      for (int i = tid; i < H / 4; i += MG_BLOCK) dst[i] = src[i];
    } else {
      for (int i = tid; i < H / 4; i += MG_BLOCK) dst[i] = short4v{0, 0, 0, 0};
    }
  }
  __syncthreads();

  const long ebase = (long)e * I * H;
  for (int o = blockIdx.x * MG_WAVES + wid; o < I; o += gridDim.x * MG_WAVES) {
    const short* grow = gate_w + ebase + (long)o * H;
    const short* urow = up_w + ebase + (long)o * H;
    float gdot[MG_TOK] = {};
    float udot[MG_TOK] = {};
    // 16 B/lane weight loads (guide G13); v_dot2c_f32_bf16 does 2
    // products + accumulate per VALU op (4 instr per 8-elem chunk per
    // operand vs 24 cvt+fma before) — the scalar kernels were VALU-
    // limited at ~4 TB/s, this lifts the per-token compute cost.
    for (int d = lane * 8; d < H; d += WAVE * 8) {
      bf16x8_t gv = *reinterpret_cast<const bf16x8_t*>(grow + d);
      bf16x8_t uv = *reinterpret_cast<const bf16x8_t*>(urow + d);
#pragma unroll
      for (int t = 0; t < MG_TOK; ++t) {
        bf16x8_t xv = *reinterpret_cast<const bf16x8_t*>(x_lds + t * H + d);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x2_t xp = {xv[2 * j], xv[2 * j + 1]};
          gdot[t] = dot2_bf16(bf16x2_t{gv[2 * j], gv[2 * j + 1]}, xp, gdot[t]);
          udot[t] = dot2_bf16(bf16x2_t{uv[2 * j], uv[2 * j + 1]}, xp, udot[t]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < MG_TOK; ++t) {
      float g = wave_sum(gdot[t]);
      float u = wave_sum(udot[t]);
      if (lane == 0 && t < cnt) {
        float a = g / (1.0f + __expf(-g));  // silu
        h[(long)(p0 + t) * I + o] = (short)__bfloat16_as_ushort(f2bf(a * u));
      }
    }
  }
}

// Down-proj + weighted atomic scatter into fp32 out.
__global__ __launch_bounds__(MG_BLOCK) void moe_down_grouped_kernel(
    const short* __restrict__ h,        // [P, I] sorted pair order
    const short* __restrict__ down_w,   // [E, H, I]
    float* __restrict__ out,            // [N, H] fp32 (pre-zeroed)
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    const float* __restrict__ sorted_wt,  // [P]
    int I, int H) {
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  short* h_lds = reinterpret_cast<short*>(smem_raw);  // [MG_TOK][I]
#pragma unroll
  for (int t = 0; t < MG_TOK; ++t) {
    short4v* dst = reinterpret_cast<short4v*>(h_lds + t * I);
    if (t < cnt) {
      const short4v* src =
          reinterpret_cast<const short4v*>(h + (long)(p0 + t) * I);
      for (int i = tid; i < I / 4; i += MG_BLOCK) dst[i] = src[i];
    } else {
      for (int i = tid; i < I / 4; i += MG_BLOCK) dst[i] = short4v{0, 0, 0, 0};
    }
  }
  __syncthreads();

  const long ebase = (long)e * H * I;
  for (int o = blockIdx.x * MG_WAVES + wid; o < H; o += gridDim.x * MG_WAVES) {
    const short* drow = down_w + ebase + (long)o * I;
    float dot[MG_TOK] = {};
    // 16 B/lane weight loads (guide G13); v_dot2c accumulate as in the
    // gate/up kernel.  There is no tail: the binding requires I % 8 == 0,
    // and the lane stride covers any such I.
    for (int d = lane * 8; d + 7 < I; d += WAVE * 8) {
      bf16x8_t dv = *reinterpret_cast<const bf16x8_t*>(drow + d);
#pragma unroll
      for (int t = 0; t < MG_TOK; ++t) {
        bf16x8_t hv = *reinterpret_cast<const bf16x8_t*>(h_lds + t * I + d);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dot[t] = dot2_bf16(bf16x2_t{dv[2 * j], dv[2 * j + 1]},
                             bf16x2_t{hv[2 * j], hv[2 * j + 1]}, dot[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < MG_TOK; ++t) {
      float v = wave_sum(dot[t]);
      if (lane == 0 && t < cnt)
        atomicAdd(out + (long)sorted_tok[p0 + t] * H + o, sorted_wt[p0 + t] * v);
    }
  }
}

extern "C" void launch_moe_gateup_grouped(const void* x, const void* gate_w,
                                          const void* up_w, void* h,
                                          const int* sub_expert,
                                          const int* sub_off,
                                          const int* sub_cnt,
                                          const int* sorted_tok, int S, int H,
                                          int I, hipStream_t stream) {
  size_t smem = (size_t)MG_TOK * H * sizeof(short);
  int gx = (I + MG_WAVES - 1) / MG_WAVES;
  if (gx > 64) gx = 64;  // rows loop inside the block: amortize x staging
  moe_gateup_grouped_kernel<<<dim3(gx, S), dim3(MG_BLOCK), smem, stream>>>(
      (const short*)x, (const short*)gate_w, (const short*)up_w, (short*)h,
      sub_expert, sub_off, sub_cnt, sorted_tok, H, I);
}

extern "C" void launch_moe_down_grouped(const void* h, const void* down_w,
                                        float* out, const int* sub_expert,
                                        const int* sub_off, const int* sub_cnt,
                                        const int* sorted_tok,
                                        const float* sorted_wt, int S, int I,
                                        int H, hipStream_t stream) {
  size_t smem = (size_t)MG_TOK * I * sizeof(short);
  int gx = (H + MG_WAVES - 1) / MG_WAVES;
  if (gx > 64) gx = 64;
  moe_down_grouped_kernel<<<dim3(gx, S), dim3(MG_BLOCK), smem, stream>>>(
      (const short*)h, (const short*)down_w, out, sub_expert, sub_off,
      sub_cnt, sorted_tok, sorted_wt, I, H);
}

// ---------------------------------------------------------------------------
// MFMA bf16 grouped expert kernels (16-token sub-ranges).
//
// The scalar dot2 kernels above pay per-token VALU for every weight
// byte, which caps the profitable sub-range width at 4 tokens — expert
// weights get re-read ~1.5x at batch 64.  On MFMA the per-token cost is
// in the matrix unit, so 16-token sub-ranges stream each activated
// expert's weights ~once:
//   A = 16 weight rows x 32 k (bf16 16 B/lane loads — the row layout IS
//       the fragment layout), B = x^T from LDS, D[row, token].
// Same fragment scheme as the w4 MFMA kernel (w4a16.hip) minus dequant.
// ---------------------------------------------------------------------------

#define MF_WAVES 4
#define MF_BLOCK (MF_WAVES * WAVE)
#define MF_TOK 16
#define MF_CH 384
#define MF_LDS (MF_CH + 16)  // rows 16B-aligned, 8-bank shift per row
#define MF_NSL (MF_CH / 32)

// No LDS, no barriers: B-fragments are read straight from the 16 token
// rows in global (same strided 16-rows-x-16B pattern as the A loads —
// quarter-wave groups cover a full 64 B line per row).  x is tiny and
// L2-resident; staging it through LDS cost two barriers per chunk that
// serialized staging against compute.  Columns of dead tokens (t >=
// cnt) compute garbage that the epilogue simply never writes, so the
// token-row index is clamped instead of zero-padded.
__global__ __launch_bounds__(MF_BLOCK) void moe_gateup_mfma_kernel(
    const short* __restrict__ x,        // [N, H]
    const short* __restrict__ gate_w,   // [E, I, H]
    const short* __restrict__ up_w,     // [E, I, H]
    short* __restrict__ h,              // [P, I]
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    int H, int I) {
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;

  const int row0 = (blockIdx.x * MF_WAVES + wid) * 16;
  if (row0 >= I) return;
  const long ebase = (long)e * I * H;
  const int wr = min(row0 + (lane & 15), I - 1);
  const short* grow = gate_w + ebase + (long)wr * H;
  const short* urow = up_w + ebase + (long)wr * H;
  const int tok_r = sorted_tok[p0 + min(lane & 15, cnt - 1)];
  const short* xrow = x + (long)tok_r * H;

  float4v gacc = {0, 0, 0, 0}, uacc = {0, 0, 0, 0};
  // full MF_NSL-slice batches (all global loads issued before the MFMA
  // block — guide trap 4(b)), then an exact tail loop: without zeroed
  // LDS columns, clamped duplicate loads would double-count.
  const int nsl_total = H / 32;  // binding requires H % 32 == 0
  int sl = 0;
  for (; sl + MF_NSL <= nsl_total; sl += MF_NSL) {
    bf16x8_t ga[MF_NSL], ua[MF_NSL], ba[MF_NSL];
#pragma unroll
    for (int i = 0; i < MF_NSL; ++i) {
      const int koff = (sl + i) * 32 + (lane >> 4) * 8;
      ga[i] = *reinterpret_cast<const bf16x8_t*>(grow + koff);
      ua[i] = *reinterpret_cast<const bf16x8_t*>(urow + koff);
      ba[i] = *reinterpret_cast<const bf16x8_t*>(xrow + koff);
    }
#pragma unroll
    for (int i = 0; i < MF_NSL; ++i) {
      gacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga[i], ba[i], gacc, 0, 0, 0);
      uacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua[i], ba[i], uacc, 0, 0, 0);
    }
  }
  for (; sl < nsl_total; ++sl) {  // < MF_NSL leftover slices, once
    const int koff = sl * 32 + (lane >> 4) * 8;
    bf16x8_t ga = *reinterpret_cast<const bf16x8_t*>(grow + koff);
    bf16x8_t ua = *reinterpret_cast<const bf16x8_t*>(urow + koff);
    bf16x8_t ba = *reinterpret_cast<const bf16x8_t*>(xrow + koff);
    gacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ga, ba, gacc, 0, 0, 0);
    uacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua, ba, uacc, 0, 0, 0);
  }

  const int tok = lane & 15;
  if (tok < cnt) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int o = row0 + (lane >> 4) * 4 + reg;
      if (o < I) {
        const float g = gacc[reg], u = uacc[reg];
        const float a = g / (1.0f + __expf(-g));  // silu
        h[(long)(p0 + tok) * I + o] = (short)__bfloat16_as_ushort(f2bf(a * u));
      }
    }
  }
}

__global__ __launch_bounds__(MF_BLOCK) void moe_down_mfma_kernel(
    const short* __restrict__ h,        // [P, I]
    const short* __restrict__ down_w,   // [E, H, I]
    float* __restrict__ out,            // [N, H] fp32 (pre-zeroed)
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

  const int row0 = (blockIdx.x * MF_WAVES + wid) * 16;
  if (row0 >= H) return;
  const long ebase = (long)e * H * I;
  const int wr = min(row0 + (lane & 15), H - 1);
  const short* drow = down_w + ebase + (long)wr * I;
  // B rows = h pair rows (clamped for dead lanes; their D columns are
  // never written)
  const short* hrow = h + (long)(p0 + min(lane & 15, cnt - 1)) * I;

  float4v acc = {0, 0, 0, 0};
  const int nsl_total = I / 32;  // binding requires I % 32 == 0
  int sl = 0;
  for (; sl + MF_NSL <= nsl_total; sl += MF_NSL) {
    bf16x8_t da[MF_NSL], ba[MF_NSL];
#pragma unroll
    for (int i = 0; i < MF_NSL; ++i) {
      const int koff = (sl + i) * 32 + (lane >> 4) * 8;
      da[i] = *reinterpret_cast<const bf16x8_t*>(drow + koff);
      ba[i] = *reinterpret_cast<const bf16x8_t*>(hrow + koff);
    }
#pragma unroll
    for (int i = 0; i < MF_NSL; ++i)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[i], ba[i], acc, 0, 0, 0);
  }
  for (; sl < nsl_total; ++sl) {
    const int koff = sl * 32 + (lane >> 4) * 8;
    bf16x8_t da = *reinterpret_cast<const bf16x8_t*>(drow + koff);
    bf16x8_t ba = *reinterpret_cast<const bf16x8_t*>(hrow + koff);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, ba, acc, 0, 0, 0);
  }

  const int tok = lane & 15;
  if (tok < cnt) {
    const float wt = sorted_wt[p0 + tok];
    const long trow = (long)sorted_tok[p0 + tok] * H;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int o = row0 + (lane >> 4) * 4 + reg;
      if (o < H) atomicAdd(out + trow + o, wt * acc[reg]);
    }
  }
}

extern "C" void launch_moe_gateup_mfma(const void* x, const void* gate_w,
                                       const void* up_w, void* h,
                                       const int* sub_expert,
                                       const int* sub_off, const int* sub_cnt,
                                       const int* sorted_tok, int S, int H,
                                       int I, hipStream_t stream) {
  const int gx = (I + MF_WAVES * 16 - 1) / (MF_WAVES * 16);
  moe_gateup_mfma_kernel<<<dim3(gx, S), dim3(MF_BLOCK), 0, stream>>>(
      (const short*)x, (const short*)gate_w, (const short*)up_w, (short*)h,
      sub_expert, sub_off, sub_cnt, sorted_tok, H, I);
}

extern "C" void launch_moe_down_mfma(const void* h, const void* down_w,
                                     float* out, const int* sub_expert,
                                     const int* sub_off, const int* sub_cnt,
                                     const int* sorted_tok,
                                     const float* sorted_wt, int S, int I,
                                     int H, hipStream_t stream) {
  const int gx = (H + MF_WAVES * 16 - 1) / (MF_WAVES * 16);
  moe_down_mfma_kernel<<<dim3(gx, S), dim3(MF_BLOCK), 0, stream>>>(
      (const short*)h, (const short*)down_w, out, sub_expert, sub_off,
      sub_cnt, sorted_tok, sorted_wt, I, H);
}

// ---------------------------------------------------------------------------
// Prefill padded-expert data movement.
//
// torch's advanced-indexing kernels for the [E, cap, H] scatter
// (`xp[dst] = x[tok]`) and the fp32 weighted `index_add_` reduce run
// ~5x off roofline at 16K-token prefill shapes; these two kernels do
// the same moves with vectorized row copies and a per-token K-way
// gather (fp32 accumulation, no atomics).
// ---------------------------------------------------------------------------

__global__ void moe_scatter_rows_kernel(const short* __restrict__ src,
                                        short* __restrict__ dst,
                                        const int* __restrict__ src_idx,
                                        const int* __restrict__ dst_idx,
                                        int H) {
  const int p = blockIdx.x;
  const short4v* s =
      reinterpret_cast<const short4v*>(src + (long)src_idx[p] * H);
  short4v* d = reinterpret_cast<short4v*>(dst + (long)dst_idx[p] * H);
  for (int i = threadIdx.x; i < H / 4; i += blockDim.x) d[i] = s[i];
}

// out[t] = sum_k wts[t,k] * d[pos[t,k]]  (bf16 rows, fp32 accumulate;
// short4 vector loads — the scalar form measured 2.3 TB/s on ~1 GB of
// traffic per prefill MoE layer)
__global__ void moe_gather_reduce_kernel(const short* __restrict__ d,
                                         const int* __restrict__ pos,    // [N,K]
                                         const float* __restrict__ wts,  // [N,K]
                                         short* __restrict__ out,        // [N,H]
                                         int K, int H) {
  const int t = blockIdx.x;
  const int* prow = pos + (long)t * K;
  const float* wrow = wts + (long)t * K;
  short* orow = out + (long)t * H;
  const int n4 = H / 4;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int k = 0; k < K; ++k) {
      const float w = wrow[k];
      short4v v = reinterpret_cast<const short4v*>(d + (long)prow[k] * H)[i];
      a0 += w * bfbits2f(v.x);
      a1 += w * bfbits2f(v.y);
      a2 += w * bfbits2f(v.z);
      a3 += w * bfbits2f(v.w);
    }
    short4v o;
    o.x = (short)__bfloat16_as_ushort(f2bf(a0));
    o.y = (short)__bfloat16_as_ushort(f2bf(a1));
    o.z = (short)__bfloat16_as_ushort(f2bf(a2));
    o.w = (short)__bfloat16_as_ushort(f2bf(a3));
    reinterpret_cast<short4v*>(orow)[i] = o;
  }
}

extern "C" void launch_moe_scatter_rows(const void* src, void* dst,
                                        const int* src_idx, const int* dst_idx,
                                        int P, int H, hipStream_t stream) {
  moe_scatter_rows_kernel<<<dim3((unsigned)P), dim3(256), 0, stream>>>(
      (const short*)src, (short*)dst, src_idx, dst_idx, H);
}

extern "C" void launch_moe_gather_reduce(const void* d, const int* pos,
                                         const float* wts, void* out, int N,
                                         int K, int H, hipStream_t stream) {
  moe_gather_reduce_kernel<<<dim3((unsigned)N), dim3(256), 0, stream>>>(
      (const short*)d, pos, wts, (short*)out, K, H);
}

// ---------------------------------------------------------------------------
// Fused MoE gating + expert sort + sub-range build (decode regime).
//
// Replaces ~20 small torch launches per MoE layer (softmax, topk,
// argsort/radix-sort, bincount, cumsums, scatter/cummax) with ONE
// kernel.  Softmax top-k, plain greedy (DeepSeek-V2-Lite) or
// group-limited greedy (DeepSeek-V2: keep the topk_group groups with the
// largest member probability, pick the top-k among their experts; the
// weights stay the full-softmax probabilities).
//
// SIG = true is DeepSeek-V3's noaux_tc router: s = sigmoid(logit),
// selection runs on c = s + e_bias (a group's score is the sum of its two
// largest c, so E / n_group >= 2), the weights are the unbiased s.
//
// Single workgroup; one wave per token; lane l holds experts l, 64+l,
// 128+l, 192+l in registers.  Limits (checked by the binding, the LDS
// arrays are fixed-size): N <= 128 tokens, E <= 256 experts, top_k <= 8,
// n_group <= 32 with E % n_group == 0, topk_group * (E / n_group) >= top_k.
// ---------------------------------------------------------------------------

#define GK_MAXK 8
#define GK_MAXN 128  // max tokens (LDS arrays below)
#define GK_MAXE 256  // max experts (LDS arrays below)
#define GK_WAVES 16

// Wave argmax of (v, idx) pairs, ties to the lowest idx; every lane ends
// up with the winner.
__device__ __forceinline__ void gk_wave_argmax(float& best, int& bidx) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(best, off, WAVE);
    int oi = __shfl_xor(bidx, off, WAVE);
    if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
  }
}

// out[e] = sum_{j<e} ceil(cnt[j] / div) for e in [0, E], by ONE wave:
// lane l owns experts 4l..4l+3 (E <= 256), then a 6-step wave scan.
__device__ __forceinline__ void gk_wave_prefix(const int* cnt, int* out, int E,
                                               int div, int lane) {
  int c[4];
  int s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane * 4 + j;
    c[j] = (e < E) ? (cnt[e] + div - 1) / div : 0;
    s += c[j];
  }
  int inc = s;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int o = __shfl_up(inc, off, WAVE);
    if (lane >= off) inc += o;
  }
  int acc = inc - s;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane * 4 + j;
    if (e < E) out[e] = acc;
    acc += c[j];
  }
  if (lane == WAVE - 1) out[E] = inc;
}

// Back half shared by every instantiation: counting-sort the chosen
// (token, k) pairs by expert and emit the <= max_tok sub-range slots.
// Needs >= 2 waves; all threads of the block must call it.
__device__ __forceinline__ void gk_sort_and_subranges(
    const int* counts, int* starts, int* fill, int* sub_base, const int* tok_e,
    const float* tok_w, int* __restrict__ sorted_tok,
    float* __restrict__ sorted_wt, int* __restrict__ sub_expert,
    int* __restrict__ sub_off, int* __restrict__ sub_cnt, int N, int E, int K,
    int s_upper, int max_tok, float routed_scaling) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;

  // ---- prefix sums: pair offsets (wave 0), sub-range slots (wave 1) ----
  if (wid == 0) gk_wave_prefix(counts, starts, E, 1, lane);
  if (wid == 1) gk_wave_prefix(counts, sub_base, E, max_tok, lane);
  __syncthreads();

  // ---- scatter pairs into expert-sorted order ----
  for (int i = threadIdx.x; i < N * K; i += blockDim.x) {
    const int t = i / K, k = i % K;
    const int e = tok_e[t * GK_MAXK + k];
    const int pos = starts[e] + atomicAdd(&fill[e], 1);
    sorted_tok[pos] = t;
    sorted_wt[pos] = tok_w[t * GK_MAXK + k] * routed_scaling;
  }

  // ---- sub-range arrays ----
  // slot layout: expert e's ceil(counts[e]/max_tok) sub-ranges are
  // contiguous, experts in order; slots past the live ones are zeroed
  const int S = sub_base[E];
  for (int i = threadIdx.x; i < s_upper; i += blockDim.x) {
    if (i >= S) {
      sub_cnt[i] = 0;
      sub_expert[i] = 0;
      sub_off[i] = 0;
    }
  }
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    const int ns = (counts[e] + max_tok - 1) / max_tok;
    for (int j = 0; j < ns; ++j) {
      const int slot = sub_base[e] + j;
      sub_expert[slot] = e;
      sub_off[slot] = starts[e] + j * max_tok;
      sub_cnt[slot] = min(max_tok, counts[e] - j * max_tok);
    }
  }
}

// 1024 threads (16 waves): the top-k argmax is a serial chain of
// dependent ds_bpermute shuffles per token — more waves = fewer tokens
// serialized per wave.  R = ceil(E / 64) probabilities per lane.
template <int R, bool SIG>
__global__ __launch_bounds__(1024) void moe_gate_subranges_kernel(
    const short* __restrict__ logits,  // [N, E] bf16
    const float* __restrict__ e_bias,  // [E] fp32 or null (SIG only)
    int* __restrict__ sorted_tok,      // [P]
    float* __restrict__ sorted_wt,     // [P]
    int* __restrict__ sub_expert,      // [s_upper]
    int* __restrict__ sub_off,         // [s_upper]
    int* __restrict__ sub_cnt,         // [s_upper]
    int N, int E, int K, int s_upper, int max_tok, float routed_scaling,
    int norm_topk, int n_group, int topk_group) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;

  __shared__ int counts[GK_MAXE];        // per-expert pair count
  __shared__ int starts[GK_MAXE + 1];    // exclusive prefix
  __shared__ int fill[GK_MAXE];          // scatter cursor per expert
  __shared__ int sub_base[GK_MAXE + 1];  // first sub-range slot per expert
  __shared__ int tok_e[GK_MAXN * GK_MAXK];    // chosen expert per (token, k)
  __shared__ float tok_w[GK_MAXN * GK_MAXK];  // chosen weight per (token, k)
  __shared__ float probs[GK_WAVES][R * WAVE];  // per-wave row (group scan)

  for (int i = threadIdx.x; i < GK_MAXE; i += blockDim.x) {
    counts[i] = 0;
    fill[i] = 0;
  }
  __syncthreads();

  // masked, padded and already-picked entries: below any probability
  // (softmax), below any finite biased score (sigmoid; c can pass -1)
  constexpr float NEG = SIG ? -__builtin_inff() : -1.0f;

  const int gsz = E / n_group;  // experts per group
  int grp[R];                   // group of this lane's r-th expert
#pragma unroll
  for (int r = 0; r < R; ++r) grp[r] = min(r * WAVE + lane, E - 1) / gsz;

  // ---- per-token softmax + (group-limited) greedy top-k, one wave per
  // token; the trip count is block-uniform so the group step may barrier
  for (int t0 = 0; t0 < N; t0 += GK_WAVES) {
    const int t = t0 + wid;
    const bool live = t < N;
    float p[R];            // selection score: probability, or c (SIG)
    float s[SIG ? R : 1];  // SIG: unbiased sigmoid score, the weight
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] = 0.0f;
    if constexpr (SIG) {
      if (live) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int e = r * WAVE + lane;
          const int ec = min(e, E - 1);  // padded lanes are masked below
          const float x = bfbits2f(logits[(long)t * E + ec]);
          s[r] = 1.0f / (1.0f + __expf(-x));
          p[r] = s[r] + (e_bias ? e_bias[ec] : 0.0f);
        }
      }
    } else if (live) {
      float sc[R];
      float mx = -1e30f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int e = r * WAVE + lane;
        sc[r] = (e < E) ? bfbits2f(logits[(long)t * E + e]) : -1e30f;
        mx = fmaxf(mx, sc[r]);
      }
      mx = wave_max(mx);
      float psum = 0.0f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        p[r] = (r * WAVE + lane < E) ? __expf(sc[r] - mx) : 0.0f;
        psum += p[r];
      }
      const float denom = wave_sum(psum);
#pragma unroll
      for (int r = 0; r < R; ++r) p[r] /= denom;
    }

    // ---- group step: bitmask of the topk_group best groups ----
    unsigned gmask = 0xffffffffu;
    if (n_group > 1) {
      if (live) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (r * WAVE + lane < E) probs[wid][r * WAVE + lane] = p[r];
      }
      __syncthreads();
      if (live) {
        // lane g scans group g for its max probability (SIG: the sum of
        // its two largest c); NEG marks lanes without a group and groups
        // already kept
        float gs = NEG;
        if (lane < n_group) {
          const float* row = &probs[wid][lane * gsz];
          if constexpr (SIG) {
            float b1 = NEG, b2 = NEG;
            for (int j = 0; j < gsz; ++j) {
              const float v = row[j];
              if (v > b1) { b2 = b1; b1 = v; }
              else if (v > b2) b2 = v;
            }
            gs = b1 + b2;  // gsz >= 2: both finite
          } else {
            gs = row[0];
            for (int j = 1; j < gsz; ++j) gs = fmaxf(gs, row[j]);
          }
        }
        gmask = 0u;
        for (int g = 0; g < topk_group; ++g) {
          float best = gs;
          int bidx = lane;
          gk_wave_argmax(best, bidx);
          gmask |= 1u << bidx;
          if (lane == bidx) gs = NEG;
        }
      }
      __syncthreads();  // row is rewritten by the next token
    }

    if (live) {
      // masked, padded and already-picked experts sit at NEG (an
      // unmasked probability that underflowed to 0 wins)
      float psel[R];
#pragma unroll
      for (int r = 0; r < R; ++r)
        psel[r] = (r * WAVE + lane < E && ((gmask >> grp[r]) & 1u)) ? p[r]
                                                                    : NEG;
      float wsum = 0.0f;
#pragma unroll
      for (int k = 0; k < GK_MAXK; ++k) {
        if (k >= K) break;
        // lane-local argmax over the R registers, then wave argmax
        float best = psel[0];
        int bidx = lane;
#pragma unroll
        for (int r = 1; r < R; ++r)
          if (psel[r] > best) { best = psel[r]; bidx = r * WAVE + lane; }
        gk_wave_argmax(best, bidx);
        if constexpr (SIG) {
          // selection ran on c; the weight is the owner lane's s
          float sv = s[0];
#pragma unroll
          for (int r = 1; r < R; ++r)
            if (bidx / WAVE == r) sv = s[r];
          best = __shfl(sv, bidx & (WAVE - 1), WAVE);
        }
        if (lane == 0) {
          tok_e[t * GK_MAXK + k] = bidx;
          tok_w[t * GK_MAXK + k] = best;
          atomicAdd(&counts[bidx], 1);
        }
        wsum += best;
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (bidx == r * WAVE + lane) psel[r] = NEG;
      }
      if (norm_topk && lane == 0) {
#pragma unroll
        for (int k = 0; k < GK_MAXK; ++k) {
          if (k >= K) break;
          tok_w[t * GK_MAXK + k] /= (wsum + 1e-20f);
        }
      }
    }
  }
  __syncthreads();

  gk_sort_and_subranges(counts, starts, fill, sub_base, tok_e, tok_w,
                        sorted_tok, sorted_wt, sub_expert, sub_off, sub_cnt, N,
                        E, K, s_upper, max_tok, routed_scaling);
}

extern "C" void launch_moe_gate_subranges(
    const void* logits, const float* e_bias, int sigmoid, int* sorted_tok,
    float* sorted_wt, int* sub_expert, int* sub_off, int* sub_cnt, int N,
    int E, int K, int s_upper, int max_tok, float routed_scaling,
    int norm_topk, int n_group, int topk_group, hipStream_t stream) {
  // limits are checked by the caller (bindings.hip::moe_gate_subranges)
#define GK_LAUNCH(R, SIG)                                                    \
  moe_gate_subranges_kernel<R, SIG>                                          \
      <<<dim3(1), dim3(GK_WAVES * WAVE), 0, stream>>>(                       \
          (const short*)logits, e_bias, sorted_tok, sorted_wt, sub_expert,   \
          sub_off, sub_cnt, N, E, K, s_upper, max_tok, routed_scaling,       \
          norm_topk, n_group, topk_group)
#define GK_SWITCH(SIG)                                                       \
  switch ((E + WAVE - 1) / WAVE) {                                           \
    case 1: GK_LAUNCH(1, SIG); break;                                        \
    case 2: GK_LAUNCH(2, SIG); break;                                        \
    case 3: GK_LAUNCH(3, SIG); break;                                        \
    default: GK_LAUNCH(4, SIG); break;                                       \
  }
  if (sigmoid) {
    GK_SWITCH(true)
  } else {
    GK_SWITCH(false)
  }
#undef GK_SWITCH
#undef GK_LAUNCH
}

// ---------------------------------------------------------------------------
// MFMA w4 grouped-expert GEMM: the w4a16_mfma structure (w4a16.hip) with
// expert gather.  Sub-ranges carry up to 32 tokens (max_tok=32 gating);
// idle MFMA columns for small cnt cost nothing — the win is dequantizing
// each weight ONCE regardless of token count (the VALU-bound scalar
// kernel paid ~38 VALU per word PER TOKEN).
// ---------------------------------------------------------------------------

#define MW_WAVES 4
#define MW_BLOCK (MW_WAVES * WAVE)
#define MW_MTOK 32
#define MW_NSL 8

// LDS-free (as the bf16 MFMA kernels above): the two B-fragment sets
// (tokens 0-15 / 16-31) are read straight from the L2-resident token
// rows — no staging barriers.  Dead-token columns (t >= cnt) read a
// clamped row and their outputs are never written.
template <int BITS>
__global__ __launch_bounds__(MW_BLOCK) void moe_w4_mfma_kernel(
    const short* __restrict__ x,          // [N, H] (or h [P, I])
    const unsigned int* __restrict__ wq,  // [E, O, H*BITS/32]
    const short* __restrict__ scales, const short* __restrict__ biases,
    short* __restrict__ y,                // [P, O] sorted pair order
    const int* __restrict__ sub_expert, const int* __restrict__ sub_off,
    const int* __restrict__ sub_cnt, const int* __restrict__ sorted_tok,
    int H, int O, int gs) {
  constexpr unsigned MASK = (1u << BITS) - 1u;
  const int s = blockIdx.y;
  const int e = sub_expert[s];
  const int p0 = sub_off[s];
  const int cnt = sub_cnt[s];
  if (cnt == 0) return;  // padded slot
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int words_per_row = H / (32 / BITS);

  const int row0 = (blockIdx.x * MW_WAVES + wid) * 16;
  if (row0 >= O) return;
  // two accumulators per output half, alternated by slice parity: PMC
  // showed 60% of wave cycles as ISSUE stalls (SQ_WAIT_INST_ANY) —
  // back-to-back MFMAs on one accumulator serialize on the dependent-
  // accumulator latency; parity-split chains double the dependency
  // distance.  Summed in the epilogue.
  float4v acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  float4v acc0b = {0, 0, 0, 0}, acc1b = {0, 0, 0, 0};
  const int wrow_r = min(row0 + (lane & 15), O - 1);
  const long ebase = (long)e * O;
  const unsigned int* wrow = wq + (ebase + wrow_r) * words_per_row;
  const short* srow = scales + (ebase + wrow_r) * (H / gs);
  const short* brow = biases + (ebase + wrow_r) * (H / gs);
  const short* xr0 = x + (long)sorted_tok[p0 + min(lane & 15, cnt - 1)] * H;
  const short* xr1 =
      x + (long)sorted_tok[p0 + min(16 + (lane & 15), cnt - 1)] * H;

  const int nsl_total = H / 32;  // binding requires H % 32 == 0
  int sl = 0;
  for (; sl + MW_NSL <= nsl_total; sl += MW_NSL) {
    unsigned int wbuf[MW_NSL * (BITS == 4 ? 1 : 2)];
    short sraw[MW_NSL], braw[MW_NSL];  // raw bf16: converting at
                                       // load-site forces a vmcnt wait
    bf16x8_t b0v[MW_NSL], b1v[MW_NSL];
#pragma unroll
    for (int i = 0; i < MW_NSL; ++i) {
      const int kk = (sl + i) * 32 + (lane >> 4) * 8;
      if (BITS == 4) {
        wbuf[i] = wrow[kk / 8];
      } else {
        wbuf[i * 2] = wrow[kk / 4];
        wbuf[i * 2 + 1] = wrow[kk / 4 + 1];
      }
      sraw[i] = srow[kk / gs];
      braw[i] = brow[kk / gs];
      b0v[i] = *reinterpret_cast<const bf16x8_t*>(xr0 + kk);
      b1v[i] = *reinterpret_cast<const bf16x8_t*>(xr1 + kk);
    }
    // dequant the WHOLE batch into registers first: a VALU-built A
    // fragment feeding its MFMA directly is a RAW issue-stall
    bf16x8_t afv[MW_NSL];
#pragma unroll
    for (int i = 0; i < MW_NSL; ++i) {
      const float sg = bfbits2f(sraw[i]);
      const float bg = bfbits2f(braw[i]);
      if (BITS == 4) {
        const unsigned int bits = wbuf[i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          afv[i][j] = (__bf16)(sg * (float)((bits >> (4 * j)) & MASK) + bg);
      } else {
        const unsigned int b0 = wbuf[i * 2];
        const unsigned int b1 = wbuf[i * 2 + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          afv[i][j] = (__bf16)(sg * (float)((b0 >> (8 * j)) & MASK) + bg);
          afv[i][4 + j] = (__bf16)(sg * (float)((b1 >> (8 * j)) & MASK) + bg);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MW_NSL; i += 2) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afv[i], b0v[i], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afv[i], b1v[i], acc1, 0, 0, 0);
      acc0b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afv[i + 1], b0v[i + 1],
                                                      acc0b, 0, 0, 0);
      acc1b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afv[i + 1], b1v[i + 1],
                                                      acc1b, 0, 0, 0);
    }
  }
  for (; sl < nsl_total; ++sl) {  // < MW_NSL leftover slices, once
    const int kk = sl * 32 + (lane >> 4) * 8;
    const float sg = bfbits2f(srow[kk / gs]);
    const float bg = bfbits2f(brow[kk / gs]);
    bf16x8_t af;
    if (BITS == 4) {
      const unsigned int bits = wrow[kk / 8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        af[j] = (__bf16)(sg * (float)((bits >> (4 * j)) & MASK) + bg);
    } else {
      const unsigned int b0 = wrow[kk / 4];
      const unsigned int b1 = wrow[kk / 4 + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        af[j] = (__bf16)(sg * (float)((b0 >> (8 * j)) & MASK) + bg);
        af[4 + j] = (__bf16)(sg * (float)((b1 >> (8 * j)) & MASK) + bg);
      }
    }
    bf16x8_t b0f = *reinterpret_cast<const bf16x8_t*>(xr0 + kk);
    bf16x8_t b1f = *reinterpret_cast<const bf16x8_t*>(xr1 + kk);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b0f, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b1f, acc1, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    acc0[r] += acc0b[r];
    acc1[r] += acc1b[r];
  }

#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int o = row0 + (lane >> 4) * 4 + reg;
    if (o < O) {
      const int t0 = lane & 15;
      if (t0 < cnt)
        y[(long)(p0 + t0) * O + o] = (short)__bfloat16_as_ushort(f2bf(acc0[reg]));
      if (t0 + 16 < cnt)
        y[(long)(p0 + t0 + 16) * O + o] =
            (short)__bfloat16_as_ushort(f2bf(acc1[reg]));
    }
  }
}

extern "C" void launch_moe_w4_mfma(const void* x, const void* wq,
                                   const void* scales, const void* biases,
                                   void* y, const int* sub_expert,
                                   const int* sub_off, const int* sub_cnt,
                                   const int* sorted_tok, int S, int H, int O,
                                   int gs, int bits, hipStream_t stream) {
  const int gx = (O + MW_WAVES * 16 - 1) / (MW_WAVES * 16);
  if (bits == 4)
    moe_w4_mfma_kernel<4><<<dim3(gx, S), dim3(MW_BLOCK), 0, stream>>>(
        (const short*)x, (const unsigned int*)wq, (const short*)scales,
        (const short*)biases, (short*)y, sub_expert, sub_off, sub_cnt,
        sorted_tok, H, O, gs);
  else
    moe_w4_mfma_kernel<8><<<dim3(gx, S), dim3(MW_BLOCK), 0, stream>>>(
        (const short*)x, (const unsigned int*)wq, (const short*)scales,
        (const short*)biases, (short*)y, sub_expert, sub_off, sub_cnt,
        sorted_tok, H, O, gs);
}
