// Fused MoE routing for prefill (N > 128 tokens): gate + stable expert
// sort + sub-range build in three launches, any number of blocks.
//
//   select  grid = ceil(N / MR_TB).  One wave per token at a time, the
//           per-token step of the decode gate.  Writes
//           indices[N, K] / weights[N, K] and the block's per-expert
//           histogram as one full row of blk_cnt[nb, E].
//   scan    one block.  Column e of blk_cnt becomes the exclusive
//           per-block offsets of expert e (in place) and yields counts[e];
//           then starts, max_count and the sub-range arrays.
//   place   grid = nb.  Pair (n, k) of expert e lands at
//           starts[e] + blk_cnt[b][e] + rank, rank = the number of earlier
//           tokens of the block that picked e.
//
// The order is the stable sort by expert of the flat pair list n*K + k
// (torch.argsort(indices.flatten(), stable=True)): blocks own consecutive
// token ranges, and a token's K experts are distinct, so "earlier pair of
// the same expert" is "earlier token that picked it".  place finds that
// rank from a 64-bit token mask per expert in LDS: one ds_or to build, one
// popcount to read, no walk over the pair list and no ordering left to an
// atomic's return value.
//
// No float atomics, no atomics on global memory, no memset, no host sync;
// every element of every output and of the workspace is written on every
// call, so the buffers come from torch::empty and the three launches can
// be captured in a graph.
//
// Limits (checked by the binding): E <= 256, K <= 8, N <= 262144 (4096
// blocks; every index fits an int with room to spare) and the group limits
// of moe_gate_subranges.

#include "hip_common.h"
#include "moe_gate_token.h"

#define MR_TB 64      // tokens per block: one bit each in the place masks
#define MR_WAVES 16   // select: 4 tokens per wave
#define MR_PLACE 256  // place threads: MR_TB * GK_MAXK / 256 = 2 pairs each
#define MR_SCAN 1024  // scan threads
#define MR_MAXSEG 16  // scan: row segments walked in parallel per expert

// Built without the packed-fp32 VALU forms, as the MLA kernels are.
#if defined(__HIP_DEVICE_COMPILE__)
#define MR_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define MR_NO_PK_F32
#endif

// The per-token step of moe_gate_subranges_kernel (moe.hip): the same
// arithmetic, tie rule (lowest index), sentinels and barrier-uniform group
// step.  It is a copy: calling one shared __device__ function from both
// kernels raised moe_gate_subranges_kernel<4, true> from 54 to 56 VGPRs
// (docs/PERFORMANCE.md), and the decode kernel is to stay as it is.
//
// One wave scores token t and picks its K experts.  Lane l holds experts
// l, 64+l, ... (R = ceil(E / 64) per lane).  Lane 0 writes pick k (in
// descending score order) to tok_e / tok_w[slot * GK_MAXK + k], the weight
// after norm_topk but before the routed scaling, and counts the expert in
// the LDS histogram `counts`.
//
// Every wave of the block must call it the same number of times: with
// n_group > 1 the group step barriers around the per-wave LDS row `row`
// (R * WAVE floats); `live` is false for the waves past the last token.
// grp[r] is the group of this lane's r-th expert, gsz = E / n_group.
template <int R, bool SIG>
__device__ __forceinline__ void mr_token_select(
    const short* __restrict__ logits, const float* __restrict__ e_bias, int t,
    bool live, int E, int K, int norm_topk, int n_group, int topk_group,
    int gsz, const int (&grp)[R], float* row, int* tok_e, float* tok_w,
    int slot, int* counts) {
  const int lane = threadIdx.x & (WAVE - 1);
  // masked, padded and already-picked entries: below any probability
  // (softmax), below any finite biased score (sigmoid; c can pass -1)
  constexpr float NEG = SIG ? -__builtin_inff() : -1.0f;

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
        if (r * WAVE + lane < E) row[r * WAVE + lane] = p[r];
    }
    __syncthreads();
    if (live) {
      // lane g scans group g for its max probability (SIG: the sum of
      // its two largest c); NEG marks lanes without a group and groups
      // already kept
      float gs = NEG;
      if (lane < n_group) {
        const float* grow = &row[lane * gsz];
        if constexpr (SIG) {
          float b1 = NEG, b2 = NEG;
          for (int j = 0; j < gsz; ++j) {
            const float v = grow[j];
            if (v > b1) { b2 = b1; b1 = v; }
            else if (v > b2) b2 = v;
          }
          gs = b1 + b2;  // gsz >= 2: both finite
        } else {
          gs = grow[0];
          for (int j = 1; j < gsz; ++j) gs = fmaxf(gs, grow[j]);
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
        tok_e[slot * GK_MAXK + k] = bidx;
        tok_w[slot * GK_MAXK + k] = best;
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
        tok_w[slot * GK_MAXK + k] /= (wsum + 1e-20f);
      }
    }
  }
}

template <int R, bool SIG>
__global__ __launch_bounds__(MR_WAVES * WAVE) MR_NO_PK_F32
void moe_route_select_kernel(
    const short* __restrict__ logits,  // [N, E] bf16
    const float* __restrict__ e_bias,  // [E] fp32 or null (SIG only)
    int* __restrict__ indices,         // [N, K]
    float* __restrict__ weights,       // [N, K]
    int* __restrict__ blk_cnt,         // [nb, E]
    int N, int E, int K, float routed_scaling, int norm_topk, int n_group,
    int topk_group, int wt_bf16) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;

  __shared__ int counts[GK_MAXE];             // the block's histogram
  __shared__ int tok_e[MR_TB * GK_MAXK];      // chosen expert per (slot, k)
  __shared__ float tok_w[MR_TB * GK_MAXK];    // chosen weight per (slot, k)
  __shared__ float probs[MR_WAVES][R * WAVE];  // per-wave row (group scan)

  // all GK_MAXE entries: the argmax of an all-masked row names a padded
  // lane, which must still land inside the array
  for (int i = threadIdx.x; i < GK_MAXE; i += blockDim.x) counts[i] = 0;
  __syncthreads();

  const int gsz = E / n_group;
  int grp[R];
#pragma unroll
  for (int r = 0; r < R; ++r) grp[r] = min(r * WAVE + lane, E - 1) / gsz;

  // fixed trip count: the group step barriers, and the rows past N of a
  // partial last block are simply not live
  const int t_base = blockIdx.x * MR_TB;
  for (int s0 = 0; s0 < MR_TB; s0 += MR_WAVES) {
    const int slot = s0 + wid;
    const int t = t_base + slot;
    mr_token_select<R, SIG>(logits, e_bias, t, t < N, E, K, norm_topk,
                            n_group, topk_group, gsz, grp, probs[wid], tok_e,
                            tok_w, slot, counts);
  }
  __syncthreads();

  const int n_live = min(MR_TB, N - t_base);
  for (int i = threadIdx.x; i < n_live * K; i += blockDim.x) {
    const int s = i / K, k = i % K;
    float w = tok_w[s * GK_MAXK + k] * routed_scaling;
    if (wt_bf16) w = bf2f(f2bf(w));  // RNE, what w.to(bfloat16) gives
    indices[(long)t_base * K + i] = tok_e[s * GK_MAXK + k];
    weights[(long)t_base * K + i] = w;
  }
  for (int e = threadIdx.x; e < E; e += blockDim.x)
    blk_cnt[(long)blockIdx.x * E + e] = counts[e];
}

__global__ __launch_bounds__(MR_SCAN) MR_NO_PK_F32 void moe_route_scan_kernel(
    int* __restrict__ blk_cnt,     // [nb, E] counts in, exclusive offsets out
    int* __restrict__ counts_out,  // [E]
    int* __restrict__ starts_out,  // [E + 1]
    int* __restrict__ max_count,   // [1]
    int* __restrict__ sub_expert,  // [s_upper]
    int* __restrict__ sub_off,     // [s_upper]
    int* __restrict__ sub_cnt,     // [s_upper]
    int nb, int E, int s_upper, int max_tok) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;

  __shared__ int seg_sum[MR_SCAN];       // [seg][e]
  __shared__ int counts[GK_MAXE];
  __shared__ int starts[GK_MAXE + 1];
  __shared__ int sub_base[GK_MAXE + 1];

  // thread (seg, e) owns rows [r0, r1) of column e; a row of blk_cnt is
  // read by E consecutive threads
  const int nseg = min(MR_MAXSEG, MR_SCAN / E);
  const int rps = (nb + nseg - 1) / nseg;
  const int seg = threadIdx.x / E;
  const int e = threadIdx.x - seg * E;
  const bool active = seg < nseg;
  const int r0 = min(nb, seg * rps), r1 = min(nb, r0 + rps);

  if (active) {
    int sum = 0;
    for (int r = r0; r < r1; ++r) sum += blk_cnt[(long)r * E + e];
    seg_sum[seg * E + e] = sum;
  }
  __syncthreads();
  if (active) {
    int run = 0, total = 0;
    for (int s = 0; s < nseg; ++s) {
      const int v = seg_sum[s * E + e];
      if (s < seg) run += v;
      total += v;
    }
    if (seg == 0) counts[e] = total;
    for (int r = r0; r < r1; ++r) {
      const int c = blk_cnt[(long)r * E + e];
      blk_cnt[(long)r * E + e] = run;
      run += c;
    }
  }
  __syncthreads();

  // pair offsets (wave 0), sub-range slot bases (wave 1), max (wave 2)
  if (wid == 0) gk_wave_prefix(counts, starts, E, 1, lane);
  if (wid == 1) gk_wave_prefix(counts, sub_base, E, max_tok, lane);
  if (wid == 2) {
    int m = 0;
    for (int i = lane; i < E; i += WAVE) m = max(m, counts[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, WAVE));
    if (lane == 0) max_count[0] = m;
  }
  __syncthreads();

  for (int i = threadIdx.x; i < E; i += blockDim.x) counts_out[i] = counts[i];
  for (int i = threadIdx.x; i <= E; i += blockDim.x) starts_out[i] = starts[i];

  // one thread per slot.  Expert e owns slots [sub_base[e], sub_base[e+1]);
  // an empty expert shares its base with its successor, so the owner of
  // slot i is the LAST e with sub_base[e] <= i.  Dead slots are zeroed.
  const int S = sub_base[E];
  for (int i = threadIdx.x; i < s_upper; i += blockDim.x) {
    int se = 0, so = 0, sc = 0;
    if (i < S) {
      int lo = 0, hi = E;  // invariant: sub_base[lo] <= i < sub_base[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (sub_base[mid] <= i) lo = mid; else hi = mid;
      }
      const int j = i - sub_base[lo];
      se = lo;
      so = starts[lo] + j * max_tok;
      sc = min(max_tok, counts[lo] - j * max_tok);
    }
    sub_expert[i] = se;
    sub_off[i] = so;
    sub_cnt[i] = sc;
  }
}

__global__ __launch_bounds__(MR_PLACE) MR_NO_PK_F32
void moe_route_place_kernel(
    const int* __restrict__ indices,    // [N, K]
    const float* __restrict__ weights,  // [N, K]
    const int* __restrict__ blk_off,    // [nb, E] exclusive offsets (scan)
    const int* __restrict__ starts,     // [E + 1]
    int* __restrict__ sorted_tok,       // [P]
    float* __restrict__ sorted_wt,      // [P]
    int* __restrict__ sorted_e,         // [P]
    int* __restrict__ pair_pos,         // [N, K]
    int N, int E, int K) {
  constexpr int PER = MR_TB * GK_MAXK / MR_PLACE;  // pairs per thread
  __shared__ unsigned tmask[GK_MAXE][MR_TB / 32];  // tokens that picked e

  for (int i = threadIdx.x; i < GK_MAXE * (MR_TB / 32); i += MR_PLACE)
    (&tmask[0][0])[i] = 0u;
  __syncthreads();

  const int t_base = blockIdx.x * MR_TB;
  const int n_pairs = min(MR_TB, N - t_base) * K;
  const long g0 = (long)t_base * K;  // flat index of the block's first pair

  int pe[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = j * MR_PLACE + threadIdx.x;
    pe[j] = -1;
    if (i < n_pairs) {
      const int e = indices[g0 + i];
      // select only emits e < E for finite logits; a NaN row may not
      if ((unsigned)e < (unsigned)E) {
        pe[j] = e;
        const int s = i / K;
        atomicOr(&tmask[e][s >> 5], 1u << (s & 31));
      }
    }
  }
  __syncthreads();

#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = j * MR_PLACE + threadIdx.x;
    const int e = pe[j];
    if (e < 0) continue;
    const int s = i / K;
    int rank = 0;
#pragma unroll
    for (int w = 0; w < MR_TB / 32; ++w) {
      const unsigned m = tmask[e][w];
      if (w < (s >> 5)) rank += __popc(m);
      else if (w == (s >> 5)) rank += __popc(m & ((1u << (s & 31)) - 1u));
    }
    const int pos = starts[e] + blk_off[(long)blockIdx.x * E + e] + rank;
    sorted_tok[pos] = t_base + s;
    sorted_wt[pos] = weights[g0 + i];
    sorted_e[pos] = e;
    pair_pos[g0 + i] = pos;
  }
}

extern "C" void launch_moe_route(
    const void* logits, const float* e_bias, int sigmoid, int* indices,
    float* weights, int* blk_cnt, int* counts, int* starts, int* max_count,
    int* sorted_tok, float* sorted_wt, int* sorted_e, int* pair_pos,
    int* sub_expert, int* sub_off, int* sub_cnt, int N, int E, int K,
    int s_upper, int max_tok, float routed_scaling, int norm_topk,
    int n_group, int topk_group, int wt_bf16, hipStream_t stream) {
  // limits are checked by the caller (bindings.hip::moe_route)
  const int nb = (N + MR_TB - 1) / MR_TB;
#define MR_LAUNCH(R, SIG)                                                    \
  moe_route_select_kernel<R, SIG>                                            \
      <<<dim3(nb), dim3(MR_WAVES * WAVE), 0, stream>>>(                      \
          (const short*)logits, e_bias, indices, weights, blk_cnt, N, E, K,  \
          routed_scaling, norm_topk, n_group, topk_group, wt_bf16)
#define MR_SWITCH(SIG)                                                       \
  switch ((E + WAVE - 1) / WAVE) {                                           \
    case 1: MR_LAUNCH(1, SIG); break;                                        \
    case 2: MR_LAUNCH(2, SIG); break;                                        \
    case 3: MR_LAUNCH(3, SIG); break;                                        \
    default: MR_LAUNCH(4, SIG); break;                                       \
  }
  if (sigmoid) {
    MR_SWITCH(true)
  } else {
    MR_SWITCH(false)
  }
#undef MR_SWITCH
#undef MR_LAUNCH
  moe_route_scan_kernel<<<dim3(1), dim3(MR_SCAN), 0, stream>>>(
      blk_cnt, counts, starts, max_count, sub_expert, sub_off, sub_cnt, nb, E,
      s_upper, max_tok);
  moe_route_place_kernel<<<dim3(nb), dim3(MR_PLACE), 0, stream>>>(
      indices, weights, blk_cnt, starts, sorted_tok, sorted_wt, sorted_e,
      pair_pos, N, E, K);
}
