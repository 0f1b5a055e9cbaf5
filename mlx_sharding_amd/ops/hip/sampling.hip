// Batched temperature / top-p sampling for continuous batching: one
// block per row of logits[B, V], reference.sample_rows semantics.
//
// The row does not fit LDS (517 KB at V = 129 280), so it is re-read
// from L2 over a fixed sequence of passes:
//   0. edits (logit_bias, repetition penalty) written back in place,
//      then a barrier;
//   1. max and argmax (lowest index on ties);
//   2. the two exponential sums: temperature 1 for lse_out, temperature
//      T for p;
//   3. the nucleus threshold: a bisection over the order-preserving
//      integer key of the logit's bits, <= 32 passes of "mass strictly
//      above t" (p is monotone in the logit, so the key orders p);
//   4. kept mass per wave chunk, then one wave scans its chunk in
//      vocabulary order to the pick.
// Every reduction combines in a fixed order (lane-strided partials, xor
// butterfly, ordered LDS sum) and there are no floating-point atomics:
// the same inputs give the same ids bit for bit on every run.  Every
// barrier is reached by the whole block; inactive rows leave before the
// first one.
#include "hip_common.h"

namespace {

constexpr int SAMPLE_BLOCK = 1024;
constexpr int SAMPLE_NW = SAMPLE_BLOCK / WAVE;

// order-preserving unsigned key of a float's bits
__device__ __forceinline__ unsigned int fkey(float x) {
  if (x == 0.0f) x = 0.0f;  // -0 and +0 are one tie class
  const unsigned int u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// (value, index) max with the lowest index on ties
__device__ __forceinline__ void argmax_combine(float& v, int& i, float ov,
                                               int oi) {
  if (ov > v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK)
sample_rows_kernel(float* logits, const float* __restrict__ temperature,
                   const float* __restrict__ top_p, const float* __restrict__ u,
                   const int* __restrict__ active, long long* __restrict__ ids_out,
                   long ids_stride, float* __restrict__ lse_out,
                   const int* __restrict__ bias_idx,
                   const float* __restrict__ bias_val, int NB,
                   const int* __restrict__ pen_idx,
                   const float* __restrict__ penalty, int W, int V) {
  constexpr int NW = BLOCK / WAVE;
  const int b = blockIdx.x;
  if (active[b] == 0) return;  // block-uniform, before the first barrier

  // one LDS object: [0, NW) float partials, [NW, 2NW) second partials
  __shared__ float smem[2 * NW];
  int* smem_i = reinterpret_cast<int*>(smem + NW);

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  float* x = logits + (long)b * V;

  // -- 0. edits -----------------------------------------------------------
  if (bias_idx != nullptr) {
    if (tid < NB) {
      const int k = bias_idx[(long)b * NB + tid];
      if (k >= 0 && k < V) x[k] += bias_val[(long)b * NB + tid];  // keys distinct
    }
    __syncthreads();
  }
  if (pen_idx != nullptr) {
    const float pen = penalty[b];
    if (tid < W && pen != 1.0f) {
      const int* row = pen_idx + (long)b * W;
      const int k = row[tid];
      bool first = k >= 0 && k < V;
      for (int j = 0; j < tid && first; ++j) first = row[j] != k;
      if (first) {  // once per distinct token
        const float v = x[k];
        x[k] = v > 0.0f ? __fdiv_rn(v, pen) : v * pen;
      }
    }
    __syncthreads();
  }

  // -- 1. max / argmax ------------------------------------------------------
  float mv = -INFINITY;
  int mi = 0;
  for (int i = tid; i < V; i += BLOCK) {
    const float v = x[i];
    if (v > mv) {  // increasing i: the lowest index of the thread's max
      mv = v;
      mi = i;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(mv, off, WAVE);
    const int oi = __shfl_xor(mi, off, WAVE);
    argmax_combine(mv, mi, ov, oi);
  }
  if (lane == 0) {
    smem[wid] = mv;
    smem_i[wid] = mi;
  }
  __syncthreads();
  mv = smem[0];
  mi = smem_i[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) argmax_combine(mv, mi, smem[w], smem_i[w]);
  __syncthreads();
  const float xmax = mv;
  const int amax = mi;

  // -- 2. exponential sums ----------------------------------------------------
  const float T = temperature[b];
  const bool greedy = !(T > 0.0f);
  const float inv_t = greedy ? 1.0f : __fdiv_rn(1.0f, T);
  float s1 = 0.0f, st = 0.0f;
  for (int i = tid; i < V; i += BLOCK) {
    const float d = x[i] - xmax;
    s1 += __expf(d);
    st += __expf(d * inv_t);
  }
  s1 = block_sum<BLOCK>(s1, smem);
  if (tid == 0) lse_out[b] = xmax + logf(s1);
  if (greedy) {
    if (tid == 0) ids_out[(long)b * ids_stride] = amax;
    return;  // block-uniform
  }
  st = block_sum<BLOCK>(st, smem);

  // -- 3. nucleus threshold ---------------------------------------------------
  // smallest key k with mass{key(x_j) > k} < top_p * st; the top class
  // is kept whatever top_p is (hi starts at its key).  The tree sum is
  // monotone in its inputs, so the predicate is monotone in k.
  const float tp = top_p[b];
  unsigned int kstar = 0u;
  if (tp < 1.0f) {
    const float target = tp * st;
    unsigned int lo = 0u, hi = fkey(xmax);
    while (lo < hi) {  // block-uniform: m comes out of LDS
      const unsigned int mid = lo + ((hi - lo) >> 1);
      float m = 0.0f;
      for (int i = tid; i < V; i += BLOCK) {
        const float v = x[i];
        const float e = __expf((v - xmax) * inv_t);
        m += fkey(v) > mid ? e : 0.0f;
      }
      m = block_sum<BLOCK>(m, smem);
      if (m < target) hi = mid; else lo = mid + 1u;
    }
    kstar = hi;
  }

  // -- 4. kept mass per wave chunk, then the pick ----------------------------
  const int chunk = (V + NW - 1) / NW;
  const int c0 = min(V, wid * chunk);
  const int c1 = min(V, c0 + chunk);
  float ws = 0.0f;
  int wc = 0;
  for (int i = c0 + lane; i < c1; i += WAVE) {
    const float v = x[i];
    if (fkey(v) >= kstar) {
      ws += __expf((v - xmax) * inv_t);
      ++wc;
    }
  }
  ws = wave_sum(ws);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) wc += __shfl_xor(wc, off, WAVE);
  if (lane == 0) {
    smem[wid] = ws;
    smem_i[wid] = wc;
  }
  __syncthreads();  // the last barrier
  float Z = 0.0f;
#pragma unroll
  for (int w = 0; w < NW; ++w) Z += smem[w];
  float target = u[b] * Z;
  int wsel = -1, wlast = -1;
  float base = 0.0f, run = 0.0f;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const float nxt = run + smem[w];
    if (wsel < 0 && nxt > target && smem_i[w] > 0) {
      wsel = w;
      base = run;
    }
    if (smem_i[w] > 0) wlast = w;
    run = nxt;
  }
  if (wsel < 0) {  // rounding left none: the chunk of the last kept index
    wsel = wlast;
    target = INFINITY;  // nothing crosses; the scan only finds the last kept
  }
  if (wid != wsel) return;  // wave-uniform; no barrier follows
  // (wlast < 0 cannot happen for finite rows: the top class is kept.  A
  // row of NaNs keeps nothing; every wave leaves and ids_out stays.)

  int pick = -1, last_kept = amax;
  float running = base;
  for (int t0 = c0; t0 < c1 && pick < 0; t0 += WAVE) {
    const int i = t0 + lane;
    float e = 0.0f;
    bool kept = false;
    if (i < c1) {
      const float v = x[i];
      kept = fkey(v) >= kstar;
      if (kept) e = __expf((v - xmax) * inv_t);
    }
    float s = e;  // inclusive scan in vocabulary order
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const float o = __shfl_up(s, off, WAVE);
      if (lane >= off) s += o;
    }
    const unsigned long long keptm = __ballot(kept);
    const unsigned long long cross = __ballot(kept && (running + s > target));
    if (cross) {
      pick = t0 + (int)__ffsll((long long)cross) - 1;
    } else {
      if (keptm) last_kept = t0 + 63 - __clzll((long long)keptm);
      running += __shfl(s, WAVE - 1, WAVE);
    }
  }
  if (pick < 0) pick = last_kept;
  if (lane == 0) ids_out[(long)b * ids_stride] = pick;
}

}  // namespace

extern "C" void launch_sample_rows(float* logits, const float* temperature,
                                   const float* top_p, const float* u,
                                   const int* active, long long* ids_out,
                                   long ids_stride, float* lse_out,
                                   const int* bias_idx, const float* bias_val,
                                   int NB, const int* pen_idx,
                                   const float* penalty, int W, int B, int V,
                                   hipStream_t stream) {
  if (B <= 0) return;
  hipLaunchKernelGGL(sample_rows_kernel<SAMPLE_BLOCK>, dim3(B),
                     dim3(SAMPLE_BLOCK), 0, stream, logits, temperature,
                     top_p, u, active, ids_out, ids_stride, lse_out, bias_idx,
                     bias_val, NB, pen_idx, penalty, W, V);
  HIP_CHECK_LAST();
}

extern "C" int sample_rows_chunks() { return SAMPLE_NW; }
