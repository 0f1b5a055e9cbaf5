// Python bindings for the gfx950 kernel library (torch extension).
// Pure HIP tree — no CUDA shims; built by hipcc via torch cpp_extension
// with PYTORCH_ROCM_ARCH=gfx950.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "hip_common.h"

extern "C" {
void launch_rms_norm(const void*, void*, const void*, long, int, float, float,
                     long, hipStream_t);
void launch_rms_norm_residual(const void*, const void*, void*, void*,
                              const void*, long, int, float, float, void*,
                              hipStream_t);
void launch_mla_decode_prep(const void*, const void*, const void*,
                            const float*, const float*, void*, void*, void*,
                            const int*, int, int, int, int, int, int, int,
                            long, long, long, long, long, float, float,
                            hipStream_t);
void launch_moe_finalize(const float*, const void*, const void*, void*, long,
                         hipStream_t);
void launch_glu(const void*, const void*, void*, long, bool, hipStream_t);
void launch_glu_strided(const void*, const void*, void*, long, int, long,
                        long, bool, hipStream_t);
void launch_softcap(const void*, void*, long, float, hipStream_t);
void launch_rope(const void*, void*, const float*, const float*, long, int,
                 int, int, bool, long, long, long, hipStream_t);
void launch_mla_append_kv(const void*, const void*, void*, void*, const int*,
                          int, int, int, int, int, int, int, int, long, long,
                          hipStream_t);
void launch_rope_append_kv(const void*, const void*, const float*,
                           const float*, void*, void*, const int*, int, int,
                           int, int, int, int, long, bool, long, long, long,
                           hipStream_t);
void launch_attn_decode(const void*, const void*, const void*, const void*,
                        void*, float*, float*, int, const int*, int, int, int,
                        int, int, long, int, int, long, float, float, int,
                        int, long, long, long, long, long, long, hipStream_t);
bool attn_decode_supported_shape(int, int);
void launch_attn_prefill(const void*, const void*, const void*, void*, int,
                         int, int, int, int, long, long, int, int, float,
                         float, int, int, hipStream_t);
bool attn_prefill_supported(int, int);
void launch_mfma_probe(const void*, const void*, float*, hipStream_t);
void launch_w4a16_gemv(const void*, const void*, const void*, const void*,
                       void*, int, int, int, int, int, hipStream_t);
int w4a16_mfma_nsplit(int, int, int);
void launch_bf16_gemv_mfma(const void*, const void*, void*, float*, int, int,
                           int, int, hipStream_t);
int bf16_gemv_nsplit(int, int, int);
void launch_bf16_gemm_m64(const void*, const void*, void*, float*, int, int,
                          int, int, hipStream_t);
int bf16_gemm_m64_nsplit(int, int, int);
void launch_w4a16_mfma(const void*, const void*, const void*, const void*,
                       void*, float*, int, int, int, int, int, int,
                       hipStream_t);
void launch_dequant(const void*, const void*, const void*, void*, long, int,
                    int, int, hipStream_t);
void launch_moe_scatter_rows(const void*, void*, const int*, const int*, int,
                             int, hipStream_t);
void launch_moe_gather_reduce(const void*, const int*, const float*, void*,
                              int, int, int, hipStream_t);
void launch_moe_gateup_mfma(const void*, const void*, const void*, void*,
                            const int*, const int*, const int*, const int*,
                            int, int, int, hipStream_t);
void launch_moe_down_mfma(const void*, const void*, float*, const int*,
                          const int*, const int*, const int*, const float*,
                          int, int, int, hipStream_t);
void launch_moe_gateup_grouped(const void*, const void*, const void*, void*,
                               const int*, const int*, const int*, const int*,
                               int, int, int, hipStream_t);
void launch_moe_down_grouped(const void*, const void*, float*, const int*,
                             const int*, const int*, const int*, const float*,
                             int, int, int, hipStream_t);
void launch_moe_w4_mfma(const void*, const void*, const void*, const void*,
                        void*, const int*, const int*, const int*,
                        const int*, int, int, int, int, int, hipStream_t);
void launch_moe_gate_subranges(const void*, const float*, int, int*, float*,
                               int*, int*, int*, int, int, int, int, int,
                               float, int, int, int, hipStream_t);
void launch_moe_w4f16_gateup(const void*, const void*, const void*,
                             const void*, const void*, const void*,
                             const void*, void*, const int*, const int*,
                             const int*, const int*, int, int, int, int, int,
                             float*, long, hipStream_t);
void launch_moe_w4f16_down(const void*, const void*, const void*, const void*,
                           float*, const int*, const int*, const int*,
                           const int*, const float*, int, int, int, int, int,
                           hipStream_t);
void launch_w4f16_gemv(const void*, const void*, const void*, const void*,
                       void*, float*, int, int, int, int, int, int,
                       hipStream_t);
int w4f16_gemv_nsplit(int, int, int);
void launch_fp8_block_dequant(const void*, const float*, void*, long, int, int,
                              hipStream_t);
void launch_fp8f16_gemv(const void*, const void*, const float*, void*, float*,
                        int, int, int, int, hipStream_t);
int fp8f16_gemv_nsplit(int, int, int);
void launch_moe_fp8f16_gateup(const void*, const void*, const void*,
                              const float*, const float*, void*, const int*,
                              const int*, const int*, const int*, int, int,
                              int, float*, long, hipStream_t);
void launch_moe_fp8f16_down(const void*, const void*, const float*, float*,
                            const int*, const int*, const int*, const int*,
                            const float*, int, int, int, hipStream_t);
int moe_fp8f16_wide_tile();
void launch_moe_fp8f16_gateup_wide(const void*, const void*, const void*,
                                   const float*, const float*, void*,
                                   const int*, const int*, const int*,
                                   const int*, int, int, int, hipStream_t);
void launch_moe_fp8f16_down_wide(const void*, const void*, const float*,
                                 float*, const int*, const int*, const int*,
                                 const int*, const float*, int, int, int,
                                 hipStream_t);
void launch_sample_rows(float*, const float*, const float*, const float*,
                        const int*, long long*, long, float*, const int*,
                        const float*, int, const int*, const float*, int, int,
                        int, hipStream_t);
void launch_gemm_kseg(const void*, const void*, void*, void*, int, int, int,
                      int, hipStream_t);
void launch_gemm_kseg_w4(const void*, const void*, const void*, const void*,
                         void*, void*, int, int, int, int, int, hipStream_t);
}

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
}

// View t as [rows, last-dim] with a uniform row stride (a fused-output
// column-slice view qualifies) — lets kernels read split views in place
// instead of the binding materializing a .contiguous() copy per call.
bool row_view2(const torch::Tensor& t, long& rows, long& rstride) {
  const int d = t.dim();
  if (d < 2 || t.stride(d - 1) != 1) return false;
  if (d == 2) {
    rows = t.size(0);
    rstride = t.stride(0);
    return true;
  }
  if (d == 3) {
    if (t.stride(0) != t.size(1) * t.stride(1)) return false;
    rows = t.size(0) * t.size(1);
    rstride = t.stride(1);
    return true;
  }
  return false;
}

// Optional fp32 split-K scratch [M, O]: allocated only when the launcher
// will split (nk > 1); otherwise undefined, and the launcher gets null.
torch::Tensor splitk_scratch(int nk, int M, int O,
                             const torch::TensorOptions& opts) {
  if (nk <= 1) return torch::Tensor();
  return torch::empty({M, O}, opts.dtype(torch::kFloat32));
}

// Device decode position: int32 [1] (every batch row at the same
// position) or int32 [B] (row b at pos[b] — ragged batched decode).
// Returns the pointer and sets the per-row element stride (0 or 1).
const int* pos_arg(const c10::optional<torch::Tensor>& pos, int B,
                   int& bstride) {
  bstride = 0;
  if (!pos.has_value()) return nullptr;
  TORCH_CHECK(pos->is_cuda() && pos->scalar_type() == torch::kInt32 &&
                  pos->is_contiguous(),
              "pos must be a contiguous int32 GPU tensor");
  const long n = pos->numel();
  TORCH_CHECK(n == 1 || n == B, "pos must hold 1 or B=", B,
              " positions, got ", n);
  bstride = (n == 1) ? 0 : 1;
  return pos->data_ptr<int>();
}

// cos/sin tables: [T, D/2] shared by every batch row, or [B, T, D/2]
// per sequence.  Returns the per-row element stride (0 when shared).
long rope_table_bstride(const torch::Tensor& cc, const torch::Tensor& sc,
                        int B, int T, int half) {
  TORCH_CHECK(cc.scalar_type() == torch::kFloat32 &&
                  sc.scalar_type() == torch::kFloat32, "cos/sin must be fp32");
  TORCH_CHECK(sc.sizes() == cc.sizes(), "cos/sin shape mismatch");
  if (cc.dim() == 3) {
    TORCH_CHECK(cc.size(0) == B && cc.size(1) == T && cc.size(2) == half,
                "cos shape mismatch: want [B, T, D/2]");
    return (long)T * half;
  }
  TORCH_CHECK(cc.dim() == 2 && cc.size(0) == T && cc.size(1) == half,
              "cos shape mismatch: want [T, D/2]");
  return 0;
}

float* f32_or_null(const torch::Tensor& t) {
  return t.defined() ? t.data_ptr<float>() : nullptr;
}

torch::Tensor rms_norm(torch::Tensor x, torch::Tensor w, double eps,
                       double w_off) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  const int H = x.size(-1);
  TORCH_CHECK(H % 4 == 0, "H must be divisible by 4");
  long rows, rstride;
  torch::Tensor xv = x;
  if (!row_view2(x, rows, rstride) || rstride % 4 != 0
      || ((uintptr_t)x.data_ptr()) % 8 != 0) {  // short4v-aligned rows
    xv = x.contiguous();
    rows = xv.numel() / H;
    rstride = H;
  }
  auto y = torch::empty(x.sizes(), x.options());
  launch_rms_norm(xv.data_ptr(), y.data_ptr(), w.contiguous().data_ptr(), rows,
                  H, (float)eps, (float)w_off, rstride, cur_stream());
  return y;
}

// with_f16: also return fp16(y) — bit-identical to y.to(float16) — as a
// third tensor, written by the same launch
std::vector<torch::Tensor> rms_norm_residual(torch::Tensor x,
                                             torch::Tensor resid,
                                             torch::Tensor w, double eps,
                                             double w_off, bool with_f16) {
  check_bf16(x, "x");
  auto xc = x.contiguous();
  auto rc = resid.contiguous();
  const int H = xc.size(-1);
  long rows = xc.numel() / H;
  auto y = torch::empty_like(xc);
  auto h = torch::empty_like(xc);
  torch::Tensor y16;
  if (with_f16) y16 = torch::empty_like(xc, xc.options().dtype(torch::kHalf));
  launch_rms_norm_residual(xc.data_ptr(), rc.data_ptr(), y.data_ptr(),
                           h.data_ptr(), w.contiguous().data_ptr(), rows, H,
                           (float)eps, (float)w_off,
                           with_f16 ? y16.data_ptr() : nullptr, cur_stream());
  if (with_f16) return {y, h, y16};
  return {y, h};
}

// Absorbed-MLA decode prep (T == 1), one launch: RMS-normalise c_kv, rope
// k_pe, store the [c_kv | k_pe] row into the compressed cache at the
// position, rope every head's q_pe, and lay q_nope out head-major for
// the W_UK bmm.
//   qh [B, 1, nh, nope+rope] and ckv [B, 1, rank+rope]: contiguous or
//   split views of a wider buffer;  cache [B, 1, Scap, rank+rope]
// Returns (q_pe [B, nh, rope], q_nope [nh, B, nope]).
std::vector<torch::Tensor> mla_decode_prep(
    torch::Tensor qh, torch::Tensor ckv, torch::Tensor w, double eps,
    double w_off, torch::Tensor cos, torch::Tensor sin, torch::Tensor cache,
    int64_t rope, c10::optional<torch::Tensor> pos, int64_t pos0) {
  check_bf16(qh, "qh");
  check_bf16(ckv, "ckv");
  check_bf16(w, "w");
  check_bf16(cache, "cache");
  TORCH_CHECK(qh.dim() == 4 && qh.size(1) == 1, "qh must be [B, 1, nh, D]");
  TORCH_CHECK(ckv.dim() == 3 && ckv.size(1) == 1 && ckv.size(0) == qh.size(0),
              "ckv must be [B, 1, rank+rope]");
  const int B = qh.size(0), nh = qh.size(2);
  const int nope = qh.size(3) - rope;
  const int rank = ckv.size(2) - rope;
  TORCH_CHECK(rope >= 2 && rope % 2 == 0 && nope >= 8 && nope % 8 == 0 &&
                  rank >= 4 && rank % 4 == 0,
              "mla_decode_prep needs rope % 2 == 0, nope % 8 == 0, "
              "rank % 4 == 0 (got rope=", rope, ", nope=", nope, ", rank=",
              rank, ")");
  TORCH_CHECK(w.numel() == rank, "norm weight must hold rank elements");
  TORCH_CHECK(cache.dim() == 4 && cache.is_contiguous() &&
                  cache.size(0) == B && cache.size(1) == 1 &&
                  cache.size(3) == rank + rope,
              "cache must be contiguous [B, 1, Scap, rank+rope]");
  const long Scap = cache.size(2);
  auto cc = cos.contiguous();
  auto sc = sin.contiguous();
  const long csb = rope_table_bstride(cc, sc, B, 1, rope / 2);
  int pbs;
  const int* pp = pos_arg(pos, B, pbs);
  if (!pp)
    TORCH_CHECK(pos0 >= 0 && pos0 < Scap, "position ", pos0,
                " outside the cache capacity ", Scap);
  // split views read in place when rows keep the vector alignment the
  // kernel loads with (16 B for q_nope, 8 B for c_kv)
  torch::Tensor qv = qh, cv = ckv;
  if (!(qh.stride(3) == 1 && qh.stride(1) % 8 == 0 && qh.stride(2) % 8 == 0 &&
        (B == 1 || qh.stride(0) % 8 == 0) &&
        ((uintptr_t)qh.data_ptr()) % 16 == 0))
    qv = qh.contiguous();
  if (!(ckv.stride(2) == 1 && (B == 1 || ckv.stride(0) % 4 == 0) &&
        ((uintptr_t)ckv.data_ptr()) % 8 == 0))
    cv = ckv.contiguous();
  auto q_pe = torch::empty({B, nh, rope}, qh.options());
  auto q_nope = torch::empty({nh, B, nope}, qh.options());
  launch_mla_decode_prep(qv.data_ptr(), cv.data_ptr(),
                         w.contiguous().data_ptr(), cc.data_ptr<float>(),
                         sc.data_ptr<float>(), cache.data_ptr(),
                         q_pe.data_ptr(), q_nope.data_ptr(), pp, pbs,
                         (int)pos0, B, nh, nope, (int)rope, rank, Scap,
                         qv.stride(0), qv.stride(2), cv.stride(0), csb,
                         (float)eps, (float)w_off, cur_stream());
  return {q_pe, q_nope};
}

// out = h + (bf16(acc) + shared), each step rounded to bf16 as the
// unfused acc.to(bf16) / y + shared / h + mlp sequence rounds it
torch::Tensor moe_finalize(torch::Tensor acc, c10::optional<torch::Tensor> shared,
                           torch::Tensor h) {
  check_bf16(h, "h");
  TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == torch::kFloat32 &&
                  acc.is_contiguous(), "acc must be contiguous fp32 on GPU");
  TORCH_CHECK(h.numel() == acc.numel(), "h/acc size mismatch");
  auto hc = h.contiguous();
  torch::Tensor sc;
  if (shared.has_value()) {
    check_bf16(*shared, "shared");
    TORCH_CHECK(shared->numel() == acc.numel(), "shared/acc size mismatch");
    sc = shared->contiguous();
  }
  auto out = torch::empty(h.sizes(), hc.options());
  launch_moe_finalize(acc.data_ptr<float>(),
                      sc.defined() ? sc.data_ptr() : nullptr, hc.data_ptr(),
                      out.data_ptr(), acc.numel(), cur_stream());
  return out;
}

torch::Tensor glu(torch::Tensor gate, torch::Tensor up, bool gelu) {
  check_bf16(gate, "gate");
  TORCH_CHECK(gate.numel() == up.numel(), "gate/up size mismatch");
  TORCH_CHECK(gate.numel() % 4 == 0, "numel must be divisible by 4");
  const int I = gate.size(-1);
  long growz, gstride, urows, ustride;
  // fused gate|up split views read in place (no .contiguous() copies)
  if (!(gate.is_contiguous() && up.is_contiguous())
      && row_view2(gate, growz, gstride) && row_view2(up, urows, ustride)
      && growz == urows && up.size(-1) == I && I % 4 == 0
      && gstride % 4 == 0 && ustride % 4 == 0
      && ((uintptr_t)gate.data_ptr()) % 8 == 0
      && ((uintptr_t)up.data_ptr()) % 8 == 0) {
    auto y = torch::empty(gate.sizes(), gate.options());
    launch_glu_strided(gate.data_ptr(), up.data_ptr(), y.data_ptr(), growz, I,
                       gstride, ustride, gelu, cur_stream());
    return y;
  }
  auto g = gate.contiguous();
  auto u = up.contiguous();
  auto y = torch::empty_like(g);
  launch_glu(g.data_ptr(), u.data_ptr(), y.data_ptr(), g.numel(), gelu,
             cur_stream());
  return y;
}

torch::Tensor softcap_op(torch::Tensor x, double cap) {
  check_bf16(x, "x");
  auto xc = x.contiguous();
  TORCH_CHECK(xc.numel() % 4 == 0, "numel must be divisible by 4");
  auto y = torch::empty_like(xc);
  launch_softcap(xc.data_ptr(), y.data_ptr(), xc.numel(), (float)cap,
                 cur_stream());
  return y;
}

// x: [B, T, nH, D]; cos/sin: [T, D/2] or [B, T, D/2] fp32
torch::Tensor apply_rope(torch::Tensor x, torch::Tensor cos, torch::Tensor sin,
                         bool interleaved) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, "x must be [B, T, nH, D]");
  auto cc = cos.contiguous();
  auto sc = sin.contiguous();
  const int B = x.size(0), T = x.size(1), nH = x.size(2), D = x.size(3);
  const long csb = rope_table_bstride(cc, sc, B, T, D / 2);
  // fused-qkv splits / nope-rope slices read in place
  torch::Tensor xv = x;
  long rstride = (long)nH * D, hstride = D;
  const bool strided_ok = x.stride(3) == 1
      && x.stride(0) == x.size(1) * x.stride(1);
  if (strided_ok) {
    rstride = x.stride(1);
    hstride = x.stride(2);
  } else {
    xv = x.contiguous();
  }
  auto y = torch::empty({B, T, nH, D}, x.options());
  launch_rope(xv.data_ptr(), y.data_ptr(), cc.data_ptr<float>(),
              sc.data_ptr<float>(), (long)B * T, T, nH, D, interleaved,
              rstride, hstride, csb, cur_stream());
  return y;
}

// k/v [B, T, Hkv, D]; caches full buffers [B, Hkv, Scap, D]
void rope_append_kv(torch::Tensor k, torch::Tensor v, torch::Tensor cos,
                    torch::Tensor sin, torch::Tensor kcache,
                    torch::Tensor vcache, c10::optional<torch::Tensor> pos,
                    int64_t pos0, bool interleaved) {
  check_bf16(k, "k");
  TORCH_CHECK(k.dim() == 4, "k must be [B, T, Hkv, D]");
  auto cc = cos.contiguous();
  auto sc = sin.contiguous();
  const int B = k.size(0), T = k.size(1), Hkv = k.size(2), D = k.size(3);
  TORCH_CHECK(D % 2 == 0, "head dim must be even");
  const long csb = rope_table_bstride(cc, sc, B, T, D / 2);
  TORCH_CHECK(kcache.is_contiguous() && vcache.is_contiguous(),
              "caches contiguous");
  TORCH_CHECK(kcache.size(3) == D && vcache.size(3) == D, "cache D mismatch");
  const long Scap = kcache.size(2);
  int pbs;
  const int* pp = pos_arg(pos, B, pbs);
  // fused-qkv split views read in place (heads contiguous within slice)
  auto view_ok = [&](const torch::Tensor& t) {
    return t.stride(3) == 1 && t.stride(2) == D
        && t.stride(0) == t.size(1) * t.stride(1);
  };
  torch::Tensor kv = k, vv = v;
  long krs = (long)Hkv * D, vrs = (long)Hkv * D;
  if (view_ok(k)) krs = k.stride(1); else kv = k.contiguous();
  if (view_ok(v)) vrs = v.stride(1); else vv = v.contiguous();
  launch_rope_append_kv(kv.data_ptr(), vv.data_ptr(), cc.data_ptr<float>(),
                        sc.data_ptr<float>(), kcache.data_ptr(),
                        vcache.data_ptr(), pp, pbs, (int)pos0, B, T, Hkv, D,
                        Scap, interleaved, krs, vrs, csb, cur_stream());
}

// kvh [B, T, nh, nope+vd]; kpe [B, T, rope]; caches full buffers
void mla_append_kv(torch::Tensor kvh, torch::Tensor kpe, torch::Tensor kcache,
                   torch::Tensor vcache, c10::optional<torch::Tensor> pos,
                   int64_t pos0) {
  check_bf16(kvh, "kvh");
  const int B = kvh.size(0), T = kvh.size(1), nh = kvh.size(2);
  const int rope = kpe.size(-1);
  const int kd = kcache.size(3);
  const int vd = vcache.size(3);
  const int nope = kd - rope;
  TORCH_CHECK(kvh.size(3) == nope + vd, "kvh dim mismatch");
  TORCH_CHECK(kcache.is_contiguous() && vcache.is_contiguous(), "caches contiguous");
  const long Scap = kcache.size(2);
  int pbs;
  const int* pp = pos_arg(pos, B, pbs);
  long kpe_rows, kpe_rs;
  torch::Tensor kpev = kpe;
  if (!row_view2(kpe, kpe_rows, kpe_rs)) {
    kpev = kpe.contiguous();
    kpe_rs = rope;
  }
  launch_mla_append_kv(kvh.contiguous().data_ptr(), kpev.data_ptr(),
                       kcache.data_ptr(), vcache.data_ptr(), pp, pbs,
                       (int)pos0, B, T, nh, nope, vd, rope, Scap, kpe_rs,
                       cur_stream());
}

// Shared body of attn_decode / attn_decode_split.
// qn: [B, Hq, Dk - Dr] view (any batch/head strides, unit last stride);
// qr: [B, Hq, Dr] view or undefined (Dr = 0).  head_major lays the
// output out as [Hq, B, Dv] (the W_UV bmm operand) instead of
// [B, Hq, 1, Dv].
torch::Tensor attn_decode_impl(const torch::Tensor& qn, const torch::Tensor& qr,
                               torch::Tensor k, torch::Tensor v, double scale,
                               double softcap, int64_t window,
                               c10::optional<torch::Tensor> pos,
                               bool head_major) {
  check_bf16(k, "k");
  const torch::Tensor& qc = qn;
  const int Dr = qr.defined() ? (int)qr.size(2) : 0;
  const int B = qn.size(0), Hq = qn.size(1), Dk = qn.size(2) + Dr;
  const int Hkv = k.size(1), S = k.size(2);
  const int Dv = v.size(3);
  TORCH_CHECK(k.stride(3) == 1 && v.stride(3) == 1, "K/V rows must be contiguous");
  TORCH_CHECK(k.stride(2) == Dk, "K seq stride mismatch");
  // V rows may live inside the K rows (absorbed MLA: V = K[..., :Dv])
  const long vstride = v.stride(2);
  TORCH_CHECK(vstride >= Dv, "V seq stride too small");
  TORCH_CHECK(Hq % Hkv == 0, "Hq must be divisible by Hkv");
  TORCH_CHECK(Dk % 8 == 0, "Dk must be a multiple of 8");
  TORCH_CHECK(attn_decode_supported_shape(Hq / Hkv, Dv),
              "unsupported GQA ratio/Dv ", Hq / Hkv, " ", Dv);
  TORCH_CHECK(Dv <= 512, "Dv too large");
  long kScap = k.stride(1) / Dk;
  long vScap = v.stride(1) / vstride;
  TORCH_CHECK(kScap == vScap, "K/V capacity mismatch");
  auto out = head_major ? torch::empty({Hq, B, Dv}, qc.options())
                        : torch::empty({B, Hq, 1, Dv}, qc.options());
  const long o_bs = head_major ? Dv : (long)Hq * Dv;
  const long o_hs = head_major ? (long)B * Dv : Dv;
  int sbs;
  const int* s_ptr = pos_arg(pos, B, sbs);
  // split-S for parallelism: target ~1024 blocks, slices of >= 512 keys
  // (>= 256 keys when B*Hkv alone leaves the chip block-starved, e.g.
  // absorbed MLA with Hkv = 1)
  long span = s_ptr ? kScap : (long)S;
  long slice = (B * Hkv <= 64) ? 256 : 512;
  int nsplit = (int)std::min<long>(
      std::min<long>(8, std::max<long>(1, 1024 / std::max(1, B * Hkv))),
      std::max<long>(1, (span + slice - 1) / slice));
  float* part_o = nullptr;
  float* part_ml = nullptr;
  torch::Tensor po, pml;
  if (nsplit > 1) {
    auto fopts = qc.options().dtype(torch::kFloat32);
    po = torch::empty({(long)B * Hq * nsplit * Dv}, fopts);
    pml = torch::empty({(long)B * Hq * nsplit * 2}, fopts);
    part_o = po.data_ptr<float>();
    part_ml = pml.data_ptr<float>();
  }
  launch_attn_decode(qn.data_ptr(), Dr ? qr.data_ptr() : nullptr,
                     k.data_ptr(), v.data_ptr(), out.data_ptr(), part_o,
                     part_ml, nsplit, s_ptr, sbs, B, Hq, Hkv, S, kScap, Dk,
                     Dv, vstride, (float)scale, (float)softcap, (int)window,
                     Dr, qn.stride(0), qn.stride(1), Dr ? qr.stride(0) : 0,
                     Dr ? qr.stride(1) : 0, o_bs, o_hs, cur_stream());
  return out;
}

// q [B, Hq, 1, Dk]; k/v: cache views [B, Hkv, S, D] with row-contiguous
// last dim over a [B, Hkv, Scap, D] buffer.
torch::Tensor attn_decode(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                          double scale, double softcap, int64_t window,
                          c10::optional<torch::Tensor> pos) {
  check_bf16(q, "q");
  TORCH_CHECK(q.dim() == 4 && q.size(2) == 1, "attn_decode needs Tq == 1");
  auto qc = q.contiguous();
  return attn_decode_impl(qc.view({qc.size(0), qc.size(1), qc.size(3)}),
                          torch::Tensor(), k, v, scale, softcap, window, pos,
                          false);
}

// Two-source q (absorbed MLA): q_nope [B, Hq, Dk - Dr] and q_rope
// [B, Hq, Dr], both read in place through their (batch, head) strides;
// returns [Hq, B, Dv].
torch::Tensor attn_decode_split(torch::Tensor q_nope, torch::Tensor q_rope,
                                torch::Tensor k, torch::Tensor v, double scale,
                                double softcap, int64_t window,
                                c10::optional<torch::Tensor> pos) {
  check_bf16(q_nope, "q_nope");
  check_bf16(q_rope, "q_rope");
  TORCH_CHECK(q_nope.dim() == 3 && q_rope.dim() == 3 &&
                  q_nope.size(0) == q_rope.size(0) &&
                  q_nope.size(1) == q_rope.size(1) && q_rope.size(2) > 0,
              "q_nope/q_rope must be [B, Hq, *] with matching B, Hq");
  TORCH_CHECK(q_nope.stride(2) == 1 && q_rope.stride(2) == 1,
              "q rows must be contiguous");
  return attn_decode_impl(q_nope, q_rope, k, v, scale, softcap, window, pos,
                          true);
}

// q [B, Hq, T, Dk]; k/v cache views [B, Hkv, S, D] (row-contiguous)
torch::Tensor attn_prefill(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                           double scale, double softcap, int64_t window,
                           int64_t causal_offset) {
  check_bf16(q, "q");
  auto qc = q.contiguous();
  const int B = qc.size(0), Hq = qc.size(1), T = qc.size(2), Dk = qc.size(3);
  const int Hkv = k.size(1), S = k.size(2), Dv = v.size(3);
  TORCH_CHECK(k.stride(3) == 1 && v.stride(3) == 1, "K/V rows must be contiguous");
  TORCH_CHECK(k.stride(2) == Dk && v.stride(2) == Dv, "K/V seq stride mismatch");
  TORCH_CHECK(Hq % Hkv == 0 && Dk % 32 == 0 && Dv % 16 == 0, "shape unsupported");
  TORCH_CHECK(Dk <= 256 && Dv <= 256, "Dk<=256, Dv<=256");
  // NEVER silently skip the launch: an uninstantiated template combo
  // once fell through and returned an uninitialized output
  TORCH_CHECK(attn_prefill_supported(Dk, Dv),
              "attn_prefill: no kernel instantiation for Dk=", Dk,
              " Dv=", Dv);
  long kScap = k.stride(1) / Dk;
  long vScap = v.stride(1) / Dv;
  auto out = torch::empty({B, Hq, T, Dv}, qc.options());
  launch_attn_prefill(qc.data_ptr(), k.data_ptr(), v.data_ptr(),
                      out.data_ptr(), B, Hq, Hkv, T, S, kScap, vScap, Dk, Dv,
                      (float)scale, (float)softcap, (int)window,
                      (int)causal_offset, cur_stream());
  return out;
}

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor Bm) {
  check_bf16(A, "A");
  auto D = torch::empty({16, 16}, A.options().dtype(torch::kFloat32));
  launch_mfma_probe(A.contiguous().data_ptr(), Bm.contiguous().data_ptr(),
                    D.data_ptr<float>(), cur_stream());
  return D;
}

// Dense bf16 decode GEMV: y = x @ w^T on MFMA (M <= 64)
torch::Tensor dense_gemv(torch::Tensor x, torch::Tensor w) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  auto xc = x.contiguous();
  const int M = xc.size(0), H = xc.size(1);
  const int O = w.size(0);
  TORCH_CHECK(w.is_contiguous(), "w must be contiguous");
  TORCH_CHECK(M <= 64 && H % 32 == 0, "dense_gemv needs M<=64, H%32==0");
  auto y = torch::empty({M, O}, xc.options());
  const int nk = bf16_gemv_nsplit(M, O, H);
  auto yf = splitk_scratch(nk, M, O, xc.options());
  launch_bf16_gemv_mfma(xc.data_ptr(), w.data_ptr(), y.data_ptr(),
                        f32_or_null(yf), nk, M, O, H, cur_stream());
  return y;
}

// K-segmented coalesced-A dense bf16 GEMM (gemm_kseg.hip): targets the
// K-long down_proj shapes where hipBLASLt plateaus (~3.3 TB/s)
torch::Tensor gemm_m64_kseg(torch::Tensor x, torch::Tensor w,
                            int64_t ksegs) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  auto xc = x.contiguous();
  const int M = xc.size(0), K = xc.size(1);
  const int N = w.size(0);
  TORCH_CHECK(w.is_contiguous(), "w must be contiguous");
  TORCH_CHECK(M >= 1 && M <= 64 && K % 256 == 0,
              "gemm_m64_kseg needs 1<=M<=64, K%256==0");
  TORCH_CHECK(ksegs >= 1);
  auto yf = torch::empty({64, N}, xc.options().dtype(torch::kFloat32));
  auto y = torch::empty({M, N}, xc.options());
  launch_gemm_kseg(xc.data_ptr(), w.data_ptr(), yf.data_ptr<float>(),
                   y.data_ptr(), M, N, K, (int)ksegs, cur_stream());
  return y;
}

// w4a16 K-segmented GEMM: packed repacked weights (ops.repack_w4) +
// fp16 activations; bf16 out
torch::Tensor gemm_m64_kseg_w4(torch::Tensor x, torch::Tensor wq,
                               torch::Tensor sc, torch::Tensor bi,
                               int64_t gs, int64_t ksegs) {
  TORCH_CHECK(x.scalar_type() == torch::kHalf, "x must be fp16");
  auto xc = x.contiguous();
  const int M = xc.size(0), K = xc.size(1);
  const int N = wq.size(0);
  TORCH_CHECK(wq.is_contiguous() && sc.is_contiguous() && bi.is_contiguous());
  TORCH_CHECK(M >= 1 && M <= 64 && K % 256 == 0,
              "gemm_m64_kseg_w4 needs 1<=M<=64, K%256==0");
  TORCH_CHECK(gs == 32 || gs == 64 || gs == 128, "gs must be 32/64/128");
  TORCH_CHECK(wq.size(1) == K / 8, "wq must be repacked w4 [N, K/8]");
  auto yf = torch::empty({64, N}, xc.options().dtype(torch::kFloat32));
  auto y = torch::empty({M, N}, xc.options().dtype(torch::kBFloat16));
  launch_gemm_kseg_w4(xc.data_ptr(), wq.data_ptr(), sc.data_ptr(),
                      bi.data_ptr(), yf.data_ptr<float>(), y.data_ptr(), M, N,
                      K, (int)gs, (int)ksegs, cur_stream());
  return y;
}

// LDS-tiled dense bf16 GEMM, M <= 64, deep-k shapes
torch::Tensor dense_gemm64(torch::Tensor x, torch::Tensor w) {
  check_bf16(x, "x");
  check_bf16(w, "w");
  auto xc = x.contiguous();
  const int M = xc.size(0), H = xc.size(1);
  const int O = w.size(0);
  TORCH_CHECK(w.is_contiguous(), "w must be contiguous");
  TORCH_CHECK(M <= 64 && H % 8 == 0, "dense_gemm64 needs M<=64, H%8==0");
  auto y = torch::empty({M, O}, xc.options());
  const int nk = bf16_gemm_m64_nsplit(M, O, H);
  auto yf = splitk_scratch(nk, M, O, xc.options());
  launch_bf16_gemm_m64(xc.data_ptr(), w.data_ptr(), y.data_ptr(),
                       f32_or_null(yf), nk, M, O, H, cur_stream());
  return y;
}

// x [M, H] bf16, wq [O, H*bits/32] uint32/int32, scales/biases [O, H/gs]
torch::Tensor w4a16_gemv(torch::Tensor x, torch::Tensor wq,
                         torch::Tensor scales, torch::Tensor biases,
                         int64_t gs, int64_t bits) {
  check_bf16(x, "x");
  auto xc = x.contiguous();
  const int M = xc.size(0), H = xc.size(1);
  const int O = wq.size(0);
  auto y = torch::empty({M, O}, xc.options());
  if (M >= 8 && H % 32 == 0 && gs % 32 == 0) {
    const int nk = w4a16_mfma_nsplit(M, O, H);
    auto yf = splitk_scratch(nk, M, O, xc.options());
    launch_w4a16_mfma(xc.data_ptr(), wq.contiguous().data_ptr(),
                      scales.contiguous().data_ptr(),
                      biases.contiguous().data_ptr(), y.data_ptr(),
                      f32_or_null(yf), nk, M, O, H, (int)gs, (int)bits,
                      cur_stream());
  } else {
    launch_w4a16_gemv(xc.data_ptr(), wq.contiguous().data_ptr(),
                      scales.contiguous().data_ptr(),
                      biases.contiguous().data_ptr(), y.data_ptr(), M, O, H,
                      (int)gs, (int)bits, cur_stream());
  }
  return y;
}

torch::Tensor dequant(torch::Tensor wq, torch::Tensor scales,
                      torch::Tensor biases, int64_t H, int64_t gs,
                      int64_t bits) {
  const long O = wq.size(0);
  auto out = torch::empty({O, H}, scales.options());
  launch_dequant(wq.contiguous().data_ptr(), scales.contiguous().data_ptr(),
                 biases.contiguous().data_ptr(), out.data_ptr(), O, (int)H,
                 (int)gs, (int)bits, cur_stream());
  return out;
}

torch::Tensor moe_gateup_grouped(torch::Tensor x, torch::Tensor gate_w,
                                 torch::Tensor up_w, torch::Tensor sub_expert,
                                 torch::Tensor sub_off, torch::Tensor sub_cnt,
                                 torch::Tensor sorted_tok, int64_t P,
                                 int64_t max_tok) {
  check_bf16(x, "x");
  const int H = x.size(1);
  const int I = gate_w.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(sub_expert.scalar_type() == torch::kInt32, "sub arrays int32");
  auto h = torch::empty({P, I}, x.options());
  if (max_tok == 16 && H % 32 == 0 && I % 16 == 0) {
    launch_moe_gateup_mfma(
        x.contiguous().data_ptr(), gate_w.data_ptr(), up_w.data_ptr(),
        h.data_ptr(), sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
        sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(), S, H, I,
        cur_stream());
  } else {
    TORCH_CHECK(max_tok <= 4, "scalar grouped kernel needs max_tok <= 4");
    // the kernel reads weights 8 elements at a time and stages x in 4s
    TORCH_CHECK(H % 8 == 0 && I % 8 == 0,
                "scalar grouped kernel needs H % 8 == 0 and I % 8 == 0 (got H=",
                H, ", I=", I, ")");
    launch_moe_gateup_grouped(
        x.contiguous().data_ptr(), gate_w.data_ptr(), up_w.data_ptr(),
        h.data_ptr(), sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
        sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(), S, H, I,
        cur_stream());
  }
  return h;
}

torch::Tensor moe_down_grouped(torch::Tensor h, torch::Tensor down_w,
                               torch::Tensor sub_expert, torch::Tensor sub_off,
                               torch::Tensor sub_cnt, torch::Tensor sorted_tok,
                               torch::Tensor sorted_wt, int64_t N,
                               int64_t max_tok) {
  const int I = h.size(1);
  const int H = down_w.size(1);
  const int S = sub_expert.size(0);
  auto out = torch::zeros({N, H}, h.options().dtype(torch::kFloat32));
  if (max_tok == 16 && I % 32 == 0 && H % 16 == 0) {
    launch_moe_down_mfma(
        h.contiguous().data_ptr(), down_w.data_ptr(), out.data_ptr<float>(),
        sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
        sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(),
        sorted_wt.data_ptr<float>(), S, I, H, cur_stream());
  } else {
    TORCH_CHECK(max_tok <= 4, "scalar grouped kernel needs max_tok <= 4");
    // the kernel reads weights 8 elements at a time and has no tail loop
    TORCH_CHECK(H % 8 == 0 && I % 8 == 0,
                "scalar grouped kernel needs H % 8 == 0 and I % 8 == 0 (got H=",
                H, ", I=", I, ")");
    launch_moe_down_grouped(
        h.contiguous().data_ptr(), down_w.data_ptr(), out.data_ptr<float>(),
        sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
        sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(),
        sorted_wt.data_ptr<float>(), S, I, H, cur_stream());
  }
  return out;
}

torch::Tensor moe_w4_mfma(torch::Tensor x, torch::Tensor wq,
                          torch::Tensor scales, torch::Tensor biases,
                          torch::Tensor sub_expert, torch::Tensor sub_off,
                          torch::Tensor sub_cnt, torch::Tensor sorted_tok,
                          int64_t P, int64_t gs, int64_t bits) {
  check_bf16(x, "x");
  const int H = x.size(1);
  const int O = wq.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(H % 32 == 0 && gs % 32 == 0, "H%32, gs%32 required");
  // a partial last group would index past the row's H / gs scales
  TORCH_CHECK(H % gs == 0, "moe_w4_mfma needs H % gs == 0 (got H=", H,
              ", gs=", gs, ")");
  auto y = torch::empty({P, O}, x.options());
  launch_moe_w4_mfma(x.contiguous().data_ptr(), wq.data_ptr(),
                     scales.data_ptr(), biases.data_ptr(), y.data_ptr(),
                     sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
                     sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(), S,
                     H, O, (int)gs, (int)bits, cur_stream());
  return y;
}

// Fused fp16-dequant gate+up+SiLU over repacked quant words.
// x [N, H] fp16; gq/uq [E, I, H*bits/32] repacked; scales/biases bf16.
// clear: optional fp32 buffer the launch zeroes (the down kernel's
// accumulator).
torch::Tensor moe_w4f16_gateup_impl(torch::Tensor x, torch::Tensor gq,
                                    torch::Tensor uq, torch::Tensor gsc,
                                    torch::Tensor gbi, torch::Tensor usc,
                                    torch::Tensor ubi, torch::Tensor sub_expert,
                                    torch::Tensor sub_off, torch::Tensor sub_cnt,
                                    torch::Tensor sorted_tok, int64_t P,
                                    int64_t gs, int64_t bits,
                                    const torch::Tensor& clear) {
  TORCH_CHECK(x.scalar_type() == torch::kHalf, "x must be fp16");
  const int H = x.size(1);
  const int I = gq.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(H % 32 == 0, "H%32 required");
  TORCH_CHECK(gs == 32 || gs == 64 || gs == 128, "gs must be 32/64/128");
  auto h = torch::empty({P, I}, x.options());
  launch_moe_w4f16_gateup(
      x.contiguous().data_ptr(), gq.data_ptr(), uq.data_ptr(), gsc.data_ptr(),
      gbi.data_ptr(), usc.data_ptr(), ubi.data_ptr(), h.data_ptr(),
      sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
      sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(), S, H, I, (int)gs,
      (int)bits, clear.defined() ? clear.data_ptr<float>() : nullptr,
      clear.defined() ? clear.numel() : 0, cur_stream());
  return h;
}

torch::Tensor moe_w4f16_gateup(torch::Tensor x, torch::Tensor gq,
                               torch::Tensor uq, torch::Tensor gsc,
                               torch::Tensor gbi, torch::Tensor usc,
                               torch::Tensor ubi, torch::Tensor sub_expert,
                               torch::Tensor sub_off, torch::Tensor sub_cnt,
                               torch::Tensor sorted_tok, int64_t P,
                               int64_t gs, int64_t bits) {
  return moe_w4f16_gateup_impl(x, gq, uq, gsc, gbi, usc, ubi, sub_expert,
                               sub_off, sub_cnt, sorted_tok, P, gs, bits,
                               torch::Tensor());
}

// gate+up that also hands moe_w4f16_down its accumulator: fp32 [N, Hout],
// allocated uninitialised here and zeroed by the gate+up launch itself
// (no separate fill launch, nothing kept between calls).
// Returns (h, acc).
std::vector<torch::Tensor> moe_w4f16_gateup_acc(
    torch::Tensor x, torch::Tensor gq, torch::Tensor uq, torch::Tensor gsc,
    torch::Tensor gbi, torch::Tensor usc, torch::Tensor ubi,
    torch::Tensor sub_expert, torch::Tensor sub_off, torch::Tensor sub_cnt,
    torch::Tensor sorted_tok, int64_t P, int64_t gs, int64_t bits, int64_t N,
    int64_t Hout) {
  TORCH_CHECK(N >= 1 && Hout >= 1, "accumulator shape must be positive");
  auto acc = torch::empty({N, Hout}, x.options().dtype(torch::kFloat32));
  auto h = moe_w4f16_gateup_impl(x, gq, uq, gsc, gbi, usc, ubi, sub_expert,
                                 sub_off, sub_cnt, sorted_tok, P, gs, bits,
                                 acc);
  return {h, acc};
}

// acc: the fp32 [N, H] accumulator that a preceding moe_w4f16_gateup_acc
// launch zeroed on this stream; without it the binding zero-fills its
// own.
torch::Tensor moe_w4f16_down(torch::Tensor hh, torch::Tensor dq,
                             torch::Tensor dsc, torch::Tensor dbi,
                             torch::Tensor sub_expert, torch::Tensor sub_off,
                             torch::Tensor sub_cnt, torch::Tensor sorted_tok,
                             torch::Tensor sorted_wt, int64_t N, int64_t gs,
                             int64_t bits, c10::optional<torch::Tensor> acc) {
  TORCH_CHECK(hh.scalar_type() == torch::kHalf, "h must be fp16");
  const int I = hh.size(1);
  const int H = dq.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(I % 32 == 0, "I%32 required");
  TORCH_CHECK(gs == 32 || gs == 64 || gs == 128, "gs must be 32/64/128");
  torch::Tensor out;
  if (acc.has_value()) {
    out = *acc;
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 &&
                    out.is_contiguous() && out.dim() == 2 &&
                    out.size(0) == N && out.size(1) == H,
                "acc must be contiguous fp32 [N, H]");
  } else {
    out = torch::zeros({N, H}, hh.options().dtype(torch::kFloat32));
  }
  launch_moe_w4f16_down(
      hh.contiguous().data_ptr(), dq.data_ptr(), dsc.data_ptr(),
      dbi.data_ptr(), out.data_ptr<float>(), sub_expert.data_ptr<int>(),
      sub_off.data_ptr<int>(), sub_cnt.data_ptr<int>(),
      sorted_tok.data_ptr<int>(), sorted_wt.data_ptr<float>(), S, I, H,
      (int)gs, (int)bits, cur_stream());
  return out;
}

// Dense fp16-dequant w4/w8 GEMV: x [M, H] fp16, wq REPACKED
// (ops.repack_w4), scales/biases bf16.  Returns bf16 [M, O].
torch::Tensor w4f16_gemv(torch::Tensor x, torch::Tensor wq,
                         torch::Tensor scales, torch::Tensor biases,
                         int64_t gs, int64_t bits) {
  TORCH_CHECK(x.scalar_type() == torch::kHalf, "x must be fp16");
  auto xc = x.contiguous();
  const int M = xc.size(0), H = xc.size(1);
  const int O = wq.size(0);
  TORCH_CHECK(M <= 64 && H % 32 == 0, "w4f16_gemv needs M<=64, H%32==0");
  TORCH_CHECK(gs == 32 || gs == 64 || gs == 128, "gs must be 32/64/128");
  auto y = torch::empty({M, O},
                        xc.options().dtype(torch::kBFloat16));
  const int nk = w4f16_gemv_nsplit(M, O, H);
  auto yf = splitk_scratch(nk, M, O, xc.options());
  launch_w4f16_gemv(xc.data_ptr(), wq.contiguous().data_ptr(),
                    scales.contiguous().data_ptr(),
                    biases.contiguous().data_ptr(), y.data_ptr(),
                    f32_or_null(yf), nk, M, O, H, (int)gs, (int)bits,
                    cur_stream());
  return y;
}

// ---- FP8 block-quantized weights (fp8_block.hip) -------------------------
// w: float8_e4m3fn [.., O, K] contiguous; sc (weight_scale_inv): fp32
// [.., ceil(O/128), ceil(K/128)] contiguous, one scale per 128x128 block.
void check_fp8_block(const torch::Tensor& w, const torch::Tensor& sc,
                     int dims, bool k128, const char* op) {
  TORCH_CHECK(w.is_cuda() && sc.is_cuda(), op, ": tensors must be on GPU");
  TORCH_CHECK(w.scalar_type() == at::kFloat8_e4m3fn, op,
              ": weight must be float8_e4m3fn");
  TORCH_CHECK(sc.scalar_type() == torch::kFloat32, op,
              ": weight_scale_inv must be fp32");
  TORCH_CHECK(w.dim() == dims && sc.dim() == dims, op, ": weight and "
              "weight_scale_inv must be ", dims, "-d");
  TORCH_CHECK(w.is_contiguous() && sc.is_contiguous(), op,
              ": weight and weight_scale_inv must be contiguous");
  const int64_t O = w.size(dims - 2), K = w.size(dims - 1);
  TORCH_CHECK(O >= 1 && K >= 1, op, ": empty weight");
  TORCH_CHECK(!k128 || K % 128 == 0, op, " needs K % 128 == 0 (got K=", K,
              ")");
  TORCH_CHECK(sc.size(dims - 2) == (O + 127) / 128 &&
                  sc.size(dims - 1) == (K + 127) / 128 &&
                  (dims == 2 || sc.size(0) == w.size(0)),
              op, ": weight_scale_inv must be [.., ceil(O/128), ceil(K/128)]"
              " (O=", O, ", K=", K, ")");
}

// [O, K] or [E, O, K] fp8 + block scales -> bf16, any O and K.
torch::Tensor fp8_block_dequant(torch::Tensor w, torch::Tensor sc) {
  TORCH_CHECK(w.dim() == 2 || w.dim() == 3,
              "fp8_block_dequant: weight must be [O, K] or [E, O, K]");
  check_fp8_block(w, sc, (int)w.dim(), false, "fp8_block_dequant");
  const int d = (int)w.dim();
  const long E = d == 3 ? w.size(0) : 1;
  const int O = w.size(d - 2), K = w.size(d - 1);
  auto out = torch::empty(w.sizes(), w.options().dtype(torch::kBFloat16));
  launch_fp8_block_dequant(w.data_ptr(), sc.data_ptr<float>(),
                           out.data_ptr(), E * O, O, K, cur_stream());
  return out;
}

// x [M, K] fp16 (M <= 64), w [O, K] fp8, sc fp32 block scales -> bf16 [M, O]
torch::Tensor fp8f16_gemv(torch::Tensor x, torch::Tensor w, torch::Tensor sc) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kHalf && x.dim() == 2,
              "fp8f16_gemv: x must be fp16 [M, K] on GPU");
  check_fp8_block(w, sc, 2, true, "fp8f16_gemv");
  auto xc = x.contiguous();
  const int M = xc.size(0), K = xc.size(1);
  const int O = w.size(0);
  TORCH_CHECK(w.size(1) == K, "fp8f16_gemv: x/weight K mismatch");
  TORCH_CHECK(M >= 1 && M <= 64, "fp8f16_gemv needs 1 <= M <= 64 (got ", M,
              ")");
  auto y = torch::empty({M, O}, xc.options().dtype(torch::kBFloat16));
  const int nk = fp8f16_gemv_nsplit(M, O, K);
  auto yf = splitk_scratch(nk, M, O, xc.options());
  launch_fp8f16_gemv(xc.data_ptr(), w.data_ptr(), sc.data_ptr<float>(),
                     y.data_ptr(), f32_or_null(yf), nk, M, O, K,
                     cur_stream());
  return y;
}

void check_subranges(const torch::Tensor& sub_expert,
                     const torch::Tensor& sub_off,
                     const torch::Tensor& sub_cnt,
                     const torch::Tensor& sorted_tok, const char* op) {
  TORCH_CHECK(sub_expert.scalar_type() == torch::kInt32 &&
                  sub_off.scalar_type() == torch::kInt32 &&
                  sub_cnt.scalar_type() == torch::kInt32 &&
                  sorted_tok.scalar_type() == torch::kInt32,
              op, ": sub-range arrays must be int32");
  TORCH_CHECK(sub_expert.is_contiguous() && sub_off.is_contiguous() &&
                  sub_cnt.is_contiguous() && sorted_tok.is_contiguous(),
              op, ": sub-range arrays must be contiguous");
  TORCH_CHECK(sub_expert.size(0) >= 1 &&
                  sub_off.size(0) == sub_expert.size(0) &&
                  sub_cnt.size(0) == sub_expert.size(0),
              op, ": sub-range arrays must have one length >= 1");
}

// Fused gate+up+SiLU over fp8 experts.  x [N, H] fp16; gw/uw [E, I, H]
// fp8; gsc/usc [E, ceil(I/128), H/128] fp32.  clear: optional fp32 buffer
// the launch zeroes (the down kernel's accumulator).  Returns h [P, I] fp16.
torch::Tensor moe_fp8f16_gateup_impl(torch::Tensor x, torch::Tensor gw,
                                     torch::Tensor uw, torch::Tensor gsc,
                                     torch::Tensor usc,
                                     torch::Tensor sub_expert,
                                     torch::Tensor sub_off,
                                     torch::Tensor sub_cnt,
                                     torch::Tensor sorted_tok, int64_t P,
                                     const torch::Tensor& clear) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kHalf && x.dim() == 2,
              "moe_fp8f16_gateup: x must be fp16 [N, H] on GPU");
  check_fp8_block(gw, gsc, 3, true, "moe_fp8f16_gateup");
  check_fp8_block(uw, usc, 3, true, "moe_fp8f16_gateup");
  check_subranges(sub_expert, sub_off, sub_cnt, sorted_tok,
                  "moe_fp8f16_gateup");
  TORCH_CHECK(gw.sizes() == uw.sizes(), "gate/up shape mismatch");
  const int H = x.size(1);
  const int I = gw.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(gw.size(2) == H, "moe_fp8f16_gateup: x/weight H mismatch");
  TORCH_CHECK(P == sorted_tok.size(0), "P must be len(sorted_tok)");
  auto h = torch::empty({P, I}, x.options());
  launch_moe_fp8f16_gateup(
      x.contiguous().data_ptr(), gw.data_ptr(), uw.data_ptr(),
      gsc.data_ptr<float>(), usc.data_ptr<float>(), h.data_ptr(),
      sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
      sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(), S, H, I,
      clear.defined() ? clear.data_ptr<float>() : nullptr,
      clear.defined() ? clear.numel() : 0, cur_stream());
  return h;
}

torch::Tensor moe_fp8f16_gateup(torch::Tensor x, torch::Tensor gw,
                                torch::Tensor uw, torch::Tensor gsc,
                                torch::Tensor usc, torch::Tensor sub_expert,
                                torch::Tensor sub_off, torch::Tensor sub_cnt,
                                torch::Tensor sorted_tok, int64_t P) {
  return moe_fp8f16_gateup_impl(x, gw, uw, gsc, usc, sub_expert, sub_off,
                                sub_cnt, sorted_tok, P, torch::Tensor());
}

// gate+up that also hands moe_fp8f16_down its accumulator (fp32 [N, Hout],
// allocated uninitialised, zeroed by the gate+up launch).  Returns (h, acc).
std::vector<torch::Tensor> moe_fp8f16_gateup_acc(
    torch::Tensor x, torch::Tensor gw, torch::Tensor uw, torch::Tensor gsc,
    torch::Tensor usc, torch::Tensor sub_expert, torch::Tensor sub_off,
    torch::Tensor sub_cnt, torch::Tensor sorted_tok, int64_t P, int64_t N,
    int64_t Hout) {
  TORCH_CHECK(N >= 1 && Hout >= 1, "accumulator shape must be positive");
  auto acc = torch::empty({N, Hout}, x.options().dtype(torch::kFloat32));
  auto h = moe_fp8f16_gateup_impl(x, gw, uw, gsc, usc, sub_expert, sub_off,
                                  sub_cnt, sorted_tok, P, acc);
  return {h, acc};
}

// hh [P, I] fp16; dw [E, H, I] fp8; dsc [E, ceil(H/128), I/128] fp32.
// acc: the fp32 [N, H] accumulator a preceding moe_fp8f16_gateup_acc
// zeroed on this stream; without it the binding zero-fills its own.
torch::Tensor moe_fp8f16_down(torch::Tensor hh, torch::Tensor dw,
                              torch::Tensor dsc, torch::Tensor sub_expert,
                              torch::Tensor sub_off, torch::Tensor sub_cnt,
                              torch::Tensor sorted_tok,
                              torch::Tensor sorted_wt, int64_t N,
                              c10::optional<torch::Tensor> acc) {
  TORCH_CHECK(hh.is_cuda() && hh.scalar_type() == torch::kHalf &&
                  hh.dim() == 2,
              "moe_fp8f16_down: h must be fp16 [P, I] on GPU");
  check_fp8_block(dw, dsc, 3, true, "moe_fp8f16_down");
  check_subranges(sub_expert, sub_off, sub_cnt, sorted_tok,
                  "moe_fp8f16_down");
  TORCH_CHECK(sorted_wt.scalar_type() == torch::kFloat32 &&
                  sorted_wt.is_contiguous() &&
                  sorted_wt.size(0) == sorted_tok.size(0) &&
                  hh.size(0) == sorted_tok.size(0),
              "moe_fp8f16_down: sorted_wt fp32 and h rows must match "
              "sorted_tok");
  const int I = hh.size(1);
  const int H = dw.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(dw.size(2) == I, "moe_fp8f16_down: h/weight I mismatch");
  torch::Tensor out;
  if (acc.has_value()) {
    out = *acc;
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 &&
                    out.is_contiguous() && out.dim() == 2 &&
                    out.size(0) == N && out.size(1) == H,
                "acc must be contiguous fp32 [N, H]");
  } else {
    out = torch::zeros({N, H}, hh.options().dtype(torch::kFloat32));
  }
  launch_moe_fp8f16_down(
      hh.contiguous().data_ptr(), dw.data_ptr(), dsc.data_ptr<float>(),
      out.data_ptr<float>(), sub_expert.data_ptr<int>(),
      sub_off.data_ptr<int>(), sub_cnt.data_ptr<int>(),
      sorted_tok.data_ptr<int>(), sorted_wt.data_ptr<float>(), S, I, H,
      cur_stream());
  return out;
}

// The prefill-regime pair (fp8_prefill.hip): the same contract over
// sub-ranges built for moe_fp8f16_wide_tile() tokens.
torch::Tensor moe_fp8f16_gateup_wide(torch::Tensor x, torch::Tensor gw,
                                     torch::Tensor uw, torch::Tensor gsc,
                                     torch::Tensor usc,
                                     torch::Tensor sub_expert,
                                     torch::Tensor sub_off,
                                     torch::Tensor sub_cnt,
                                     torch::Tensor sorted_tok, int64_t P) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kHalf && x.dim() == 2,
              "moe_fp8f16_gateup_wide: x must be fp16 [N, H] on GPU");
  check_fp8_block(gw, gsc, 3, true, "moe_fp8f16_gateup_wide");
  check_fp8_block(uw, usc, 3, true, "moe_fp8f16_gateup_wide");
  check_subranges(sub_expert, sub_off, sub_cnt, sorted_tok,
                  "moe_fp8f16_gateup_wide");
  TORCH_CHECK(gw.sizes() == uw.sizes(),
              "moe_fp8f16_gateup_wide: gate/up shape mismatch");
  const int H = x.size(1);
  const int I = gw.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(gw.size(2) == H, "moe_fp8f16_gateup_wide: x/weight H mismatch");
  TORCH_CHECK(P == sorted_tok.size(0),
              "moe_fp8f16_gateup_wide: P must be len(sorted_tok)");
  auto h = torch::empty({P, I}, x.options());
  launch_moe_fp8f16_gateup_wide(
      x.contiguous().data_ptr(), gw.data_ptr(), uw.data_ptr(),
      gsc.data_ptr<float>(), usc.data_ptr<float>(), h.data_ptr(),
      sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
      sub_cnt.data_ptr<int>(), sorted_tok.data_ptr<int>(), S, H, I,
      cur_stream());
  return h;
}

torch::Tensor moe_fp8f16_down_wide(torch::Tensor hh, torch::Tensor dw,
                                   torch::Tensor dsc,
                                   torch::Tensor sub_expert,
                                   torch::Tensor sub_off,
                                   torch::Tensor sub_cnt,
                                   torch::Tensor sorted_tok,
                                   torch::Tensor sorted_wt, int64_t N) {
  TORCH_CHECK(hh.is_cuda() && hh.scalar_type() == torch::kHalf &&
                  hh.dim() == 2,
              "moe_fp8f16_down_wide: h must be fp16 [P, I] on GPU");
  check_fp8_block(dw, dsc, 3, true, "moe_fp8f16_down_wide");
  check_subranges(sub_expert, sub_off, sub_cnt, sorted_tok,
                  "moe_fp8f16_down_wide");
  TORCH_CHECK(sorted_wt.scalar_type() == torch::kFloat32 &&
                  sorted_wt.is_contiguous() &&
                  sorted_wt.size(0) == sorted_tok.size(0) &&
                  hh.size(0) == sorted_tok.size(0),
              "moe_fp8f16_down_wide: sorted_wt fp32 and h rows must match "
              "sorted_tok");
  TORCH_CHECK(N >= 1, "moe_fp8f16_down_wide: N must be positive");
  const int I = hh.size(1);
  const int H = dw.size(1);
  const int S = sub_expert.size(0);
  TORCH_CHECK(dw.size(2) == I, "moe_fp8f16_down_wide: h/weight I mismatch");
  auto out = torch::zeros({N, H}, hh.options().dtype(torch::kFloat32));
  launch_moe_fp8f16_down_wide(
      hh.contiguous().data_ptr(), dw.data_ptr(), dsc.data_ptr<float>(),
      out.data_ptr<float>(), sub_expert.data_ptr<int>(),
      sub_off.data_ptr<int>(), sub_cnt.data_ptr<int>(),
      sorted_tok.data_ptr<int>(), sorted_wt.data_ptr<float>(), S, I, H,
      cur_stream());
  return out;
}

std::vector<torch::Tensor> moe_gate_subranges(torch::Tensor logits, int64_t K,
                                              int64_t s_upper, int64_t max_tok,
                                              double routed_scaling,
                                              bool norm_topk, int64_t n_group,
                                              int64_t topk_group,
                                              const std::string& scoring,
                                              c10::optional<torch::Tensor> e_bias) {
  check_bf16(logits, "logits");
  TORCH_CHECK(scoring == "softmax" || scoring == "sigmoid",
              "fused gate scoring must be 'softmax' or 'sigmoid' (got '",
              scoring, "')");
  const bool sigmoid = scoring == "sigmoid";
  TORCH_CHECK(logits.dim() == 2, "logits must be [N, E]");
  auto lc = logits.contiguous();
  const int64_t N = lc.size(0), E = lc.size(1);
  // the kernel's LDS arrays are sized for exactly these limits
  TORCH_CHECK(N <= 128 && E >= 1 && E <= 256 && K >= 1 && K <= 8,
              "fused gate limits: N<=128, 1<=E<=256, 1<=K<=8 (got N=", N,
              ", E=", E, ", K=", K, ")");
  TORCH_CHECK(n_group >= 1 && n_group <= 32 && E % n_group == 0,
              "fused gate limits: 1<=n_group<=32 and E % n_group == 0 (got E=",
              E, ", n_group=", n_group, ")");
  TORCH_CHECK(topk_group >= 1 && topk_group <= n_group,
              "fused gate limits: 1<=topk_group<=n_group (got topk_group=",
              topk_group, ", n_group=", n_group, ")");
  TORCH_CHECK(topk_group * (E / n_group) >= K,
              "fused gate limits: topk_group*(E/n_group) >= K (got ",
              topk_group, "*", E / n_group, " < ", K, ")");
  TORCH_CHECK(max_tok >= 1 && s_upper >= E + (N * K) / max_tok,
              "fused gate needs max_tok>=1 and s_upper >= E + N*K/max_tok");
  // a sigmoid group is scored by its two best members
  TORCH_CHECK(!sigmoid || n_group == 1 || E / n_group >= 2,
              "fused gate limits: sigmoid scoring with groups needs "
              "E/n_group >= 2 (got E=", E, ", n_group=", n_group, ")");
  const float* bias_ptr = nullptr;
  if (e_bias.has_value()) {
    const torch::Tensor& eb = *e_bias;
    TORCH_CHECK(sigmoid, "e_bias applies to sigmoid scoring only");
    TORCH_CHECK(eb.scalar_type() == torch::kFloat32 && eb.is_contiguous() &&
                    eb.device() == lc.device() && eb.dim() == 1 &&
                    eb.size(0) == E,
                "e_bias must be a contiguous fp32 [E] tensor on the logits' "
                "device (E=", E, ")");
    bias_ptr = eb.data_ptr<float>();
  }
  const long P = (long)N * K;
  auto opts = torch::TensorOptions().dtype(torch::kInt32).device(lc.device());
  auto sorted_tok = torch::empty({P}, opts);
  auto sorted_wt = torch::empty({P}, opts.dtype(torch::kFloat32));
  auto sub_expert = torch::empty({s_upper}, opts);
  auto sub_off = torch::empty({s_upper}, opts);
  auto sub_cnt = torch::empty({s_upper}, opts);
  launch_moe_gate_subranges(lc.data_ptr(), bias_ptr, sigmoid ? 1 : 0,
                            sorted_tok.data_ptr<int>(),
                            sorted_wt.data_ptr<float>(),
                            sub_expert.data_ptr<int>(), sub_off.data_ptr<int>(),
                            sub_cnt.data_ptr<int>(), (int)N, (int)E, (int)K,
                            (int)s_upper, (int)max_tok, (float)routed_scaling,
                            norm_topk ? 1 : 0, (int)n_group, (int)topk_group,
                            cur_stream());
  return {sub_expert, sub_off, sub_cnt, sorted_tok, sorted_wt};
}

// reference.sample_rows on device: edits logits in place, writes ids_out
// and lse_out for the active rows.  No allocation: safe under capture.
void sample_rows(torch::Tensor logits, torch::Tensor temperature,
                 torch::Tensor top_p, torch::Tensor u, torch::Tensor active,
                 torch::Tensor ids_out, torch::Tensor lse_out,
                 c10::optional<torch::Tensor> bias_idx,
                 c10::optional<torch::Tensor> bias_val,
                 c10::optional<torch::Tensor> pen_idx,
                 c10::optional<torch::Tensor> penalty) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kFloat32 &&
                  logits.dim() == 2 && logits.is_contiguous(),
              "logits must be a contiguous 2-D fp32 tensor on GPU");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (1LL << 31) && B < (1LL << 31),
              "logits must have 1 <= V < 2^31 columns");
  auto vec = [&](const torch::Tensor& t, torch::ScalarType ty,
                 const char* name, const char* tyname) {
    TORCH_CHECK(t.is_cuda() && t.get_device() == logits.get_device(), name,
                " must be on the logits' GPU");
    TORCH_CHECK(t.scalar_type() == ty, name, " must be ", tyname);
    TORCH_CHECK(t.dim() == 1 && t.size(0) == B && t.is_contiguous(), name,
                " must be a contiguous vector of length B = ", B);
  };
  vec(temperature, torch::kFloat32, "temperature", "fp32");
  vec(top_p, torch::kFloat32, "top_p", "fp32");
  vec(u, torch::kFloat32, "u", "fp32");
  vec(active, torch::kInt32, "active", "int32");
  vec(lse_out, torch::kFloat32, "lse_out", "fp32");
  TORCH_CHECK(ids_out.is_cuda() && ids_out.get_device() == logits.get_device(),
              "ids_out must be on the logits' GPU");
  TORCH_CHECK(ids_out.scalar_type() == torch::kInt64, "ids_out must be int64");
  TORCH_CHECK((ids_out.dim() == 1 && ids_out.size(0) == B) ||
                  (ids_out.dim() == 2 && ids_out.size(0) == B &&
                   ids_out.size(1) == 1),
              "ids_out must have shape [B] or [B, 1] with B = ", B);
  const long ids_stride = B > 0 ? (long)ids_out.stride(0) : 1;
  TORCH_CHECK(B <= 1 || ids_stride >= 1, "ids_out rows must not overlap");

  auto table = [&](const torch::Tensor& t, torch::ScalarType ty,
                   const char* name, const char* tyname, int64_t limit) {
    TORCH_CHECK(t.is_cuda() && t.get_device() == logits.get_device(), name,
                " must be on the logits' GPU");
    TORCH_CHECK(t.scalar_type() == ty, name, " must be ", tyname);
    TORCH_CHECK(t.dim() == 2 && t.size(0) == B && t.is_contiguous(), name,
                " must be a contiguous [B, n] tensor with B = ", B);
    TORCH_CHECK(t.size(1) <= limit, name, " holds at most ", limit,
                " entries per row (got ", t.size(1), ")");
  };
  TORCH_CHECK(bias_idx.has_value() == bias_val.has_value(),
              "bias_idx and bias_val must be given together");
  TORCH_CHECK(pen_idx.has_value() == penalty.has_value(),
              "pen_idx and penalty must be given together");
  const int* bi = nullptr;
  const float* bv = nullptr;
  int NB = 0;
  if (bias_idx.has_value()) {
    table(*bias_idx, torch::kInt32, "bias_idx", "int32", 32);
    table(*bias_val, torch::kFloat32, "bias_val", "fp32", 32);
    TORCH_CHECK(bias_idx->size(1) == bias_val->size(1),
                "bias_idx and bias_val must have the same shape");
    NB = (int)bias_idx->size(1);
    if (NB > 0) {
      bi = bias_idx->data_ptr<int>();
      bv = bias_val->data_ptr<float>();
    }
  }
  const int* pi = nullptr;
  const float* pv = nullptr;
  int W = 0;
  if (pen_idx.has_value()) {
    table(*pen_idx, torch::kInt32, "pen_idx", "int32", 64);
    vec(*penalty, torch::kFloat32, "penalty", "fp32");
    W = (int)pen_idx->size(1);
    if (W > 0) {
      pi = pen_idx->data_ptr<int>();
      pv = penalty->data_ptr<float>();
    }
  }
  launch_sample_rows(logits.data_ptr<float>(), temperature.data_ptr<float>(),
                     top_p.data_ptr<float>(), u.data_ptr<float>(),
                     active.data_ptr<int>(),
                     reinterpret_cast<long long*>(ids_out.data_ptr<int64_t>()),
                     ids_stride, lse_out.data_ptr<float>(), bi, bv, NB, pi, pv,
                     W, (int)B, (int)V, cur_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("sample_rows", &sample_rows, pybind11::arg("logits"),
        pybind11::arg("temperature"), pybind11::arg("top_p"),
        pybind11::arg("u"), pybind11::arg("active"), pybind11::arg("ids_out"),
        pybind11::arg("lse_out"), pybind11::arg("bias_idx") = pybind11::none(),
        pybind11::arg("bias_val") = pybind11::none(),
        pybind11::arg("pen_idx") = pybind11::none(),
        pybind11::arg("penalty") = pybind11::none());
  m.def("rms_norm", &rms_norm, "fused RMSNorm (gfx950)");
  m.def("rms_norm_residual", &rms_norm_residual, pybind11::arg("x"),
        pybind11::arg("resid"), pybind11::arg("w"), pybind11::arg("eps"),
        pybind11::arg("w_off"), pybind11::arg("with_f16") = false);
  m.def("mla_decode_prep", &mla_decode_prep, pybind11::arg("qh"),
        pybind11::arg("ckv"), pybind11::arg("w"), pybind11::arg("eps"),
        pybind11::arg("w_off"), pybind11::arg("cos"), pybind11::arg("sin"),
        pybind11::arg("cache"), pybind11::arg("rope"),
        pybind11::arg("pos") = pybind11::none(), pybind11::arg("pos0") = 0);
  m.def("moe_finalize", &moe_finalize, pybind11::arg("acc"),
        pybind11::arg("shared"), pybind11::arg("h"));
  m.def("glu", &glu);
  m.def("softcap", &softcap_op);
  m.def("apply_rope", &apply_rope);
  m.def("rope_append_kv", &rope_append_kv, pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("cos"), pybind11::arg("sin"),
        pybind11::arg("kcache"), pybind11::arg("vcache"),
        pybind11::arg("pos") = pybind11::none(), pybind11::arg("pos0") = 0,
        pybind11::arg("interleaved") = false);
  m.def("mla_append_kv", &mla_append_kv,
        pybind11::arg("kvh"), pybind11::arg("kpe"), pybind11::arg("kcache"),
        pybind11::arg("vcache"), pybind11::arg("pos") = pybind11::none(),
        pybind11::arg("pos0") = 0);
  m.def("attn_decode", &attn_decode, pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("scale"), pybind11::arg("softcap"),
        pybind11::arg("window"), pybind11::arg("pos") = pybind11::none());
  m.def("attn_decode_split", &attn_decode_split, pybind11::arg("q_nope"),
        pybind11::arg("q_rope"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("scale"), pybind11::arg("softcap"),
        pybind11::arg("window"), pybind11::arg("pos") = pybind11::none());
  m.def("attn_decode_shape_ok", [](int64_t g, int64_t dv) {
    return attn_decode_supported_shape((int)g, (int)dv);
  });
  m.def("attn_prefill", &attn_prefill);
  m.def("attn_prefill_shape_ok", [](int64_t dk, int64_t dv) {
    return attn_prefill_supported((int)dk, (int)dv);
  });
  m.def("mfma_probe", &mfma_probe);
  m.def("w4a16_gemv", &w4a16_gemv);
  m.def("w4f16_gemv", &w4f16_gemv);
  // split-K factors the two quantized GEMV bindings will use (tests pin
  // which store path a shape takes)
  m.def("w4a16_mfma_nsplit", [](int64_t M, int64_t O, int64_t H) {
    return w4a16_mfma_nsplit((int)M, (int)O, (int)H);
  });
  m.def("w4f16_gemv_nsplit", [](int64_t M, int64_t O, int64_t H) {
    return w4f16_gemv_nsplit((int)M, (int)O, (int)H);
  });
  m.def("dense_gemv", &dense_gemv);
  m.def("dense_gemm64", &dense_gemm64);
  m.def("gemm_m64_kseg", &gemm_m64_kseg);
  m.def("gemm_m64_kseg_w4", &gemm_m64_kseg_w4);
  m.def("dequant", &dequant);
  m.def("moe_gateup_grouped", &moe_gateup_grouped);
  m.def("moe_down_grouped", &moe_down_grouped);
  m.def("moe_w4_mfma", &moe_w4_mfma);
  m.def("moe_w4f16_gateup", &moe_w4f16_gateup);
  m.def("moe_w4f16_gateup_acc", &moe_w4f16_gateup_acc);
  m.def("moe_w4f16_down", &moe_w4f16_down, pybind11::arg("hh"),
        pybind11::arg("dq"), pybind11::arg("dsc"), pybind11::arg("dbi"),
        pybind11::arg("sub_expert"), pybind11::arg("sub_off"),
        pybind11::arg("sub_cnt"), pybind11::arg("sorted_tok"),
        pybind11::arg("sorted_wt"), pybind11::arg("N"), pybind11::arg("gs"),
        pybind11::arg("bits"), pybind11::arg("acc") = pybind11::none());
  m.def("fp8_block_dequant", &fp8_block_dequant);
  m.def("fp8f16_gemv", &fp8f16_gemv);
  m.def("fp8f16_gemv_nsplit", [](int64_t M, int64_t O, int64_t K) {
    return fp8f16_gemv_nsplit((int)M, (int)O, (int)K);
  });
  m.def("moe_fp8f16_gateup", &moe_fp8f16_gateup);
  m.def("moe_fp8f16_gateup_acc", &moe_fp8f16_gateup_acc);
  m.def("moe_fp8f16_down", &moe_fp8f16_down, pybind11::arg("hh"),
        pybind11::arg("dw"), pybind11::arg("dsc"),
        pybind11::arg("sub_expert"), pybind11::arg("sub_off"),
        pybind11::arg("sub_cnt"), pybind11::arg("sorted_tok"),
        pybind11::arg("sorted_wt"), pybind11::arg("N"),
        pybind11::arg("acc") = pybind11::none());
  m.def("moe_fp8f16_gateup_wide", &moe_fp8f16_gateup_wide);
  m.def("moe_fp8f16_down_wide", &moe_fp8f16_down_wide);
  m.def("moe_fp8f16_wide_tile", []() { return moe_fp8f16_wide_tile(); });
  m.def("moe_gate_subranges", &moe_gate_subranges, pybind11::arg("logits"),
        pybind11::arg("top_k"), pybind11::arg("s_upper"),
        pybind11::arg("max_tok"), pybind11::arg("routed_scaling"),
        pybind11::arg("norm_topk"), pybind11::arg("n_group") = 1,
        pybind11::arg("topk_group") = 1,
        pybind11::arg("scoring") = "softmax",
        pybind11::arg("e_bias") = pybind11::none());
  m.def("moe_scatter_rows",
        [](torch::Tensor src, torch::Tensor dst, torch::Tensor src_idx,
           torch::Tensor dst_idx) {
          check_bf16(src, "src");
          const int P = src_idx.size(0), H = src.size(-1);
          TORCH_CHECK(H % 4 == 0 && dst.size(-1) == H, "row shape");
          TORCH_CHECK(src_idx.scalar_type() == torch::kInt32 &&
                          dst_idx.scalar_type() == torch::kInt32,
                      "indices int32");
          launch_moe_scatter_rows(src.contiguous().data_ptr(), dst.data_ptr(),
                                  src_idx.data_ptr<int>(),
                                  dst_idx.data_ptr<int>(), P, H,
                                  cur_stream());
        });
  m.def("moe_gather_reduce",
        [](torch::Tensor d, torch::Tensor pos, torch::Tensor wts, int64_t N) {
          check_bf16(d, "d");
          const int K = pos.size(1), H = d.size(-1);
          TORCH_CHECK(pos.scalar_type() == torch::kInt32, "pos int32");
          TORCH_CHECK(wts.scalar_type() == torch::kFloat32, "wts fp32");
          auto out = torch::empty({N, H}, d.options());
          launch_moe_gather_reduce(d.contiguous().data_ptr(),
                                   pos.contiguous().data_ptr<int>(),
                                   wts.contiguous().data_ptr<float>(),
                                   out.data_ptr(), (int)N, K, H,
                                   cur_stream());
          return out;
        });
}
