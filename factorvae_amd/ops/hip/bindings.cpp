// Torch extension bindings for the FactorVAE gfx950 kernels.
// Thin layer: validate tensors, extract raw pointers, forward to the
// extern "C" launchers declared in launchers.h.

#include <torch/extension.h>
// Direct ATen/hip include (torch-ROCm's native header; no CUDA-named
// compatibility path — the hipify build pass is a no-op on this file).
#include <ATen/hip/HIPContext.h>

#include <climits>

#include "launchers.h"

namespace {

using torch::Tensor;
using OptTensor = c10::optional<torch::Tensor>;

inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// The argument checks of one binding call. Every pointer handed to a
// launcher comes out of ptr(): the tensor is on the GPU, on the device of
// the call's first tensor, of the expected dtype, contiguous, and holds
// the element count the call's dimensions need. Host metadata only — the
// bindings run under graph capture. The kernel limits (H <= 64, ...) stay
// in the launchers.
class Op {
 public:
  Op(const char* name, const Tensor& first, const char* first_arg)
      : name_(name), dev_(first.device()) {
    TORCH_CHECK(first.is_cuda(), name_, ": ", first_arg,
                " must be on the GPU");
  }

  // exact = false: at least n elements (activations, workspaces, outputs);
  // exact = true: exactly n (parameters)
  template <typename T>
  T* ptr(const Tensor& t, const char* arg, at::ScalarType st, int64_t n,
         bool exact) const {
    TORCH_CHECK(n >= 0, name_, ": ", arg, " would need ", n, " elements");
    TORCH_CHECK(t.is_cuda(), name_, ": ", arg, " must be on the GPU");
    TORCH_CHECK(t.device() == dev_, name_, ": ", arg, " is on ", t.device(),
                ", the call's first tensor on ", dev_);
    TORCH_CHECK(t.scalar_type() == st, name_, ": ", arg, " must be ", st,
                ", got ", t.scalar_type());
    TORCH_CHECK(t.is_contiguous(), name_, ": ", arg, " must be contiguous");
    TORCH_CHECK(exact ? t.numel() == n : t.numel() >= n, name_, ": ", arg,
                " has ", t.numel(), " elements, needs ",
                exact ? "exactly " : "at least ", n);
    return static_cast<T*>(t.data_ptr());
  }
  // an absent optional tensor is a null pointer
  template <typename T>
  T* ptr(const OptTensor& t, const char* arg, at::ScalarType st, int64_t n,
         bool exact) const {
    return t.has_value() ? ptr<T>(*t, arg, st, n, exact) : nullptr;
  }

  // size i of t (i = -1: the last) as a value that fits the launchers' int
  long dim(const Tensor& t, const char* arg, int64_t i) const {
    TORCH_CHECK(t.dim() > (i < 0 ? 0 : i), name_, ": ", arg, " must have ",
                (i < 0 ? 1 : i + 1), " or more dimensions, got ", t.dim());
    return num(t.size(i), arg);
  }
  // a size or count from Python, range-checked before it becomes an int
  long num(int64_t v, const char* what) const {
    TORCH_CHECK(v >= 0 && v <= INT_MAX, name_, ": ", what, " = ", v,
                " is outside the range of int");
    return v;
  }
  // the count that two tensors give together
  int64_t same_numel(const Tensor& a, const char* an, const Tensor& b,
                     const char* bn) const {
    TORCH_CHECK(a.numel() == b.numel(), name_, ": ", an, " and ", bn,
                " differ in size: ", a.numel(), " and ", b.numel(),
                " elements");
    return a.numel();
  }
  template <typename... Msg>
  void require(bool ok, const Msg&... msg) const {
    TORCH_CHECK(ok, name_, ": ", msg...);
  }

 private:
  const char* name_;
  c10::Device dev_;
};

// OP opens a binding; the other macros use its `op` and report the argument
// under its own name. n counts elements; the _EQ forms want exactly n.
#define OP(name, first) const Op op(name, first, #first)
#define P_F32(t, n) op.ptr<float>(t, #t, torch::kFloat32, n, false)
#define P_F32_EQ(t, n) op.ptr<float>(t, #t, torch::kFloat32, n, true)
#define P_BF16(t, n) op.ptr<void>(t, #t, torch::kBFloat16, n, false)
#define P_BF16_EQ(t, n) op.ptr<void>(t, #t, torch::kBFloat16, n, true)
#define P_FP8(t, n) op.ptr<void>(t, #t, torch::kFloat8_e4m3fn, n, false)
#define P_I32(t, n) op.ptr<int>(t, #t, torch::kInt32, n, false)
#define P_F64(t, n) op.ptr<double>(t, #t, torch::kFloat64, n, false)
#define DIM(t, i) op.dim(t, #t, i)
#define NUM(v) op.num(v, #v)

#define RUN(call)                                                      \
  do {                                                                 \
    hipError_t e_ = (call);                                            \
    TORCH_CHECK(e_ == hipSuccess, "HIP kernel failed: ", #call, " (", \
                (int)e_, ")");                                         \
  } while (0)

// ---------------------------------------------------------------- fp32
void gemm_nt(Tensor A, Tensor W, OptTensor bias, Tensor out, double alpha,
             bool accumulate, bool act_lrelu) {
  OP("gemm_nt", A);
  const long R = DIM(A, 0), Ci = DIM(A, 1), Co = DIM(W, 0);
  op.require(DIM(W, 1) == Ci && DIM(out, 0) == R && DIM(out, 1) == Co,
             "want A (R,Ci), W (Co,Ci), out (R,Co)");
  RUN(fv_gemm_nt(P_F32(A, R * Ci), P_F32(W, Co * Ci), P_F32(bias, Co),
                 P_F32(out, R * Co), R, Ci, Co, (float)alpha, accumulate,
                 act_lrelu, cur_stream()));
}

// optional epilogue: out *= lrelu'(Y), Y = lrelu_bwd_of the post-activation
// (R,Co)
// variant 0: the original kernel; 1: the pipelined one (bit-identical)
void gemm_nn(Tensor A, Tensor B, OptTensor bias, Tensor out, double alpha,
             bool accumulate, bool act_lrelu,
             OptTensor lrelu_bwd_of = c10::nullopt, long variant = 1) {
  OP("gemm_nn", A);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             " is not 0 or 1");
  const long R = DIM(A, 0), Ci = DIM(A, 1), Co = DIM(B, 1);
  op.require(DIM(B, 0) == Ci && DIM(out, 0) == R && DIM(out, 1) == Co,
             "want A (R,Ci), B (Ci,Co), out (R,Co)");
  op.require(!lrelu_bwd_of.has_value() ||
                 (lrelu_bwd_of->dim() == 2 && lrelu_bwd_of->size(0) == R &&
                  lrelu_bwd_of->size(1) == Co),
             "lrelu_bwd_of must be (R,Co)");
  RUN(fv_gemm_nn(P_F32(A, R * Ci), P_F32(B, Ci * Co), P_F32(bias, Co),
                 P_F32(out, R * Co), R, Ci, Co, (float)alpha, accumulate,
                 act_lrelu, P_F32(lrelu_bwd_of, R * Co), (int)variant,
                 cur_stream()));
}

// The LayerNorm parameter-gradient partials of dxln = A (R,Ci) @ B (Ci,C)
// straight from the GEMM (dxln is never stored): part receives what
// ln_bwd_params' first kernel writes, ln_bwd_reduce finishes. Returns
// false, with nothing launched, where ln_bwd_params does not work on
// 64-row blocks; the caller then runs gemm_nn and ln_bwd_params.
bool gemm_nn_ln(Tensor A, Tensor B, Tensor x, Tensor mean, Tensor rstd,
                Tensor part) {
  OP("gemm_nn_ln", A);
  const long R = DIM(A, 0), Ci = DIM(A, 1), C = DIM(B, 1);
  op.require(DIM(B, 0) == Ci, "want A (R,Ci), B (Ci,C)");
  op.require(C >= 1, "B has no columns");
  const long yblocks = fv_ln_bwd_yblocks(R, C);
  int ran = 0;
  RUN(fv_gemm_nn_ln(P_F32(A, R * Ci), P_F32(B, Ci * C), P_F32(x, R * C),
                    P_F32(mean, R), P_F32(rstd, R),
                    P_F32(part, yblocks * 2 * C), R, Ci, C, 1.0f, &ran,
                    cur_stream()));
  return ran != 0;
}

// variant 0: the original loop; 1: the pipelined one (bit-identical).
// reduce = false: a sliced call leaves its slices in part/db_part for
// tn_reduce_list (part, and db_part with db, are then required).
void gemm_tn(Tensor A, Tensor B, Tensor out, OptTensor part, long r_chunks,
             bool accumulate, OptTensor db, OptTensor db_part, long variant,
             bool reduce) {
  OP("gemm_tn", A);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             " is not 0 or 1");
  op.require(reduce || (part.has_value() &&
                        (!db.has_value() || db_part.has_value())),
             "reduce = false needs part, and db_part with db");
  const long R = DIM(A, 0), M = DIM(A, 1), N = DIM(B, 1);
  op.require(DIM(B, 0) == R && DIM(out, 0) == M && DIM(out, 1) == N,
             "want A (R,M), B (R,N), out (M,N)");
  // the launcher splits R into at most 32 slices
  float* dbp = P_F32_EQ(db, M);
  float* dbpp = dbp ? P_F32(db_part, 32 * M) : nullptr;
  RUN(fv_gemm_tn(P_F32(A, R * M), P_F32(B, R * N), P_F32(out, M * N),
                 P_F32(part, 32 * M * N), dbp, dbpp, R, M, N, NUM(r_chunks),
                 accumulate, (int)variant, reduce, cur_stream()));
}

// Two weight gradients over a common R and M in one launch (+ one
// reduce): bit-identical to two gemm_tn calls with the same arguments.
void gemm_tn_pair(Tensor A0, Tensor B0, Tensor out0, Tensor A1, Tensor B1,
                  Tensor out1, OptTensor part0, OptTensor part1,
                  long r_chunks, bool accumulate, OptTensor db0,
                  OptTensor db1, OptTensor db_part0, OptTensor db_part1,
                  long variant, bool reduce) {
  OP("gemm_tn_pair", A0);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             " is not 0 or 1");
  op.require(reduce || (part0.has_value() &&
                        (!db0.has_value() || db_part0.has_value())),
             "reduce = false needs part0/part1, and db_part0/1 with db0/1");
  const long R = DIM(A0, 0), M = DIM(A0, 1);
  const long N0 = DIM(B0, 1), N1 = DIM(B1, 1);
  op.require(DIM(A1, 0) == R && DIM(A1, 1) == M && DIM(B0, 0) == R &&
                 DIM(B1, 0) == R, "pair needs a common R and M");
  op.require(DIM(out0, 0) == M && DIM(out0, 1) == N0 && DIM(out1, 0) == M &&
                 DIM(out1, 1) == N1, "want out0 (M,N0), out1 (M,N1)");
  op.require(part0.has_value() == part1.has_value() &&
                 db0.has_value() == db1.has_value() &&
                 db_part0.has_value() == db_part1.has_value(),
             "pair arguments come in twos");
  float* pp0 = P_F32(part0, 32 * M * N0);
  float* pp1 = P_F32(part1, 32 * M * N1);
  op.require(!pp0 || pp0 != pp1, "pair needs two distinct partial workspaces");
  float* dbp0 = P_F32_EQ(db0, M);
  float* dbp1 = P_F32_EQ(db1, M);
  float* dbpp0 = dbp0 ? P_F32(db_part0, 32 * M) : nullptr;
  float* dbpp1 = dbp0 ? P_F32(db_part1, 32 * M) : nullptr;
  op.require(!dbpp0 || dbpp0 != dbpp1,
             "pair needs two distinct db partial workspaces");
  RUN(fv_gemm_tn_pair(P_F32(A0, R * M), P_F32(B0, R * N0),
                      P_F32(out0, M * N0), pp0, dbp0, dbpp0, N0,
                      P_F32(A1, R * M), P_F32(B1, R * N1),
                      P_F32(out1, M * N1), pp1, dbp1, dbpp1, N1, R, M,
                      NUM(r_chunks), accumulate, (int)variant, reduce,
                      cur_stream()));
}

// One reduce launch for up to four sliced weight gradients over a common
// R (gemm_tn / gemm_tn_pair calls with reduce = false and the same
// r_chunks): out_i (+)= sum of part_i's slices, db_i likewise from
// db_part_i where db_i is given. Bit-identical to the reduces those calls
// would have launched themselves. Returns the slice count; at 1 the GEMMs
// wrote out/db directly and nothing is launched.
long tn_reduce_list(std::vector<Tensor> outs, std::vector<Tensor> parts,
                    std::vector<OptTensor> dbs,
                    std::vector<OptTensor> db_parts, long R, long r_chunks,
                    bool accumulate) {
  TORCH_CHECK(!outs.empty(), "tn_reduce_list: outs is empty");
  OP("tn_reduce_list", outs[0]);
  const size_t n = outs.size();
  op.require(n <= 4, "at most 4 problems, got ", n);
  op.require(parts.size() == n && dbs.size() == n && db_parts.size() == n,
             "outs, parts, dbs and db_parts must have one entry per problem");
  NUM(R);
  const long z = r_chunks > 1 ? fv_tn_xhat_slices((int)R) : 1;
  const float* part[4];
  float* out[4];
  const float* db_part[4];
  float* db[4];
  int M[4], N[4];
  for (size_t i = 0; i < n; ++i) {
    const long Mi = op.dim(outs[i], "outs[i]", 0);
    const long Ni = op.dim(outs[i], "outs[i]", 1);
    M[i] = (int)Mi;
    N[i] = (int)Ni;
    out[i] = op.ptr<float>(outs[i], "outs[i]", torch::kFloat32, Mi * Ni,
                           false);
    part[i] = op.ptr<float>(parts[i], "parts[i]", torch::kFloat32,
                            z * Mi * Ni, false);
    db[i] = op.ptr<float>(dbs[i], "dbs[i]", torch::kFloat32, Mi, true);
    op.require(!db[i] || db_parts[i].has_value(),
               "dbs[i] needs db_parts[i]");
    db_part[i] = db[i] ? op.ptr<float>(db_parts[i], "db_parts[i]",
                                       torch::kFloat32, z * Mi, false)
                       : nullptr;
  }
  RUN(fv_tn_reduce_list((int)n, part, out, db_part, db, M, N, (int)z,
                        accumulate, cur_stream()));
  return z;
}

// part[z](M,N) = A[slice z]^T @ ((x - mean) * rstd)[slice z],
// db_part[z](M) = colsum(A[slice z]); returns the slice count z.
long gemm_tn_xhat(Tensor A, Tensor x, Tensor mean, Tensor rstd, Tensor part,
                  Tensor db_part, long variant) {
  OP("gemm_tn_xhat", A);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             " is not 0 or 1");
  const long R = DIM(A, 0), M = DIM(A, 1), N = DIM(x, 1);
  op.require(DIM(x, 0) == R, "want A (R,M), x (R,N)");
  const long nz = fv_tn_xhat_slices(R);
  RUN(fv_gemm_tn_xhat(P_F32(A, R * M), P_F32(x, R * N), P_F32_EQ(mean, R),
                      P_F32_EQ(rstd, R), P_F32(part, nz * M * N),
                      P_F32(db_part, nz * M), R, M, N, (int)variant,
                      cur_stream()));
  return nz;
}

// LayerNorm + W1x parameter gradients from gemm_tn_xhat's slices
void ln_w1x_finish(Tensor part, Tensor db_part, long nz, Tensor W1x,
                   Tensor gamma, Tensor beta, Tensor gW1x, Tensor gb1x,
                   Tensor dgamma, Tensor dbeta) {
  OP("ln_w1x_finish", part);
  const long C = DIM(W1x, 0);
  op.require(W1x.dim() == 2 && W1x.size(1) == C, "W1x must be (C,C)");
  op.require(nz >= 1 && nz <= 32, "nz = ", nz, " is outside 1..32");
  RUN(fv_ln_w1x_finish(P_F32(part, nz * C * C), P_F32(db_part, nz * C),
                       P_F32_EQ(W1x, C * C), P_F32_EQ(gamma, C),
                       P_F32_EQ(beta, C), P_F32_EQ(gW1x, C * C),
                       P_F32_EQ(gb1x, C), P_F32_EQ(dgamma, C),
                       P_F32_EQ(dbeta, C), C, nz, cur_stream()));
}

void colsum(Tensor A, Tensor out, long r_chunks) {
  OP("colsum", A);
  const long R = DIM(A, 0), C = DIM(A, 1);
  RUN(fv_colsum(P_F32(A, R * C), P_F32_EQ(out, C), R, C, NUM(r_chunks),
                cur_stream()));
}

void lrelu_bwd(Tensor dY, Tensor Y, Tensor dZ) {
  OP("lrelu_bwd", dY);
  const int64_t n = dY.numel();
  RUN(fv_lrelu_bwd(P_F32(dY, n), P_F32(Y, n), P_F32(dZ, n), n, cur_stream()));
}

// ---------------------------------------------------------------- bf16
void gemm_nt_bf16(Tensor A, Tensor W, OptTensor bias, OptTensor out_f32,
                  OptTensor out_bf16, double alpha, bool accumulate,
                  bool act_lrelu) {
  OP("gemm_nt_bf16", A);
  const long R = DIM(A, 0), Ci = DIM(A, 1), Co = DIM(W, 0);
  op.require(DIM(W, 1) == Ci, "want A (R,Ci), W (Co,Ci)");
  float* of = P_F32_EQ(out_f32, R * Co);
  void* ob = P_BF16_EQ(out_bf16, R * Co);
  op.require(of || ob, "need at least one output");
  RUN(fv_gemm_nt_bf16(P_BF16(A, R * Ci), P_BF16(W, Co * Ci), P_F32(bias, Co),
                      of, ob, R, Ci, Co, (float)alpha, accumulate, act_lrelu,
                      cur_stream()));
}

void gemm_nn_bf16(Tensor A, Tensor B, OptTensor bias, OptTensor out_f32,
                  OptTensor out_bf16, double alpha, bool accumulate,
                  bool act_lrelu, OptTensor lrelu_bwd_of = c10::nullopt) {
  OP("gemm_nn_bf16", A);
  const long R = DIM(A, 0), Ci = DIM(A, 1), Co = DIM(B, 1);
  op.require(DIM(B, 0) == Ci, "want A (R,Ci), B (Ci,Co)");
  float* of = P_F32_EQ(out_f32, R * Co);
  void* ob = P_BF16_EQ(out_bf16, R * Co);
  op.require(of || ob, "need at least one output");
  RUN(fv_gemm_nn_bf16(P_BF16(A, R * Ci), P_BF16(B, Ci * Co), P_F32(bias, Co),
                      of, ob, P_BF16_EQ(lrelu_bwd_of, R * Co), R, Ci, Co,
                      (float)alpha, accumulate, act_lrelu, cur_stream()));
}

void gemm_tn_bf16(Tensor A, Tensor B, Tensor out, OptTensor part,
                  long r_chunks, bool accumulate, OptTensor db,
                  OptTensor db_part) {
  OP("gemm_tn_bf16", A);
  const long R = DIM(A, 0), M = DIM(A, 1), N = DIM(B, 1);
  op.require(DIM(B, 0) == R && DIM(out, 0) == M && DIM(out, 1) == N,
             "want A (R,M), B (R,N), out (M,N)");
  // the most slices the launcher can choose (its FV_TN_Z cap defaults to
  // and never usefully exceeds 128)
  long zmax = (R + 511) / 512;
  if (zmax > 128) zmax = 128;
  if (zmax < 1 || r_chunks <= 1) zmax = 1;
  float* dbp = P_F32_EQ(db, M);
  float* dbpp = dbp ? P_F32(db_part, zmax * M) : nullptr;
  RUN(fv_gemm_tn_bf16(P_BF16(A, R * M), P_BF16(B, R * N), P_F32(out, M * N),
                      P_F32(part, zmax * M * N), dbp, dbpp, R, M, N,
                      NUM(r_chunks), accumulate, cur_stream()));
}

void gemm_nt_bf16_rs(Tensor A, Tensor Wp, OptTensor bias, OptTensor out_f32,
                     OptTensor out_bf16, OptTensor lrelu_bwd_of, double alpha,
                     bool act_lrelu) {
  OP("gemm_nt_bf16_rs", A);
  const long R = DIM(A, 0), Ci = DIM(A, 1), KP = DIM(Wp, 1);
  op.require(KP == ((Ci + 31) / 32) * 32, "Wp must be k-padded to 32");
  // Co comes from whichever of bias / out_f32 / out_bf16 is given last
  long Co = -1;
  if (bias.has_value()) Co = NUM(bias->numel());
  if (out_f32.has_value()) Co = DIM(*out_f32, 1);
  if (out_bf16.has_value()) Co = DIM(*out_bf16, 1);
  op.require(out_f32.has_value() || out_bf16.has_value(),
             "need at least one output");
  op.require(DIM(Wp, 0) >= Co, "Wp rows < Co");
  RUN(fv_gemm_nt_bf16_rs(P_BF16(A, R * Ci), P_BF16(Wp, Co * KP),
                         P_F32(bias, Co), P_F32_EQ(out_f32, R * Co),
                         P_BF16_EQ(out_bf16, R * Co),
                         P_BF16_EQ(lrelu_bwd_of, R * Co), R, Ci, Co, KP,
                         (float)alpha, act_lrelu, cur_stream()));
}

// s1 (M1,N1) -> d1 (M1,KPn1) and its transpose d1t (N1,KPm1), the same for
// s2, and s3 -> d3 elementwise
void cast_shadows(Tensor s1, Tensor d1, Tensor d1t, Tensor s2, Tensor d2,
                  Tensor d2t, Tensor s3, Tensor d3) {
  OP("cast_shadows", s1);
  const long M1 = DIM(s1, 0), N1 = DIM(s1, 1);
  const long M2 = DIM(s2, 0), N2 = DIM(s2, 1);
  op.require(DIM(d1, 0) == M1 && DIM(d1t, 0) == N1 && DIM(d2, 0) == M2 &&
                 DIM(d2t, 0) == N2, "shadow rows do not match their source");
  const long KPn1 = DIM(d1, 1), KPm1 = DIM(d1t, 1);
  const long KPn2 = DIM(d2, 1), KPm2 = DIM(d2t, 1);
  op.require(KPn1 >= N1 && KPm1 >= M1 && KPn2 >= N2 && KPm2 >= M2,
             "shadow rows are shorter than their source");
  const int64_t n3 = s3.numel();
  RUN(fv_cast_shadows(P_F32(s1, M1 * N1), P_BF16(d1, M1 * KPn1),
                      P_BF16(d1t, N1 * KPm1), M1, N1, KPn1, KPm1,
                      P_F32(s2, M2 * N2), P_BF16(d2, M2 * KPn2),
                      P_BF16(d2t, N2 * KPm2), M2, N2, KPn2, KPm2,
                      P_F32(s3, n3), P_BF16(d3, n3), n3, cur_stream()));
}

void cast_f32_bf16(Tensor src, Tensor dst) {
  OP("cast_f32_bf16", src);
  const int64_t n = src.numel();
  RUN(fv_cast_f32_bf16(P_F32(src, n), P_BF16_EQ(dst, n), n, cur_stream()));
}

void lrelu_bwd_bf16(Tensor dY, Tensor Y, Tensor dZ) {
  OP("lrelu_bwd_bf16", dY);
  const int64_t n = dY.numel();
  RUN(fv_lrelu_bwd_bf16(P_BF16(dY, n), P_BF16(Y, n), P_BF16(dZ, n), n,
                        cur_stream()));
}

// fixed-order sum of z per-block wgrad partials: out = sum part[z],
// db = sum db_part[z]
void wgrad_reduce(Tensor part, Tensor out, Tensor db_part, Tensor db, long z,
                  bool accumulate) {
  OP("wgrad_reduce", part);
  const int64_t elems = out.numel(), m_elems = db.numel();
  NUM(z);
  RUN(fv_wgrad_reduce(P_F32(part, z * elems), P_F32(out, elems), elems,
                      P_F32(db_part, z * m_elems), P_F32(db, m_elems),
                      m_elems, z, accumulate, cur_stream()));
}

// ------------------------------------------------------------ extractor
void ln_fwd(Tensor x, Tensor gamma, Tensor beta, OptTensor xln, Tensor mean,
            Tensor rstd, double eps, OptTensor xln_bf = c10::nullopt,
            OptTensor xln_f8 = c10::nullopt) {
  OP("ln_fwd", x);
  const long C = DIM(x, -1);
  op.require(C >= 1, "x has no columns");
  const int64_t R = x.numel() / C;
  const long f8_ld = xln_f8.has_value() ? DIM(*xln_f8, -1) : 0;
  op.require(!xln_f8.has_value() || f8_ld >= C, "xln_f8 rows shorter than C");
  float* xo = P_F32(xln, R * C);
  void* xb = P_BF16(xln_bf, R * C);
  void* x8 = P_FP8(xln_f8, R * f8_ld);
  op.require(xo || xb || x8, "needs an output");
  RUN(fv_ln_fwd(P_F32(x, R * C), P_F32_EQ(gamma, C), P_F32_EQ(beta, C), xo,
                xb, x8, f8_ld, P_F32(mean, R), P_F32(rstd, R), R, C,
                (float)eps, cur_stream()));
}

// LayerNorm -> lrelu(xln @ W1x^T + b1x) -> xp @ Wih^T + bih in one launch,
// bit-identical to ln_fwd + two gemm_nt calls. Returns false, launching
// nothing, when the shape is outside the kernel's limits (extractor.hip).
bool extractor_head_fwd(Tensor x, Tensor gamma, Tensor beta, Tensor W1x,
                        Tensor b1x, Tensor Wih, Tensor bih, OptTensor xln,
                        Tensor mean, Tensor rstd, Tensor xp, Tensor gi,
                        double eps, int64_t strip) {
  OP("extractor_head_fwd", x);
  const long C = DIM(x, -1), G = DIM(Wih, 0);
  op.require(C >= 1, "x has no columns");
  const int64_t R = x.numel() / C;
  op.require(W1x.dim() == 2 && W1x.size(0) == C && W1x.size(1) == C,
             "W1x must be (C,C)");
  op.require(Wih.dim() == 2 && Wih.size(1) == C, "Wih must be (G,C)");
  int ran = 0;
  RUN(fv_extractor_head_fwd(
      P_F32(x, R * C), P_F32_EQ(gamma, C), P_F32_EQ(beta, C),
      P_F32_EQ(W1x, C * C), P_F32_EQ(b1x, C), P_F32_EQ(Wih, G * C),
      P_F32_EQ(bih, G), P_F32_EQ(xln, R * C), P_F32_EQ(mean, R),
      P_F32_EQ(rstd, R), P_F32_EQ(xp, R * C), P_F32_EQ(gi, R * G), R, C, G,
      (float)eps, NUM(strip), &ran, cur_stream()));
  return ran != 0;
}

void ln_bwd_params(Tensor x, Tensor dxln, Tensor mean, Tensor rstd,
                   Tensor part, Tensor dgamma, Tensor dbeta, long r_chunks) {
  OP("ln_bwd_params", x);
  const long C = DIM(x, -1);
  op.require(C >= 1, "x has no columns");
  const int64_t R = x.numel() / C;
  const long yblocks = fv_ln_bwd_yblocks(R, C);
  RUN(fv_ln_bwd_params(P_F32(x, R * C), P_F32(dxln, R * C), P_F32(mean, R),
                       P_F32(rstd, R), P_F32(part, yblocks * 2 * C),
                       P_F32_EQ(dgamma, C), P_F32_EQ(dbeta, C), R, C,
                       NUM(r_chunks), cur_stream()));
}

// ln_bwd_params' second kernel alone: dgamma, dbeta from the partials that
// gemm_nn_ln wrote for R rows of C columns
void ln_bwd_reduce(Tensor part, Tensor dgamma, Tensor dbeta, long R, long C) {
  OP("ln_bwd_reduce", part);
  op.require(R >= 1 && C >= 1, "R = ", R, ", C = ", C, " must be positive");
  NUM(C);
  const long yblocks = fv_ln_bwd_yblocks(R, (int)C);
  RUN(fv_ln_bwd_reduce(P_F32(part, yblocks * 2 * C), P_F32_EQ(dgamma, C),
                       P_F32_EQ(dbeta, C), R, (int)C, cur_stream()));
}

// ----------------------------------------------------------------- fp8
// A/W fp8 (R, lda)/(Co, ldw) padded; logical K = Ci. Outputs optional.
void gemm_nt_fp8(Tensor A, Tensor W, OptTensor bias, OptTensor inv_sw,
                 OptTensor out_f32, OptTensor out_bf16, OptTensor out_fp8,
                 long R, long Ci, long Co, double alpha, bool act_lrelu) {
  OP("gemm_nt_fp8", A);
  NUM(R); NUM(Ci); NUM(Co);
  const long lda = DIM(A, 1), ldw = DIM(W, 1);
  op.require(DIM(A, 0) >= R && lda >= Ci && DIM(W, 0) >= Co && ldw >= Ci,
             "A / W smaller than R, Ci, Co");
  const long ldo = out_fp8.has_value() ? DIM(*out_fp8, -1) : 0;
  op.require(!out_fp8.has_value() || ldo >= Co, "out_fp8 rows shorter than Co");
  const float* b = P_F32(bias, Co);
  float* of = P_F32(out_f32, R * Co);
  void* ob = P_BF16(out_bf16, R * Co);
  void* o8 = P_FP8(out_fp8, R * ldo);
  op.require(of || ob || o8, "need at least one output");
  RUN(fv_gemm_nt_fp8(P_FP8(A, R * lda), P_FP8(W, Co * ldw), b,
                     P_F32(inv_sw, 1), of, ob, o8, ldo, R, Ci, Co, lda, ldw,
                     (float)alpha, act_lrelu, b != nullptr, cur_stream()));
}

void gemm_nt_fp8_rs(Tensor A, Tensor Wp, OptTensor bias, OptTensor inv_sw,
                    OptTensor out_f32, OptTensor out_bf16, OptTensor out_fp8,
                    long R, long Ci, long Co, double alpha, bool act_lrelu,
                    OptTensor inv_sa = c10::nullopt,
                    OptTensor lrelu_bwd_of = c10::nullopt,
                    OptTensor s_out = c10::nullopt,
                    OptTensor amax_out = c10::nullopt) {
  OP("gemm_nt_fp8_rs", A);
  NUM(R); NUM(Ci); NUM(Co);
  const long KP = DIM(A, 1);
  op.require(DIM(Wp, 1) == KP && (KP & 127) == 0 && KP >= Ci,
             "A/Wp must share a 128-padded k stride");
  op.require(DIM(A, 0) >= R && DIM(Wp, 0) >= Co,
             "A / Wp smaller than R, Co");
  const long ldo = out_fp8.has_value() ? DIM(*out_fp8, -1) : 0;
  op.require(!out_fp8.has_value() || ldo >= Co, "out_fp8 rows shorter than Co");
  const float* b = P_F32(bias, Co);
  float* of = P_F32(out_f32, R * Co);
  void* ob = P_BF16(out_bf16, R * Co);
  void* o8 = P_FP8(out_fp8, R * ldo);
  op.require(of || ob || o8, "need at least one output");
  RUN(fv_gemm_nt_fp8_rs(P_FP8(A, R * KP), P_FP8(Wp, Co * KP), b,
                        P_F32(inv_sw, 1), P_F32(inv_sa, 1),
                        P_BF16(lrelu_bwd_of, R * Co), P_F32(s_out, 1),
                        P_F32(amax_out, 1), of, ob, o8, ldo, R, Ci, Co, KP,
                        (float)alpha, act_lrelu, b != nullptr, cur_stream()));
}

void scale_from_amax2(Tensor amax1, Tensor s1, Tensor is1, Tensor amax2,
                      Tensor s2, Tensor is2) {
  OP("scale_from_amax2", amax1);
  RUN(fv_scale_from_amax2(P_F32(amax1, 1), P_F32(s1, 1), P_F32(is1, 1),
                          P_F32(amax2, 1), P_F32(s2, 1), P_F32(is2, 1),
                          cur_stream()));
}

void cast_f32_fp8_damax(Tensor src, Tensor dst, Tensor s, Tensor amax_out) {
  OP("cast_f32_fp8_damax", src);
  const long cols = DIM(src, -1), ldp = DIM(dst, -1);
  op.require(cols >= 1 && ldp >= cols, "dst rows shorter than src's");
  const int64_t rows = src.numel() / cols;
  RUN(fv_cast_f32_fp8_damax(P_F32(src, rows * cols), P_FP8(dst, rows * ldp),
                            P_F32(s, 1), P_F32(amax_out, 1), rows, cols, ldp,
                            cur_stream()));
}

void cast_f32_fp8_scaled_t(Tensor src, Tensor dstT, Tensor scale) {
  OP("cast_f32_fp8_scaled_t", src);
  const long M = DIM(src, 0), N = DIM(src, 1), ldp = DIM(dstT, 1);
  op.require(DIM(dstT, 0) >= N && ldp >= M, "dstT smaller than (N,M)");
  RUN(fv_cast_f32_fp8_scaled_t(P_F32(src, M * N), P_FP8(dstT, N * ldp),
                               P_F32(scale, 1), M, N, ldp, cur_stream()));
}

void absmax_scale(Tensor src, Tensor scale, Tensor inv_scale) {
  OP("absmax_scale", src);
  const int64_t n = src.numel();
  RUN(fv_absmax_scale(P_F32(src, n), n, P_F32(scale, 1),
                      P_F32(inv_scale, 1), cur_stream()));
}

void cast_f32_fp8_scaled(Tensor src, Tensor dst, OptTensor scale) {
  OP("cast_f32_fp8_scaled", src);
  const long cols = DIM(src, -1), ldp = DIM(dst, -1);
  op.require(cols >= 1 && ldp >= cols, "dst rows shorter than src's");
  const int64_t rows = src.numel() / cols;
  RUN(fv_cast_f32_fp8_scaled(P_F32(src, rows * cols), P_FP8(dst, rows * ldp),
                             P_F32(scale, 1), rows, cols, ldp, cur_stream()));
}

// ----------------------------------------------------------------- GRU
// gi (N,T,3H); h_final (N,H); h_seq / h_prev (N,T,H); gates4 (N,T,4H)
// variant: 1 = wave-per-stock kernels where they apply (default), 0 = the
// kernels from before them (bit-identical)
void gru_fwd(Tensor gi, Tensor Whh, Tensor bhh, Tensor h_final,
             OptTensor h_seq, Tensor h_prev, Tensor gates4, long N, long T,
             long H, long variant = 1) {
  OP("gru_fwd", gi);
  NUM(N); NUM(T); NUM(H);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             ", must be 0 or 1");
  RUN(fv_gru_fwd(P_F32(gi, N * T * 3 * H), P_F32_EQ(Whh, 3 * H * H),
                 P_F32_EQ(bhh, 3 * H), P_F32(h_final, N * H),
                 P_F32(h_seq, N * T * H), P_F32(h_prev, N * T * H),
                 P_F32(gates4, N * T * 4 * H), N, T, H, (int)variant,
                 cur_stream()));
}

// With the six dh_combine operands (ds / a (N,K), qk / du (K,H), dscores
// (N,M), Wenc (M,H)) dh_final is the decoder's dh, and the kernel forms
// dh_combine's sum itself and leaves it in dh_final. That exists on the
// wave route only (H = 64, N <= gru_wave_max_n(), fp32 outputs, variant 1):
// returns true when it ran that way. With the operands and off that route
// it launches NOTHING and returns false; the caller runs dh_combine and
// calls again without them. Without the operands it returns false.
bool gru_bwd(Tensor dh_final, Tensor h_prev, Tensor gates4, Tensor Whh,
             Tensor dgi, Tensor dgh, long N, long T, long H,
             OptTensor dgi_bf = c10::nullopt,
             OptTensor dgh_bf = c10::nullopt, long variant = 1,
             OptTensor ds = c10::nullopt, OptTensor qk = c10::nullopt,
             OptTensor a = c10::nullopt, OptTensor du = c10::nullopt,
             OptTensor dscores = c10::nullopt,
             OptTensor Wenc = c10::nullopt) {
  OP("gru_bwd", dh_final);
  NUM(N); NUM(T); NUM(H);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             ", must be 0 or 1");
  const long G = N * T * 3 * H;
  const bool comb = ds.has_value();
  op.require(comb == qk.has_value() && comb == a.has_value() &&
                 comb == du.has_value() && comb == dscores.has_value() &&
                 comb == Wenc.has_value(),
             "ds, qk, a, du, dscores, Wenc come as a set of six");
  if (comb) {
    if (dgi_bf.has_value() || dgh_bf.has_value()) return false;
    const long K = op.dim(*qk, "qk", 0), M = op.dim(*Wenc, "Wenc", 0);
    op.require(op.dim(*qk, "qk", 1) == H && op.dim(*Wenc, "Wenc", 1) == H,
               "qk / Wenc must have H columns");
    int fused = 0;
    RUN(fv_gru_bwd_combine(
        P_F32(dh_final, N * H), P_F32(ds, N * K), P_F32(qk, K * H),
        P_F32(a, N * K), P_F32(du, K * H), P_F32(dscores, N * M),
        P_F32_EQ(Wenc, M * H), K, M, P_F32(h_prev, N * T * H),
        P_F32(gates4, N * T * 4 * H), P_F32_EQ(Whh, 3 * H * H), P_F32(dgi, G),
        P_F32(dgh, G), N, T, H, (int)variant, &fused, cur_stream()));
    return fused != 0;
  }
  RUN(fv_gru_bwd(P_F32(dh_final, N * H), P_F32(h_prev, N * T * H),
                 P_F32(gates4, N * T * 4 * H), P_F32_EQ(Whh, 3 * H * H),
                 P_F32(dgi, G), P_F32(dgh, G), P_BF16(dgi_bf, G),
                 P_BF16(dgh_bf, G), N, T, H, (int)variant, cur_stream()));
  return false;
}

void gru_fwd_mfma(Tensor gi, Tensor whh_bf, Tensor bhh, Tensor h_final,
                  OptTensor h_seq, Tensor h_prev, Tensor gates4, long N,
                  long T, long H) {
  OP("gru_fwd_mfma", gi);
  NUM(N); NUM(T); NUM(H);
  RUN(fv_gru_fwd_mfma(P_F32(gi, N * T * 3 * H), P_BF16_EQ(whh_bf, 3 * H * H),
                      P_F32_EQ(bhh, 3 * H), P_F32(h_final, N * H),
                      P_F32(h_seq, N * T * H), P_F32(h_prev, N * T * H),
                      P_F32(gates4, N * T * 4 * H), N, T, H, cur_stream()));
}

// dgi_f8 (N*T, ld8) e4m3 comes with s_dgi and amax_dgi; whh_part / bhh_part
// take one (3H,H) / (3H) wgrad partial per workgroup
void gru_bwd_mfma(Tensor dh_final, Tensor h_prev, Tensor gates4,
                  Tensor whh_bf, OptTensor dgi, OptTensor dgh, long N, long T,
                  long H, OptTensor dgi_bf = c10::nullopt,
                  OptTensor dgh_bf = c10::nullopt,
                  OptTensor dgi_f8 = c10::nullopt,
                  OptTensor s_dgi = c10::nullopt,
                  OptTensor amax_dgi = c10::nullopt,
                  OptTensor whh_part = c10::nullopt,
                  OptTensor bhh_part = c10::nullopt) {
  OP("gru_bwd_mfma", dh_final);
  NUM(N); NUM(T); NUM(H);
  const long G = N * T * 3 * H;
  const long ld8 = dgi_f8.has_value() ? DIM(*dgi_f8, -1) : 0;
  op.require(!dgi_f8.has_value() || (ld8 >= 3 * H && s_dgi.has_value() &&
                                     amax_dgi.has_value()),
             "dgi_f8 needs rows of 3H or more, s_dgi and amax_dgi");
  op.require(!whh_part.has_value() || bhh_part.has_value(),
             "whh_part needs bhh_part");
  const long nblk = fv_gru_wgrad_blocks(N);
  float* gi = P_F32(dgi, G);
  void* gib = P_BF16(dgi_bf, G);
  void* g8 = P_FP8(dgi_f8, N * T * ld8);
  op.require(gi || gib || g8, "needs a dgi output");
  float* wp = P_F32(whh_part, nblk * 3 * H * H);
  RUN(fv_gru_bwd_mfma(P_F32(dh_final, N * H), P_F32(h_prev, N * T * H),
                      P_F32(gates4, N * T * 4 * H),
                      P_BF16_EQ(whh_bf, 3 * H * H), gi, P_F32(dgh, G), gib,
                      P_BF16(dgh_bf, G), g8, ld8,
                      g8 ? P_F32(s_dgi, 1) : nullptr,
                      g8 ? P_F32(amax_dgi, 1) : nullptr, wp,
                      wp ? P_F32(bhh_part, nblk * 3 * H) : nullptr, N, T, H,
                      cur_stream()));
}

// Inference forward: h_final only, no backward state
void gru_fwd_infer(Tensor gi, Tensor Whh, Tensor bhh, Tensor h_final, long N,
                   long T, long H, long variant = 1) {
  OP("gru_fwd_infer", gi);
  NUM(N); NUM(T); NUM(H);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             ", must be 0 or 1");
  RUN(fv_gru_fwd_infer(P_F32(gi, N * T * 3 * H), P_F32_EQ(Whh, 3 * H * H),
                       P_F32_EQ(bhh, 3 * H), P_F32(h_final, N * H), N, T, H,
                       (int)variant, cur_stream()));
}

void gru_fwd_mfma_infer(Tensor gi, Tensor whh_bf, Tensor bhh, Tensor h_final,
                        long N, long T, long H) {
  OP("gru_fwd_mfma_infer", gi);
  NUM(N); NUM(T); NUM(H);
  RUN(fv_gru_fwd_mfma_infer(P_F32(gi, N * T * 3 * H),
                            P_BF16_EQ(whh_bf, 3 * H * H),
                            P_F32_EQ(bhh, 3 * H), P_F32(h_final, N * H), N, T,
                            H, cur_stream()));
}

// The gather forms: gi_rows (U,3H), idx int32 (N,T); step t of stock n reads
// row idx[n*T + t], an index outside [0,U) is a missing row (NaN h_final)
void gru_fwd_infer_gather(Tensor gi_rows, long U, Tensor idx, Tensor Whh,
                          Tensor bhh, Tensor h_final, long N, long T, long H,
                          long variant = 1) {
  OP("gru_fwd_infer_gather", gi_rows);
  NUM(U); NUM(N); NUM(T); NUM(H);
  op.require(variant == 0 || variant == 1, "variant = ", variant,
             ", must be 0 or 1");
  RUN(fv_gru_fwd_infer_gather(P_F32(gi_rows, U * 3 * H), U, P_I32(idx, N * T),
                              P_F32_EQ(Whh, 3 * H * H), P_F32_EQ(bhh, 3 * H),
                              P_F32(h_final, N * H), N, T, H, (int)variant,
                              cur_stream()));
}

void gru_fwd_mfma_infer_gather(Tensor gi_rows, long U, Tensor idx,
                               Tensor whh_bf, Tensor bhh, Tensor h_final,
                               long N, long T, long H) {
  OP("gru_fwd_mfma_infer_gather", gi_rows);
  NUM(U); NUM(N); NUM(T); NUM(H);
  RUN(fv_gru_fwd_mfma_infer_gather(P_F32(gi_rows, U * 3 * H), U,
                                   P_I32(idx, N * T),
                                   P_BF16_EQ(whh_bf, 3 * H * H),
                                   P_F32_EQ(bhh, 3 * H), P_F32(h_final, N * H),
                                   N, T, H, cur_stream()));
}

// ------------------------------------------------------------ attention
// h (N,H); qk (K,H); per-head weights Wv (K,H,H), bv (K,H); the predictor
// MLP Wl (H,H), bl / wmu / wsig (H), bmu / bsig (1); a / sd / mask (N,K);
// u / ctx / hm2 (K,H); guard int32 (K); pmu ... psig_c (K).
// variant: 1 = latency-oriented kernel (default), 0 = original kernel
void attn_fused_fwd(Tensor h, Tensor qk, Tensor cb, OptTensor mask, Tensor Wv,
                    Tensor bv, Tensor Wl, Tensor bl, Tensor wmu, Tensor bmu,
                    Tensor wsig, Tensor bsig, Tensor a, Tensor sd,
                    Tensor guard, Tensor u, Tensor ctx, Tensor hm2,
                    Tensor pmu, Tensor psig_pre, Tensor psig, Tensor psig_c,
                    double alpha, double keep_inv, int variant) {
  OP("attn_fused_fwd", h);
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(qk, 0);
  op.require(DIM(qk, 1) == H, "qk must be (K,H)");
  RUN(fv_attn_fused_fwd(
      P_F32(h, N * H), P_F32_EQ(qk, K * H), P_F32_EQ(cb, K),
      P_F32(mask, N * K), P_F32_EQ(Wv, K * H * H), P_F32_EQ(bv, K * H),
      P_F32_EQ(Wl, H * H), P_F32_EQ(bl, H), P_F32_EQ(wmu, H),
      P_F32_EQ(bmu, 1), P_F32_EQ(wsig, H), P_F32_EQ(bsig, 1),
      P_F32(a, N * K), P_F32(sd, N * K), P_I32(guard, K), P_F32(u, K * H),
      P_F32(ctx, K * H), P_F32(hm2, K * H), P_F32(pmu, K),
      P_F32(psig_pre, K), P_F32(psig, K), P_F32(psig_c, K), N, K, H,
      (float)alpha, (float)keep_inv, variant, cur_stream()));
}

// q / bk (K,H), Wk (K,H,H) and their gradients; hpart K * (2H + 2) floats.
// In-kernel KL gradients: kl_* all four or none; dpmu and dpsig_c are then
// outputs.
void attn_fused_bwd(Tensor dpmu, Tensor dpsig_c, Tensor psig,
                    Tensor psig_pre, Tensor hm2, Tensor wmu, Tensor wsig,
                    Tensor Wl, Tensor h, Tensor a, Tensor sd, OptTensor mask,
                    Tensor guard, Tensor u, Tensor Wv, Tensor q, Tensor Wk,
                    Tensor bk, Tensor dz2, Tensor du, Tensor ds, Tensor dc,
                    Tensor dWv, Tensor dbv, Tensor dq, Tensor dWk, Tensor dbk,
                    Tensor hpart, Tensor dwmu, Tensor dbmu, Tensor dwsig,
                    Tensor dbsig, double alpha, double keep_inv, int variant,
                    OptTensor kl_fmu = c10::nullopt,
                    OptTensor kl_fsig_c = c10::nullopt,
                    OptTensor kl_pmu = c10::nullopt,
                    OptTensor kl_psig_c = c10::nullopt,
                    double kl_gscale = 1.0) {
  OP("attn_fused_bwd", dpmu);
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(q, 0);
  op.require(DIM(q, 1) == H, "q must be (K,H)");
  op.require(kl_fmu.has_value() == kl_fsig_c.has_value() &&
                 kl_fmu.has_value() == kl_pmu.has_value() &&
                 kl_fmu.has_value() == kl_psig_c.has_value(),
             "kl_* come as a set of four");
  RUN(fv_attn_fused_bwd(
      P_F32(dpmu, K), P_F32(dpsig_c, K), P_F32(psig, K), P_F32(psig_pre, K),
      P_F32(hm2, K * H), P_F32_EQ(wmu, H), P_F32_EQ(wsig, H),
      P_F32_EQ(Wl, H * H), P_F32(h, N * H), P_F32(a, N * K), P_F32(sd, N * K),
      P_F32(mask, N * K), P_I32(guard, K), P_F32(u, K * H),
      P_F32_EQ(Wv, K * H * H), P_F32_EQ(q, K * H), P_F32_EQ(Wk, K * H * H),
      P_F32_EQ(bk, K * H), P_F32(dz2, K * H), P_F32(du, K * H),
      P_F32(ds, N * K), P_F32(dc, K), P_F32_EQ(dWv, K * H * H),
      P_F32_EQ(dbv, K * H), P_F32_EQ(dq, K * H), P_F32_EQ(dWk, K * H * H),
      P_F32_EQ(dbk, K * H), P_F32(hpart, K * (2 * H + 2)), P_F32_EQ(dwmu, H),
      P_F32_EQ(dbmu, 1), P_F32_EQ(dwsig, H), P_F32_EQ(dbsig, 1), N, K, H,
      (float)alpha, (float)keep_inv, variant, P_F32(kl_fmu, K),
      P_F32(kl_fsig_c, K), P_F32(kl_pmu, K), P_F32(kl_psig_c, K),
      (float)kl_gscale, cur_stream()));
}

void attn_qk_fwd(Tensor q, Tensor Wk, Tensor bk, Tensor qk, Tensor c) {
  OP("attn_qk_fwd", q);
  const long K = DIM(q, 0), H = DIM(q, 1);
  RUN(fv_attn_qk_fwd(P_F32_EQ(q, K * H), P_F32_EQ(Wk, K * H * H),
                     P_F32_EQ(bk, K * H), P_F32(qk, K * H), P_F32(c, K), K, H,
                     cur_stream()));
}

void attn_softmax_fwd(Tensor s, OptTensor mask, Tensor a, Tensor sd,
                      Tensor guard, double keep_inv) {
  OP("attn_softmax_fwd", s);
  const long N = DIM(s, 0), K = DIM(s, 1);
  RUN(fv_attn_softmax_fwd(P_F32(s, N * K), P_F32(mask, N * K),
                          P_F32(a, N * K), P_F32(sd, N * K), P_I32(guard, K),
                          N, K, (float)keep_inv, cur_stream()));
}

void attn_ctx_fwd(Tensor u, Tensor Wv, Tensor bv, Tensor guard, Tensor ctx) {
  OP("attn_ctx_fwd", u);
  const long K = DIM(u, 0), H = DIM(u, 1);
  RUN(fv_attn_ctx_fwd(P_F32(u, K * H), P_F32_EQ(Wv, K * H * H),
                      P_F32_EQ(bv, K * H), P_I32(guard, K), P_F32(ctx, K * H),
                      K, H, cur_stream()));
}

void attn_head_bwd(Tensor dctx, Tensor u, Tensor Wv, Tensor guard, Tensor du,
                   Tensor dWv, Tensor dbv) {
  OP("attn_head_bwd", dctx);
  const long K = DIM(u, 0), H = DIM(u, 1);
  RUN(fv_attn_head_bwd(P_F32(dctx, K * H), P_F32(u, K * H),
                       P_F32_EQ(Wv, K * H * H), P_I32(guard, K),
                       P_F32(du, K * H), P_F32_EQ(dWv, K * H * H),
                       P_F32_EQ(dbv, K * H), K, H, cur_stream()));
}

void attn_softmax_bwd(Tensor da, Tensor a, Tensor sd, OptTensor mask,
                      Tensor guard, Tensor ds, Tensor dc, double keep_inv,
                      double alpha) {
  OP("attn_softmax_bwd", da);
  const long N = DIM(a, 0), K = DIM(a, 1);
  RUN(fv_attn_softmax_bwd(P_F32(da, N * K), P_F32(a, N * K), P_F32(sd, N * K),
                          P_F32(mask, N * K), P_I32(guard, K),
                          P_F32(ds, N * K), P_F32(dc, K), N, K,
                          (float)keep_inv, (float)alpha, cur_stream()));
}

void attn_qk_bwd(Tensor dqk, Tensor dc, Tensor q, Tensor Wk, Tensor bk,
                 Tensor dq, Tensor dWk, Tensor dbk) {
  OP("attn_qk_bwd", dqk);
  const long K = DIM(q, 0), H = DIM(q, 1);
  RUN(fv_attn_qk_bwd(P_F32(dqk, K * H), P_F32(dc, K), P_F32_EQ(q, K * H),
                     P_F32_EQ(Wk, K * H * H), P_F32_EQ(bk, K * H),
                     P_F32_EQ(dq, K * H), P_F32_EQ(dWk, K * H * H),
                     P_F32_EQ(dbk, K * H), K, H, cur_stream()));
}

void pred_mlp_fwd(Tensor ctx, Tensor Wl, Tensor bl, Tensor wmu, Tensor bmu,
                  Tensor wsig, Tensor bsig, Tensor hm2, Tensor pmu,
                  Tensor psig_pre, Tensor psig, Tensor psig_c) {
  OP("pred_mlp_fwd", ctx);
  const long K = DIM(ctx, 0), H = DIM(ctx, 1);
  RUN(fv_pred_mlp_fwd(P_F32(ctx, K * H), P_F32_EQ(Wl, H * H), P_F32_EQ(bl, H),
                      P_F32_EQ(wmu, H), P_F32_EQ(bmu, 1), P_F32_EQ(wsig, H),
                      P_F32_EQ(bsig, 1), P_F32(hm2, K * H), P_F32(pmu, K),
                      P_F32(psig_pre, K), P_F32(psig, K), P_F32(psig_c, K), K,
                      H, cur_stream()));
}

void pred_mlp_bwd(Tensor dpmu, Tensor dpsig_c, Tensor psig, Tensor psig_pre,
                  Tensor hm2, Tensor wmu, Tensor wsig, Tensor dz2,
                  Tensor hpart, Tensor dwmu, Tensor dbmu, Tensor dwsig,
                  Tensor dbsig) {
  OP("pred_mlp_bwd", dpmu);
  const long K = DIM(hm2, 0), H = DIM(hm2, 1);
  RUN(fv_pred_mlp_bwd(P_F32(dpmu, K), P_F32(dpsig_c, K), P_F32(psig, K),
                      P_F32(psig_pre, K), P_F32(hm2, K * H), P_F32_EQ(wmu, H),
                      P_F32_EQ(wsig, H), P_F32(dz2, K * H),
                      P_F32(hpart, K * (2 * H + 2)), P_F32_EQ(dwmu, H),
                      P_F32_EQ(dbmu, 1), P_F32_EQ(dwsig, H),
                      P_F32_EQ(dbsig, 1), K, H, cur_stream()));
}

void dh_combine(Tensor dh, Tensor ds, Tensor qk, Tensor a, Tensor du,
                Tensor dscores, Tensor Wenc) {
  OP("dh_combine", dh);
  const long N = DIM(dh, 0), H = DIM(dh, 1);
  const long K = DIM(qk, 0), M = DIM(Wenc, 0);
  op.require(DIM(ds, 0) == N && DIM(ds, 1) == K, "ds must be (N,K)");
  op.require(a.sizes() == ds.sizes(), "a must be (N,K)");
  op.require(du.sizes() == qk.sizes(), "du must be (K,H)");
  op.require(DIM(dscores, 0) == N && DIM(dscores, 1) == M,
             "dscores must be (N,M)");
  op.require(DIM(Wenc, 1) == H && DIM(qk, 1) == H, "Wenc / qk must have H columns");
  RUN(fv_dh_combine(P_F32(dh, N * H), P_F32(ds, N * K), P_F32(qk, K * H),
                    P_F32(a, N * K), P_F32(du, K * H), P_F32(dscores, N * M),
                    P_F32_EQ(Wenc, M * H), N, K, M, H, cur_stream()));
}

// -------------------------------------------------------------- encoder
// h (N,H); Wenc (M,H); scores / a (N,M); yp (M); the heads Wmu / Wsig (K,M),
// bmu / bsig (K) write fmu ... fsig_c (K) and need the int32 done counter
void enc_fused_fwd(Tensor h, Tensor Wenc, Tensor benc, Tensor y,
                   Tensor scores, Tensor a, Tensor yp,
                   OptTensor Wmu = c10::nullopt, OptTensor bmu = c10::nullopt,
                   OptTensor Wsig = c10::nullopt,
                   OptTensor bsig = c10::nullopt,
                   OptTensor fmu = c10::nullopt,
                   OptTensor fsig_pre = c10::nullopt,
                   OptTensor fsig = c10::nullopt,
                   OptTensor fsig_c = c10::nullopt,
                   OptTensor done = c10::nullopt, int variant = 1) {
  OP("enc_fused_fwd", h);
  const long N = DIM(h, 0), H = DIM(h, 1), M = DIM(Wenc, 0);
  const bool heads = fmu.has_value();
  op.require(!heads || (Wmu.has_value() && bmu.has_value() &&
                        Wsig.has_value() && bsig.has_value() &&
                        fsig_pre.has_value() && fsig.has_value() &&
                        fsig_c.has_value() && done.has_value()),
             "fused heads need Wmu, bmu, Wsig, bsig, the four outputs and "
             "an int32 done counter");
  // without fmu the head arguments are not looked at
  const long K = heads ? op.num(fmu->numel(), "fmu") : 0;
  const float *wm = nullptr, *bm = nullptr, *ws = nullptr, *bs = nullptr;
  float *fm = nullptr, *fsp = nullptr, *fs = nullptr, *fsc = nullptr;
  int* dn = nullptr;
  if (heads) {
    wm = P_F32_EQ(Wmu, K * M); bm = P_F32_EQ(bmu, K);
    ws = P_F32_EQ(Wsig, K * M); bs = P_F32_EQ(bsig, K);
    fm = P_F32(fmu, K); fsp = P_F32(fsig_pre, K); fs = P_F32(fsig, K);
    fsc = P_F32(fsig_c, K); dn = P_I32(done, 1);
  }
  RUN(fv_enc_fused_fwd(P_F32(h, N * H), P_F32_EQ(Wenc, M * H),
                       P_F32_EQ(benc, M), P_F32(y, N), P_F32(scores, N * M),
                       P_F32(a, N * M), P_F32(yp, M), wm, bm, ws, bs, fm, fsp,
                       fs, fsc, dn, K, N, M, H, variant, cur_stream()));
}

void enc_bwd_fused(Tensor dfmu, Tensor dfsig_c, Tensor fsig, Tensor fsig_pre,
                   Tensor yp, Tensor Wmu, Tensor Wsig, Tensor a, Tensor y,
                   Tensor dscores, Tensor dWmu, Tensor dbmu, Tensor dWsig,
                   Tensor dbsig) {
  OP("enc_bwd_fused", dfmu);
  const long N = DIM(a, 0), M = DIM(a, 1), K = DIM(Wmu, 0);
  RUN(fv_enc_bwd_fused(P_F32(dfmu, K), P_F32(dfsig_c, K), P_F32(fsig, K),
                       P_F32(fsig_pre, K), P_F32(yp, M), P_F32_EQ(Wmu, K * M),
                       P_F32_EQ(Wsig, K * M), P_F32(a, N * M), P_F32(y, N),
                       P_F32(dscores, N * M), P_F32(dWmu, K * M),
                       P_F32(dbmu, K), P_F32(dWsig, K * M), P_F32(dbsig, K),
                       N, M, K, cur_stream()));
}

// enc_bwd_fused that forms dfmu / dfsig_c itself from the KL inputs and the
// decoder's nblk block partials; dfmu and dfsig_c are outputs
void enc_bwd_mid(Tensor part, long nblk, Tensor fmu, Tensor fsig_c,
                 Tensor pmu, Tensor psig_c, Tensor fsig, Tensor fsig_pre,
                 Tensor yp, Tensor Wmu, Tensor Wsig, Tensor a, Tensor y,
                 Tensor dscores, Tensor dWmu, Tensor dbmu, Tensor dWsig,
                 Tensor dbsig, Tensor dfmu, Tensor dfsig_c, double gscale) {
  OP("enc_bwd_mid", part);
  const long N = DIM(a, 0), M = DIM(a, 1), K = DIM(Wmu, 0);
  NUM(nblk);
  RUN(fv_enc_bwd_mid(
      P_F32(part, 2 * K * nblk), P_F32(fmu, K), P_F32(fsig_c, K),
      P_F32(pmu, K), P_F32(psig_c, K), P_F32(fsig, K), P_F32(fsig_pre, K),
      P_F32(yp, M), P_F32_EQ(Wmu, K * M), P_F32_EQ(Wsig, K * M),
      P_F32(a, N * M), P_F32(y, N), P_F32(dscores, N * M), P_F32(dWmu, K * M),
      P_F32(dbmu, K), P_F32(dWsig, K * M), P_F32(dbsig, K), P_F32(dfmu, K),
      P_F32(dfsig_c, K), nblk, N, M, K, (float)gscale, cur_stream()));
}

void enc_softmax_fwd(Tensor scores, Tensor y, Tensor a, Tensor yp) {
  OP("enc_softmax_fwd", scores);
  const long N = DIM(scores, 0), M = DIM(scores, 1);
  RUN(fv_enc_softmax_fwd(P_F32(scores, N * M), P_F32(y, N), P_F32(a, N * M),
                         P_F32(yp, M), N, M, cur_stream()));
}

void enc_softmax_bwd(Tensor dyp, Tensor a, Tensor y, Tensor dscores) {
  OP("enc_softmax_bwd", dyp);
  const long N = DIM(a, 0), M = DIM(a, 1);
  RUN(fv_enc_softmax_bwd(P_F32(dyp, M), P_F32(a, N * M), P_F32(y, N),
                         P_F32(dscores, N * M), N, M, cur_stream()));
}

void enc_heads_fwd(Tensor yp, Tensor Wmu, Tensor bmu, Tensor Wsig,
                   Tensor bsig, Tensor fmu, Tensor fsig_pre, Tensor fsig,
                   Tensor fsig_c) {
  OP("enc_heads_fwd", yp);
  const long M = NUM(yp.numel()), K = DIM(Wmu, 0);
  RUN(fv_enc_heads_fwd(P_F32(yp, M), P_F32_EQ(Wmu, K * M), P_F32_EQ(bmu, K),
                       P_F32_EQ(Wsig, K * M), P_F32_EQ(bsig, K),
                       P_F32(fmu, K), P_F32(fsig_pre, K), P_F32(fsig, K),
                       P_F32(fsig_c, K), M, K, cur_stream()));
}

void enc_heads_bwd(Tensor dfmu, Tensor dfsig_c, Tensor fsig, Tensor fsig_pre,
                   Tensor yp, Tensor Wmu, Tensor Wsig, Tensor dyp,
                   Tensor dWmu, Tensor dbmu, Tensor dWsig, Tensor dbsig) {
  OP("enc_heads_bwd", dfmu);
  const long M = NUM(yp.numel()), K = DIM(Wmu, 0);
  RUN(fv_enc_heads_bwd(P_F32(dfmu, K), P_F32(dfsig_c, K), P_F32(fsig, K),
                       P_F32(fsig_pre, K), P_F32(yp, M), P_F32_EQ(Wmu, K * M),
                       P_F32_EQ(Wsig, K * M), P_F32(dyp, M),
                       P_F32(dWmu, K * M), P_F32(dbmu, K), P_F32(dWsig, K * M),
                       P_F32(dbsig, K), M, K, cur_stream()));
}

// ------------------------------------------------------------- geometry
int as_int(const char* fn, long v) {
  TORCH_CHECK(v >= 0 && v <= INT_MAX, fn, ": ", v,
              " is outside the range of int");
  return (int)v;
}

// launch geometry, owned by the .hip files: callers size buffers with these
long dec_nblk(long N) { return fv_dec_nblk(as_int("dec_nblk", N)); }
long gru_wave_max_n() { return fv_gru_wave_max_n(); }
long gru_wgrad_blocks(long N) {
  return fv_gru_wgrad_blocks(as_int("gru_wgrad_blocks", N));
}
long ln_bwd_yblocks(long R, long C) {
  TORCH_CHECK(R >= 0, "ln_bwd_yblocks: R = ", R);
  return fv_ln_bwd_yblocks(R, as_int("ln_bwd_yblocks", C));
}

// -------------------------------------------------------------- decoder
// h (N,H); W1 (H,H), b1 / wmu / wsig (H), bmu / bsig (1), Wb (K,H), bb (K);
// fmu / fsig_c (K); per-row buffers of N, N*H or N*K floats; part holds
// dec_nblk(N) block partials of 2K + 2H + 2 floats.
void dec_fwd(Tensor h, Tensor W1, Tensor b1, Tensor wmu, Tensor bmu,
             Tensor wsig, Tensor bsig, Tensor Wb, Tensor bb, Tensor fmu,
             Tensor fsig_c, Tensor eps, Tensor recon, Tensor a1, Tensor beta,
             Tensor asig_pre, Tensor sigma) {
  OP("dec_fwd", h);
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(Wb, 0);
  op.require(DIM(Wb, 1) == H, "Wb must be (K,H)");
  RUN(fv_dec_fwd(P_F32(h, N * H), P_F32_EQ(W1, H * H), P_F32_EQ(b1, H),
                 P_F32_EQ(wmu, H), P_F32_EQ(bmu, 1), P_F32_EQ(wsig, H),
                 P_F32_EQ(bsig, 1), P_F32_EQ(Wb, K * H), P_F32_EQ(bb, K),
                 P_F32(fmu, K), P_F32(fsig_c, K), P_F32(eps, N),
                 P_F32(recon, N), P_F32(a1, N * H), P_F32(beta, N * K),
                 P_F32(asig_pre, N), P_F32(sigma, N), N, K, H, cur_stream()));
}

void dec_bwd(Tensor drecon, Tensor h, Tensor a1, Tensor beta,
             Tensor asig_pre, Tensor sigma, Tensor eps, Tensor fmu,
             Tensor fsig_c, Tensor W1, Tensor wmu, Tensor wsig, Tensor Wb,
             Tensor dh, Tensor dz1, Tensor dbeta, Tensor part, Tensor dfmu,
             Tensor dfsig_c, Tensor dwmu, Tensor dbmu, Tensor dwsig,
             Tensor dbsig) {
  OP("dec_bwd", drecon);
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(Wb, 0);
  op.require(DIM(Wb, 1) == H, "Wb must be (K,H)");
  RUN(fv_dec_bwd(
      P_F32(drecon, N), P_F32(h, N * H), P_F32(a1, N * H), P_F32(beta, N * K),
      P_F32(asig_pre, N), P_F32(sigma, N), P_F32(eps, N), P_F32(fmu, K),
      P_F32(fsig_c, K), P_F32_EQ(W1, H * H), P_F32_EQ(wmu, H),
      P_F32_EQ(wsig, H), P_F32_EQ(Wb, K * H), P_F32(dh, N * H),
      P_F32(dz1, N * H), P_F32(dbeta, N * K),
      P_F32(part, fv_dec_nblk(N) * (2 * K + 2 * H + 2)), P_F32(dfmu, K),
      P_F32(dfsig_c, K), P_F32_EQ(dwmu, H), P_F32_EQ(dbmu, 1),
      P_F32_EQ(dwsig, H), P_F32_EQ(dbsig, 1), N, K, H, cur_stream()));
}

// ---- the training step's middle chain (docs/KERNELS.md)
void dec_fwd_bwd(Tensor h, Tensor W1, Tensor b1, Tensor wmu, Tensor bmu,
                 Tensor wsig, Tensor bsig, Tensor Wb, Tensor bb, Tensor fmu,
                 Tensor fsig_c, Tensor eps, Tensor y, Tensor recon, Tensor a1,
                 Tensor beta, Tensor asig_pre, Tensor sigma, Tensor drecon,
                 Tensor dh, Tensor dz1, Tensor dbeta, Tensor part,
                 double gscale) {
  OP("dec_fwd_bwd", h);
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(Wb, 0);
  op.require(DIM(Wb, 1) == H, "Wb must be (K,H)");
  RUN(fv_dec_fwd_bwd(
      P_F32(h, N * H), P_F32_EQ(W1, H * H), P_F32(b1, H), P_F32(wmu, H),
      P_F32(bmu, 1), P_F32(wsig, H), P_F32(bsig, 1), P_F32_EQ(Wb, K * H),
      P_F32(bb, K), P_F32(fmu, K), P_F32(fsig_c, K), P_F32(eps, N),
      P_F32(y, N), P_F32(recon, N), P_F32(a1, N * H), P_F32(beta, N * K),
      P_F32(asig_pre, N), P_F32(sigma, N), P_F32(drecon, N),
      P_F32(dh, N * H), P_F32(dz1, N * H), P_F32(dbeta, N * K),
      P_F32(part, fv_dec_nblk(N) * (2 * K + 2 * H + 2)), N, K, H,
      (float)gscale, cur_stream()));
}

// the 2H+2 decoder head gradients out of dec_fwd_bwd's partials (N rows)
void dec_bwd_reduce_heads(Tensor part, Tensor dwmu, Tensor dbmu,
                          Tensor dwsig, Tensor dbsig, long N, long K) {
  OP("dec_bwd_reduce_heads", part);
  NUM(N); NUM(K);
  const long H = NUM(dwmu.numel());
  op.require(N >= 1 && K >= 1, "needs N >= 1 and K >= 1");
  RUN(fv_dec_bwd_reduce_heads(
      P_F32(part, fv_dec_nblk(N) * (2 * K + 2 * H + 2)), P_F32_EQ(dwmu, H),
      P_F32(dbmu, 1), P_F32_EQ(dwsig, H), P_F32(dbsig, 1), N, K, H,
      cur_stream()));
}

// ---- the fused middle (docs/KERNELS.md): attn_fused_fwd + enc_fused_fwd
// (with the heads) as one launch, argument for argument. Returns false,
// launching nothing, outside mid_fuse.hip's limits.
bool mid_fwd(Tensor h, Tensor qk, Tensor cb, OptTensor mask, Tensor Wv,
             Tensor bv, Tensor Wl, Tensor bl, Tensor wmu, Tensor bmu,
             Tensor wsig, Tensor bsig, Tensor a, Tensor sd, Tensor guard,
             Tensor u, Tensor ctx, Tensor hm2, Tensor pmu, Tensor psig_pre,
             Tensor psig, Tensor psig_c, Tensor Wenc, Tensor benc, Tensor y,
             Tensor scores, Tensor a_enc, Tensor yp, Tensor Wmu_e,
             Tensor bmu_e, Tensor Wsig_e, Tensor bsig_e, Tensor fmu,
             Tensor fsig_pre, Tensor fsig, Tensor fsig_c, Tensor done,
             double alpha, double keep_inv) {
  OP("mid_fwd", h);
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(qk, 0), M = DIM(Wenc, 0);
  op.require(DIM(qk, 1) == H, "qk must be (K,H)");
  op.require(DIM(Wenc, 1) == H, "Wenc must be (M,H)");
  int ran = 0;
  RUN(fv_mid_fwd(
      P_F32(h, N * H), P_F32_EQ(qk, K * H), P_F32_EQ(cb, K),
      P_F32(mask, N * K), P_F32_EQ(Wv, K * H * H), P_F32_EQ(bv, K * H),
      P_F32_EQ(Wl, H * H), P_F32_EQ(bl, H), P_F32_EQ(wmu, H),
      P_F32_EQ(bmu, 1), P_F32_EQ(wsig, H), P_F32_EQ(bsig, 1),
      P_F32(a, N * K), P_F32(sd, N * K), P_I32(guard, K), P_F32(u, K * H),
      P_F32(ctx, K * H), P_F32(hm2, K * H), P_F32(pmu, K),
      P_F32(psig_pre, K), P_F32(psig, K), P_F32(psig_c, K),
      P_F32_EQ(Wenc, M * H), P_F32_EQ(benc, M), P_F32(y, N),
      P_F32(scores, N * M), P_F32(a_enc, N * M), P_F32(yp, M),
      P_F32_EQ(Wmu_e, K * M), P_F32_EQ(bmu_e, K), P_F32_EQ(Wsig_e, K * M),
      P_F32_EQ(bsig_e, K), P_F32(fmu, K), P_F32(fsig_pre, K), P_F32(fsig, K),
      P_F32(fsig_c, K), P_I32(done, 1), N, K, M, H, (float)alpha,
      (float)keep_inv, &ran, cur_stream()));
  return ran != 0;
}

// attn_fused_bwd in its KL-gradient form (dpmu / dpsig_c are outputs) +
// dec_fwd_bwd as one launch. It does NOT run pred_head_reduce: hpart is
// left for the caller's pred_head_reduce. Returns false, launching
// nothing, outside mid_fuse.hip's limits.
bool mid_bwd(Tensor psig, Tensor psig_pre, Tensor hm2, Tensor wmu,
             Tensor wsig, Tensor Wl, Tensor h, Tensor a, Tensor sd,
             OptTensor mask, Tensor guard, Tensor u, Tensor Wv, Tensor q,
             Tensor Wk, Tensor bk, Tensor dz2, Tensor du, Tensor ds,
             Tensor dc, Tensor dWv, Tensor dbv, Tensor dq, Tensor dWk,
             Tensor dbk, Tensor hpart, Tensor fmu, Tensor fsig_c, Tensor pmu,
             Tensor psig_c, Tensor dpmu, Tensor dpsig_c, Tensor W1, Tensor b1,
             Tensor wmu_d, Tensor bmu_d, Tensor wsig_d, Tensor bsig_d,
             Tensor Wb, Tensor bb, Tensor eps, Tensor y, Tensor recon,
             Tensor a1, Tensor beta, Tensor asig_pre, Tensor sigma,
             Tensor drecon, Tensor dh, Tensor dz1, Tensor dbeta, Tensor part,
             double alpha, double keep_inv, double gscale) {
  OP("mid_bwd", psig);
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(q, 0);
  op.require(DIM(q, 1) == H, "q must be (K,H)");
  op.require(DIM(Wb, 0) == K && DIM(Wb, 1) == H, "Wb must be (K,H)");
  op.require(N >= 1, "h has no rows");
  int ran = 0;
  RUN(fv_mid_bwd(
      P_F32(psig, K), P_F32(psig_pre, K), P_F32(hm2, K * H),
      P_F32_EQ(wmu, H), P_F32_EQ(wsig, H), P_F32_EQ(Wl, H * H),
      P_F32(h, N * H), P_F32(a, N * K), P_F32(sd, N * K), P_F32(mask, N * K),
      P_I32(guard, K), P_F32(u, K * H), P_F32_EQ(Wv, K * H * H),
      P_F32_EQ(q, K * H), P_F32_EQ(Wk, K * H * H), P_F32_EQ(bk, K * H),
      P_F32(dz2, K * H), P_F32(du, K * H), P_F32(ds, N * K), P_F32(dc, K),
      P_F32_EQ(dWv, K * H * H), P_F32_EQ(dbv, K * H), P_F32_EQ(dq, K * H),
      P_F32_EQ(dWk, K * H * H), P_F32_EQ(dbk, K * H),
      P_F32(hpart, K * (2 * H + 2)), P_F32(fmu, K), P_F32(fsig_c, K),
      P_F32(pmu, K), P_F32(psig_c, K), P_F32(dpmu, K), P_F32(dpsig_c, K),
      P_F32_EQ(W1, H * H), P_F32(b1, H), P_F32(wmu_d, H), P_F32(bmu_d, 1),
      P_F32(wsig_d, H), P_F32(bsig_d, 1), P_F32_EQ(Wb, K * H), P_F32(bb, K),
      P_F32(eps, N), P_F32(y, N), P_F32(recon, N), P_F32(a1, N * H),
      P_F32(beta, N * K), P_F32(asig_pre, N), P_F32(sigma, N),
      P_F32(drecon, N), P_F32(dh, N * H), P_F32(dz1, N * H),
      P_F32(dbeta, N * K),
      P_F32(part, fv_dec_nblk(N) * (2 * K + 2 * H + 2)), N, K, H,
      (float)alpha, (float)keep_inv, (float)gscale, &ran, cur_stream()));
  return ran != 0;
}

// the (2H + 2) predictor head gradients out of hpart, K * (2H + 2) floats
void pred_head_reduce(Tensor hpart, Tensor dwmu, Tensor dbmu, Tensor dwsig,
                      Tensor dbsig, long K, long H) {
  OP("pred_head_reduce", hpart);
  NUM(K); NUM(H);
  op.require(K >= 1 && H >= 1, "needs K >= 1 and H >= 1");
  RUN(fv_pred_head_reduce(P_F32(hpart, K * (2 * H + 2)), P_F32_EQ(dwmu, H),
                          P_F32_EQ(dbmu, 1), P_F32_EQ(dwsig, H),
                          P_F32_EQ(dbsig, 1), K, H, cur_stream()));
}

// ----------------------------------------------------------------- loss
// recon / y / drecon hold N floats, the KL inputs and gradients K each
void loss_fused(Tensor recon, Tensor y, Tensor fmu, Tensor fsig_c, Tensor pmu,
                Tensor psig_c, Tensor loss, Tensor mse, Tensor kl,
                Tensor drecon, Tensor dfmu, Tensor dfsig_c, Tensor dpmu,
                Tensor dpsig_c, double gscale) {
  OP("loss_fused", recon);
  const long N = op.num(op.same_numel(recon, "recon", y, "y"), "recon");
  const long K = op.num(op.same_numel(fmu, "fmu", fsig_c, "fsig_c"), "fmu");
  RUN(fv_loss_fused(P_F32(recon, N), P_F32(y, N), P_F32(fmu, K),
                    P_F32(fsig_c, K), P_F32(pmu, K), P_F32(psig_c, K),
                    P_F32(loss, 1), P_F32(mse, 1), P_F32(kl, 1),
                    P_F32(drecon, N), P_F32(dfmu, K), P_F32(dfsig_c, K),
                    P_F32(dpmu, K), P_F32(dpsig_c, K), N, K, (float)gscale,
                    cur_stream()));
}

// loss, mse and kl only (loss_fused without its gradient stores)
void loss_scalars(Tensor recon, Tensor y, Tensor fmu, Tensor fsig_c,
                  Tensor pmu, Tensor psig_c, Tensor loss, Tensor mse,
                  Tensor kl) {
  OP("loss_scalars", recon);
  const long N = op.num(op.same_numel(recon, "recon", y, "y"), "recon");
  const long K = op.num(op.same_numel(fmu, "fmu", fsig_c, "fsig_c"), "fmu");
  RUN(fv_loss_scalars(P_F32(recon, N), P_F32(y, N), P_F32(fmu, K),
                      P_F32(fsig_c, K), P_F32(pmu, K), P_F32(psig_c, K),
                      P_F32(loss, 1), P_F32(mse, 1), P_F32(kl, 1), N, K,
                      cur_stream()));
}

// ---- batched multi-day scoring ------------------------------------
// h (sumN,H) packed days; seg_off int32 (D+1) device row offsets; max_n
// the longest day (host-side knowledge: sizes the launch's LDS).
// Outputs pmu / psig_c (D,K) fp32 and guard (D,K) int32.
void attn_seg_fwd(Tensor h, Tensor seg_off, long max_n, Tensor qk, Tensor cb,
                  Tensor Wv, Tensor bv, Tensor Wl, Tensor bl, Tensor wmu,
                  Tensor bmu, Tensor wsig, Tensor bsig, Tensor pmu,
                  Tensor psig_c, Tensor guard, double alpha) {
  OP("attn_seg_fwd", h);
  op.require(h.dim() == 2 && qk.dim() == 2 && qk.size(1) == h.size(1),
             "want h (total,H), qk (K,H)");
  const long total = DIM(h, 0), H = DIM(h, 1), K = DIM(qk, 0);
  const long D = NUM(seg_off.numel()) - 1;
  op.require(D >= 0, "seg_off needs D+1 entries");
  op.require(max_n >= 0 && max_n <= total, "max_n outside the packed rows");
  RUN(fv_attn_seg_fwd(
      P_F32(h, total * H), P_I32(seg_off, D + 1), P_F32_EQ(qk, K * H),
      P_F32_EQ(cb, K), P_F32_EQ(Wv, K * H * H), P_F32_EQ(bv, K * H),
      P_F32_EQ(Wl, H * H), P_F32_EQ(bl, H), P_F32_EQ(wmu, H), P_F32(bmu, 1),
      P_F32_EQ(wsig, H), P_F32(bsig, 1), P_F32(pmu, D * K),
      P_F32(psig_c, D * K), P_I32(guard, D * K), total, D, max_n, K, H,
      (float)alpha, cur_stream()));
}

// fmu / fsig_c are (D,K): each row takes its own day's factor prior.
// eps/sample, beta and svar are optional; sample = fma(eps, sigma, mu),
// svar (N) = alpha_sigma^2 + 1e-6, the row's idiosyncratic variance.
void dec_seg_fwd(Tensor h, Tensor seg_off, Tensor W1, Tensor b1, Tensor wmu,
                 Tensor bmu, Tensor wsig, Tensor bsig, Tensor Wb, Tensor bb,
                 Tensor fmu, Tensor fsig_c, OptTensor eps, Tensor mu,
                 Tensor sigma, OptTensor sample, OptTensor beta,
                 OptTensor svar) {
  OP("dec_seg_fwd", h);
  op.require(h.dim() == 2 && Wb.dim() == 2 && Wb.size(1) == h.size(1),
             "want h (N,H), Wb (K,H)");
  const long N = DIM(h, 0), H = DIM(h, 1), K = DIM(Wb, 0);
  const long D = NUM(seg_off.numel()) - 1;
  op.require(D >= 0, "seg_off needs D+1 entries");
  op.require(!eps.has_value() || sample.has_value(),
             "eps needs a sample output");
  const float* ep = P_F32(eps, N);
  RUN(fv_dec_seg_fwd(
      P_F32(h, N * H), P_I32(seg_off, D + 1), P_F32_EQ(W1, H * H),
      P_F32_EQ(b1, H), P_F32_EQ(wmu, H), P_F32(bmu, 1), P_F32_EQ(wsig, H),
      P_F32(bsig, 1), P_F32_EQ(Wb, K * H), P_F32_EQ(bb, K),
      P_F32(fmu, D * K), P_F32(fsig_c, D * K), ep, P_F32(mu, N),
      P_F32(sigma, N), ep ? P_F32(sample, N) : nullptr, P_F32(beta, N * K),
      P_F32(svar, N), N, D, K, H, cur_stream()));
}

// ---- factor risk model ----------------------------------------------
// beta (total,K), svar / mu / w (total) packed days, seg_off int32 (D+1),
// pmu / psig_c (D,K). Outputs: stats (D,5) = mean, mean_factor,
// var_factor, var_specific, vol; exposure, factor_var (D,K); mcr (total).
// A day without rows gets NaN in its per-day rows.
void risk_seg(Tensor beta, Tensor svar, Tensor mu, Tensor w, Tensor seg_off,
              Tensor pmu, Tensor psig_c, Tensor stats, Tensor exposure,
              Tensor factor_var, Tensor mcr) {
  OP("risk_seg", beta);
  op.require(beta.dim() == 2 && pmu.dim() == 2 &&
                 pmu.size(1) == beta.size(1),
             "want beta (total,K), pmu (D,K)");
  const long total = DIM(beta, 0), K = DIM(beta, 1), D = DIM(pmu, 0);
  op.require(K >= 1 && K <= 128, "supports 1 <= K <= 128, got K=", K);
  RUN(fv_risk_seg(P_F32(beta, total * K), P_F32(svar, total),
                  P_F32(mu, total), P_F32(w, total), P_I32(seg_off, D + 1),
                  P_F32(pmu, D * K), P_F32(psig_c, D * K),
                  P_F32(stats, D * 5), P_F32(exposure, D * K),
                  P_F32(factor_var, D * K), P_F32(mcr, total), total, D, K,
                  cur_stream()));
}

// x (total,R) = Sigma_d^-1 b for b (total,R), 1 <= R <= 4, through the
// factor structure; info (D) int32: 0 solved, 1 failed pivot (the day's x
// is NaN), 2 rows outside the packed buffer. psig_c (D,K) gives D. norms
// (D,2,R), optional: the day's sum x and sum |x| per column.
void risk_solve_seg(Tensor beta, Tensor svar, Tensor seg_off, Tensor psig_c,
                    Tensor b, Tensor x, Tensor info,
                    OptTensor norms) {
  OP("risk_solve_seg", beta);
  op.require(beta.dim() == 2 && psig_c.dim() == 2 &&
                 psig_c.size(1) == beta.size(1),
             "want beta (total,K), psig_c (D,K)");
  const long total = DIM(beta, 0), K = DIM(beta, 1), D = DIM(psig_c, 0);
  op.require(b.dim() == 2 && b.size(0) == total, "b must be (total,R)");
  const long R = DIM(b, 1);
  op.require(K >= 1 && K <= 128, "supports 1 <= K <= 128, got K=", K);
  op.require(R >= 1 && R <= 4, "supports 1 <= R <= 4, got R=", R);
  RUN(fv_risk_solve_seg(P_F32(beta, total * K), P_F32(svar, total),
                        P_I32(seg_off, D + 1), P_F32(psig_c, D * K),
                        P_F32(b, total * R), P_F32(x, total * R),
                        P_I32(info, D), P_F32(norms, D * 2 * R), total, D, K,
                        R, cur_stream()));
}

// ---- batched multi-day posterior pass ------------------------------
// h (total,H) and y (total) packed days, seg_off int32 (D+1), max_n the
// longest day; yp (D,M) gives D. A refused segment comes back as NaN.
void enc_seg_fwd(Tensor h, Tensor seg_off, long max_n, Tensor Wenc,
                 Tensor benc, Tensor y, Tensor yp) {
  OP("enc_seg_fwd", h);
  const long total = DIM(h, 0), H = DIM(h, 1);
  op.require(h.dim() == 2, "h must be (total,H)");
  op.require(DIM(Wenc, 1) == H && Wenc.dim() == 2, "Wenc must be (M,H)");
  const long M = DIM(Wenc, 0);
  op.require(DIM(yp, 1) == M && yp.dim() == 2, "yp must be (D,M)");
  const long D = DIM(yp, 0);
  op.require(max_n >= 0 && max_n <= total, "max_n outside the packed rows");
  RUN(fv_enc_seg_fwd(P_F32(h, total * H), P_I32(seg_off, D + 1),
                     P_F32_EQ(Wenc, M * H), P_F32_EQ(benc, M),
                     P_F32(y, total), P_F32(yp, D * M), total, D, max_n, M, H,
                     cur_stream()));
}

// yp (D,M) -> fmu, fsig_c (D,K): the posterior heads of every day
void enc_seg_heads(Tensor yp, Tensor Wmu, Tensor bmu, Tensor Wsig,
                   Tensor bsig, Tensor fmu, Tensor fsig_c) {
  OP("enc_seg_heads", yp);
  const long D = DIM(yp, 0), M = DIM(yp, 1);
  op.require(yp.dim() == 2, "yp must be (D,M)");
  op.require(DIM(Wmu, 1) == M && Wmu.dim() == 2, "Wmu must be (K,M)");
  const long K = DIM(Wmu, 0);
  RUN(fv_enc_seg_heads(P_F32(yp, D * M), P_F32_EQ(Wmu, K * M),
                       P_F32_EQ(bmu, K), P_F32_EQ(Wsig, K * M),
                       P_F32_EQ(bsig, K), P_F32(fmu, D * K),
                       P_F32(fsig_c, D * K), D, M, K, cur_stream()));
}

// recon / y (total) packed, seg_off int32 (D+1), the four factor tensors
// (D,K) — fmu gives D and K; loss, mse, kl (D) fp32, NaN for a day without
// rows or outside the packed buffer
void loss_seg(Tensor recon, Tensor y, Tensor seg_off, Tensor fmu,
              Tensor fsig_c, Tensor pmu, Tensor psig_c, Tensor loss,
              Tensor mse, Tensor kl) {
  OP("loss_seg", recon);
  const long total =
      op.num(op.same_numel(recon, "recon", y, "y"), "recon");
  const long D = DIM(fmu, 0), K = DIM(fmu, 1);
  op.require(fmu.dim() == 2, "fmu must be (D,K)");
  RUN(fv_loss_seg(P_F32(recon, total), P_F32(y, total),
                  P_I32(seg_off, D + 1), P_F32(fmu, D * K),
                  P_F32(fsig_c, D * K), P_F32(pmu, D * K),
                  P_F32(psig_c, D * K), P_F32(loss, D), P_F32(mse, D),
                  P_F32(kl, D), total, D, K, cur_stream()));
}

// pred (P,total) fp32 rows with any row stride (a row slice of the scoring
// workspace's (3,Nn) output), label (>= total) fp32, seg_off int32 (D+1);
// max_n the longest day (sizes the launch's LDS, <= 8192). Outputs, fully
// written: stats (D,P,4) float64 = ic, rank_ic, long, short; count (D,P)
// int32 = valid rows, -1 for a refused segment.
void daily_ic_seg(Tensor pred, Tensor label, Tensor seg_off, long max_n,
                  long topk, Tensor stats, Tensor count) {
  OP("daily_ic_seg", pred);
  // pred is the one strided argument: its own checks
  op.require(pred.is_cuda() && pred.scalar_type() == torch::kFloat32,
             "pred must be fp32 on GPU");
  op.require(pred.dim() == 2, "pred must be (P, total)");
  const long P = DIM(pred, 0), total = DIM(pred, 1);
  op.require(P >= 1, "pred needs at least one row");
  op.require(total <= 1 || pred.stride(1) == 1,
             "pred rows must be contiguous");
  op.require(P == 1 || pred.stride(0) >= 0, "pred row stride is negative");
  const long D = NUM(seg_off.numel()) - 1;
  op.require(D >= 0, "seg_off needs D+1 entries");
  op.require(max_n >= 0 && max_n <= 8192,
             "supports days of up to 8192 rows, got max_n=", max_n);
  NUM(topk);
  RUN(fv_daily_ic_seg(pred.data_ptr<float>(),
                      P > 1 ? (long)pred.stride(0) : 0L, P_F32(label, total),
                      P_I32(seg_off, D + 1), P_F64(stats, D * P * 4),
                      P_I32(count, D * P), total, D, P, max_n, topk,
                      cur_stream()));
}

// ------------------------------------------------------------ optimizer
void step_inc(Tensor step_t) {
  OP("step_inc", step_t);
  RUN(fv_step_inc(P_I32(step_t, 1), cur_stream()));
}

void adam(Tensor p, Tensor g, Tensor m, Tensor v, Tensor step_t, double lr0,
          double eta_min, double t_max, double beta1, double beta2,
          double eps) {
  OP("adam", p);
  const int64_t n = op.same_numel(p, "p", g, "g");
  RUN(fv_adam(P_F32(p, n), P_F32_EQ(g, n), P_F32_EQ(m, n), P_F32_EQ(v, n),
              P_I32(step_t, 1), n, (float)lr0, (float)eta_min, (float)t_max,
              (float)beta1, (float)beta2, (float)eps, cur_stream()));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("gemm_nt", &gemm_nt);
  mod.def("gemm_nn", &gemm_nn, py::arg("A"), py::arg("B"), py::arg("bias"),
          py::arg("out"), py::arg("alpha"), py::arg("accumulate"),
          py::arg("act_lrelu"), py::arg("lrelu_bwd_of") = py::none(),
          py::arg("variant") = 1);
  mod.def("gemm_nn_ln", &gemm_nn_ln);
  mod.def("ln_bwd_reduce", &ln_bwd_reduce);
  mod.def("tn_reduce_list", &tn_reduce_list, py::arg("outs"),
          py::arg("parts"), py::arg("dbs"), py::arg("db_parts"), py::arg("R"),
          py::arg("r_chunks"), py::arg("accumulate"));
  mod.def("gemm_tn_pair", &gemm_tn_pair, py::arg("A0"), py::arg("B0"),
          py::arg("out0"), py::arg("A1"), py::arg("B1"), py::arg("out1"),
          py::arg("part0"), py::arg("part1"), py::arg("r_chunks"),
          py::arg("accumulate"), py::arg("db0") = py::none(),
          py::arg("db1") = py::none(), py::arg("db_part0") = py::none(),
          py::arg("db_part1") = py::none(), py::arg("variant") = 1,
          py::arg("reduce") = true);
  mod.def("gemm_tn_xhat", &gemm_tn_xhat, py::arg("A"), py::arg("x"),
          py::arg("mean"), py::arg("rstd"), py::arg("part"),
          py::arg("db_part"), py::arg("variant") = 1);
  mod.def("ln_w1x_finish", &ln_w1x_finish);
  mod.def("gemm_tn", &gemm_tn, py::arg("A"), py::arg("B"), py::arg("out"),
          py::arg("part"), py::arg("r_chunks"), py::arg("accumulate"),
          py::arg("db") = py::none(), py::arg("db_part") = py::none(),
          py::arg("variant") = 1, py::arg("reduce") = true);
  mod.def("colsum", &colsum);
  mod.def("gemm_nt_bf16", &gemm_nt_bf16, py::arg("A"), py::arg("W"),
          py::arg("bias"), py::arg("out_f32"), py::arg("out_bf16"),
          py::arg("alpha"), py::arg("accumulate"), py::arg("act_lrelu"));
  mod.def("gemm_nn_bf16", &gemm_nn_bf16, py::arg("A"), py::arg("B"),
          py::arg("bias"), py::arg("out_f32"), py::arg("out_bf16"),
          py::arg("alpha"), py::arg("accumulate"), py::arg("act_lrelu"),
          py::arg("lrelu_bwd_of") = py::none());
  mod.def("gemm_tn_bf16", &gemm_tn_bf16, py::arg("A"), py::arg("B"),
          py::arg("out"), py::arg("part"), py::arg("r_chunks"),
          py::arg("accumulate"), py::arg("db") = py::none(),
          py::arg("db_part") = py::none());
  mod.def("cast_f32_bf16", &cast_f32_bf16);
  mod.def("lrelu_bwd_bf16", &lrelu_bwd_bf16);
  mod.def("lrelu_bwd", &lrelu_bwd);
  mod.def("ln_fwd", &ln_fwd, py::arg("x"), py::arg("gamma"), py::arg("beta"),
          py::arg("xln"), py::arg("mean"), py::arg("rstd"), py::arg("eps"),
          py::arg("xln_bf") = py::none(), py::arg("xln_f8") = py::none());
  mod.def("extractor_head_fwd", &extractor_head_fwd, py::arg("x"),
          py::arg("gamma"), py::arg("beta"), py::arg("W1x"), py::arg("b1x"),
          py::arg("Wih"), py::arg("bih"), py::arg("xln"), py::arg("mean"),
          py::arg("rstd"), py::arg("xp"), py::arg("gi"), py::arg("eps"),
          py::arg("strip") = 0);
  mod.def("gemm_nt_fp8", &gemm_nt_fp8, py::arg("A"), py::arg("W"),
          py::arg("bias"), py::arg("inv_sw"), py::arg("out_f32"),
          py::arg("out_bf16"), py::arg("out_fp8"), py::arg("R"),
          py::arg("Ci"), py::arg("Co"), py::arg("alpha"),
          py::arg("act_lrelu"));
  mod.def("absmax_scale", &absmax_scale);
  mod.def("cast_f32_fp8_scaled", &cast_f32_fp8_scaled);
  mod.def("ln_bwd_params", &ln_bwd_params);
  // variant: 1 = wave-per-stock kernels where they apply (default), 0 =
  // the kernels from before them
  mod.def("gru_fwd", &gru_fwd, py::arg("gi"), py::arg("Whh"), py::arg("bhh"),
          py::arg("h_final"), py::arg("h_seq"), py::arg("h_prev"),
          py::arg("gates4"), py::arg("N"), py::arg("T"), py::arg("H"),
          py::arg("variant") = 1);
  mod.def("gru_fwd_mfma", &gru_fwd_mfma);
  // variant: 1 = latency-oriented kernel (default), 0 = original kernel
  mod.def("attn_fused_fwd", &attn_fused_fwd,
          py::arg("h"), py::arg("qk"), py::arg("cb"), py::arg("mask"),
          py::arg("Wv"), py::arg("bv"), py::arg("Wl"), py::arg("bl"),
          py::arg("wmu"), py::arg("bmu"), py::arg("wsig"), py::arg("bsig"),
          py::arg("a"), py::arg("sd"), py::arg("guard"), py::arg("u"),
          py::arg("ctx"), py::arg("hm2"), py::arg("pmu"), py::arg("psig_pre"),
          py::arg("psig"), py::arg("psig_c"), py::arg("alpha"),
          py::arg("keep_inv"),
          py::arg("variant") = 1);
  mod.def("enc_fused_fwd", &enc_fused_fwd, py::arg("h"),
          py::arg("Wenc"), py::arg("benc"), py::arg("y"),
          py::arg("scores"), py::arg("a"), py::arg("yp"),
          py::arg("Wmu") = py::none(), py::arg("bmu") = py::none(),
          py::arg("Wsig") = py::none(), py::arg("bsig") = py::none(),
          py::arg("fmu") = py::none(),
          py::arg("fsig_pre") = py::none(),
          py::arg("fsig") = py::none(),
          py::arg("fsig_c") = py::none(),
          py::arg("done") = py::none(), py::arg("variant") = 1);
  mod.def("enc_bwd_fused", &enc_bwd_fused);
  mod.def("attn_fused_bwd", &attn_fused_bwd,
          py::arg("dpmu"), py::arg("dpsig_c"), py::arg("psig"),
          py::arg("psig_pre"), py::arg("hm2"), py::arg("wmu"),
          py::arg("wsig"), py::arg("Wl"), py::arg("h"), py::arg("a"),
          py::arg("sd"), py::arg("mask"), py::arg("guard"), py::arg("u"),
          py::arg("Wv"), py::arg("q"), py::arg("Wk"), py::arg("bk"),
          py::arg("dz2"), py::arg("du"), py::arg("ds"), py::arg("dc"),
          py::arg("dWv"), py::arg("dbv"), py::arg("dq"), py::arg("dWk"),
          py::arg("dbk"), py::arg("hpart"), py::arg("dwmu"), py::arg("dbmu"),
          py::arg("dwsig"), py::arg("dbsig"), py::arg("alpha"),
          py::arg("keep_inv"),
          py::arg("variant") = 1, py::arg("kl_fmu") = py::none(),
          py::arg("kl_fsig_c") = py::none(), py::arg("kl_pmu") = py::none(),
          py::arg("kl_psig_c") = py::none(), py::arg("kl_gscale") = 1.0);
  // launch geometry the .hip files own: block counts that size buffers
  mod.def("dec_nblk", &dec_nblk);
  mod.def("gru_wgrad_blocks", &gru_wgrad_blocks);
  mod.def("gru_wave_max_n", &gru_wave_max_n);
  mod.def("ln_bwd_yblocks", &ln_bwd_yblocks);
  mod.def("dec_fwd_bwd", &dec_fwd_bwd);
  mod.def("dec_bwd_reduce_heads", &dec_bwd_reduce_heads);
  mod.def("enc_bwd_mid", &enc_bwd_mid);
  mod.def("loss_scalars", &loss_scalars);
  mod.def("gru_bwd_mfma", &gru_bwd_mfma, py::arg("dh_final"),
          py::arg("h_prev"), py::arg("gates4"), py::arg("whh_bf"),
          py::arg("dgi"), py::arg("dgh"), py::arg("N"), py::arg("T"),
          py::arg("H"), py::arg("dgi_bf") = py::none(),
          py::arg("dgh_bf") = py::none(), py::arg("dgi_f8") = py::none(),
          py::arg("s_dgi") = py::none(), py::arg("amax_dgi") = py::none(),
          py::arg("whh_part") = py::none(),
          py::arg("bhh_part") = py::none());
  mod.def("wgrad_reduce", &wgrad_reduce, py::arg("part"), py::arg("out"),
          py::arg("db_part"), py::arg("db"), py::arg("z"),
          py::arg("accumulate") = false);
  mod.def("gru_bwd", &gru_bwd, py::arg("dh_final"), py::arg("h_prev"),
          py::arg("gates4"), py::arg("Whh"), py::arg("dgi"), py::arg("dgh"),
          py::arg("N"), py::arg("T"), py::arg("H"),
          py::arg("dgi_bf") = py::none(), py::arg("dgh_bf") = py::none(),
          py::arg("variant") = 1, py::arg("ds") = py::none(),
          py::arg("qk") = py::none(), py::arg("a") = py::none(),
          py::arg("du") = py::none(), py::arg("dscores") = py::none(),
          py::arg("Wenc") = py::none());
  mod.def("mid_fwd", &mid_fwd);
  mod.def("mid_bwd", &mid_bwd);
  mod.def("pred_head_reduce", &pred_head_reduce);
  mod.def("enc_softmax_fwd", &enc_softmax_fwd);
  mod.def("enc_softmax_bwd", &enc_softmax_bwd);
  mod.def("enc_heads_fwd", &enc_heads_fwd);
  mod.def("enc_heads_bwd", &enc_heads_bwd);
  mod.def("attn_qk_fwd", &attn_qk_fwd);
  mod.def("attn_softmax_fwd", &attn_softmax_fwd);
  mod.def("attn_ctx_fwd", &attn_ctx_fwd);
  mod.def("attn_head_bwd", &attn_head_bwd);
  mod.def("attn_softmax_bwd", &attn_softmax_bwd);
  mod.def("attn_qk_bwd", &attn_qk_bwd);
  mod.def("loss_fused", &loss_fused);
  mod.def("dh_combine", &dh_combine);
  mod.def("gemm_nt_bf16_rs", &gemm_nt_bf16_rs, py::arg("A"), py::arg("Wp"),
          py::arg("bias") = py::none(), py::arg("out_f32") = py::none(),
          py::arg("out_bf16") = py::none(),
          py::arg("lrelu_bwd_of") = py::none(), py::arg("alpha") = 1.0,
          py::arg("act_lrelu") = false);
  mod.def("cast_shadows", &cast_shadows);
  mod.def("gemm_nt_fp8_rs", &gemm_nt_fp8_rs, py::arg("A"), py::arg("Wp"),
          py::arg("bias") = py::none(), py::arg("inv_sw") = py::none(),
          py::arg("out_f32") = py::none(), py::arg("out_bf16") = py::none(),
          py::arg("out_fp8") = py::none(), py::arg("R"), py::arg("Ci"),
          py::arg("Co"), py::arg("alpha") = 1.0,
          py::arg("act_lrelu") = false, py::arg("inv_sa") = py::none(),
          py::arg("lrelu_bwd_of") = py::none(),
          py::arg("s_out") = py::none(), py::arg("amax_out") = py::none());
  mod.def("scale_from_amax2", &scale_from_amax2);
  mod.def("cast_f32_fp8_damax", &cast_f32_fp8_damax);
  mod.def("cast_f32_fp8_scaled_t", &cast_f32_fp8_scaled_t);
  mod.def("pred_mlp_fwd", &pred_mlp_fwd);
  mod.def("pred_mlp_bwd", &pred_mlp_bwd);
  mod.def("dec_fwd", &dec_fwd);
  mod.def("dec_bwd", &dec_bwd);
  // batched multi-day scoring (inference only)
  mod.def("gru_fwd_infer", &gru_fwd_infer, py::arg("gi"), py::arg("Whh"),
          py::arg("bhh"), py::arg("h_final"), py::arg("N"), py::arg("T"),
          py::arg("H"), py::arg("variant") = 1);
  mod.def("gru_fwd_mfma_infer", &gru_fwd_mfma_infer);
  mod.def("gru_fwd_infer_gather", &gru_fwd_infer_gather, py::arg("gi_rows"),
          py::arg("U"), py::arg("idx"), py::arg("Whh"), py::arg("bhh"),
          py::arg("h_final"), py::arg("N"), py::arg("T"), py::arg("H"),
          py::arg("variant") = 1);
  mod.def("gru_fwd_mfma_infer_gather", &gru_fwd_mfma_infer_gather);
  mod.def("attn_seg_fwd", &attn_seg_fwd,
          py::arg("h"), py::arg("seg_off"), py::arg("max_n"), py::arg("qk"),
          py::arg("cb"), py::arg("Wv"), py::arg("bv"), py::arg("Wl"),
          py::arg("bl"), py::arg("wmu"), py::arg("bmu"), py::arg("wsig"),
          py::arg("bsig"), py::arg("pmu"), py::arg("psig_c"),
          py::arg("guard"), py::arg("alpha"));
  mod.def("dec_seg_fwd", &dec_seg_fwd,
          py::arg("h"), py::arg("seg_off"), py::arg("W1"), py::arg("b1"),
          py::arg("wmu"), py::arg("bmu"), py::arg("wsig"), py::arg("bsig"),
          py::arg("Wb"), py::arg("bb"), py::arg("fmu"), py::arg("fsig_c"),
          py::arg("eps"), py::arg("mu"), py::arg("sigma"),
          py::arg("sample") = py::none(), py::arg("beta") = py::none(),
          py::arg("svar") = py::none());
  // factor risk model of the prior decoder
  mod.def("risk_seg", &risk_seg,
          py::arg("beta"), py::arg("svar"), py::arg("mu"), py::arg("w"),
          py::arg("seg_off"), py::arg("pmu"), py::arg("psig_c"),
          py::arg("stats"), py::arg("exposure"), py::arg("factor_var"),
          py::arg("mcr"));
  mod.def("risk_solve_seg", &risk_solve_seg,
          py::arg("beta"), py::arg("svar"), py::arg("seg_off"),
          py::arg("psig_c"), py::arg("b"), py::arg("x"), py::arg("info"),
          py::arg("norms") = py::none());
  // batched multi-day posterior pass (inference only)
  mod.def("enc_seg_fwd", &enc_seg_fwd,
          py::arg("h"), py::arg("seg_off"), py::arg("max_n"),
          py::arg("Wenc"), py::arg("benc"), py::arg("y"), py::arg("yp"));
  mod.def("enc_seg_heads", &enc_seg_heads,
          py::arg("yp"), py::arg("Wmu"), py::arg("bmu"), py::arg("Wsig"),
          py::arg("bsig"), py::arg("fmu"), py::arg("fsig_c"));
  mod.def("loss_seg", &loss_seg,
          py::arg("recon"), py::arg("y"), py::arg("seg_off"), py::arg("fmu"),
          py::arg("fsig_c"), py::arg("pmu"), py::arg("psig_c"),
          py::arg("loss"), py::arg("mse"), py::arg("kl"));
  mod.def("daily_ic_seg", &daily_ic_seg,
          py::arg("pred"), py::arg("label"), py::arg("seg_off"),
          py::arg("max_n"), py::arg("topk"), py::arg("stats"),
          py::arg("count"));
  mod.def("step_inc", &step_inc);
  mod.def("adam", &adam);
}
