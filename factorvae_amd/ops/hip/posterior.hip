// Batched multi-day posterior pass (inference only): the encoder
// q(z | x, y) and the MSE + KL loss over days packed as in predict.hip —
// rows of all days back to back, int32 seg_off[D+1] on the device.
//
//   enc_seg_fwd_kernel:   enc_fused_fwd_kernel's portfolio chain (score
//     GEMV + stock-axis softmax + weighted return), one workgroup per
//     (portfolio, day); writes only yp (D,M).
//   enc_seg_heads_kernel: the mu / softplus-sigma heads of every day, one
//     thread per (day, factor). A launch of its own: the kernel boundary
//     orders it behind all of yp, no inter-workgroup handoff.
//   loss_seg_kernel:      loss_fused_kernel<false>'s two reductions with
//     segment-local n, one workgroup per day.
//
// The decoder between the heads and the loss is dec_seg_fwd (predict.hip),
// fed the posterior (fmu, fsig_c) rows and an eps.
//
// As in predict.hip every reduction is ordered by segment-local indices
// only (row n on thread n % 256, the same wave tree), so a day's result
// does not depend on its position in the batch, on its neighbours, or on
// whether its h rows were staged in LDS.

#include "common.h"
#include "launchers.h"

// ---------------------------------------------------------------------
// LDS map of enc_seg_fwd_kernel (floats, every carve a multiple of 4):
//   scratch[8] wS[64] aS[a_cap] hS[stage_cap*(H+1)]
#define ESEG_FIXED (8 + 64)
#define ESEG_LDS_MAX (144 * 1024)

// sv = benc[m] + h[n]·Wenc[m] as one fmaf chain over c (thread <-> stock
// row), into aS, with the running max. STAGED: h rows come from the LDS
// image (stride H+1); otherwise they are re-read from global/L2 (stride
// H). The chain is the same.
template <bool STAGED>
DEVINL void eseg_scores(const float* __restrict__ hg, const float* hS,
                        const float* wS, float* aS, int N, int H, float bm,
                        int tid, float& mx) {
  const int SH = H + 1;
  for (int n = tid; n < N; n += 256) {
    float sv = bm;
    if (STAGED) {
      const float* hr = &hS[(size_t)n * SH];
      for (int c = 0; c < H; ++c) sv = fmaf(hr[c], wS[c], sv);
    } else if ((H & 3) == 0) {
      const float4* hr4 = (const float4*)&hg[(size_t)n * H];
      for (int c4 = 0; c4 < (H >> 2); ++c4) {
        const float4 v = hr4[c4];
        sv = fmaf(v.x, wS[4 * c4], sv);
        sv = fmaf(v.y, wS[4 * c4 + 1], sv);
        sv = fmaf(v.z, wS[4 * c4 + 2], sv);
        sv = fmaf(v.w, wS[4 * c4 + 3], sv);
      }
    } else {
      const float* hr = &hg[(size_t)n * H];
      for (int c = 0; c < H; ++c) sv = fmaf(hr[c], wS[c], sv);
    }
    aS[n] = sv;
    mx = fmaxf(mx, sv);
  }
}

__global__ __launch_bounds__(256) void enc_seg_fwd_kernel(
    const float* __restrict__ h, const int* __restrict__ seg_off,
    const float* __restrict__ Wenc, const float* __restrict__ benc,
    const float* __restrict__ y, float* __restrict__ yp, int total, int M,
    int H, int a_cap, int stage_cap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* scratch = (float*)smem;  // [8] block reduces
  float* wS = scratch + 8;        // [64] Wenc row m
  float* aS = wS + 64;            // [a_cap] scores
  float* hS = aS + a_cap;         // [stage_cap][H+1]

  const int m = blockIdx.x;
  const int d = blockIdx.y;
  const int tid = threadIdx.x;
  const int SH = H + 1;

  const int r0 = seg_off[d];
  const int N = seg_off[d + 1] - r0;
  if (N <= 0) return;  // empty day: nothing to encode, output untouched
  const long oi = (long)d * M + m;
  if (r0 < 0 || r0 > total - N || N > a_cap) {
    // a segment outside the packed buffer or the launch's LDS plan is
    // never read: the day comes back marked instead
    if (tid == 0) yp[oi] = NAN;
    return;
  }
  const float* hg = h + (size_t)r0 * H;
  const float* yg = y + r0;
  const bool staged = N <= stage_cap;  // workgroup-uniform

  if (tid < H) wS[tid] = Wenc[(long)m * H + tid];
  if (staged) {
    for (int idx = tid; idx < N * H; idx += 256)
      hS[(idx / H) * SH + (idx % H)] = hg[idx];
  }
  __syncthreads();
  const float bm = benc[m];

  float mx = -INFINITY;
  if (staged)
    eseg_scores<true>(hg, hS, wS, aS, N, H, bm, tid, mx);
  else
    eseg_scores<false>(hg, hS, wS, aS, N, H, bm, tid, mx);
  mx = block_reduce_max(mx, scratch);

  // a thread reads back only the aS entries it wrote itself
  float sum = 0.0f;
  for (int n = tid; n < N; n += 256) sum += __expf(aS[n] - mx);
  sum = block_reduce_sum(sum, scratch);
  const float inv = 1.0f / sum;

  float wy = 0.0f;
  for (int n = tid; n < N; n += 256) {
    const float an = __expf(aS[n] - mx) * inv;
    wy = fmaf(an, yg[n], wy);
  }
  wy = block_reduce_sum(wy, scratch);
  if (tid == 0) yp[oi] = wy;
}

// yp (D,M) -> fmu, fsig_c (D,K): enc_fused_fwd_kernel's heads tail per day.
__global__ __launch_bounds__(256) void enc_seg_heads_kernel(
    const float* __restrict__ yp, const float* __restrict__ Wmu,
    const float* __restrict__ bmu, const float* __restrict__ Wsig,
    const float* __restrict__ bsig, float* __restrict__ fmu,
    float* __restrict__ fsig_c, int D, int M, int K) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)D * K) return;
  const int d = (int)(idx / K);
  const int k = (int)(idx % K);
  const float* ypd = yp + (long)d * M;
  const float* wm = &Wmu[(long)k * M];
  const float* ws = &Wsig[(long)k * M];
  float sm = bmu[k], ss = bsig[k];
  for (int i = 0; i < M; ++i) {
    sm = fmaf(ypd[i], wm[i], sm);
    ss = fmaf(ypd[i], ws[i], ss);
  }
  fmu[idx] = sm;
  const float s = softplusf_(ss);
  fsig_c[idx] = (s == 0.0f) ? 1e-6f : s;
}

// recon / y (total) packed, factor rows (D,K) -> loss, mse, kl (D).
__global__ __launch_bounds__(256) void loss_seg_kernel(
    const float* __restrict__ recon, const float* __restrict__ y,
    const int* __restrict__ seg_off, const float* __restrict__ fmu,
    const float* __restrict__ fsig_c, const float* __restrict__ pmu,
    const float* __restrict__ psig_c, float* __restrict__ loss_out,
    float* __restrict__ mse_out, float* __restrict__ kl_out, int total,
    int K) {
  __shared__ float scratch[8];
  const int d = blockIdx.x;
  const int tid = threadIdx.x;

  const int r0 = seg_off[d];
  const int N = seg_off[d + 1] - r0;
  if (N <= 0 || r0 < 0 || r0 > total - N) {
    // no rows, or rows outside the packed buffer: nothing is read
    if (tid == 0) {
      loss_out[d] = NAN;
      mse_out[d] = NAN;
      kl_out[d] = NAN;
    }
    return;
  }
  const float* rg = recon + r0;
  const float* yg = y + r0;
  const long f0 = (long)d * K;

  float se = 0.0f;
  for (int n = tid; n < N; n += 256) {
    const float dd = rg[n] - yg[n];
    se = fmaf(dd, dd, se);
  }
  se = block_reduce_sum(se, scratch);
  const float mse = se / N;

  float kl = 0.0f;
  for (int k = tid; k < K; k += 256) {
    const float fs = fsig_c[f0 + k], ps = psig_c[f0 + k];
    const float dmu = fmu[f0 + k] - pmu[f0 + k];
    const float ps2 = ps * ps;
    kl += __logf(ps / fs) + (fs * fs + dmu * dmu) / (2.0f * ps2) - 0.5f;
  }
  kl = block_reduce_sum(kl, scratch);

  if (tid == 0) {
    mse_out[d] = mse;
    kl_out[d] = kl;
    loss_out[d] = mse + kl;
  }
}

extern "C" {

// max_n: the longest segment (the host knows the day lengths; the kernel
// still refuses a longer one). Segments of up to stage_cap rows stage h
// in LDS; longer ones keep only the score vector there.
hipError_t fv_enc_seg_fwd(const float* h, const int* seg_off,
                          const float* Wenc, const float* benc,
                          const float* y, float* yp, int total, int D,
                          int max_n, int M, int H, hipStream_t s) {
  if (H < 1 || H > 64 || M < 1 || D > 65535) return hipErrorInvalidValue;
  if (D <= 0 || total <= 0 || max_n <= 0) return hipSuccess;
  const long budget = ESEG_LDS_MAX / (long)sizeof(float) - ESEG_FIXED;
  const long a_cap_l = ((long)max_n + 3) & ~3L;
  if (a_cap_l > budget) return hipErrorInvalidValue;
  const int a_cap = (int)a_cap_l;
  // rows of h image that fit next to the score vector; whether a segment
  // is staged changes where h is read from, never the arithmetic
  const long stage_lim = (budget - a_cap) / (H + 1);
  const int stage_cap = (int)(max_n < stage_lim ? max_n : stage_lim);
  const size_t lds =
      (size_t)(ESEG_FIXED + a_cap + (long)stage_cap * (H + 1)) * sizeof(float);
  if (lds > ESEG_LDS_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(enc_seg_fwd_kernel, dim3(M, D), dim3(256), lds, s, h,
                     seg_off, Wenc, benc, y, yp, total, M, H, a_cap,
                     stage_cap);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_enc_seg_heads(const float* yp, const float* Wmu,
                            const float* bmu, const float* Wsig,
                            const float* bsig, float* fmu, float* fsig_c,
                            int D, int M, int K, hipStream_t s) {
  if (M < 1) return hipErrorInvalidValue;
  if (D <= 0 || K <= 0) return hipSuccess;
  const long n = (long)D * K;
  hipLaunchKernelGGL(enc_seg_heads_kernel, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, s, yp, Wmu, bmu, Wsig, bsig, fmu, fsig_c,
                     D, M, K);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_loss_seg(const float* recon, const float* y, const int* seg_off,
                       const float* fmu, const float* fsig_c,
                       const float* pmu, const float* psig_c, float* loss,
                       float* mse, float* kl, int total, int D, int K,
                       hipStream_t s) {
  if (K < 1 || total < 0) return hipErrorInvalidValue;
  if (D <= 0) return hipSuccess;
  hipLaunchKernelGGL(loss_seg_kernel, dim3(D), dim3(256), 0, s, recon, y,
                     seg_off, fmu, fsig_c, pmu, psig_c, loss, mse, kl, total,
                     K);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
