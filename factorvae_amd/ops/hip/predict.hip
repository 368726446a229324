// Batched multi-day scoring kernels (inference only).
//
// Many trading days are packed back to back into one (sumN, ...) buffer;
// an int32 device array seg_off[D+1] gives each day's row range. Only two
// places in the model couple stocks — the predictor's softmax over the
// stock axis and the per-day prior (pmu, psig_c) — so those two are the
// segmented kernels here; everything else (extractor head, GRU) is per
// row and runs unchanged over the packed rows.
//
//   attn_seg_fwd_kernel: attn_fused_fwd_kernel's chain without dropout,
//     one workgroup per (head, day); writes only pmu / psig_c / guard.
//   dec_seg_fwd_kernel:  dec_fwd_kernel's row arithmetic with the factor
//     prior of the row's own day; writes mu / sigma (+ sample, + beta).
//
// Every reduction is ordered by segment-local indices only (same
// 256-thread partition, four-way wave split and wave tree as the per-day
// kernels), so a day's result does not depend on its position in the
// batch, on its neighbours, or on whether its h rows were staged in LDS.

#include "common.h"
#include "launchers.h"

// ---------------------------------------------------------------------
// LDS map of attn_seg_fwd_kernel (floats, every carve a multiple of 4):
//   scratch[8] part[256] qkS[64] uS[64] hm2S[64] ctxS[64] bad[4]
//   WS[H*(H+1) rounded up to 4] aS[a_cap] hS[stage_cap*(H+1)]
#define SEG_FIXED (8 + 256 + 4 * 64 + 4)
#define SEG_LDS_MAX (144 * 1024)

DEVINL int seg_ws_floats(int H) { return (H * (H + 1) + 3) & ~3; }

// scores + NaN scan + max (thread <-> stock row), then softmax into aS.
// STAGED: h rows come from the LDS image (stride H+1); otherwise they are
// re-read from global/L2 (stride H). The fmaf chain over c is the same.
template <bool STAGED>
DEVINL void seg_scores(const float* __restrict__ hg, const float* hS,
                       const float* qkS, float* aS, int N, int H, float ck,
                       float alpha, int tid, int& bad, float& mx) {
  const int SH = H + 1;
  for (int n = tid; n < N; n += 256) {
    float s = 0.0f;
    if (STAGED) {
      const float* hr = &hS[(size_t)n * SH];
      for (int c = 0; c < H; ++c) s = fmaf(hr[c], qkS[c], s);
    } else if ((H & 3) == 0) {
      const float4* hr4 = (const float4*)&hg[(size_t)n * H];
      for (int c4 = 0; c4 < (H >> 2); ++c4) {
        const float4 v = hr4[c4];
        s = fmaf(v.x, qkS[4 * c4], s);
        s = fmaf(v.y, qkS[4 * c4 + 1], s);
        s = fmaf(v.z, qkS[4 * c4 + 2], s);
        s = fmaf(v.w, qkS[4 * c4 + 3], s);
      }
    } else {
      const float* hr = &hg[(size_t)n * H];
      for (int c = 0; c < H; ++c) s = fmaf(hr[c], qkS[c], s);
    }
    s = (s + ck) * alpha;
    aS[n] = s;
    if (isnan(s) || s == INFINITY) bad = 1;
    mx = fmaxf(mx, (s > 0.0f) ? s : 0.0f);
  }
}

__global__ __launch_bounds__(256) void attn_seg_fwd_kernel(
    const float* __restrict__ h, const int* __restrict__ seg_off,
    const float* __restrict__ qk, const float* __restrict__ cb,
    const float* __restrict__ Wv, const float* __restrict__ bv,
    const float* __restrict__ Wl, const float* __restrict__ bl,
    const float* __restrict__ wmu, const float* __restrict__ bmu,
    const float* __restrict__ wsig, const float* __restrict__ bsig,
    float* __restrict__ pmu, float* __restrict__ psig_c,
    int* __restrict__ guard, int total, int K, int H, float alpha,
    int a_cap, int stage_cap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* scratch = (float*)smem;        // [8] block reduces
  float* part = scratch + 8;            // [4][64]
  float* qkS = part + 256;              // [64]
  float* uS = qkS + 64;                 // [64]
  float* hm2S = uS + 64;                // [64]
  float* ctxS = hm2S + 64;              // [64]
  int* bad_s = (int*)(ctxS + 64);       // [4] (one used)
  float* WS = ctxS + 64 + 4;            // [H][H+1]: Wv then Wl staged
  float* aS = WS + seg_ws_floats(H);    // [a_cap]
  float* hS = aS + a_cap;               // [stage_cap][H+1]

  const int k = blockIdx.x;
  const int d = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int SH = H + 1;

  const int r0 = seg_off[d];
  const int N = seg_off[d + 1] - r0;
  if (N <= 0) return;  // empty day: nothing to score, outputs untouched
  const long oi = (long)d * K + k;
  if (r0 < 0 || r0 > total - N || N > a_cap) {
    // a segment outside the packed buffer or the launch's LDS plan is
    // never read: the day comes back marked instead
    if (tid == 0) {
      pmu[oi] = NAN;
      psig_c[oi] = NAN;
      guard[oi] = 2;
    }
    return;
  }
  const float* hg = h + (size_t)r0 * H;
  const bool staged = N <= stage_cap;  // workgroup-uniform

  if (tid == 0) bad_s[0] = 0;
  if (tid < H) qkS[tid] = qk[(long)k * H + tid];
  if (staged) {
    for (int idx = tid; idx < N * H; idx += 256)
      hS[(idx / H) * SH + (idx % H)] = hg[idx];
  }
  __syncthreads();
  const float ck = cb[k];

  int bad = 0;
  float mx = -INFINITY;
  if (staged)
    seg_scores<true>(hg, hS, qkS, aS, N, H, ck, alpha, tid, bad, mx);
  else
    seg_scores<false>(hg, hS, qkS, aS, N, H, ck, alpha, tid, bad, mx);
  if (bad) atomicOr(bad_s, 1);
  mx = block_reduce_max(mx, scratch);

  float sum = 0.0f;
  for (int n = tid; n < N; n += 256) {
    const float v = aS[n];
    sum += __expf(((v > 0.0f) ? v : 0.0f) - mx);
  }
  sum = block_reduce_sum(sum, scratch);
  const float inv = 1.0f / sum;
  for (int n = tid; n < N; n += 256) {
    const float v = aS[n];
    aS[n] = __expf(((v > 0.0f) ? v : 0.0f) - mx) * inv;
  }
  __syncthreads();
  const bool g = bad_s[0] != 0;
  if (tid == 0) guard[oi] = g ? 1 : 0;

  // u[c] = sum_n a[n] * h[n][c]  (4 waves split the stock range)
  float acc = 0.0f;
  if (lane < H) {
    if (staged) {
      for (int n = w; n < N; n += 4)
        acc = fmaf(aS[n], hS[(size_t)n * SH + lane], acc);
    } else {
      for (int n = w; n < N; n += 4)
        acc = fmaf(aS[n], hg[(size_t)n * H + lane], acc);
    }
  }
  part[w * 64 + lane] = acc;
  __syncthreads();
  if (w == 0 && lane < H)
    uS[lane] = part[lane] + part[64 + lane] + part[128 + lane] +
               part[192 + lane];
  __syncthreads();

  // ctx[j] = Wv[k][j]·u + bv (guarded -> 0); Wv staged in LDS first
  const int SW = H + 1;
  for (int idx = tid; idx < H * H; idx += 256)
    WS[(idx / H) * SW + (idx % H)] = Wv[(long)k * H * H + idx];
  __syncthreads();
  const float ul = (lane < H) ? uS[lane] : 0.0f;
  const int jpw = (H + 3) / 4;
  for (int j = w * jpw; j < min((w + 1) * jpw, H); ++j) {
    float v = (!g && lane < H) ? WS[(size_t)j * SW + lane] * ul : 0.0f;
    v = wave_reduce_sum(v);
    if (lane == 0) ctxS[j] = g ? 0.0f : v + bv[(long)k * H + j];
  }
  __syncthreads();

  // shared MLP: hm2 = lrelu(ctx@Wl^T + bl); Wl staged over Wv's slot
  for (int idx = tid; idx < H * H; idx += 256)
    WS[(idx / H) * SW + (idx % H)] = Wl[idx];
  __syncthreads();
  const float cl = (lane < H) ? ctxS[lane] : 0.0f;
  for (int j = w * jpw; j < min((w + 1) * jpw, H); ++j) {
    float v = (lane < H) ? WS[(size_t)j * SW + lane] * cl : 0.0f;
    v = wave_reduce_sum(v);
    if (lane == 0) hm2S[j] = lrelu_(v + bl[j]);
  }
  __syncthreads();
  if (w == 0) {
    const float z = (lane < H) ? hm2S[lane] : 0.0f;
    float pm = (lane < H) ? z * wmu[lane] : 0.0f;
    float ps = (lane < H) ? z * wsig[lane] : 0.0f;
    pm = wave_reduce_sum(pm);
    ps = wave_reduce_sum(ps);
    if (lane == 0) {
      pmu[oi] = pm + bmu[0];
      const float pre = ps + bsig[0];
      const float sp = softplusf_(pre);
      psig_c[oi] = (sp == 0.0f) ? 1e-6f : sp;
    }
  }
}

// ---------------------------------------------------------------------
// Segmented decoder. Geometry as dec_fwd_kernel (wave <-> row, lane <->
// hidden unit, W1/Wb transposed in LDS), but a workgroup walks `iters`
// row groups per weight staging (dec_fwd restages for every 4 rows) and
// writes none of the backward state (a1, asig_pre). The row's day is
// found by a search of seg_off on the device.
#define DSEG_RPW 4

__global__ __launch_bounds__(256) void dec_seg_fwd_kernel(
    const float* __restrict__ h, const int* __restrict__ seg_off,
    const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ wmu, const float* __restrict__ bmu,
    const float* __restrict__ wsig, const float* __restrict__ bsig,
    const float* __restrict__ Wb, const float* __restrict__ bb,
    const float* __restrict__ fmu, const float* __restrict__ fsig_c,
    const float* __restrict__ eps,   // (sumN) or null
    float* __restrict__ mu_out, float* __restrict__ sigma_out,
    float* __restrict__ sample_out,  // written only with eps
    float* __restrict__ beta_out,    // (sumN,K) or null
    float* __restrict__ svar_out,    // (sumN) or null: asig^2 + 1e-6
    int N, int D, int K, int H, int iters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* W1T = (float*)smem;                   // [H][H]
  float* WbT = W1T + (size_t)H * H;            // [H][K]
  float* hS = WbT + (size_t)H * K;             // [DSEG_RPW][H]

  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = tid & 63;

  for (int idx = tid; idx < H * H; idx += 256) {
    const int j = idx / H, i = idx % H;
    W1T[(size_t)i * H + j] = W1[idx];
  }
  for (int idx = tid; idx < K * H; idx += 256) {
    const int k = idx / H, i = idx % H;
    WbT[(size_t)i * K + k] = Wb[idx];
  }
  __syncthreads();

  const float* hr = &hS[w * H];
  for (int it = 0; it < iters; ++it) {
    const int row = (blockIdx.x * iters + it) * DSEG_RPW + w;
    if (row >= N) break;  // wave-uniform; no barriers below
    // hS[w] is private to wave w: in-wave LDS dependency only
    if (lane < H) hS[w * H + lane] = h[(long)row * H + lane];

    // day of this row: largest d with seg_off[d] <= row (empty days
    // share an offset with their successor and are never selected)
    int lo = 0, hi = D - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seg_off[mid] <= row) lo = mid; else hi = mid - 1;
    }
    const float* fm = fmu + (long)lo * K;
    const float* fsc = fsig_c + (long)lo * K;

    // a1
    float a1v = 0.0f;
    if (lane < H) {
      a1v = b1[lane];
      for (int i = 0; i < H; ++i)
        a1v = fmaf(hr[i], W1T[(size_t)i * H + lane], a1v);
      a1v = lrelu_(a1v);
    }
    // alpha heads (wave reductions)
    float pm = (lane < H) ? a1v * wmu[lane] : 0.0f;
    float ps = (lane < H) ? a1v * wsig[lane] : 0.0f;
    pm = wave_reduce_sum(pm);
    ps = wave_reduce_sum(ps);
    pm = __shfl(pm, 0, 64);
    ps = __shfl(ps, 0, 64);
    const float amu = pm + bmu[0];
    const float asig_pre = ps + bsig[0];
    const float asig = softplusf_(asig_pre);

    // beta + factor combine
    float mu_b = 0.0f, var_b = 0.0f;
    for (int k = lane; k < K; k += 64) {
      float bv = bb[k];
      for (int i = 0; i < H; ++i) bv = fmaf(hr[i], WbT[(size_t)i * K + k], bv);
      if (beta_out) beta_out[(long)row * K + k] = bv;
      const float fs = fsc[k];
      mu_b = fmaf(bv, fm[k], mu_b);
      var_b = fmaf(bv * bv, fs * fs, var_b);
    }
    mu_b = wave_reduce_sum(mu_b);
    var_b = wave_reduce_sum(var_b);

    if (lane == 0) {
      const float mu = amu + mu_b;
      const float var = asig * asig + var_b + 1e-6f;
      const float sig = sqrtf(var);
      mu_out[row] = mu;
      sigma_out[row] = sig;
      if (eps) sample_out[row] = fmaf(eps[row], sig, mu);
      // the row's idiosyncratic variance, from the same softplus; an
      // explicit fmaf, so no multiply is shared with var above and its
      // contraction (and sigma's bits) stay as they were
      if (svar_out) svar_out[row] = fmaf(asig, asig, 1e-6f);
    }
  }
}

extern "C" {

// max_n: the longest segment (the host knows the day lengths; the kernel
// still refuses a longer one). Segments of up to stage_cap rows stage h
// in LDS; longer ones keep only the score vector there.
hipError_t fv_attn_seg_fwd(const float* h, const int* seg_off,
                           const float* qk, const float* cb, const float* Wv,
                           const float* bv, const float* Wl, const float* bl,
                           const float* wmu, const float* bmu,
                           const float* wsig, const float* bsig, float* pmu,
                           float* psig_c, int* guard, int total, int D,
                           int max_n, int K, int H, float alpha,
                           hipStream_t s) {
  if (H > 64 || K > 128) return hipErrorInvalidValue;
  if (D <= 0 || total <= 0 || max_n <= 0) return hipSuccess;
  const long fixed = SEG_FIXED + ((H * (H + 1) + 3) & ~3);
  const long budget = SEG_LDS_MAX / (long)sizeof(float) - fixed;
  const int a_cap = (max_n + 3) & ~3;
  if (a_cap > budget) return hipErrorInvalidValue;
  // rows of h image that fit next to the score vector; whether a segment
  // is staged changes where h is read from, never the arithmetic
  long stage_lim = (budget - a_cap) / (H + 1);
  const int stage_cap = (int)(max_n < stage_lim ? max_n : stage_lim);
  const size_t lds =
      (size_t)(fixed + a_cap + (long)stage_cap * (H + 1)) * sizeof(float);
  if (lds > SEG_LDS_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_seg_fwd_kernel, dim3(K, D), dim3(256), lds, s, h,
                     seg_off, qk, cb, Wv, bv, Wl, bl, wmu, bmu, wsig, bsig,
                     pmu, psig_c, guard, total, K, H, alpha, a_cap,
                     stage_cap);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_dec_seg_fwd(const float* h, const int* seg_off,
                          const float* W1, const float* b1, const float* wmu,
                          const float* bmu, const float* wsig,
                          const float* bsig, const float* Wb, const float* bb,
                          const float* fmu, const float* fsig_c,
                          const float* eps, float* mu, float* sigma,
                          float* sample, float* beta, float* svar, int N,
                          int D, int K, int H, hipStream_t s) {
  if (H > 64 || K > 128) return hipErrorInvalidValue;
  if (N <= 0 || D <= 0) return hipSuccess;
  if (eps && !sample) return hipErrorInvalidValue;
  const size_t lds =
      ((size_t)H * H + (size_t)H * K + DSEG_RPW * H) * sizeof(float);
  // ~1024 workgroups keep the chip full; beyond that a workgroup walks
  // more row groups per weight staging (<= 16)
  int iters = (N + DSEG_RPW * 1024 - 1) / (DSEG_RPW * 1024);
  if (iters > 16) iters = 16;
  if (iters < 1) iters = 1;
  const int nblk = (N + DSEG_RPW * iters - 1) / (DSEG_RPW * iters);
  hipLaunchKernelGGL(dec_seg_fwd_kernel, dim3(nblk), dim3(256), lds, s, h,
                     seg_off, W1, b1, wmu, bmu, wsig, bsig, Wb, bb, fmu,
                     fsig_c, eps, mu, sigma, sample, beta, svar, N, D, K, H,
                     iters);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
