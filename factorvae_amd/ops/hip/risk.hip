// Factor risk model of the prior decoder, per packed day (inference only).
//
//   Sigma_d = B diag(sz^2) B^T + diag(s2)
//     B  = beta (N_d,K), sz = psig_c (the prior sigma after its zero clamp),
//     s2 = svar = alpha_sigma^2 + 1e-6 (dec_seg_fwd's svar output)
//
//   risk_seg_kernel:       w^T Sigma w of one portfolio per day, split into
//     its factor and specific parts, the factor exposures B^T w and the
//     marginal contribution to risk of every stock.
//   risk_solve_seg_kernel: x = Sigma^-1 b for up to 4 right-hand sides
//     through the factor structure, C = diag(1/s) B diag(sz),
//     M = I + C^T C (SPD, eigenvalues >= 1), Cholesky of M in LDS,
//     x = b/s2 - C (M^-1 C^T (b/s)) / s. The dense matrix is never formed.
//
// One workgroup of 256 threads per day, as loss_seg_kernel. No float
// atomics; every reduction is ordered by segment-local indices only (row n
// of a day goes to wave n % 4 or thread n % 256, partial sums are combined
// in a fixed tree), so a day's bits do not depend on its position in the
// pack, on its neighbours or on the chunking. An empty day writes nothing
// per row and NaN in its per-day rows.

#include "common.h"
#include "launchers.h"

#define RISK_KMAX 128
// dynamic LDS ceiling of the segmented kernels (SEG_LDS_MAX of predict.hip)
#define RISK_LDS_MAX (144 * 1024)

// ---------------------------------------------------------------------
// stats row of a day: mean, mean_factor, var_factor, var_specific, vol
#define RISK_NSTAT 5
// rows a wave reads ahead of its arithmetic
#define RSEG_AHEAD 8

__global__ __launch_bounds__(256) void risk_seg_kernel(
    const float* __restrict__ beta, const float* __restrict__ svar,
    const float* __restrict__ mu, const float* __restrict__ w,
    const int* __restrict__ seg_off, const float* __restrict__ pmu,
    const float* __restrict__ psig_c, float* __restrict__ stats,
    float* __restrict__ exposure, float* __restrict__ factor_var,
    float* __restrict__ mcr, int total, int K) {
  __shared__ float scratch[8];
  __shared__ float part[4 * RISK_KMAX];  // [wave][k] exposure partials
  __shared__ float gS[RISK_KMAX];        // sz_k^2 * f_k

  const int d = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const long f0 = (long)d * K;

  const int r0 = seg_off[d];
  const int N = seg_off[d + 1] - r0;
  if (N <= 0 || r0 < 0 || r0 > total - N) {
    // no rows, or rows outside the packed buffer: nothing is read
    if (tid < RISK_NSTAT) stats[(long)d * RISK_NSTAT + tid] = NAN;
    for (int k = tid; k < K; k += 256) {
      exposure[f0 + k] = NAN;
      factor_var[f0 + k] = NAN;
    }
    return;
  }
  const float* bg = beta + (size_t)r0 * K;
  const float* sg = svar + r0;
  const float* mg = mu + r0;
  const float* wg = w + r0;

  // pass one: mean = w.mu, var_specific = sum w_i^2 s2_i (thread <-> row)
  float sm = 0.0f, sv = 0.0f;
  for (int n = tid; n < N; n += 256) {
    const float wi = wg[n];
    sm = fmaf(wi, mg[n], sm);
    sv = fmaf(wi * wi, sg[n], sv);
  }
  sm = block_reduce_sum(sm, scratch);
  sv = block_reduce_sum(sv, scratch);

  // exposure f_k = sum_n B[n][k] w_n (4 waves split the rows, lane <-> k).
  // RSEG_AHEAD rows of a wave are loaded before the first is used: the
  // loop is bound by load latency, and the fmaf chain keeps its row order.
  const bool k0 = lane < K, k1 = lane + 64 < K;
  float a0 = 0.0f, a1 = 0.0f;
  int n = wv;
  for (; n + 4 * (RSEG_AHEAD - 1) < N; n += 4 * RSEG_AHEAD) {
    float ww[RSEG_AHEAD], b0[RSEG_AHEAD], b1[RSEG_AHEAD];
#pragma unroll
    for (int u = 0; u < RSEG_AHEAD; ++u) {
      const float* row = bg + (size_t)(n + 4 * u) * K;
      ww[u] = wg[n + 4 * u];
      b0[u] = k0 ? row[lane] : 0.0f;
      b1[u] = k1 ? row[lane + 64] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < RSEG_AHEAD; ++u) {
      a0 = fmaf(b0[u], ww[u], a0);
      a1 = fmaf(b1[u], ww[u], a1);
    }
  }
  for (; n < N; n += 4) {
    const float wi = wg[n];
    const float* row = bg + (size_t)n * K;
    if (k0) a0 = fmaf(row[lane], wi, a0);
    if (k1) a1 = fmaf(row[lane + 64], wi, a1);
  }
  part[wv * RISK_KMAX + lane] = a0;
  part[wv * RISK_KMAX + 64 + lane] = a1;
  __syncthreads();
  float fv = 0.0f, mf = 0.0f;
  if (tid < K) {
    const float f = (part[tid] + part[RISK_KMAX + tid]) +
                    (part[2 * RISK_KMAX + tid] + part[3 * RISK_KMAX + tid]);
    const float sz = psig_c[f0 + tid];
    const float g = sz * sz * f;
    fv = f * g;  // f_k^2 sz_k^2
    mf = f * pmu[f0 + tid];
    gS[tid] = g;
    exposure[f0 + tid] = f;
    factor_var[f0 + tid] = fv;
  }
  fv = block_reduce_sum(fv, scratch);  // its barriers publish gS too
  mf = block_reduce_sum(mf, scratch);
  const float vol = sqrtf(fv + sv);
  if (tid == 0) {
    float* st = stats + (long)d * RISK_NSTAT;
    st[0] = sm;
    st[1] = mf;
    st[2] = fv;
    st[3] = sv;
    st[4] = vol;
  }

  // pass two: mcr_n = (sum_k B[n][k] sz_k^2 f_k + w_n s2_n) / vol
  const float g0 = (lane < K) ? gS[lane] : 0.0f;
  const float g1 = (lane + 64 < K) ? gS[lane + 64] : 0.0f;
  n = wv;
  for (; n + 4 * (RSEG_AHEAD - 1) < N; n += 4 * RSEG_AHEAD) {
    float b0[RSEG_AHEAD], b1[RSEG_AHEAD], ws[RSEG_AHEAD];
#pragma unroll
    for (int u = 0; u < RSEG_AHEAD; ++u) {
      const float* row = bg + (size_t)(n + 4 * u) * K;
      b0[u] = k0 ? row[lane] : 0.0f;
      b1[u] = k1 ? row[lane + 64] : 0.0f;
      ws[u] = wg[n + 4 * u] * sg[n + 4 * u];
    }
#pragma unroll
    for (int u = 0; u < RSEG_AHEAD; ++u) {
      float v = fmaf(b1[u], g1, b0[u] * g0);
      v = wave_reduce_sum(v);
      if (lane == 0) {
        const float num = add_rn_(v, ws[u]);
        mcr[r0 + n + 4 * u] = (vol == 0.0f) ? NAN : num / vol;
      }
    }
  }
  for (; n < N; n += 4) {
    const float* row = bg + (size_t)n * K;
    float v = fmaf(k1 ? row[lane + 64] : 0.0f, g1,
                   (k0 ? row[lane] : 0.0f) * g0);
    v = wave_reduce_sum(v);
    if (lane == 0) {
      const float num = add_rn_(v, wg[n] * sg[n]);  // as above
      mcr[r0 + n] = (vol == 0.0f) ? NAN : num / vol;
    }
  }
}

// ---------------------------------------------------------------------
// risk_solve_seg_kernel<TS>: the 256 threads form a 16 x 16 grid, thread
// (ti, tj) keeps the TS x TS tile of M at (ti*TS, tj*TS) in registers for
// the whole day; TS = 2 / 4 / 8 covers K <= 32 / 64 / 128. Row tiles of C
// (RSOLVE_RT stock rows, zero-padded to KP = 16*TS columns) are staged
// through LDS and every thread adds its outer-product share row by row, so
// an entry of M is one fmaf chain over the day's rows in order.
//
// LDS map (floats):
//   sgS[128]  sz_k (0 beyond K)        vS[4][128] C^T(b/s), later u
//   yS[4][128] forward-substitution y  bS[RT][4]  staged b/s
//   isS[RT]   staged 1/s               nS[4][8]   per-wave sums of x, |x|
//   cS[RT][KP+4]  staged C rows (16-byte aligned rows)
//   MS[K][K|1]    M, then its Cholesky factor L (lower); the odd stride
//                 keeps column walks off one bank
// At K = 128: 1344 + 32*132 + 128*129 floats = 86.3 KiB of RISK_LDS_MAX.
#define RSOLVE_RT 32
#define RSOLVE_RMAX 4
#define RSOLVE_FIXED \
  (128 + 4 * 128 + 4 * 128 + RSOLVE_RT * 4 + RSOLVE_RT + 4 * 8)

template <int TS>
__global__ __launch_bounds__(256) void risk_solve_seg_kernel(
    const float* __restrict__ beta, const float* __restrict__ svar,
    const int* __restrict__ seg_off, const float* __restrict__ psig_c,
    const float* __restrict__ b, float* __restrict__ x,
    int* __restrict__ info, float* __restrict__ norms,  // (D,2,R) or null
    int total, int K, int R) {
  constexpr int KP = 16 * TS;
  constexpr int SC = KP + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sgS = (float*)smem;
  float* vS = sgS + 128;
  float* yS = vS + 4 * 128;
  float* bS = yS + 4 * 128;
  float* isS = bS + RSOLVE_RT * 4;
  float* nS = isS + RSOLVE_RT;
  float* cS = nS + 4 * 8;
  float* MS = cS + RSOLVE_RT * SC;
  const int SK = K | 1;

  const int d = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;

  const int r0 = seg_off[d];
  const int N = seg_off[d + 1] - r0;
  if (N <= 0 || r0 < 0 || r0 > total - N) {
    // no rows (info 0), or rows outside the packed buffer (info 2):
    // nothing is read and no row is written
    if (tid == 0) info[d] = (N <= 0) ? 0 : 2;
    if (norms && tid < 2 * R) norms[(long)d * 2 * R + tid] = NAN;
    return;
  }
  const float* bg = beta + (size_t)r0 * K;
  const float* sg = svar + r0;
  const float* rhs = b + (size_t)r0 * R;
  float* xg = x + (size_t)r0 * R;

  if (tid < 128) sgS[tid] = (tid < K) ? psig_c[(long)d * K + tid] : 0.0f;

  // ---- M = I + C^T C and v = C^T (b/s), one pass over the rows
  const int ti = tid >> 4, tj = tid & 15;
  const int vk = tid & 127, vc = tid >> 7;  // v[vk][vc], v[vk][vc+2]
  float acc[TS][TS];
#pragma unroll
  for (int i = 0; i < TS; ++i)
#pragma unroll
    for (int j = 0; j < TS; ++j) acc[i][j] = 0.0f;
  float v0 = 0.0f, v1 = 0.0f;

  for (int t0 = 0; t0 < N; t0 += RSOLVE_RT) {
    const int rows = min(RSOLVE_RT, N - t0);
    __syncthreads();  // the previous tile is consumed (first: sgS is set)
    if (tid < RSOLVE_RT) {
      const int n = t0 + tid;
      const float is = (tid < rows) ? 1.0f / sqrtf(sg[n]) : 0.0f;
      isS[tid] = is;
#pragma unroll
      for (int c = 0; c < RSOLVE_RMAX; ++c)
        bS[tid * 4 + c] =
            (tid < rows && c < R) ? rhs[(size_t)n * R + c] * is : 0.0f;
    }
    __syncthreads();
    for (int idx = tid; idx < RSOLVE_RT * KP; idx += 256) {
      const int r = idx / KP, k = idx % KP;  // KP is a power of two
      float c = 0.0f;
      if (r < rows && k < K)
        c = bg[(size_t)(t0 + r) * K + k] * sgS[k] * isS[r];
      cS[r * SC + k] = c;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const float* cr = &cS[r * SC];
      float a[TS], bb[TS];
#pragma unroll
      for (int i = 0; i < TS; ++i) a[i] = cr[ti * TS + i];
#pragma unroll
      for (int j = 0; j < TS; ++j) bb[j] = cr[tj * TS + j];
#pragma unroll
      for (int i = 0; i < TS; ++i)
#pragma unroll
        for (int j = 0; j < TS; ++j) acc[i][j] = fmaf(a[i], bb[j], acc[i][j]);
      if (vk < KP) {
        const float cv = cr[vk];
        v0 = fmaf(cv, bS[r * 4 + vc], v0);
        v1 = fmaf(cv, bS[r * 4 + vc + 2], v1);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TS; ++i)
#pragma unroll
    for (int j = 0; j < TS; ++j) {
      const int gi = ti * TS + i, gj = tj * TS + j;
      if (gi < K && gj < K)
        MS[gi * SK + gj] = acc[i][j] + (gi == gj ? 1.0f : 0.0f);
    }
  if (vk < K) {
    vS[vc * 128 + vk] = v0;
    vS[(vc + 2) * 128 + vk] = v1;
  }
  __syncthreads();

  // ---- Cholesky M = L L^T in place (lower triangle), right-looking.
  // The pivot is one LDS word read by every thread behind a barrier, so
  // the failure branch is workgroup-uniform.
  bool fail = false;
  for (int j = 0; j < K; ++j) {
    const float p = MS[j * SK + j];
    if (!(p > 0.0f) || !(p < INFINITY)) {
      fail = true;
      break;
    }
    const float dj = sqrtf(p);
    __syncthreads();  // every thread has read the pivot
    if (tid == 0) MS[j * SK + j] = dj;
    for (int i = j + 1 + tid; i < K; i += 256) MS[i * SK + j] /= dj;
    __syncthreads();
    // trailing update: wave <-> row i, lane <-> column k <= i
    for (int i = j + 1 + wv; i < K; i += 4) {
      const float lij = MS[i * SK + j];
      for (int k = j + 1 + lane; k <= i; k += 64)
        MS[i * SK + k] = fmaf(-lij, MS[k * SK + j], MS[i * SK + k]);
    }
    __syncthreads();
  }

  if (!fail) {
    // L y = v, then L^T u = y: wave <-> right-hand side, lane <-> row.
    // Column c of v / y / u is element-wise sequential in j.
    for (int j = 0; j < K; ++j) {
      __syncthreads();
      if (wv < R) {
        const float t = vS[wv * 128 + j] / MS[j * SK + j];
        for (int i = j + 1 + lane; i < K; i += 64)
          vS[wv * 128 + i] = fmaf(-MS[i * SK + j], t, vS[wv * 128 + i]);
        if (lane == 0) yS[wv * 128 + j] = t;
      }
    }
    for (int j = K - 1; j >= 0; --j) {
      __syncthreads();
      if (wv < R) {
        const float t = yS[wv * 128 + j] / MS[j * SK + j];
        for (int i = lane; i < j; i += 64)
          yS[wv * 128 + i] = fmaf(-MS[j * SK + i], t, yS[wv * 128 + i]);
        if (lane == 0) vS[wv * 128 + j] = t;  // u over v's slot
      }
    }
    __syncthreads();
  }

  // ---- x_n = b_n / s2_n - (C u)_n / s_n (wave <-> row, lane <-> k)
  float u0[RSOLVE_RMAX], u1[RSOLVE_RMAX];
#pragma unroll
  for (int c = 0; c < RSOLVE_RMAX; ++c) {
    u0[c] = (!fail && c < R && lane < K) ? vS[c * 128 + lane] : 0.0f;
    u1[c] = (!fail && c < R && lane + 64 < K) ? vS[c * 128 + 64 + lane] : 0.0f;
  }
  const float z0 = (lane < K) ? sgS[lane] : 0.0f;
  const float z1 = (lane + 64 < K) ? sgS[lane + 64] : 0.0f;
  float xs[RSOLVE_RMAX], xa[RSOLVE_RMAX];  // lane 0: sums of x and |x|
#pragma unroll
  for (int c = 0; c < RSOLVE_RMAX; ++c) xs[c] = xa[c] = 0.0f;
  for (int n = wv; n < N; n += 4) {
    const float s2 = sg[n];
    const float is = 1.0f / sqrtf(s2);
    const float* row = bg + (size_t)n * K;
    float c0 = 0.0f, c1 = 0.0f;
    if (!fail) {
      if (lane < K) c0 = row[lane] * z0 * is;
      if (lane + 64 < K) c1 = row[lane + 64] * z1 * is;
    }
#pragma unroll
    for (int c = 0; c < RSOLVE_RMAX; ++c) {
      if (c < R) {  // workgroup-uniform
        float t = fmaf(c1, u1[c], c0 * u0[c]);
        t = wave_reduce_sum(t);
        if (lane == 0) {
          const float xv =
              fail ? NAN : rhs[(size_t)n * R + c] / s2 - t * is;
          xg[(size_t)n * R + c] = xv;
          xs[c] += xv;
          xa[c] += fabsf(xv);
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < RSOLVE_RMAX; ++c) {
      nS[wv * 8 + c] = xs[c];
      nS[wv * 8 + 4 + c] = xa[c];
    }
  }
  __syncthreads();
  if (tid == 0) info[d] = fail ? 1 : 0;
  if (norms && tid < 2 * R) {
    const int q = tid / R, c = tid % R;  // q = 0: sum x, 1: sum |x|
    const int o = q * 4 + c;
    norms[(long)d * 2 * R + tid] =
        (nS[o] + nS[8 + o]) + (nS[16 + o] + nS[24 + o]);
  }
}

template <int TS>
static hipError_t rsolve_launch(const float* beta, const float* svar,
                                const int* seg_off, const float* psig_c,
                                const float* b, float* x, int* info,
                                float* norms, int total, int D, int K, int R,
                                hipStream_t s) {
  const size_t lds = (size_t)(RSOLVE_FIXED + RSOLVE_RT * (16 * TS + 4) +
                              (long)K * (K | 1)) *
                     sizeof(float);
  if (lds > RISK_LDS_MAX) return hipErrorInvalidValue;
  static bool attr_set = false;  // dynamic LDS above the 64 KiB default
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(
        (const void*)risk_solve_seg_kernel<TS>,
        hipFuncAttributeMaxDynamicSharedMemorySize, RISK_LDS_MAX);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(risk_solve_seg_kernel<TS>, dim3(D), dim3(256), lds, s,
                     beta, svar, seg_off, psig_c, b, x, info, norms, total, K,
                     R);
  HIP_CHECK_LAST();
  return hipSuccess;
}

extern "C" {

hipError_t fv_risk_seg(const float* beta, const float* svar, const float* mu,
                       const float* w, const int* seg_off, const float* pmu,
                       const float* psig_c, float* stats, float* exposure,
                       float* factor_var, float* mcr, int total, int D, int K,
                       hipStream_t s) {
  if (K < 1 || K > RISK_KMAX || total < 0) return hipErrorInvalidValue;
  if (D <= 0) return hipSuccess;
  hipLaunchKernelGGL(risk_seg_kernel, dim3(D), dim3(256), 0, s, beta, svar,
                     mu, w, seg_off, pmu, psig_c, stats, exposure, factor_var,
                     mcr, total, K);
  HIP_CHECK_LAST();
  return hipSuccess;
}

// x (sumN,R) = Sigma_d^-1 b per day; info (D): 0 solved (or no rows), 1 a
// non-positive or non-finite pivot (the day's x is NaN), 2 rows outside the
// packed buffer (nothing written). norms (D,2,R), nullable: the day's
// sum x and sum |x| per column, for the weight normalisations.
hipError_t fv_risk_solve_seg(const float* beta, const float* svar,
                             const int* seg_off, const float* psig_c,
                             const float* b, float* x, int* info,
                             float* norms, int total, int D, int K, int R,
                             hipStream_t s) {
  if (K < 1 || K > RISK_KMAX || R < 1 || R > RSOLVE_RMAX || total < 0)
    return hipErrorInvalidValue;
  if (D <= 0) return hipSuccess;
  if (K <= 32)
    return rsolve_launch<2>(beta, svar, seg_off, psig_c, b, x, info, norms,
                            total, D, K, R, s);
  if (K <= 64)
    return rsolve_launch<4>(beta, svar, seg_off, psig_c, b, x, info, norms,
                            total, D, K, R, s);
  return rsolve_launch<8>(beta, svar, seg_off, psig_c, b, x, info, norms,
                          total, D, K, R, s);
}

}  // extern "C"
