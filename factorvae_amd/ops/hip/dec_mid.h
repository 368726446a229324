// Body of dec_fwd_bwd_kernel as a __device__ function of the block index
// and the block count, shared by decoder.hip (whose __global__ kernel is a
// thin wrapper around it) and mid_fuse.hip. What it computes and why it is
// bit-identical to dec_fwd + loss_fused + dec_bwd is described in
// decoder.hip, above the wrapper.
#pragma once

#include "common.h"
#include "stage.h"

#define DEC_RPW 4

// dec_bwd's launch geometry: ~128+ blocks to fill the chip, <= 8
// row-iterations per block
static inline void dec_bwd_geometry(int N, int* iters, int* nblk) {
  int it = (N + DEC_RPW * 128 - 1) / (DEC_RPW * 128);
  if (it > 8) it = 8;
  if (it < 1) it = 1;
  *iters = it;
  *nblk = (N + DEC_RPW * it - 1) / (DEC_RPW * it);
}

// Dynamic LDS of the body, in bytes
static inline size_t dec_fwd_bwd_lds(int K, int H) {
  return ((size_t)(H + K) * (H + 1) + 3 * DEC_RPW * H + (size_t)DEC_RPW * K +
          4 * 64) * sizeof(float);
}

// Block bid of NB: rows (bid * iters + it) * DEC_RPW + wave, and column bid
// of the (2K + 2H + 2, NB) partials.
DEVINL void dec_fwd_bwd_body(
    const float* __restrict__ h, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ wmu,
    const float* __restrict__ bmu, const float* __restrict__ wsig,
    const float* __restrict__ bsig, const float* __restrict__ Wb,
    const float* __restrict__ bb, const float* __restrict__ fmu,
    const float* __restrict__ fsig_c, const float* __restrict__ eps,
    const float* __restrict__ y, float* __restrict__ recon,
    float* __restrict__ a1_out, float* __restrict__ beta_out,
    float* __restrict__ asig_pre_out, float* __restrict__ sigma_out,
    float* __restrict__ drecon_out, float* __restrict__ dh,
    float* __restrict__ dz1, float* __restrict__ dbeta_out,
    float* __restrict__ part, int N, int K, int H, int iters, float gscale,
    const int bid, const int NB) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int SH = H + 1;
  float* W1S = (float*)smem;                 // [H][H+1] as-is
  float* WbS = W1S + (size_t)H * SH;         // [K][H+1] as-is
  float* hS = WbS + (size_t)K * SH;          // [DEC_RPW][H]
  float* dz1S = hS + (size_t)DEC_RPW * H;    // [DEC_RPW][H]
  float* dbS = dz1S + (size_t)DEC_RPW * H;   // [DEC_RPW][K]
  float* red = dbS + (size_t)DEC_RPW * K;    // [4][64] reduce pad

  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = tid & 63;
  const bool inH = lane < H;
  const bool kh2 = (lane + 64) < K;
  const int lc = min(lane, H - 1);
  const int k0 = min(lane, K - 1), k1 = min(lane + 64, K - 1);

  // per-lane parameters, loaded once (clamped: dead lanes never use them)
  const float b1_r = b1[lc], wmu_r = wmu[lc], wsig_r = wsig[lc];
  const float bmu0 = bmu[0], bsig0 = bsig[0];
  const float bb_r0 = bb[k0], bb_r1 = bb[k1];
  const float fmu_r0 = fmu[k0], fmu_r1 = fmu[k1];
  const float fs_r0 = fsig_c[k0], fs_r1 = fsig_c[k1];
  const float dscale = gscale * 2.0f / N;

  if ((H & 3) == 0) {
    stage_rows_lds<true, 16>(W1S, W1, H, H, tid);
    stage_rows_lds<true, 16>(WbS, Wb, K, H, tid);
  } else {
    stage_rows_lds<false, 16>(W1S, W1, H, H, tid);
    stage_rows_lds<false, 16>(WbS, Wb, K, H, tid);
  }
  __syncthreads();

  // register accumulators for the block-shared grads
  float rfmu0 = 0.f, rfsig0 = 0.f, rfmu1 = 0.f, rfsig1 = 0.f;  // k=lane,+64
  float rwmu = 0.f, rwsig = 0.f;                               // i=lane
  float rbmu = 0.f, rbsig = 0.f;

  float* hr = &hS[w * H];
  for (int it = 0; it < iters; ++it) {
    const int row = (bid * iters + it) * DEC_RPW + w;
    if (row < N) {  // wave-uniform
      if (inH) hr[lane] = h[(long)row * H + lane];
      const float eps_r = eps[row], y_r = y[row];
      __builtin_amdgcn_wave_barrier();

      // ---- forward (dec_fwd_kernel)
      float a1v = 0.0f;
      if (inH) {
        a1v = b1_r;
        const float* wr = &W1S[(size_t)lane * SH];
        for (int i = 0; i < H; ++i) a1v = fmaf(hr[i], wr[i], a1v);
        a1v = lrelu_(a1v);
        a1_out[(long)row * H + lane] = a1v;
      }
      float pm = inH ? a1v * wmu_r : 0.0f;
      float ps = inH ? a1v * wsig_r : 0.0f;
      pm = wave_reduce_sum(pm);
      ps = wave_reduce_sum(ps);
      pm = __shfl(pm, 0, 64);
      ps = __shfl(ps, 0, 64);
      const float amu = pm + bmu0;
      const float asig_pre = ps + bsig0;
      const float asig = softplusf_(asig_pre);

      float mu_b = 0.0f, var_b = 0.0f;
      float bv0 = 0.0f, bv1 = 0.0f;
      for (int k = lane; k < K; k += 64) {
        const bool lo = k == lane;
        float bv = lo ? bb_r0 : bb_r1;
        const float* wr = &WbS[(size_t)k * SH];
        for (int i = 0; i < H; ++i) bv = fmaf(hr[i], wr[i], bv);
        beta_out[(long)row * K + k] = bv;
        const float fs = lo ? fs_r0 : fs_r1;
        mu_b = fmaf(bv, lo ? fmu_r0 : fmu_r1, mu_b);
        var_b = fmaf(bv * bv, fs * fs, var_b);
        if (lo) bv0 = bv; else bv1 = bv;
      }
      mu_b = wave_reduce_sum(mu_b);
      var_b = wave_reduce_sum(var_b);

      // lane 0 holds the row's scalars; the backward needs them wave-wide
      const float mu = amu + mu_b;
      const float var = asig * asig + var_b + 1e-6f;
      float sig = sqrtf(var);
      const float rec = fmaf(eps_r, sig, mu);
      const float d = rec - y_r;
      float dmu = dscale * d;
      if (lane == 0) {
        asig_pre_out[row] = asig_pre;
        sigma_out[row] = sig;
        recon[row] = rec;
        drecon_out[row] = dmu;
      }
      sig = __shfl(sig, 0, 64);
      dmu = __shfl(dmu, 0, 64);

      // ---- backward (dec_bwd_kernel)
      const float dsig = dmu * eps_r;
      const float dvar = dsig / (2.0f * sig);
      const float dasig = 2.0f * asig * dvar;
      const float dasig_pre = dasig * softplus_gradf_(asig_pre);

      for (int k = lane; k < K; k += 64) {
        const bool lo = k == lane;
        const float bv = lo ? bv0 : bv1;
        const float fs = lo ? fs_r0 : fs_r1;
        const float fm = lo ? fmu_r0 : fmu_r1;
        const float db = dmu * fm + dvar * 2.0f * bv * fs * fs;
        dbeta_out[(long)row * K + k] = db;
        dbS[w * K + k] = db;
        // dec_bwd_kernel's `r += a * b` accumulations compile to fused
        // multiply-adds (multiply and add share a basic block there). Here
        // the compiler peels the k >= 64 trip and moves its add into
        // another block, where nothing fuses it, so the fusion is spelled
        // out: r = fma(a, b, r), with the last factor of the product chain
        // as b, as the contraction picks it.
        const float t = dvar * bv * bv * 2.0f;
        if (lo) {
          rfmu0 = fmaf(dmu, bv, rfmu0);
          rfsig0 = fmaf(t, fs, rfsig0);
        } else {
          rfmu1 = fmaf(dmu, bv, rfmu1);
          rfsig1 = fmaf(t, fs, rfsig1);
        }
      }
      if (inH) {
        const float da1 = dmu * wmu_r + dasig_pre * wsig_r;
        const float dz = da1 * lrelu_grad_from_out_(a1v);
        dz1[(long)row * H + lane] = dz;
        dz1S[w * H + lane] = dz;
        rwmu = fmaf(dmu, a1v, rwmu);
        rwsig = fmaf(dasig_pre, a1v, rwsig);
      }
      if (lane == 0) {
        rbmu += dmu;
        rbsig += dasig_pre;
      }
      __builtin_amdgcn_wave_barrier();

      if (inH) {
        // dh[i] = sum_j dz1[j]*W1[j][i] + sum_k dbeta[k]*Wb[k][i]
        float acc = 0.0f;
        const float* dz = &dz1S[w * H];
        for (int j = 0; j < H; ++j)
          acc = fmaf(dz[j], W1S[(size_t)j * SH + lane], acc);
        const float* db = &dbS[w * K];
        for (int k = 0; k < K; ++k)
          acc = fmaf(db[k], WbS[(size_t)k * SH + lane], acc);
        dh[(long)row * H + lane] = acc;
      }
    }
  }

  // cross-wave reduce -> per-block partial, as in dec_bwd_kernel
  float* po = part;
#define DP(e) po[(long)(e) * NB + bid]
  __syncthreads();
  red[w * 64 + lane] = rfmu0;
  __syncthreads();
  if (w == 0 && lane < K && lane < 64)
    DP(lane) =
        red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
  __syncthreads();
  red[w * 64 + lane] = rfsig0;
  __syncthreads();
  if (w == 0 && lane < K && lane < 64)
    DP(K + lane) =
        red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
  if (K > 64) {
    __syncthreads();
    red[w * 64 + lane] = kh2 ? rfmu1 : 0.0f;
    __syncthreads();
    if (w == 0 && lane + 64 < K)
      DP(lane + 64) =
          red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
    __syncthreads();
    red[w * 64 + lane] = kh2 ? rfsig1 : 0.0f;
    __syncthreads();
    if (w == 0 && lane + 64 < K)
      DP(K + lane + 64) =
          red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
  }
  __syncthreads();
  red[w * 64 + lane] = rwmu;
  __syncthreads();
  if (w == 0 && lane < H)
    DP(2 * K + lane) =
        red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
  __syncthreads();
  red[w * 64 + lane] = rwsig;
  __syncthreads();
  if (w == 0 && lane < H)
    DP(2 * K + H + lane) =
        red[lane] + red[64 + lane] + red[128 + lane] + red[192 + lane];
  __syncthreads();
  if (lane == 0) {
    red[w] = rbmu;
    red[4 + w] = rbsig;
  }
  __syncthreads();
  if (tid == 0) {
    DP(2 * K + 2 * H) = red[0] + red[1] + red[2] + red[3];
    DP(2 * K + 2 * H + 1) = red[4] + red[5] + red[6] + red[7];
  }
#undef DP
}
