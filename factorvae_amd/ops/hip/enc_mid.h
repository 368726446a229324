// Body of the latency-oriented fused encoder kernel as a __device__
// function of the portfolio index, shared by encoder.hip (whose __global__
// kernel is a thin wrapper around it) and mid_fuse.hip. What the variant is
// and why it is bit-identical to enc_fused_fwd_kernel is described in
// encoder.hip, above the wrapper.
#pragma once

#include "common.h"
#include "stage.h"

// One thread's row of h into registers; r[c] valid for c < H.
DEVINL void row_load(float (&r)[64], const float* __restrict__ src, int H) {
  if ((reinterpret_cast<size_t>(src) & 15) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (4 * q < H) {
        const float4 t = s4[q];
        r[4 * q] = t.x;
        r[4 * q + 1] = t.y;
        r[4 * q + 2] = t.z;
        r[4 * q + 3] = t.w;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (4 * q < H) {
        r[4 * q] = src[4 * q];
        r[4 * q + 1] = src[4 * q + 1];
        r[4 * q + 2] = src[4 * q + 2];
        r[4 * q + 3] = src[4 * q + 3];
      }
    }
  }
}

// Portfolio m of enc_fused_fwd_lat_kernel. The handoff counts the M
// portfolio workgroups, whatever else the launch holds: the one that finds
// done == M - 1 runs the heads tail and resets the counter. No workgroup
// waits for another.
DEVINL void enc_fused_fwd_lat_body(
    const float* __restrict__ h,      // (N,H)
    const float* __restrict__ Wenc,   // (M,H)
    const float* __restrict__ benc,   // (M)
    const float* __restrict__ y,      // (N,1)
    float* __restrict__ scores_out,   // (N,M) saved for backward
    float* __restrict__ a,            // (N,M)
    float* __restrict__ yp,           // (M)
    const float* __restrict__ Wmu, const float* __restrict__ bmu,
    const float* __restrict__ Wsig, const float* __restrict__ bsig,
    float* __restrict__ fmu, float* __restrict__ fsig_pre,
    float* __restrict__ fsig, float* __restrict__ fsig_c,
    int* __restrict__ done, int K,
    int N, int M, int H, int img_floats, const int m) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* wS = (float*)smem;               // [64] Wenc row m
  float* scratch = wS + 64;               // [8]
  float* imgS = scratch + 8;              // heads image (last workgroup)

  const int tid = threadIdx.x;

  MID_STAMP(0);
  // ---- all global loads, up front
  const int n0 = tid, n1 = tid + 256;
  const bool has0 = n0 < N, has1 = n1 < N;
  const int r0 = min(n0, N - 1), r1 = min(n1, N - 1);
  float hr0[64], hr1[64];
  row_load(hr0, h + (size_t)r0 * H, H);
  row_load(hr1, h + (size_t)r1 * H, H);
  const float w_r = Wenc[(long)m * H + min(tid, H - 1)];
  const float bm = benc[m];
  const float y0 = y[r0], y1 = y[r1];
  const int KM = K * M;
  const bool pre = fmu && KM <= 256 * 16;
  float pm[16], ps[16];
  if (pre) {
    tile_load<false, 16>(pm, Wmu, KM, tid);
    tile_load<false, 16>(ps, Wsig, KM, tid);
  }
  if (tid < H) wS[tid] = w_r;
  __syncthreads();
  MID_STAMP(1);

  float sv0 = bm, sv1 = bm;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    if (4 * q < H) {
      const float4 w4 = reinterpret_cast<const float4*>(wS)[q];
      sv0 = fmaf(hr0[4 * q], w4.x, sv0);
      sv1 = fmaf(hr1[4 * q], w4.x, sv1);
      sv0 = fmaf(hr0[4 * q + 1], w4.y, sv0);
      sv1 = fmaf(hr1[4 * q + 1], w4.y, sv1);
      sv0 = fmaf(hr0[4 * q + 2], w4.z, sv0);
      sv1 = fmaf(hr1[4 * q + 2], w4.z, sv1);
      sv0 = fmaf(hr0[4 * q + 3], w4.w, sv0);
      sv1 = fmaf(hr1[4 * q + 3], w4.w, sv1);
    }
  }
  float mx = -INFINITY;
  if (has0) {
    scores_out[(long)n0 * M + m] = sv0;
    mx = fmaxf(mx, sv0);
  }
  if (has1) {
    scores_out[(long)n1 * M + m] = sv1;
    mx = fmaxf(mx, sv1);
  }
  mx = block_reduce_max(mx, scratch);

  float e0 = 0.0f, e1 = 0.0f;
  float sum = 0.0f;
  if (has0) {
    e0 = __expf(sv0 - mx);
    sum += e0;
  }
  if (has1) {
    e1 = __expf(sv1 - mx);
    sum += e1;
  }
  sum = block_reduce_sum(sum, scratch);
  const float inv = 1.0f / sum;

  float wy = 0.0f;
  if (has0) {
    const float an = e0 * inv;
    a[(long)n0 * M + m] = an;
    wy = fmaf(an, y0, wy);
  }
  if (has1) {
    const float an = e1 * inv;
    a[(long)n1 * M + m] = an;
    wy = fmaf(an, y1, wy);
  }
  wy = block_reduce_sum(wy, scratch);
  MID_STAMP(2);
  __shared__ int lastS;
  if (tid == 0) {
    yp[m] = wy;
    if (fmu) {
      const int prev = __hip_atomic_fetch_add(done, 1, __ATOMIC_ACQ_REL,
                                              __HIP_MEMORY_SCOPE_AGENT);
      lastS = (prev == M - 1) ? 1 : 0;
      if (lastS)
        __hip_atomic_store(done, 0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    } else {
      lastS = 0;
    }
  }
  if (!fmu) return;
  __syncthreads();
  if (!lastS) return;

  // ---- heads tail (enc_heads_fwd_kernel's chains, fed from LDS)
  MID_STAMP_LAST(3);
  float* ypS = imgS;                        // [M]
  float* WmS = ypS + M;                     // [K][M+1]
  float* WsS = WmS + (size_t)K * (M + 1);   // [K][M+1]
  const int SM = M + 1;
  const int kc = min(tid, K - 1);
  const float bmu_r = bmu[kc];
  const float bsig_r = bsig[kc];
  if (tid < 64)
    for (int i = tid; i < M; i += 64) ypS[i] = yp[i];
  {
    RowCol rc1 = tile_cursor(false, tid, M);
    RowCol rc2 = rc1;
    if (pre) {
      tile_store_lds<false, 16>(WmS, pm, KM, tid, rc1, SM);
      tile_store_lds<false, 16>(WsS, ps, KM, tid, rc2, SM);
    } else {
      for (int base = 0; base < KM; base += 256 * 16) {
        float v1[16], v2[16];
        tile_load<false, 16>(v1, Wmu + base, KM - base, tid);
        tile_load<false, 16>(v2, Wsig + base, KM - base, tid);
        tile_store_lds<false, 16>(WmS, v1, KM - base, tid, rc1, SM);
        tile_store_lds<false, 16>(WsS, v2, KM - base, tid, rc2, SM);
      }
    }
  }
  __syncthreads();
  if (tid < K) {
    // K <= 256 (the launcher checks); thread k owns head k
    float sm = bmu_r, ss = bsig_r;
    const float* wm = &WmS[(size_t)tid * SM];
    const float* ws = &WsS[(size_t)tid * SM];
#pragma unroll 8
    for (int i = 0; i < M; ++i) {
      const float yi = ypS[i];
      sm = fmaf(yi, wm[i], sm);
      ss = fmaf(yi, ws[i], ss);
    }
    fmu[tid] = sm;
    fsig_pre[tid] = ss;
    const float s = softplusf_(ss);
    fsig[tid] = s;
    fsig_c[tid] = (s == 0.0f) ? 1e-6f : s;
  }
  MID_STAMP_LAST(4);
}
