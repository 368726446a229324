// Bodies of the latency-oriented fused attention kernels as __device__
// functions of the head index, shared by attention.hip (whose __global__
// kernels are thin wrappers around them) and mid_fuse.hip (where a
// workgroup picks one of two bodies from its block index). Every .hip file
// is compiled on its own, without relocatable device code, so what two of
// them run lives here.
//
// What the variants are and why every output is bit-identical to the
// original kernels' is described in attention.hip, above the wrappers.
#pragma once

#include "common.h"
#include "stage.h"

#define MID_NT_H 80   // floats per thread per h staging round (20 x 16 B)

// Head k of attn_fused_fwd_lat_kernel. Dynamic LDS: hS, aS, scratch, part,
// five 64-float vectors and WS, as laid out below.
template <bool QUAD>
DEVINL void attn_fused_fwd_lat_body(
    const float* __restrict__ h, const float* __restrict__ qk,
    const float* __restrict__ cb, const float* __restrict__ mask,
    const float* __restrict__ Wv, const float* __restrict__ bv,
    const float* __restrict__ Wl, const float* __restrict__ bl,
    const float* __restrict__ wmu, const float* __restrict__ bmu,
    const float* __restrict__ wsig, const float* __restrict__ bsig,
    float* __restrict__ a_out, float* __restrict__ sd_out,
    int* __restrict__ guard, float* __restrict__ u_out,
    float* __restrict__ ctx_out, float* __restrict__ hm2_out,
    float* __restrict__ pmu, float* __restrict__ psig_pre,
    float* __restrict__ psig, float* __restrict__ psig_c,
    int N, int K, int H, float alpha, float keep_inv, const int k) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* hS = (float*)smem;              // [N][H+1]
  float* aS = hS + (size_t)N * (H + 1);  // [N]
  float* scratch = aS + N;               // [8] block reduces
  float* part = scratch + 8;             // [4][64]
  float* qkS = part + 256;               // [64]
  float* uS = qkS + 64;                  // [64]
  float* hm2S = uS + 64;                 // [64]
  float* bvS = hm2S + 64;                // [64]
  float* blS = bvS + 64;                 // [64]
  float* WS = blS + 64;                  // [H][H+1]: Wv then Wl
  __shared__ int bad_s;
  __shared__ float ctxS[64];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int SH = H + 1;
  const int HH = H * H;

  MID_STAMP(0);
  // ---- all global loads, up front
  float wv[16], wl[16];
  tile_load<QUAD, 16>(wv, Wv + (long)k * HH, HH, tid);
  tile_load<QUAD, 16>(wl, Wl, HH, tid);
  const int tc = min(tid, H - 1);
  const float qk_r = qk[(long)k * H + tc];
  const float bv_r = bv[(long)k * H + tc];
  const float bl_r = bl[tc];
  const float wmu_r = wmu[tc];
  const float wsig_r = wsig[tc];
  const float ck = cb[k];
  const float bmu0 = bmu[0];
  const float bsig0 = bsig[0];
  const int n0 = tid, n1 = tid + 256;
  const bool has0 = n0 < N, has1 = n1 < N;
  const int r0 = min(n0, N - 1), r1 = min(n1, N - 1);
  float mk0 = 0.0f, mk1 = 0.0f;
  if (mask) {
    mk0 = mask[(long)r0 * K + k];
    mk1 = mask[(long)r1 * K + k];
  }
  stage_rows_lds<QUAD, MID_NT_H>(hS, h, N, H, tid);
  if (tid == 0) bad_s = 0;
  if (tid < H) {
    qkS[tid] = qk_r;
    bvS[tid] = bv_r;
    blS[tid] = bl_r;
  }
  {
    RowCol rc = tile_cursor(QUAD, tid, H);
    tile_store_lds<QUAD, 16>(WS, wv, HH, tid, rc, SH);
  }
  __syncthreads();
  MID_STAMP(1);

  // ---- scores + dropout + NaN scan + max; rows t and t+256 side by side
  float s0 = 0.0f, s1 = 0.0f;
  {
    const float* hr0 = &hS[(size_t)r0 * SH];
    const float* hr1 = &hS[(size_t)r1 * SH];
    for (int c = 0; c < H; ++c) {
      const float qc = qkS[c];
      s0 = fmaf(hr0[c], qc, s0);
      s1 = fmaf(hr1[c], qc, s1);
    }
  }
  int bad = 0;
  float mx = -INFINITY;
  if (has0) {
    float s = s0;
    s = (s + ck) * alpha;
    if (mask) s *= mk0 * keep_inv;
    sd_out[(long)n0 * K + k] = s;
    if (isnan(s) || s == INFINITY) bad = 1;
    mx = fmaxf(mx, (s > 0.0f) ? s : 0.0f);
    s0 = s;
  }
  if (has1) {
    float s = s1;
    s = (s + ck) * alpha;
    if (mask) s *= mk1 * keep_inv;
    sd_out[(long)n1 * K + k] = s;
    if (isnan(s) || s == INFINITY) bad = 1;
    mx = fmaxf(mx, (s > 0.0f) ? s : 0.0f);
    s1 = s;
  }
  if (bad) atomicOr(&bad_s, 1);
  mx = block_reduce_max(mx, scratch);

  float e0 = 0.0f, e1 = 0.0f;
  float sum = 0.0f;
  if (has0) {
    e0 = __expf(((s0 > 0.0f) ? s0 : 0.0f) - mx);
    sum += e0;
  }
  if (has1) {
    e1 = __expf(((s1 > 0.0f) ? s1 : 0.0f) - mx);
    sum += e1;
  }
  sum = block_reduce_sum(sum, scratch);
  const float inv = 1.0f / sum;
  if (has0) {
    const float av = e0 * inv;
    aS[n0] = av;
    a_out[(long)n0 * K + k] = av;
  }
  if (has1) {
    const float av = e1 * inv;
    aS[n1] = av;
    a_out[(long)n1 * K + k] = av;
  }
  __syncthreads();
  const bool g = bad_s != 0;
  MID_STAMP(2);
  if (tid == 0) guard[k] = bad_s;

  // ---- u[c] = sum_n a[n] * h[n][c]  (4 waves split the stock range)
  float acc = 0.0f;
  if (lane < H) {
#pragma unroll 8
    for (int n = w; n < N; n += 4)
      acc = fmaf(aS[n], hS[(size_t)n * SH + lane], acc);
  }
  part[w * 64 + lane] = acc;
  __syncthreads();
  if (w == 0 && lane < H) {
    const float uv = part[lane] + part[64 + lane] + part[128 + lane] +
                     part[192 + lane];
    uS[lane] = uv;
    u_out[(long)k * H + lane] = uv;
  }
  __syncthreads();
  MID_STAMP(3);

  // ---- ctx[j] = Wv[k][j]·u + bv (guarded -> 0); a wave's columns together
  const int jpw = (H + 3) / 4;
  const int lc = min(lane, H - 1);
  {
    const float ul = (lane < H) ? uS[lane] : 0.0f;
    float v[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = min(w * jpw + jj, H - 1);
      v[jj] = (!g && lane < H) ? WS[(size_t)j * SH + lc] * ul : 0.0f;
    }
    wave_reduce_sum_n<16>(v);
    if (lane == 0) {
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = w * jpw + jj;
        if (jj < jpw && j < H) {
          const float cv = g ? 0.0f : v[jj] + bvS[j];
          ctxS[j] = cv;
          ctx_out[(long)k * H + j] = cv;
        }
      }
    }
  }
  __syncthreads();
  MID_STAMP(4);

  // ---- shared MLP: hm2 = lrelu(ctx@Wl^T + bl); Wl (held in registers
  // since the top) goes over Wv's slot
  {
    RowCol rc = tile_cursor(QUAD, tid, H);
    tile_store_lds<QUAD, 16>(WS, wl, HH, tid, rc, SH);
  }
  __syncthreads();
  {
    const float cl = (lane < H) ? ctxS[lane] : 0.0f;
    float v[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = min(w * jpw + jj, H - 1);
      v[jj] = (lane < H) ? WS[(size_t)j * SH + lc] * cl : 0.0f;
    }
    wave_reduce_sum_n<16>(v);
    if (lane == 0) {
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = w * jpw + jj;
        if (jj < jpw && j < H) {
          const float z = lrelu_(v[jj] + blS[j]);
          hm2S[j] = z;
          hm2_out[(long)k * H + j] = z;
        }
      }
    }
  }
  __syncthreads();
  MID_STAMP(5);
  if (w == 0) {
    const float z = (lane < H) ? hm2S[lane] : 0.0f;
    float pm = (lane < H) ? z * wmu_r : 0.0f;
    float ps = (lane < H) ? z * wsig_r : 0.0f;
    pm = wave_reduce_sum(pm);
    ps = wave_reduce_sum(ps);
    if (lane == 0) {
      pmu[k] = pm + bmu0;
      const float pre = ps + bsig0;
      psig_pre[k] = pre;
      const float sp = softplusf_(pre);
      psig[k] = sp;
      psig_c[k] = (sp == 0.0f) ? 1e-6f : sp;
    }
  }
  MID_STAMP(6);
}

// Head k of attn_fused_bwd_lat_kernel.
// KLG (the middle chain, docs/KERNELS.md): head k forms its two KL
// gradients itself with kl_grad_ from (fmu, fsig_c, pmu, psig_c)[k] and
// stores them to dpmu / dpsig_c, instead of reading what loss_fused wrote.
template <bool QUAD, bool KLG>
DEVINL void attn_fused_bwd_lat_body(
    const float* __restrict__ dpmu, const float* __restrict__ dpsig_c,
    const float* __restrict__ psig, const float* __restrict__ psig_pre,
    const float* __restrict__ hm2, const float* __restrict__ wmu,
    const float* __restrict__ wsig, const float* __restrict__ Wl,
    const float* __restrict__ h, const float* __restrict__ a,
    const float* __restrict__ sd, const float* __restrict__ mask,
    const int* __restrict__ guard, const float* __restrict__ u,
    const float* __restrict__ Wv, const float* __restrict__ q,
    const float* __restrict__ Wk, const float* __restrict__ bk,
    float* __restrict__ dz2_out, float* __restrict__ du_out,
    float* __restrict__ ds_out, float* __restrict__ dc_out,
    float* __restrict__ dWv, float* __restrict__ dbv,
    float* __restrict__ dq, float* __restrict__ dWk,
    float* __restrict__ dbk, float* __restrict__ hpart,
    int N, int K, int H, float alpha, float keep_inv,
    const float* __restrict__ kl_fmu, const float* __restrict__ kl_fsig_c,
    const float* __restrict__ kl_pmu, const float* __restrict__ kl_psig_c,
    float kl_gscale, float* __restrict__ dpmu_out,
    float* __restrict__ dpsig_c_out, const int k) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* hS = (float*)smem;               // [N][H+1]
  float* WlS = hS + (size_t)N * (H + 1);  // [H][H+1]: Wl, Wv, then Wk
  float* dsS = WlS + (size_t)H * (H + 1); // [N]
  float* scratch = dsS + N;               // [8]
  float* part = scratch + 8;              // [4][64]
  float* dz2S = part + 256;               // [64]
  float* dcS = dz2S + 64;                 // [64] dctx
  float* duS = dcS + 64;                  // [64]
  float* dqkS = duS + 64;                 // [64]
  float* uS = dqkS + 64;                  // [64]
  float* qS = uS + 64;                    // [64]
  float* bkS = qS + 64;                   // [64]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int SH = H + 1;
  const int HH = H * H;

  MID_STAMP(0);
  // ---- all global loads, up front
  float wl[16], wv[16], wk[16];
  tile_load<QUAD, 16>(wl, Wl, HH, tid);
  tile_load<QUAD, 16>(wv, Wv + (long)k * HH, HH, tid);
  tile_load<QUAD, 16>(wk, Wk + (long)k * HH, HH, tid);
  const bool g = guard[k] != 0;
  const int tc = min(tid, H - 1);
  const float u_r = u[(long)k * H + tc];
  const float h2 = hm2[(long)k * H + tc];
  const float wmu_r = wmu[tc];
  const float wsig_r = wsig[tc];
  const float q_r = q[(long)k * H + tc];
  const float bk_r = bk[(long)k * H + tc];
  float dm, dpsig_ck;
  if (KLG) {
    const KlGrad kg = kl_grad_(kl_fmu[k], kl_fsig_c[k], kl_pmu[k],
                               kl_psig_c[k], kl_gscale);
    dm = kg.dpmu;
    dpsig_ck = kg.dpsig_c;
    if (tid == 0) {
      dpmu_out[k] = dm;
      dpsig_c_out[k] = dpsig_ck;
    }
  } else {
    dm = dpmu[k];
    dpsig_ck = dpsig_c[k];
  }
  const float psig_k = psig[k];
  const float psig_pre_k = psig_pre[k];
  const int n0 = tid, n1 = tid + 256;
  const bool has0 = n0 < N, has1 = n1 < N;
  const int r0 = min(n0, N - 1), r1 = min(n1, N - 1);
  const long i0 = (long)r0 * K + k, i1 = (long)r1 * K + k;
  const float a0 = a[i0], a1 = a[i1];
  const float sd0 = sd[i0], sd1 = sd[i1];
  float mk0 = 0.0f, mk1 = 0.0f;
  if (mask) {
    mk0 = mask[i0];
    mk1 = mask[i1];
  }
  stage_rows_lds<QUAD, MID_NT_H>(hS, h, N, H, tid);
  {
    RowCol rc = tile_cursor(QUAD, tid, H);
    tile_store_lds<QUAD, 16>(WlS, wl, HH, tid, rc, SH);
  }
  if (tid < H) {
    uS[tid] = u_r;
    qS[tid] = q_r;
    bkS[tid] = bk_r;
  }
  MID_STAMP(1);

  // ---- shared-MLP backward (pred_mlp_bwd math)
  const float dsc = (psig_k == 0.0f) ? 0.0f : dpsig_ck;
  const float dsp = dsc * softplus_gradf_(psig_pre_k);
  if (tid < H) {
    const float dh2 = dm * wmu_r + dsp * wsig_r;
    const float dz = dh2 * lrelu_grad_from_out_(h2);
    dz2S[tid] = dz;
    dz2_out[(long)k * H + tid] = dz;
    float* po = hpart + (long)k * (2 * H + 2);
    po[tid] = dm * h2;
    po[H + tid] = dsp * h2;
    if (tid == 0) {
      po[2 * H] = dm;
      po[2 * H + 1] = dsp;
    }
  }
  __syncthreads();

  // ---- dctx[j] = sum_i dz2[i] * Wl[i][j]; a wave's columns together
  const int jpw = (H + 3) / 4;
  const int lc = min(lane, H - 1);
  {
    const float dzl = (lane < H) ? dz2S[lane] : 0.0f;
    float v[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = min(w * jpw + jj, H - 1);
      v[jj] = (lane < H) ? dzl * WlS[(size_t)lc * SH + j] : 0.0f;
    }
    wave_reduce_sum_n<16>(v);
    if (lane == 0) {
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = w * jpw + jj;
        if (jj < jpw && j < H) dcS[j] = g ? 0.0f : v[jj];
      }
    }
  }
  __syncthreads();
  MID_STAMP(2);

  // ---- value-path backward: dWv/dbv (head-owned), du; Wv[k] (in
  // registers since the top) goes over the Wl slot
  {
    RowCol rc = tile_cursor(QUAD, tid, H);
    tile_store_lds<QUAD, 16>(WlS, wv, HH, tid, rc, SH);
  }
  tile_outer_store<QUAD, 16>(dWv + (long)k * HH, dcS, uS, HH, tid, H);
  if (tid < H) dbv[(long)k * H + tid] = dcS[tid];
  __syncthreads();
  {
    float acc = 0.0f;
    if (!g && lane < H) {
#pragma unroll 8
      for (int j = w; j < H; j += 4)
        acc = fmaf(WlS[(size_t)j * SH + lane], dcS[j], acc);
    }
    part[w * 64 + lane] = acc;
  }
  __syncthreads();
  if (w == 0 && lane < H) {
    const float d = part[lane] + part[64 + lane] + part[128 + lane] +
                    part[192 + lane];
    duS[lane] = d;
    du_out[(long)k * H + lane] = d;
  }
  __syncthreads();
  MID_STAMP(3);

  // ---- da[n] = h[n]·du; softmax/relu/dropout bwd -> ds, dc
  if (g) {
    if (has0) {
      ds_out[(long)n0 * K + k] = 0.0f;
      dsS[n0] = 0.0f;
    }
    if (has1) {
      ds_out[(long)n1 * K + k] = 0.0f;
      dsS[n1] = 0.0f;
    }
    if (tid == 0) dc_out[k] = 0.0f;
    __syncthreads();
  } else {
    float da0 = 0.0f, da1 = 0.0f;
    {
      const float* hr0 = &hS[(size_t)r0 * SH];
      const float* hr1 = &hS[(size_t)r1 * SH];
      for (int c = 0; c < H; ++c) {
        const float dc_ = duS[c];
        da0 = fmaf(hr0[c], dc_, da0);
        da1 = fmaf(hr1[c], dc_, da1);
      }
    }
    float t = 0.0f;
    if (has0) t = fmaf(a0, da0, t);
    if (has1) t = fmaf(a1, da1, t);
    t = block_reduce_sum(t, scratch);
    float csum = 0.0f;
    if (has0) {
      float dr = a0 * (da0 - t);
      dr = (sd0 > 0.0f) ? dr : 0.0f;
      if (mask) dr *= mk0 * keep_inv;
      dr *= alpha;
      dsS[n0] = dr;
      ds_out[(long)n0 * K + k] = dr;
      csum += dr;
    }
    if (has1) {
      float dr = a1 * (da1 - t);
      dr = (sd1 > 0.0f) ? dr : 0.0f;
      if (mask) dr *= mk1 * keep_inv;
      dr *= alpha;
      dsS[n1] = dr;
      ds_out[(long)n1 * K + k] = dr;
      csum += dr;
    }
    csum = block_reduce_sum(csum, scratch);
    if (tid == 0) {
      dc_out[k] = csum;
      scratch[0] = csum;
    }
    __syncthreads();
  }
  const float dck = g ? 0.0f : scratch[0];
  MID_STAMP(4);

  // ---- dqk[i] = sum_n ds[n] * h[n][i]
  {
    float acc = 0.0f;
    if (lane < H) {
#pragma unroll 8
      for (int n = w; n < N; n += 4)
        acc = fmaf(dsS[n], hS[(size_t)n * SH + lane], acc);
    }
    __syncthreads();
    part[w * 64 + lane] = acc;
  }
  __syncthreads();
  if (w == 0 && lane < H)
    dqkS[lane] = part[lane] + part[64 + lane] + part[128 + lane] +
                 part[192 + lane];
  // Wk[k] (in registers since the top) over the Wv slot: du's reads of it
  // ended two barriers ago
  {
    RowCol rc = tile_cursor(QUAD, tid, H);
    tile_store_lds<QUAD, 16>(WlS, wk, HH, tid, rc, SH);
  }
  __syncthreads();
  MID_STAMP(5);

  // ---- query/key wgrads (attn_qk_bwd math; head-owned)
  tile_outer_store<QUAD, 16>(dWk + (long)k * HH, qS, dqkS, HH, tid, H);
  if (tid < H) dbk[(long)k * H + tid] = dck * qS[tid];
  {
    const float dl = (lane < H) ? dqkS[lane] : 0.0f;
    float v[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = min(w * jpw + jj, H - 1);
      v[jj] = (lane < H) ? WlS[(size_t)j * SH + lc] * dl : 0.0f;
    }
    wave_reduce_sum_n<16>(v);
    if (lane == 0) {
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = w * jpw + jj;
        if (jj < jpw && j < H) dq[(long)k * H + j] = dck * bkS[j] + v[jj];
      }
    }
  }
  MID_STAMP(6);
}
