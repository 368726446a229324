// Persistent GRU recurrence kernels (forward + BPTT backward).
//
// The reference's nn.GRU (/root/reference/module.py:20,30) maps to cuDNN
// RNN kernels; here the whole T-step recurrence is ONE kernel launch:
// the input projection gi = xp @ W_ih^T + b_ih for ALL timesteps is a
// single gemm_nt beforehand, and this kernel walks the T-sequential
// h-dependence with W_hh staged in LDS (transposed for conflict-free
// lane reads). PyTorch gate order r,z,n preserved:
//   r = sigmoid(gi_r + gh_r); z = sigmoid(gi_z + gh_z)
//   q = gh_n (+ b_hh_n);      n = tanh(gi_n + r*q)
//   h' = (1-z)*n + z*h
//
// Geometry: 256 threads = 4 waves; wave <-> stock, lane <-> hidden unit
// (H <= 64). Grid = ceil(N/4). Stocks are independent, so there is no
// cross-workgroup traffic at any t.
//
// Saved for backward: h_seq (N,T,H), h_prev (N,T,H), gates4 (N,T,4H) =
// [r, z, n, q].

#include "common.h"
#include "gru_gather.h"
#include "launchers.h"

#define GRU_SPW 4  // stocks per workgroup (= waves)

// SAVE=false (inference): the backward state (h_seq, h_prev, gates4) is
// neither written nor touched; the pointers may be null. GATHER
// (gru_gather.h): gi is (U,3H) and step t of stock s reads row idx[s*T + t].
template <bool SAVE, bool GATHER = false>
__global__ __launch_bounds__(256) void gru_fwd_generic_kernel(
    const float* __restrict__ gi,     // (N,T,3H)
    const float* __restrict__ Whh,    // (3H,H)
    const float* __restrict__ bhh,    // (3H)
    float* __restrict__ h_final,      // (N,H)
    float* __restrict__ h_seq,        // (N,T,H)
    float* __restrict__ h_prev_out,   // (N,T,H)
    float* __restrict__ gates4,       // (N,T,4H)
    int N, int T, int H, const int* __restrict__ idx, int U) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* WhhT = (float*)smem;                   // [H][3H] transposed
  float* hprev = WhhT + (size_t)H * 3 * H;      // [GRU_SPW][H]

  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = tid & 63;
  const int s = blockIdx.x * GRU_SPW + w;       // global stock
  const bool live = (s < N) && (lane < H);

  // stage Whh transposed: WhhT[i][j] = Whh[j][i], conflict-free lane reads
  for (int idx = tid; idx < 3 * H * H; idx += 256) {
    const int j = idx / H, i = idx % H;
    WhhT[(size_t)i * 3 * H + j] = Whh[idx];
  }
  if (lane < H) hprev[w * H + lane] = 0.0f;
  __syncthreads();

  const float br = bhh[lane < H ? lane : 0];
  const float bz = bhh[lane < H ? H + lane : 0];
  const float bn = bhh[lane < H ? 2 * H + lane : 0];

  for (int t = 0; t < T; ++t) {
    float hn = 0.0f;
    if (live) {
      // the gather form's row number, loaded ahead of the dot products
      const int ix = GATHER ? idx[(long)s * T + t] : 0;
      float ghr = br, ghz = bz, q = bn;
      const float* hp = &hprev[w * H];
      for (int i = 0; i < H; ++i) {
        const float hv = hp[i];
        const float* wrow = &WhhT[(size_t)i * 3 * H];
        ghr = fmaf(hv, wrow[lane], ghr);
        ghz = fmaf(hv, wrow[H + lane], ghz);
        q = fmaf(hv, wrow[2 * H + lane], q);
      }
      float gir, giz, gin;
      if (GATHER) {
        gather3_(gi, ix, U, H, lane, gir, giz, gin);
      } else {
        const long base = ((long)s * T + t) * 3 * H;
        gir = gi[base + lane];
        giz = gi[base + H + lane];
        gin = gi[base + 2 * H + lane];
      }
      const float r = sigmoidf_(gir + ghr);
      const float z = sigmoidf_(giz + ghz);
      const float n = tanhf_(fmaf(r, q, gin));
      const float hp_l = hprev[w * H + lane];
      hn = fmaf(z, hp_l - n, n);  // (1-z)*n + z*hp

      if (SAVE) {
        const long ob = ((long)s * T + t) * H + lane;
        if (h_seq) h_seq[ob] = hn;
        h_prev_out[ob] = hp_l;
        const long gb = ((long)s * T + t) * 4 * H + lane;
        gates4[gb] = r;
        gates4[gb + H] = z;
        gates4[gb + 2 * H] = n;
        gates4[gb + 3 * H] = q;
      }
      if (t == T - 1) h_final[(long)s * H + lane] = hn;
    }
    // hprev[w][*] is private to wave w: in-wave LDS dependency only,
    // no barrier needed between timesteps.
    if (live) hprev[w * H + lane] = hn;
  }
}

// BPTT backward. Inputs: dh_final (N,H) = dL/dh_T, saved tensors.
// Outputs: dgi (N,T,3H) for the input-projection grads, dgh (N,T,3H) for
// dW_hh = sum dgh^T h_prev (gemm_tn) and db_hh (colsum).
__global__ __launch_bounds__(256) void gru_bwd_generic_kernel(
    const float* __restrict__ dh_final,   // (N,H)
    const float* __restrict__ h_prev_in,  // (N,T,H)
    const float* __restrict__ gates4,     // (N,T,4H)
    const float* __restrict__ Whh,        // (3H,H)
    float* __restrict__ dgi,              // (N,T,3H)
    float* __restrict__ dgh,              // (N,T,3H)
    __bf16* __restrict__ dgi_bf, __bf16* __restrict__ dgh_bf,
    int N, int T, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* WhhS = (float*)smem;                    // [3H][H] as-is
  float* dghS = WhhS + (size_t)3 * H * H;        // [GRU_SPW][3H]
  float* dhS = dghS + (size_t)GRU_SPW * 3 * H;   // [GRU_SPW][H]

  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = tid & 63;
  const int s = blockIdx.x * GRU_SPW + w;
  const bool live = (s < N) && (lane < H);

  for (int idx = tid; idx < 3 * H * H; idx += 256) WhhS[idx] = Whh[idx];
  if (live) dhS[w * H + lane] = dh_final[(long)s * H + lane];
  __syncthreads();

  for (int t = T - 1; t >= 0; --t) {
    float zv = 0.0f;
    if (live) {
      const long gb = ((long)s * T + t) * 4 * H + lane;
      const float r = gates4[gb];
      const float z = gates4[gb + H];
      const float n = gates4[gb + 2 * H];
      const float q = gates4[gb + 3 * H];
      const long hb = ((long)s * T + t) * H + lane;
      const float hp = h_prev_in[hb];
      const float dh = dhS[w * H + lane];

      const float dz = dh * (hp - n);
      const float dn = dh * (1.0f - z);
      const float da = dn * (1.0f - n * n);
      const float dgi_n = da;
      const float dgh_n = da * r;
      const float dr = da * q;
      const float dgate_r = dr * r * (1.0f - r);
      const float dgate_z = dz * z * (1.0f - z);

      const long ob = ((long)s * T + t) * 3 * H + lane;
      dgi[ob] = dgate_r;
      dgi[ob + H] = dgate_z;
      dgi[ob + 2 * H] = dgi_n;
      dgh[ob] = dgate_r;
      dgh[ob + H] = dgate_z;
      dgh[ob + 2 * H] = dgh_n;
      if (dgi_bf) {
        dgi_bf[ob] = (__bf16)dgate_r;
        dgi_bf[ob + H] = (__bf16)dgate_z;
        dgi_bf[ob + 2 * H] = (__bf16)dgi_n;
      }
      if (dgh_bf) {
        dgh_bf[ob] = (__bf16)dgate_r;
        dgh_bf[ob + H] = (__bf16)dgate_z;
        dgh_bf[ob + 2 * H] = (__bf16)dgh_n;
      }

      dghS[w * 3 * H + lane] = dgate_r;
      dghS[w * 3 * H + H + lane] = dgate_z;
      dghS[w * 3 * H + 2 * H + lane] = dgh_n;
      zv = z;
    }
    // dghS/dhS slices are per-wave private: no barriers in the t-loop.
    float acc = 0.0f;
    if (live) {
      // dh_prev = dh*z + sum_j dgh[j] * Whh[j][lane]
      acc = dhS[w * H + lane] * zv;
      const float* dg = &dghS[w * 3 * H];
      for (int j = 0; j < 3 * H; ++j)
        acc = fmaf(dg[j], WhhS[(size_t)j * H + lane], acc);
    }
    if (live) dhS[w * H + lane] = acc;
  }
}


// ---------------------------------------------------------------- fast path
// H % 4 == 0: float4 LDS layout, 8 stocks per 512-thread WG (2 waves/SIMD
// restores most of the LDS b128 issue rate; the generic kernels above are
// the H-agnostic fallback).
//
// W LDS image (fwd): WT4[ib][g][j][c] = Whh[g*H + j][4*ib + c]
//   -> lane j reads ds_read_b128 at ((ib*3+g)*64 + j)*16 bytes: 16-lane
//      groups hit disjoint bank quads (bank = j*4 % 64), conflict-free.
#define GRU_SPW_F 8

template <bool SAVE, bool GATHER = false>
__global__ __launch_bounds__(512) void gru_fwd_fast_kernel(
    const float* __restrict__ gi, const float* __restrict__ Whh,
    const float* __restrict__ bhh, float* __restrict__ h_final,
    float* __restrict__ h_seq, float* __restrict__ h_prev_out,
    float* __restrict__ gates4, int N, int T, int H,
    const int* __restrict__ idx, int U) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* WT4 = (float*)smem;                       // [H/4][3][64][4]
  float* hprev = WT4 + (size_t)3 * 64 * H;         // [GRU_SPW_F][64]

  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = tid & 63;
  const int s = blockIdx.x * GRU_SPW_F + w;
  const bool live = (s < N) && (lane < H);
  const int HB = H >> 2;

  for (int idx = tid; idx < 3 * 64 * H; idx += 512) {
    const int c = idx & 3;
    const int j = (idx >> 2) & 63;
    const int g = (idx >> 8) % 3;
    const int ib = idx / 768;
    WT4[idx] = (j < H) ? Whh[((size_t)g * H + j) * H + 4 * ib + c] : 0.0f;
  }
  if (lane * 4 < H * 4) {
    // zero full 64-wide row so float4 broadcast reads are defined
    hprev[w * 64 + lane] = 0.0f;
  }
  __syncthreads();

  const float br = bhh[lane < H ? lane : 0];
  const float bz = bhh[lane < H ? H + lane : 0];
  const float bn = bhh[lane < H ? 2 * H + lane : 0];

  // prefetch t=0 gate-input rows so global latency hides under the dot
  float gir = 0.f, giz = 0.f, gin = 0.f;
  WaveIdx wi;   // every lane of the wave takes part in at()
  if (GATHER) {
    wi.init(idx + (long)s * T, s < N ? T : 0, lane);
    const int ix = wi.at(0, lane);
    if (live) gather3_(gi, ix, U, H, lane, gir, giz, gin);
  } else if (live) {
    const long b0 = (long)s * T * 3 * H;
    gir = gi[b0 + lane];
    giz = gi[b0 + H + lane];
    gin = gi[b0 + 2 * H + lane];
  }
  for (int t = 0; t < T; ++t) {
    float hn = 0.0f;
    float nir = 0.f, niz = 0.f, nin = 0.f;
    if (GATHER) {
      const int ix = t + 1 < T ? wi.at(t + 1, lane) : -1;
      if (live) gather3_(gi, ix, U, H, lane, nir, niz, nin);
    } else if (live && t + 1 < T) {
      const long bnx = ((long)s * T + t + 1) * 3 * H;
      nir = gi[bnx + lane];
      niz = gi[bnx + H + lane];
      nin = gi[bnx + 2 * H + lane];
    }
    if (live) {
      float ghr = br, ghz = bz, q = bn;
      const float4* hp4 = (const float4*)&hprev[w * 64];
      for (int ib = 0; ib < HB; ++ib) {
        const float4 hv = hp4[ib];
        const float4 wr = *(const float4*)&WT4[(((size_t)ib * 3 + 0) * 64 + lane) * 4];
        const float4 wz = *(const float4*)&WT4[(((size_t)ib * 3 + 1) * 64 + lane) * 4];
        const float4 wn = *(const float4*)&WT4[(((size_t)ib * 3 + 2) * 64 + lane) * 4];
        ghr = fmaf(hv.x, wr.x, fmaf(hv.y, wr.y, fmaf(hv.z, wr.z, fmaf(hv.w, wr.w, ghr))));
        ghz = fmaf(hv.x, wz.x, fmaf(hv.y, wz.y, fmaf(hv.z, wz.z, fmaf(hv.w, wz.w, ghz))));
        q   = fmaf(hv.x, wn.x, fmaf(hv.y, wn.y, fmaf(hv.z, wn.z, fmaf(hv.w, wn.w, q))));
      }
      const float r = sigmoidf_(gir + ghr);
      const float z = sigmoidf_(giz + ghz);
      const float n = tanhf_(fmaf(r, q, gin));
      const float hp_l = hprev[w * 64 + lane];
      hn = fmaf(z, hp_l - n, n);

      if (SAVE) {
        const long ob = ((long)s * T + t) * H + lane;
        if (h_seq) h_seq[ob] = hn;
        h_prev_out[ob] = hp_l;
        const long gb = ((long)s * T + t) * 4 * H + lane;
        gates4[gb] = r;
        gates4[gb + H] = z;
        gates4[gb + 2 * H] = n;
        gates4[gb + 3 * H] = q;
      }
      if (t == T - 1) h_final[(long)s * H + lane] = hn;
    }
    gir = nir; giz = niz; gin = nin;
    // per-wave-private slice: no barrier
    if (s < N && lane < H) hprev[w * 64 + lane] = hn;
  }
}

// bwd W image: WB4[jb][l][c] = Whh[4*jb + c][l]  (j over all 3H gate rows)
__global__ __launch_bounds__(512) void gru_bwd_fast_kernel(
    const float* __restrict__ dh_final, const float* __restrict__ h_prev_in,
    const float* __restrict__ gates4, const float* __restrict__ Whh,
    float* __restrict__ dgi, float* __restrict__ dgh,
    __bf16* __restrict__ dgi_bf, __bf16* __restrict__ dgh_bf,
    int N, int T, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* WB4 = (float*)smem;                        // [3H/4][64][4]
  float* dghS = WB4 + (size_t)3 * H * 64;           // [GRU_SPW_F][3H]
  float* dhS = dghS + (size_t)GRU_SPW_F * 3 * H;    // [GRU_SPW_F][64]

  const int tid = threadIdx.x;
  const int w = tid >> 6;
  const int lane = tid & 63;
  const int s = blockIdx.x * GRU_SPW_F + w;
  const bool live = (s < N) && (lane < H);
  const int JB = (3 * H) >> 2;

  for (int idx = tid; idx < 3 * H * 64; idx += 512) {
    const int c = idx & 3;
    const int l = (idx >> 2) & 63;
    const int jb = idx >> 8;
    WB4[idx] = (l < H) ? Whh[((size_t)4 * jb + c) * H + l] : 0.0f;
  }
  if (live) dhS[w * 64 + lane] = dh_final[(long)s * H + lane];
  __syncthreads();

  // software prefetch of the (t-1) gate rows across the dot product
  float pr = 0.f, pz = 0.f, pn = 0.f, pq = 0.f, php = 0.f;
  if (live) {
    const long gb = ((long)s * T + (T - 1)) * 4 * H + lane;
    pr = gates4[gb];
    pz = gates4[gb + H];
    pn = gates4[gb + 2 * H];
    pq = gates4[gb + 3 * H];
    php = h_prev_in[((long)s * T + (T - 1)) * H + lane];
  }
  for (int t = T - 1; t >= 0; --t) {
    float zv = 0.0f;
    float xr = 0.f, xz = 0.f, xn = 0.f, xq = 0.f, xhp = 0.f;
    if (live && t > 0) {
      const long gb = ((long)s * T + t - 1) * 4 * H + lane;
      xr = gates4[gb];
      xz = gates4[gb + H];
      xn = gates4[gb + 2 * H];
      xq = gates4[gb + 3 * H];
      xhp = h_prev_in[((long)s * T + t - 1) * H + lane];
    }
    if (live) {
      const float r = pr;
      const float z = pz;
      const float n = pn;
      const float q = pq;
      const float hp = php;
      const float dh = dhS[w * 64 + lane];

      const float dz = dh * (hp - n);
      const float dn = dh * (1.0f - z);
      const float da = dn * (1.0f - n * n);
      const float dgh_n = da * r;
      const float dr = da * q;
      const float dgate_r = dr * r * (1.0f - r);
      const float dgate_z = dz * z * (1.0f - z);

      const long ob = ((long)s * T + t) * 3 * H + lane;
      dgi[ob] = dgate_r;
      dgi[ob + H] = dgate_z;
      dgi[ob + 2 * H] = da;
      dgh[ob] = dgate_r;
      dgh[ob + H] = dgate_z;
      dgh[ob + 2 * H] = dgh_n;
      if (dgi_bf) {
        dgi_bf[ob] = (__bf16)dgate_r;
        dgi_bf[ob + H] = (__bf16)dgate_z;
        dgi_bf[ob + 2 * H] = (__bf16)da;
      }
      if (dgh_bf) {
        dgh_bf[ob] = (__bf16)dgate_r;
        dgh_bf[ob + H] = (__bf16)dgate_z;
        dgh_bf[ob + 2 * H] = (__bf16)dgh_n;
      }

      dghS[w * 3 * H + lane] = dgate_r;
      dghS[w * 3 * H + H + lane] = dgate_z;
      dghS[w * 3 * H + 2 * H + lane] = dgh_n;
      zv = z;
    }
    pr = xr; pz = xz; pn = xn; pq = xq; php = xhp;
    float acc = 0.0f;
    if (live) {
      acc = dhS[w * 64 + lane] * zv;
      const float4* dg4 = (const float4*)&dghS[w * 3 * H];
      for (int jb = 0; jb < JB; ++jb) {
        const float4 dg = dg4[jb];
        const float4 wv = *(const float4*)&WB4[((size_t)jb * 64 + lane) * 4];
        acc = fmaf(dg.x, wv.x, fmaf(dg.y, wv.y, fmaf(dg.z, wv.z, fmaf(dg.w, wv.w, acc))));
      }
    }
    if (live) dhS[w * 64 + lane] = acc;
  }
}

extern "C" {

// The wave-per-stock kernels of gru_wave.hip apply at H == 64 up to
// fv_gru_wave_max_n() stocks (bit-identical to the MFMA kernels).
static bool use_wave_(int variant, int N, int H) {
  return variant == 1 && H == 64 && N >= 1 && N <= fv_gru_wave_max_n();
}

// H == 64 goes to the f32 recurrences in gru_wave.hip (variant 1, small N)
// or gru_mfma.hip (exact f32, the same bits); variant 0: always gru_mfma.hip
hipError_t fv_gru_fwd(const float* gi, const float* Whh, const float* bhh,
                      float* h_final, float* h_seq, float* h_prev,
                      float* gates4, int N, int T, int H, int variant,
                      hipStream_t stream) {
  if (H > 64) return hipErrorInvalidValue;
  if (use_wave_(variant, N, H))
    return fv_gru_fwd_wave_f32(gi, Whh, bhh, h_final, h_seq, h_prev, gates4,
                               N, T, H, stream);
  if (H == 64)
    return fv_gru_fwd_mfma_f32(gi, Whh, bhh, h_final, h_seq, h_prev, gates4,
                               N, T, H, stream);
  if ((H & 3) == 0) {
    const size_t lds = ((size_t)3 * 64 * H + GRU_SPW_F * 64) * sizeof(float);
    dim3 grid((N + GRU_SPW_F - 1) / GRU_SPW_F);
    hipLaunchKernelGGL(gru_fwd_fast_kernel<true>, grid, dim3(512), lds, stream,
                       gi, Whh, bhh, h_final, h_seq, h_prev, gates4, N, T, H,
                       nullptr, 0);
  } else {
    const size_t lds = ((size_t)H * 3 * H + GRU_SPW * H) * sizeof(float);
    dim3 grid((N + GRU_SPW - 1) / GRU_SPW);
    hipLaunchKernelGGL(gru_fwd_generic_kernel<true>, grid, dim3(256), lds, stream,
                       gi, Whh, bhh, h_final, h_seq, h_prev, gates4, N, T, H,
                       nullptr, 0);
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}

// Inference forward: same recurrence, same h_final bits, no backward
// state written (the SAVE=false instantiations).
hipError_t fv_gru_fwd_infer(const float* gi, const float* Whh,
                            const float* bhh, float* h_final, int N, int T,
                            int H, int variant, hipStream_t stream) {
  if (H > 64) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  if (use_wave_(variant, N, H))
    return fv_gru_fwd_wave_f32_infer(gi, Whh, bhh, h_final, N, T, H, stream);
  if (H == 64)
    return fv_gru_fwd_mfma_f32_infer(gi, Whh, bhh, h_final, N, T, H, stream);
  if ((H & 3) == 0) {
    const size_t lds = ((size_t)3 * 64 * H + GRU_SPW_F * 64) * sizeof(float);
    dim3 grid((N + GRU_SPW_F - 1) / GRU_SPW_F);
    hipLaunchKernelGGL(gru_fwd_fast_kernel<false>, grid, dim3(512), lds,
                       stream, gi, Whh, bhh, h_final, nullptr, nullptr,
                       nullptr, N, T, H, nullptr, 0);
  } else {
    const size_t lds = ((size_t)H * 3 * H + GRU_SPW * H) * sizeof(float);
    dim3 grid((N + GRU_SPW - 1) / GRU_SPW);
    hipLaunchKernelGGL(gru_fwd_generic_kernel<false>, grid, dim3(256), lds,
                       stream, gi, Whh, bhh, h_final, nullptr, nullptr,
                       nullptr, N, T, H, nullptr, 0);
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}

// fv_gru_fwd_infer with gathered gate inputs (gru_gather.h): the same
// dispatch, and with equal gate inputs the same h_final bits.
hipError_t fv_gru_fwd_infer_gather(const float* gi_rows, int U,
                                   const int* idx, const float* Whh,
                                   const float* bhh, float* h_final, int N,
                                   int T, int H, int variant,
                                   hipStream_t stream) {
  if (H > 64 || U < 0) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  if (use_wave_(variant, N, H))
    return fv_gru_fwd_wave_f32_infer_gather(gi_rows, U, idx, Whh, bhh,
                                            h_final, N, T, H, stream);
  if (H == 64)
    return fv_gru_fwd_mfma_f32_infer_gather(gi_rows, U, idx, Whh, bhh,
                                            h_final, N, T, H, stream);
  if ((H & 3) == 0) {
    const size_t lds = ((size_t)3 * 64 * H + GRU_SPW_F * 64) * sizeof(float);
    dim3 grid((N + GRU_SPW_F - 1) / GRU_SPW_F);
    hipLaunchKernelGGL((gru_fwd_fast_kernel<false, true>), grid, dim3(512),
                       lds, stream, gi_rows, Whh, bhh, h_final, nullptr,
                       nullptr, nullptr, N, T, H, idx, U);
  } else {
    const size_t lds = ((size_t)H * 3 * H + GRU_SPW * H) * sizeof(float);
    dim3 grid((N + GRU_SPW - 1) / GRU_SPW);
    hipLaunchKernelGGL((gru_fwd_generic_kernel<false, true>), grid,
                       dim3(256), lds, stream, gi_rows, Whh, bhh, h_final,
                       nullptr, nullptr, nullptr, N, T, H, idx, U);
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_gru_bwd(const float* dh_final, const float* h_prev,
                      const float* gates4, const float* Whh,
                      float* dgi, float* dgh, void* dgi_bf, void* dgh_bf,
                      int N, int T, int H, int variant, hipStream_t stream) {
  if (H > 64) return hipErrorInvalidValue;
  if (use_wave_(variant, N, H) && !dgi_bf && !dgh_bf)
    return fv_gru_bwd_wave_f32(dh_final, h_prev, gates4, Whh, dgi, dgh,
                               N, T, H, stream);
  if (H == 64 && !dgi_bf && !dgh_bf)
    return fv_gru_bwd_mfma_f32(dh_final, h_prev, gates4, Whh, dgi, dgh,
                               N, T, H, stream);
  if ((H & 3) == 0) {
    const size_t lds = ((size_t)3 * H * 64 + GRU_SPW_F * 3 * H +
                        (size_t)GRU_SPW_F * 64) * sizeof(float);
    dim3 grid((N + GRU_SPW_F - 1) / GRU_SPW_F);
    hipLaunchKernelGGL(gru_bwd_fast_kernel, grid, dim3(512), lds, stream,
                       dh_final, h_prev, gates4, Whh, dgi, dgh,
                       (__bf16*)dgi_bf, (__bf16*)dgh_bf, N, T, H);
  } else {
    const size_t lds =
        ((size_t)3 * H * H + GRU_SPW * 3 * H + GRU_SPW * H) * sizeof(float);
    dim3 grid((N + GRU_SPW - 1) / GRU_SPW);
    hipLaunchKernelGGL(gru_bwd_generic_kernel, grid, dim3(256), lds, stream,
                       dh_final, h_prev, gates4, Whh, dgi, dgh,
                       (__bf16*)dgi_bf, (__bf16*)dgh_bf, N, T, H);
  }
  HIP_CHECK_LAST();
  return hipSuccess;
}

// fv_dh_combine followed by fv_gru_bwd as one launch, on the wave route
// only (what use_wave_ accepts; fp32 outputs). *fused = 0 and nothing is
// launched otherwise: the caller then runs the two launchers.
hipError_t fv_gru_bwd_combine(float* dh, const float* ds, const float* qk,
                              const float* a, const float* du,
                              const float* dscores, const float* Wenc, int K,
                              int M, const float* h_prev, const float* gates4,
                              const float* Whh, float* dgi, float* dgh, int N,
                              int T, int H, int variant, int* fused,
                              hipStream_t stream) {
  *fused = 0;
  if (!use_wave_(variant, N, H)) return hipSuccess;
  hipError_t e = fv_gru_bwd_wave_f32_combine(dh, ds, qk, a, du, dscores, Wenc,
                                             K, M, h_prev, gates4, Whh, dgi,
                                             dgh, N, T, H, stream);
  if (e == hipSuccess) *fused = 1;
  return e;
}

}  // extern "C"
