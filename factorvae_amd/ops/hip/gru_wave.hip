// fp32 GRU recurrence, one wave per stock (H = 64, fp32 engine mode).
//
// The f32 MFMA kernels in gru_mfma.hip put 16 stocks on one workgroup
// because the matrix tile has 16 rows: 19 workgroups at N = 300, each
// serializing 16 stocks per time step behind two workgroup barriers.
// The f32 MFMA runs at the f32 VALU rate and is bitwise a k-ascending
// fmaf chain from +0, so the same bits come out of plain v_fma_f32 with
// any number of stocks per workgroup. Here:
//
//   geometry: 256 threads = 4 waves, wave <-> stock, grid = ceil(N/4).
//   fwd  lane <-> hidden unit j. The lane keeps Whh[j], Whh[64+j],
//        Whh[128+j] (3 x 64 floats) in registers for the whole kernel.
//        Per time step the stock's h row is read back from the wave's own
//        LDS row as 16 broadcast ds_read_b128 and three chains
//        acc = fmaf(h[k], W[.][k], acc), k = 0..63 ascending from +0,
//        feed the gate expressions of gru_fwd_mfma_f32_kernel verbatim.
//   bwd  lane <-> h column i. The lane keeps Whh[0..191][i] in registers.
//        Per time step the three gate gradients go to the wave's
//        192-float LDS row, one chain acc = fmaf(dg[k], Whh[k][i], acc),
//        k = 0..191 ascending from +0, then dh = acc + (dh*z) with the
//        product rounded on its own (the MFMA kernel stores it to LDS
//        before the add).
//
// A wave only ever reads the LDS row it wrote itself, and a wave's LDS
// operations complete in order, so the time loops hold no workgroup
// barrier. Dead waves (stock >= N) leave after the forward's one
// prologue barrier; the backward has none.

#include <stdint.h>

#include "common.h"
#include "gru_gather.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

#define GW_WPB 4    // waves = stocks per workgroup
#define GW_WS 68    // staged Whh row stride: lane j's b128 reads hit
                    // bank quad (4j + 4kb) % 64, conflict-free

// Orders this wave's LDS writes before its following LDS reads (and the
// reverse) for the compiler; the hardware keeps one wave's LDS
// operations in order, so no instruction is emitted.
DEVINL void wave_lds_order_() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Instruction order of a chain section that the compiler would otherwise
// run one or two LDS reads ahead of their use (a read's latency is several
// times the 4 or 12 fmas between two reads): AHEAD ds_read first, then one
// more read behind every PER fmas, then the fmas of the last AHEAD reads. It
// closes its scheduling region, so nothing else drifts into the pattern.
#define GW_READ_AHEAD(READS, AHEAD, PER)                               \
  do {                                                                 \
    __builtin_amdgcn_sched_group_barrier(0x100, (AHEAD), 0);           \
    _Pragma("unroll") for (int i_ = 0; i_ < (READS) - (AHEAD); ++i_) { \
      __builtin_amdgcn_sched_group_barrier(0x002, (PER), 0);           \
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);               \
    }                                                                  \
    __builtin_amdgcn_sched_group_barrier(0x002, (PER) * (AHEAD), 0);   \
    __builtin_amdgcn_sched_barrier(0);                                 \
  } while (0)
#define GW_FA 6   // forward: 6 of 16 b128 reads ahead (24 registers)
#define GW_BA 8   // backward: 8 of 48 b128 reads ahead (32 registers)

// SAVE=false (inference): no h_seq / h_prev / gates4 stores; the pointers
// may be null. GATHER (gru_gather.h): gi is (U,192) and step t of stock s
// reads row idx[s*T + t] of it; without it idx and U are not looked at.
template <bool SAVE, bool GATHER = false>
__global__ __launch_bounds__(256) void gru_fwd_wave_f32_kernel(
    const float* __restrict__ gi,      // (N,T,192)
    const float* __restrict__ Whh,     // (192,64)
    const float* __restrict__ bhh,     // (192)
    float* __restrict__ h_final,       // (N,64)
    float* __restrict__ h_seq,         // (N,T,64) optional
    float* __restrict__ h_prev_out,    // (N,T,64)
    float* __restrict__ gates4,        // (N,T,256)
    int N, int T, const int* __restrict__ idx, int U) {
  __shared__ __attribute__((aligned(16))) float wS[192 * GW_WS];
  __shared__ __attribute__((aligned(16))) float hS[GW_WPB][64];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int s = blockIdx.x * GW_WPB + wv;

  // stage Whh through LDS: coalesced global reads, then each lane picks
  // up its three rows. Whh is a view into the parameter arena, so the
  // 16-byte loads sit behind an alignment test.
  if ((((uintptr_t)Whh) & 15) == 0) {
    f32x4 v[12];   // 192 * 16 float4 over 256 threads, all in flight
#pragma unroll
    for (int i = 0; i < 12; ++i) v[i] = ((const f32x4*)Whh)[tid + 256 * i];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int idx = tid + 256 * i;
      *(f32x4*)&wS[(idx >> 4) * GW_WS + (idx & 15) * 4] = v[i];
    }
  } else {
    float v[48];   // 192 * 64 floats over 256 threads
#pragma unroll
    for (int i = 0; i < 48; ++i) v[i] = Whh[tid + 256 * i];
#pragma unroll
    for (int i = 0; i < 48; ++i) {
      const int idx = tid + 256 * i;
      wS[(idx >> 6) * GW_WS + (idx & 63)] = v[i];
    }
  }
  hS[wv][lane] = 0.0f;
  __syncthreads();
  if (s >= N) return;   // no barrier below this line

  float w[3][64];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
      const f32x4 v = *(const f32x4*)&wS[(g * 64 + lane) * GW_WS + kb * 4];
#pragma unroll
      for (int c = 0; c < 4; ++c) w[g][kb * 4 + c] = v[c];
    }
  const float bh_r = bhh[lane];
  const float bh_z = bhh[64 + lane];
  const float bh_n = bhh[128 + lane];

  const long row = (long)s * T;
  float pgr, pgz, pgn;
  WaveIdx wi;
  if (GATHER) {
    wi.init(idx + row, T, lane);
    gather3_(gi, wi.at(0, lane), U, 64, lane, pgr, pgz, pgn);
  } else {
    const float* g0 = gi + row * 192;
    pgr = g0[lane], pgz = g0[64 + lane], pgn = g0[128 + lane];
  }
  float hp = 0.0f;

  for (int t = 0; t < T; ++t) {
    // next time step's gi, in flight across the chains and the gate math
    // (the last step loads its own row again: no branch in the loop body;
    // the gather form, which branches on a missing row anyway, loads none)
    float xgr, xgz, xgn;
    if (GATHER) {
      gather3_(gi, t + 1 < T ? wi.at(t + 1, lane) : -1, U, 64, lane, xgr,
               xgz, xgn);
    } else {
      const float* gx = gi + (row + (t + 1 < T ? t + 1 : t)) * 192;
      xgr = gx[lane];
      xgz = gx[64 + lane];
      xgn = gx[128 + lane];
    }

    float ar = 0.0f, az = 0.0f, an = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
      const f32x4 hv = *(const f32x4*)&hS[wv][kb * 4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ar = fmaf(hv[c], w[0][kb * 4 + c], ar);
        az = fmaf(hv[c], w[1][kb * 4 + c], az);
        an = fmaf(hv[c], w[2][kb * 4 + c], an);
      }
    }
    // keep GW_FA row reads ahead of the chains instead of one or two
    GW_READ_AHEAD(16, GW_FA, 12);

    const float r = sigmoidf_(pgr + ar + bh_r);
    const float z = sigmoidf_(pgz + az + bh_z);
    const float q = an + bh_n;
    const float n = tanhf_(fmaf(r, q, pgn));
    const float hn = fmaf(z, hp - n, n);

    const long tb = row + t;
    if (SAVE) {
      if (h_seq) h_seq[tb * 64 + lane] = hn;
      h_prev_out[tb * 64 + lane] = hp;
      float* g4 = &gates4[tb * 256];
      g4[lane] = r;
      g4[64 + lane] = z;
      g4[128 + lane] = n;
      g4[192 + lane] = q;
    }
    if (t == T - 1) h_final[(long)s * 64 + lane] = hn;

    wave_lds_order_();   // this step's reads of the row are done
    hS[wv][lane] = hn;
    wave_lds_order_();   // the next step's reads see the new row
    hp = hn;
    pgr = xgr; pgz = xgz; pgn = xgn;
  }
}

// COMBINE (the fused middle, docs/KERNELS.md): dh_combine_kernel as this
// kernel's prologue. That kernel has this one's mapping, wave <-> stock row
// and lane <-> H column, and runs one fmaf chain per element from the
// decoder's dh: over k fmaf(ds[n][k], qk[k][lane], .) then
// fmaf(a[n][k], du[k][lane], .), over m fmaf(dscores[n][m], Wenc[m][lane], .).
// The same explicit fmafs in the same order run here, so dh has the same
// bits. The qk / du / Wenc rows come as coalesced 256-byte rows from L2
// (dh_combine reads an LDS copy of the same values), the row's ds / a /
// dscores through wave-uniform addresses. K and M are runtime bounds, so
// the two loops are unrolled 4 and 8 times and each trip waits for its own
// eight row loads: only the first trip overlaps the 192 Whh loads, the rest
// are K/4 + M/8 load round trips in a row (21 at K = 20, M = 128). With the
// weights holding 192 of the 250 VGPRs there is no room to keep more rows
// in flight. The prologue therefore costs about as much as dh_combine did
// (profiles/mid_fuse.md); what it removes is the launch and its join. The
// combined dh goes back to dh_io, where dh_combine leaves it. Without
// COMBINE the operands after T are not looked at.
template <bool COMBINE = false>
__global__ __launch_bounds__(256) void gru_bwd_wave_f32_kernel(
    const float* __restrict__ dh_final,   // (N,64)
    const float* __restrict__ h_prev_in,  // (N,T,64)
    const float* __restrict__ gates4,     // (N,T,256)
    const float* __restrict__ Whh,        // (192,64)
    float* __restrict__ dgi,              // (N,T,192)
    float* __restrict__ dgh,              // (N,T,192)
    int N, int T,
    float* __restrict__ dh_io,            // (N,64) in: decoder's, out: sum
    const float* __restrict__ ds,         // (N,K)
    const float* __restrict__ qk,         // (K,64)
    const float* __restrict__ a,          // (N,K)
    const float* __restrict__ du,         // (K,64)
    const float* __restrict__ dscores,    // (N,M)
    const float* __restrict__ Wenc,       // (M,64)
    int K, int M) {
  __shared__ __attribute__((aligned(16))) float dgS[GW_WPB][192];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int s = blockIdx.x * GW_WPB + wv;
  if (s >= N) return;   // the kernel has no workgroup barrier

  // column `lane` of Whh: every load is one coalesced 256-byte row
  float w[192];
#pragma unroll
  for (int k = 0; k < 192; ++k) w[k] = Whh[k * 64 + lane];

  const long row = (long)s * T;
  float dh;
  if (COMBINE) {
    // s is the same in every lane of the wave; say so, and the row's
    // operands are read once per wave
    const long su = __builtin_amdgcn_readfirstlane(s);
    const float* dsr = ds + su * K;
    const float* ar = a + su * K;
    const float* dr = dscores + su * M;
    float acc = dh_io[(long)s * 64 + lane];
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      acc = fmaf(dsr[k], qk[k * 64 + lane], acc);
      acc = fmaf(ar[k], du[k * 64 + lane], acc);
    }
#pragma unroll 8
    for (int m = 0; m < M; ++m) acc = fmaf(dr[m], Wenc[m * 64 + lane], acc);
    dh_io[(long)s * 64 + lane] = acc;
    dh = acc;
  } else {
    dh = dh_final[(long)s * 64 + lane];
  }

  float pr = 0.f, pz = 0.f, pn = 0.f, pq = 0.f, php = 0.f;
  if (T > 0) {
    const float* g4 = &gates4[(row + T - 1) * 256];
    pr = g4[lane];
    pz = g4[64 + lane];
    pn = g4[128 + lane];
    pq = g4[192 + lane];
    php = h_prev_in[(row + T - 1) * 64 + lane];
  }

  for (int t = T - 1; t >= 0; --t) {
    const float r = pr, z = pz, n = pn, q = pq, hp = php;
    // time step t-1's saved state, in flight across the chain (step 0
    // loads its own row again: no branch in the loop body)
    {
      const long tp = row + (t > 0 ? t - 1 : 0);
      const float* g4 = &gates4[tp * 256];
      pr = g4[lane];
      pz = g4[64 + lane];
      pn = g4[128 + lane];
      pq = g4[192 + lane];
      php = h_prev_in[tp * 64 + lane];
    }

    const float dz = dh * (hp - n);
    const float dn = dh * (1.0f - z);
    const float da = dn * (1.0f - n * n);
    const float dgh_n = da * r;
    const float dr = da * q;
    const float dgate_r = dr * r * (1.0f - r);
    const float dgate_z = dz * z * (1.0f - z);
    const float zdh = dh * z;

    const long tb = row + t;
    float* di = &dgi[tb * 192];
    float* dg = &dgh[tb * 192];
    di[lane] = dgate_r;
    di[64 + lane] = dgate_z;
    di[128 + lane] = da;
    dg[lane] = dgate_r;
    dg[64 + lane] = dgate_z;
    dg[128 + lane] = dgh_n;

    wave_lds_order_();   // the previous step's reads of the row are done
    dgS[wv][lane] = dgate_r;
    dgS[wv][64 + lane] = dgate_z;
    dgS[wv][128 + lane] = dgh_n;
    wave_lds_order_();
    __builtin_amdgcn_sched_barrier(0);

    float acc = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 48; ++kb) {
      const f32x4 d = *(const f32x4*)&dgS[wv][kb * 4];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc = fmaf(d[c], w[kb * 4 + c], acc);
    }
    GW_READ_AHEAD(48, GW_BA, 4);
    // dh*z is a rounded product of its own; the add must not contract
    dh = add_rn_(acc, zdh);
  }
}

extern "C" {

// Largest N the router sends to the wave kernels (docs/KERNELS.md has the
// measurements behind it). -DGW_MAX_N=... moves it for a measuring build.
#ifndef GW_MAX_N
#define GW_MAX_N 2048
#endif
int fv_gru_wave_max_n(void) { return GW_MAX_N; }

hipError_t fv_gru_fwd_wave_f32(const float* gi, const float* Whh,
                               const float* bhh, float* h_final,
                               float* h_seq, float* h_prev, float* gates4,
                               int N, int T, int H, hipStream_t stream) {
  if (H != 64) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  dim3 grid((N + GW_WPB - 1) / GW_WPB);
  hipLaunchKernelGGL(gru_fwd_wave_f32_kernel<true>, grid, dim3(256), 0,
                     stream, gi, Whh, bhh, h_final, h_seq, h_prev, gates4, N,
                     T, nullptr, 0);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_gru_fwd_wave_f32_infer(const float* gi, const float* Whh,
                                     const float* bhh, float* h_final, int N,
                                     int T, int H, hipStream_t stream) {
  if (H != 64) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  dim3 grid((N + GW_WPB - 1) / GW_WPB);
  hipLaunchKernelGGL(gru_fwd_wave_f32_kernel<false>, grid, dim3(256), 0,
                     stream, gi, Whh, bhh, h_final, nullptr, nullptr, nullptr,
                     N, T, nullptr, 0);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_gru_fwd_wave_f32_infer_gather(const float* gi_rows, int U,
                                            const int* idx, const float* Whh,
                                            const float* bhh, float* h_final,
                                            int N, int T, int H,
                                            hipStream_t stream) {
  if (H != 64 || U < 0) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  dim3 grid((N + GW_WPB - 1) / GW_WPB);
  hipLaunchKernelGGL((gru_fwd_wave_f32_kernel<false, true>), grid, dim3(256),
                     0, stream, gi_rows, Whh, bhh, h_final, nullptr, nullptr,
                     nullptr, N, T, idx, U);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_gru_bwd_wave_f32(const float* dh_final, const float* h_prev,
                               const float* gates4, const float* Whh,
                               float* dgi, float* dgh, int N, int T, int H,
                               hipStream_t stream) {
  if (H != 64) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  dim3 grid((N + GW_WPB - 1) / GW_WPB);
  hipLaunchKernelGGL(gru_bwd_wave_f32_kernel<false>, grid, dim3(256), 0,
                     stream, dh_final, h_prev, gates4, Whh, dgi, dgh, N, T,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, 0, 0);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_gru_bwd_wave_f32_combine(float* dh, const float* ds,
                                       const float* qk, const float* a,
                                       const float* du, const float* dscores,
                                       const float* Wenc, int K, int M,
                                       const float* h_prev,
                                       const float* gates4, const float* Whh,
                                       float* dgi, float* dgh, int N, int T,
                                       int H, hipStream_t stream) {
  if (H != 64 || K < 0 || M < 0) return hipErrorInvalidValue;
  if (N <= 0) return hipSuccess;
  dim3 grid((N + GW_WPB - 1) / GW_WPB);
  hipLaunchKernelGGL(gru_bwd_wave_f32_kernel<true>, grid, dim3(256), 0,
                     stream, nullptr, h_prev, gates4, Whh, dgi, dgh, N, T, dh,
                     ds, qk, a, du, dscores, Wenc, K, M);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
