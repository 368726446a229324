// Generic fp32 GEMM kernels for the FactorVAE engine (gfx950).
//
// The model's GEMMs are small (inner dim 20..256, rows up to ~200k), so
// these are LDS-tiled VALU-f32 kernels tuned for launch-count and
// correctness first; the fused hot ops (GRU recurrence, stock-axis
// softmax chains, decoder rows) live in their own kernels.
//
//   gemm_nt:  out(R,Co)  = act(alpha * (A(R,Ci) @ W(Co,Ci)^T + bias))   [+=]
//   gemm_nn:  out(R,Co)  = act(alpha * (A(R,Ci) @ B(Ci,Co) + bias))    [+=]
//   gemm_tn:  out(M,N)  (+)= A(R,M)^T @ B(R,N)    (weight grads; R-chunked
//             slices write partials, reduced in fixed order: deterministic)
//   gemm_tn_pair: two gemm_tn problems over a common R, M in one launch
//   gemm_tn_xhat + ln_w1x_finish: W1x/b1x/LayerNorm gradients from
//             dzx^T @ xhat slices (no dxln; docs/KERNELS.md)
//   colsum:   out(C)    (+)= sum_r A(R,C)         (bias grads)
// gemm_nn and the gemm_tn family each have a second, pipelined kernel
// (variant 1 of the launchers, bit-identical; docs/KERNELS.md, "The fp32
// GEMM mainloops"); gemm_nn_ln is the pipelined gemm_nn with ln_bwd_params'
// loop as its epilogue, tn_reduce_list one reduce for several gemm_tn calls.

#include <type_traits>

#include "common.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

#define BR 64
#define BC 64
#define BK 32

// act: 0 = none, 1 = leaky_relu(0.01)
// flags bit0: accumulate into out; bit1: apply act; bit2: bias present;
// bit3 (gemm_nn only): multiply by lrelu'(Y) recovered from the
// post-activation Y(R,Co) — the fused form of gemm_nn -> lrelu_bwd
// Register double buffer: the next k-tile's global loads issue while
// the current tile's MFMAs run (f32 MFMA is only 1/16 of bf16 peak, but
// without the prefetch these mid-size GEMMs were global-latency-bound
// at ~12 TF/s).
__global__ __launch_bounds__(256) void gemm_nt_kernel(
    const float* __restrict__ A, const float* __restrict__ W,
    const float* __restrict__ bias, float* __restrict__ out,
    int R, int Ci, int Co, float alpha, int flags) {
  __shared__ float As[2][BR][BK + 1];
  __shared__ float Ws[2][BC][BK + 1];

  const int r0 = blockIdx.y * BR;  // y-major rows: A stays L2-resident
  const int c0 = blockIdx.x * BC;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;        // wave -> 16-row strip
  const int fi = lane & 15;       // fragment row/col index
  const int fk = lane >> 4;       // fragment k index (0..3)

  // staging: thread -> (row = tid/32 + 8u, k-pair kp = (tid%32))
  const int s_row0 = tid >> 5;     // + 8*u
  const int s_k = tid & 31;        // BK = 32 columns

  f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

  const int ktiles = (Ci + BK - 1) / BK;
  float pa[8], pw[8];
  auto stage_regs = [&](int k0) {
    const bool interior = (r0 + BR <= R) && (c0 + BC <= Co) &&
                          (k0 + BK <= Ci);
    if (interior) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = s_row0 + 8 * u;
        pa[u] = A[(long)(r0 + row) * Ci + k0 + s_k];
        pw[u] = W[(long)(c0 + row) * Ci + k0 + s_k];
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = s_row0 + 8 * u;
        const int gk = k0 + s_k;
        pa[u] = (r0 + row < R && gk < Ci)
                    ? A[(long)(r0 + row) * Ci + gk] : 0.0f;
        pw[u] = (c0 + row < Co && gk < Ci)
                    ? W[(long)(c0 + row) * Ci + gk] : 0.0f;
      }
    }
  };
  auto regs_to_lds = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = s_row0 + 8 * u;
      As[buf][row][s_k] = pa[u];
      Ws[buf][row][s_k] = pw[u];
    }
  };

  stage_regs(0);
  regs_to_lds(0);

  for (int kt = 0; kt < ktiles; ++kt) {
    __syncthreads();
    if (kt + 1 < ktiles) stage_regs((kt + 1) * BK);
    const int buf = kt & 1;
#pragma unroll
    for (int k4 = 0; k4 < BK; k4 += 4) {
      const float a = As[buf][wv * 16 + fi][k4 + fk];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const float b = Ws[buf][jt * 16 + fi][k4 + fk];
        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[jt], 0, 0, 0);
      }
    }
    if (kt + 1 < ktiles) {
      __syncthreads();
      regs_to_lds(1 - buf);
    }
  }

#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const int gc = c0 + jt * 16 + fi;
    if (gc >= Co) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int gr = r0 + wv * 16 + (lane >> 4) * 4 + rr;
      if (gr >= R) continue;
      float v = acc[jt][rr];
      if (flags & 4) v += bias[gc];
      v *= alpha;
      if (flags & 2) v = lrelu_(v);
      float* o = &out[(long)gr * Co + gc];
      if (flags & 1) v += *o;
      *o = v;
    }
  }
}

__global__ __launch_bounds__(256) void gemm_nn_kernel(
    const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ bias, const float* __restrict__ Y,
    float* __restrict__ out, int R, int Ci, int Co, float alpha, int flags) {
  __shared__ float As[2][BR][BK + 1];
  __shared__ float Bs[2][BK][BC + 1];

  const int r0 = blockIdx.y * BR;  // y-major rows: A stays L2-resident
  const int c0 = blockIdx.x * BC;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int fi = lane & 15;
  const int fk = lane >> 4;

  const int s_row0 = tid >> 5;     // A: + 8*u ; B: k-row = tid>>6 + 4*u
  const int s_k = tid & 31;
  const int b_k0 = tid >> 6;       // B staging: k-row + 4*u
  const int b_c = tid & 63;        // B column

  f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

  const int ktiles = (Ci + BK - 1) / BK;
  float pa[8], pb[8];
  auto stage_regs = [&](int k0) {
    const bool interior = (r0 + BR <= R) && (c0 + BC <= Co) &&
                          (k0 + BK <= Ci);
    if (interior) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        pa[u] = A[(long)(r0 + s_row0 + 8 * u) * Ci + k0 + s_k];
        pb[u] = B[(long)(k0 + b_k0 + 4 * u) * Co + c0 + b_c];
      }
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int row = s_row0 + 8 * u;
        const int gk = k0 + s_k;
        pa[u] = (r0 + row < R && gk < Ci)
                    ? A[(long)(r0 + row) * Ci + gk] : 0.0f;
        const int bk = k0 + b_k0 + 4 * u;
        pb[u] = (bk < Ci && c0 + b_c < Co)
                    ? B[(long)bk * Co + c0 + b_c] : 0.0f;
      }
    }
  };
  auto regs_to_lds = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      As[buf][s_row0 + 8 * u][s_k] = pa[u];
      Bs[buf][b_k0 + 4 * u][b_c] = pb[u];
    }
  };

  stage_regs(0);
  regs_to_lds(0);

  for (int kt = 0; kt < ktiles; ++kt) {
    __syncthreads();
    if (kt + 1 < ktiles) stage_regs((kt + 1) * BK);
    const int buf = kt & 1;
#pragma unroll
    for (int k4 = 0; k4 < BK; k4 += 4) {
      const float a = As[buf][wv * 16 + fi][k4 + fk];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const float b = Bs[buf][k4 + fk][jt * 16 + fi];
        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[jt], 0, 0, 0);
      }
    }
    if (kt + 1 < ktiles) {
      __syncthreads();
      regs_to_lds(1 - buf);
    }
  }

#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const int gc = c0 + jt * 16 + fi;
    if (gc >= Co) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int gr = r0 + wv * 16 + (lane >> 4) * 4 + rr;
      if (gr >= R) continue;
      float v = acc[jt][rr];
      if (flags & 4) v += bias[gc];
      v *= alpha;
      if (flags & 2) v = lrelu_(v);
      if (flags & 8) v *= lrelu_grad_from_out_(Y[(long)gr * Co + gc]);
      float* o = &out[(long)gr * Co + gc];
      if (flags & 1) v += *o;
      *o = v;
    }
  }
}

// gemm_nn with the waits taken out of its loops (variant >= 1 of
// fv_gemm_nn; docs/KERNELS.md, profiles/f32_gemm.md). Same tiles, same
// LDS image, same MFMA order per accumulator as gemm_nn_kernel, so every
// output is bit-identical; what changes is when things are waited for:
//  - global loads are branch-free (addresses clamped into range, padding
//    zeros selected at the LDS store) and run D k-tiles ahead through a ring
//    of D register sets, so the wait before an LDS store is a counted one
//    for the oldest set only;
//  - the fragments of k-groups 2p+2, 2p+3 are read from LDS before the
//    MFMAs of groups 2p, 2p+1 issue (eh_mma_ktile's scheme);
//  - everything the epilogue reads from memory is loaded before the last
//    k-tile's MFMAs, so the epilogue only computes and stores.
// LN: the 64x64 result tile goes to LDS instead of `out` and the workgroup
// runs ln_bwd_params_kernel's loop on it (64 rows per block: the launcher
// checks the geometry), writing that kernel's partials; dxln is never
// stored. Needs R, Ci, Co >= 1 (the clamps).
template <int D, bool LN>
__global__ __launch_bounds__(256) void gemm_nn_pipe_kernel(
    const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ bias, const float* __restrict__ Y,
    float* __restrict__ out, const float* __restrict__ lx,
    const float* __restrict__ lmean, const float* __restrict__ lrstd,
    float* __restrict__ lpart, int R, int Ci, int Co, float alpha,
    int flags) {
  // row strides 34 and 80: a 32-lane read group (16 fi x 2 fk) then touches
  // 32 different banks (2 fi + fk, 16 fk + fi); with 33 and 65 every read
  // was a 2-way conflict
  __shared__ float As[2][BR][BK + 2];
  __shared__ float Bs[2][BK][BC + 16];

  const int r0 = blockIdx.y * BR;
  const int c0 = blockIdx.x * BC;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int fi = lane & 15;
  const int fk = lane >> 4;

  const int s_row0 = tid >> 5;
  const int s_k = tid & 31;
  const int b_k0 = tid >> 6;
  const int b_c = tid & 63;

  f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

  const int ktiles = (Ci + BK - 1) / BK;
  const int last = ktiles - 1;
  float pa[D][8], pb[D][8];
  // tile t may lie past the last one: its loads are clamped duplicates
  // that are never stored
  auto stage_regs = [&](float (&qa)[8], float (&qb)[8], int t) {
    const int k0 = t * BK;
    const int gk = min(k0 + s_k, Ci - 1);
    const int bc = min(c0 + b_c, Co - 1);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int row = min(r0 + s_row0 + 8 * u, R - 1);
      qa[u] = A[(long)row * Ci + gk];
      const int bk = min(k0 + b_k0 + 4 * u, Ci - 1);
      qb[u] = B[(long)bk * Co + bc];
    }
  };
  auto regs_to_lds = [&](const float (&qa)[8], const float (&qb)[8], int t,
                         int buf) {
    const int k0 = t * BK;
    const bool ka = k0 + s_k < Ci;
    const bool cb = c0 + b_c < Co;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool oa = ka && (r0 + s_row0 + 8 * u < R);
      const bool ob = cb && (k0 + b_k0 + 4 * u < Ci);
      As[buf][s_row0 + 8 * u][s_k] = oa ? qa[u] : 0.0f;
      Bs[buf][b_k0 + 4 * u][b_c] = ob ? qb[u] : 0.0f;
    }
  };
  auto mma_tile = [&](int buf) {
    float a[2][2], b[2][4][2];
    auto frag = [&](int set, int kk) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        a[set][h] = As[buf][wv * 16 + fi][kk + 4 * h + fk];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
          b[set][jt][h] = Bs[buf][kk + 4 * h + fk][jt * 16 + fi];
      }
    };
    frag(0, 0);
#pragma unroll
    for (int p = 0; p < BK / 8; ++p) {
      if (p + 1 < BK / 8) frag((p + 1) & 1, (p + 1) * 8);
      __builtin_amdgcn_sched_barrier(0);  // keep the reads above the MFMAs
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
          acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a[p & 1][h], b[p & 1][jt][h], acc[jt], 0, 0, 0);
      }
    }
  };

  // the sets are loaded in ring order, oldest first (the scheduler would
  // mix them, and the loop's counted waits rely on the order)
  stage_regs(pa[0], pb[0], 0);
  __builtin_amdgcn_sched_barrier(0);
  regs_to_lds(pa[0], pb[0], 0, 0);
#pragma unroll
  for (int d = 1; d < D; ++d) {
    stage_regs(pa[d], pb[d], d);
    __builtin_amdgcn_sched_barrier(0);
  }

  // step kt < last: set kt % D is free (tile kt is in LDS) and takes tile
  // kt + D; set (kt + 1) % D holds tile kt + 1, the oldest in flight.
  // Whole groups of D steps run in a loop without a branch in its body: a
  // path that skipped a step's loads would, where it joins, turn the
  // counted waits of the later steps into nearly full ones.
  int kt = 0;
  for (; kt + D <= last; kt += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      __syncthreads();
      stage_regs(pa[d], pb[d], kt + d + D);
      mma_tile((kt + d) & 1);
      __syncthreads();
      regs_to_lds(pa[(d + 1) % D], pb[(d + 1) % D], kt + d + 1,
                  1 - ((kt + d) & 1));
    }
  }
  // the last - kt < D steps left load nothing: their tiles are in flight
  // in sets 1, 2, ... (nested, so that no step is entered from two sides)
  auto rest = [&](auto self, auto rc) {
    constexpr int r = decltype(rc)::value;
    if constexpr (r < D - 1) {
      if (kt + r < last) {
        __syncthreads();
        mma_tile((kt + r) & 1);
        __syncthreads();
        regs_to_lds(pa[r + 1], pb[r + 1], kt + r + 1, 1 - ((kt + r) & 1));
        self(self, std::integral_constant<int, r + 1>{});
      }
    }
  };
  rest(rest, std::integral_constant<int, 0>{});

  // the last k-tile, with the epilogue's operands loaded under its MFMAs
  __syncthreads();
  float ey[16], eo[16], eb[4], ex[16], emu[16], ers[16];
  if (LN) {
    const int c = min(c0 + lane, Co - 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = min(r0 + wv + 4 * i, R - 1);
      ex[i] = lx[(long)r * Co + c];
      emu[i] = lmean[r];
      ers[i] = lrstd[r];
    }
  } else {
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const int gc = min(c0 + jt * 16 + fi, Co - 1);
      eb[jt] = 0.0f;
      if (flags & 4) eb[jt] = bias[gc];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int gr = min(r0 + wv * 16 + fk * 4 + rr, R - 1);
        ey[jt * 4 + rr] = 0.0f;
        eo[jt * 4 + rr] = 0.0f;
        if (flags & 8) ey[jt * 4 + rr] = Y[(long)gr * Co + gc];
        if (flags & 1) eo[jt * 4 + rr] = out[(long)gr * Co + gc];
      }
    }
  }
  mma_tile(last & 1);

  if (LN) {
    // 64 x 65 floats fit in As (2 x 64 x 34)
    float(*Ts)[BC + 1] = reinterpret_cast<float(*)[BC + 1]>(&As[0][0][0]);
    float(*pg)[64] = reinterpret_cast<float(*)[64]>(&Bs[0][0][0]);
    float(*pbs)[64] = pg + 4;
    __syncthreads();  // every wave is done with the last tile's fragments
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float v = acc[jt][rr];
        v *= alpha;
        Ts[wv * 16 + fk * 4 + rr][jt * 16 + fi] = v;
      }
    }
    __syncthreads();
    // ln_bwd_params_kernel's loop: wave wv walks rows wv, wv+4, ... of the
    // block's 64, lane = column
    float dg = 0.0f, db = 0.0f;
    if (c0 + lane < Co) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (r0 + wv + 4 * i < R) {
          const float g = Ts[wv + 4 * i][lane];
          const float xh = (ex[i] - emu[i]) * ers[i];
          dg = fmaf(g, xh, dg);
          db += g;
        }
      }
    }
    pg[wv][lane] = dg;
    pbs[wv][lane] = db;
    __syncthreads();
    if (wv == 0 && c0 + lane < Co) {
      const int c = c0 + lane;
      lpart[(long)c * gridDim.y + blockIdx.y] =
          pg[0][lane] + pg[1][lane] + pg[2][lane] + pg[3][lane];
      lpart[((long)Co + c) * gridDim.y + blockIdx.y] =
          pbs[0][lane] + pbs[1][lane] + pbs[2][lane] + pbs[3][lane];
    }
    return;
  }

#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const int gc = c0 + jt * 16 + fi;
    if (gc >= Co) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int gr = r0 + wv * 16 + fk * 4 + rr;
      if (gr >= R) continue;
      float v = acc[jt][rr];
      if (flags & 4) v += eb[jt];
      v *= alpha;
      if (flags & 2) v = lrelu_(v);
      if (flags & 8) v *= lrelu_grad_from_out_(ey[jt * 4 + rr]);
      if (flags & 1) v += eo[jt * 4 + rr];
      out[(long)gr * Co + gc] = v;
    }
  }
}

// out(M,N) (+)= A(R,M)^T @ B(R,N); R-chunked over gridDim.z.
// gridDim.z == 1: plain write to out. gridDim.z > 1: each z-slice writes
// its partial tile to part[z][M][N] (plain stores); tn_reduce_kernel then
// sums slices in FIXED order into out — deterministic, no atomics.
// Fused bias-grad epilogue: when db != null, blocks with blockIdx.y == 0
// also emit db(M) (+)= sum_r A(R,M) — the bias gradient of the same
// layer — from the A tiles they already stage (kills the separate
// colsum pass; partials go to db_part[z][M] when chunked).
#define TM 32
#define TN_ 32
#define TKR 32
//
// The body is shared by three entry points: gemm_tn_kernel (tile = block
// x/y), gemm_tn_pair_kernel (two problems with a common R and M, tile
// index flattened over both) and gemm_tn_xhat_kernel (XHAT: the B
// operand is staged as LayerNorm's xhat = (x - mean[r]) * rstd[r],
// ln_fwd's expression, computed while loading x; always per-slice
// partials). (bx, by, bz) is the tile/slice, nz the slice count.
template <bool XHAT>
__device__ __forceinline__ void gemm_tn_body(
    const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ out, float* __restrict__ part,
    float* __restrict__ db, float* __restrict__ db_part,
    int R, int M, int N, int accumulate, int bx, int by, int bz, int nz) {
  __shared__ float As[2][TKR][TM + 1];
  __shared__ float Bs[2][TKR][TN_ + 1];

  const int m0 = bx * TM;
  const int n0 = by * TN_;
  const int chunk = (R + nz - 1) / nz;
  const int rbeg = bz * chunk;
  const int rend = min(rbeg + chunk, R);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;        // wave -> one 16x16 out tile (2x2 grid)
  const int fi = lane & 15;
  const int fk = lane >> 4;
  const int mt = (wv & 1) * 16;   // m-tile offset
  const int nt = (wv >> 1) * 16;  // n-tile offset

  const bool do_bias = (db != nullptr || (XHAT && db_part != nullptr)) &&
                       (by == 0);
  float bsum = 0.0f;

  f32x4 acc = {0, 0, 0, 0};

  // register double buffer (4 floats per operand per thread):
  // thread -> (k-row kr = tid/32 + 8u, col = tid%32)
  const int s_kr0 = tid >> 5;
  const int s_c = tid & 31;
  const int ktiles = (rend - rbeg + TKR - 1) / TKR;
  float pa[4], pb[4], pmu[4], prs[4];
  auto stage_regs = [&](int r0_) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int gr = r0_ + s_kr0 + 8 * u;
      pa[u] = (gr < rend && m0 + s_c < M) ? A[(long)gr * M + m0 + s_c] : 0.0f;
      pb[u] = (gr < rend && n0 + s_c < N) ? B[(long)gr * N + n0 + s_c]
                                          : 0.0f;
      if (XHAT) {
        // raw x, mean, rstd stay in registers; xhat is formed at the LDS
        // store so the loads keep flying under the MFMAs (rstd = 0 makes
        // out-of-range rows/columns contribute exactly 0)
        const bool ok = gr < rend && n0 + s_c < N;
        pmu[u] = ok ? mean[gr] : 0.0f;
        prs[u] = ok ? rstd[gr] : 0.0f;
      }
    }
  };
  auto regs_to_lds = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      As[buf][s_kr0 + 8 * u][s_c] = pa[u];
      Bs[buf][s_kr0 + 8 * u][s_c] =
          XHAT ? (pb[u] - pmu[u]) * prs[u] : pb[u];
    }
  };
  auto bias_from_regs = [&]() {
#pragma unroll
    for (int u = 0; u < 4; ++u) bsum += pa[u];
  };

  if (ktiles > 0) {
    stage_regs(rbeg);
    if (do_bias) bias_from_regs();
    regs_to_lds(0);
  }
  for (int kt = 0; kt < ktiles; ++kt) {
    __syncthreads();
    if (kt + 1 < ktiles) {
      stage_regs(rbeg + (kt + 1) * TKR);
      if (do_bias) bias_from_regs();
    }
    const int buf = kt & 1;
    // out[m][n] = sum_r A[r][m]*B[r][n]: MFMA with k = r
#pragma unroll
    for (int r4 = 0; r4 < TKR; r4 += 4) {
      const float a = As[buf][r4 + fk][mt + fi];
      const float b = Bs[buf][r4 + fk][nt + fi];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    if (kt + 1 < ktiles) {
      __syncthreads();
      regs_to_lds(1 - buf);
    }
  }

  const bool direct = !XHAT && (nz == 1);
  if (do_bias) {
    // LDS-reduce the 8 row-group partials per column (reuse As storage)
    __syncthreads();
    As[0][s_kr0][s_c] = bsum;
    __syncthreads();
    if (tid < TM) {
      float s = 0.0f;
#pragma unroll
      for (int gq = 0; gq < 8; ++gq) s += As[0][gq][tid];
      const int gm = m0 + tid;
      if (gm < M) {
        if (direct) {
          if (accumulate) db[gm] += s; else db[gm] = s;
        } else {
          db_part[(long)bz * M + gm] = s;
        }
      }
    }
  }

  const int gn = n0 + nt + fi;
  if (gn >= N) return;
  float* dst;
  float* po = direct ? out : part + (long)bz * M * N;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int gm = m0 + mt + (lane >> 4) * 4 + rr;
    if (gm >= M) continue;
    dst = &po[(long)gm * N + gn];
    if (direct && accumulate)
      *dst += acc[rr];
    else
      *dst = acc[rr];
  }
}

// gemm_tn_body with its prefetch left in flight (variant >= 1 of the three
// launchers; docs/KERNELS.md, profiles/f32_gemm.md). Same slices, same
// tiles, same LDS image and the same ascending MFMA chain per accumulator,
// so out, part, db and db_part are bit-identical. The differences:
//  - global loads are branch-free (clamped addresses; the zeros of rows
//    past the slice and columns past M/N are selected at the LDS store) and
//    run D 32-row tiles ahead through a ring of D register sets;
//  - bsum is formed where the staged registers are consumed, at the LDS
//    store after the tile's MFMAs (same pa[u] values, same u and tile
//    order), so nothing waits for the loads above the MFMAs;
//  - the tile's eight fragment pairs are read from LDS ahead of the MFMA
//    chain, which then runs on counted waits.
template <bool XHAT, int D>
__device__ __forceinline__ void gemm_tn_pipe_body(
    const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ out, float* __restrict__ part,
    float* __restrict__ db, float* __restrict__ db_part,
    int R, int M, int N, int accumulate, int bx, int by, int bz, int nz) {
  // row stride 48: a 32-lane read group (16 fi x 2 fk) touches 32 different
  // banks (16 fk + fi); with 33 every read was a 2-way conflict
  __shared__ float As[2][TKR][TM + 16];
  __shared__ float Bs[2][TKR][TN_ + 16];

  const int m0 = bx * TM;
  const int n0 = by * TN_;
  const int chunk = (R + nz - 1) / nz;
  const int rbeg = bz * chunk;
  const int rend = min(rbeg + chunk, R);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int fi = lane & 15;
  const int fk = lane >> 4;
  const int mt = (wv & 1) * 16;
  const int nt = (wv >> 1) * 16;

  const bool do_bias = (db != nullptr || (XHAT && db_part != nullptr)) &&
                       (by == 0);
  float bsum = 0.0f;

  f32x4 acc = {0, 0, 0, 0};

  const int s_kr0 = tid >> 5;
  const int s_c = tid & 31;
  const int ktiles = (rend - rbeg + TKR - 1) / TKR;
  const bool ca = m0 + s_c < M;
  const bool cb = n0 + s_c < N;
  const int ga = min(m0 + s_c, M - 1);
  const int gb = min(n0 + s_c, N - 1);
  float pa[D][4], pb[D][4], pmu[D][4], prs[D][4];
  // tile t may lie past the slice: its loads are clamped duplicates of the
  // slice's last row and are never stored (ktiles > 0, so rend > rbeg)
  auto stage_regs = [&](int s, int t) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int gr = min(rbeg + t * TKR + s_kr0 + 8 * u, rend - 1);
      pa[s][u] = A[(long)gr * M + ga];
      pb[s][u] = B[(long)gr * N + gb];
      if (XHAT) {
        pmu[s][u] = mean[gr];
        prs[s][u] = rstd[gr];
      }
    }
  };
  auto regs_to_lds = [&](int s, int t, int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool rok = rbeg + t * TKR + s_kr0 + 8 * u < rend;
      const float av = (rok && ca) ? pa[s][u] : 0.0f;
      const float bv = XHAT ? (pb[s][u] - pmu[s][u]) * prs[s][u] : pb[s][u];
      if (do_bias) bsum += av;
      As[buf][s_kr0 + 8 * u][s_c] = av;
      Bs[buf][s_kr0 + 8 * u][s_c] = (rok && cb) ? bv : 0.0f;
    }
  };

  if (ktiles > 0) {
    // the sets are loaded in ring order, oldest first (the scheduler would
    // mix them, and the loop's counted waits rely on the order)
    stage_regs(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    regs_to_lds(0, 0, 0);
#pragma unroll
    for (int d = 1; d < D; ++d) {
      stage_regs(d, d);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  auto mma_tile = [&](int buf) {
    float fa[TKR / 4], fb[TKR / 4];
#pragma unroll
    for (int q = 0; q < TKR / 4; ++q) {
      fa[q] = As[buf][4 * q + fk][mt + fi];
      fb[q] = Bs[buf][4 * q + fk][nt + fi];
    }
    __builtin_amdgcn_sched_barrier(0);  // reads and loads stay above
#pragma unroll
    for (int q = 0; q < TKR / 4; ++q)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[q], fb[q], acc, 0, 0, 0);
  };
  // step kt < last: set kt % D is free (tile kt is in LDS) and takes tile
  // kt + D; set (kt + 1) % D holds tile kt + 1, the oldest in flight.
  // Whole groups of D steps run in a loop without a branch in its body: a
  // path that skipped a step's loads would, where it joins, turn the
  // counted waits of the later steps into nearly full ones.
  if (ktiles > 0) {
    const int last = ktiles - 1;
    int kt = 0;
    for (; kt + D <= last; kt += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        __syncthreads();
        stage_regs(d, kt + d + D);
        mma_tile((kt + d) & 1);
        __syncthreads();
        regs_to_lds((d + 1) % D, kt + d + 1, 1 - ((kt + d) & 1));
      }
    }
    // the last - kt < D steps left load nothing: their tiles are in flight
    // in sets 1, 2, ... (nested, so that no step is entered from two sides)
    auto rest = [&](auto self, auto rc) {
      constexpr int r = decltype(rc)::value;
      if constexpr (r < D - 1) {
        if (kt + r < last) {
          __syncthreads();
          mma_tile((kt + r) & 1);
          __syncthreads();
          regs_to_lds(r + 1, kt + r + 1, 1 - ((kt + r) & 1));
          self(self, std::integral_constant<int, r + 1>{});
        }
      }
    };
    rest(rest, std::integral_constant<int, 0>{});
    __syncthreads();
    mma_tile(last & 1);
  }

  const bool direct = !XHAT && (nz == 1);
  if (do_bias) {
    __syncthreads();
    As[0][s_kr0][s_c] = bsum;
    __syncthreads();
    if (tid < TM) {
      float s = 0.0f;
#pragma unroll
      for (int gq = 0; gq < 8; ++gq) s += As[0][gq][tid];
      const int gm = m0 + tid;
      if (gm < M) {
        if (direct) {
          if (accumulate) db[gm] += s; else db[gm] = s;
        } else {
          db_part[(long)bz * M + gm] = s;
        }
      }
    }
  }

  const int gn = n0 + nt + fi;
  if (gn >= N) return;
  float* po = direct ? out : part + (long)bz * M * N;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int gm = m0 + mt + (lane >> 4) * 4 + rr;
    if (gm >= M) continue;
    float* dst = &po[(long)gm * N + gn];
    if (direct && accumulate)
      *dst += acc[rr];
    else
      *dst = acc[rr];
  }
}

// D = 0: the original body; D >= 1: the pipelined one, D tiles ahead
template <bool XHAT, int D>
__device__ __forceinline__ void gemm_tn_sel(
    const float* __restrict__ A, const float* __restrict__ B,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ out, float* __restrict__ part,
    float* __restrict__ db, float* __restrict__ db_part,
    int R, int M, int N, int accumulate, int bx, int by, int bz, int nz) {
  if constexpr (D == 0)
    gemm_tn_body<XHAT>(A, B, mean, rstd, out, part, db, db_part, R, M, N,
                       accumulate, bx, by, bz, nz);
  else
    gemm_tn_pipe_body<XHAT, D>(A, B, mean, rstd, out, part, db, db_part, R,
                               M, N, accumulate, bx, by, bz, nz);
}

template <int D>
__global__ __launch_bounds__(256) void gemm_tn_kernel(
    const float* __restrict__ A, const float* __restrict__ B,
    float* __restrict__ out, float* __restrict__ part,
    float* __restrict__ db, float* __restrict__ db_part,
    int R, int M, int N, int accumulate) {
  gemm_tn_sel<false, D>(A, B, nullptr, nullptr, out, part, db, db_part, R, M,
                        N, accumulate, blockIdx.x, blockIdx.y, blockIdx.z,
                        gridDim.z);
}

// Two TN problems with a common R and M in one launch (the GRU's Whh and
// Wih weight gradients): blockIdx.x enumerates problem 0's
// (m-tile, n-tile) pairs, then problem 1's. Each tile runs the shared
// body, so every element sees the summation order of a separate
// gemm_tn call.
struct TnProblem {
  const float* A;
  const float* B;
  float* out;
  float* part;
  float* db;
  float* db_part;
  int N;
};
template <int D>
__global__ __launch_bounds__(256) void gemm_tn_pair_kernel(
    TnProblem p0, TnProblem p1, int R, int M, int accumulate) {
  const int mtiles = (M + TM - 1) / TM;
  const int tiles0 = mtiles * ((p0.N + TN_ - 1) / TN_);
  const bool second = (int)blockIdx.x >= tiles0;
  const int tile = second ? (int)blockIdx.x - tiles0 : (int)blockIdx.x;
  gemm_tn_sel<false, D>(second ? p1.A : p0.A, second ? p1.B : p0.B, nullptr,
                        nullptr, second ? p1.out : p0.out,
                        second ? p1.part : p0.part, second ? p1.db : p0.db,
                        second ? p1.db_part : p0.db_part, R, M,
                        second ? p1.N : p0.N, accumulate, tile % mtiles,
                        tile / mtiles, blockIdx.z, gridDim.z);
}

// part[z](M,N) = A[slice z]^T @ xhat[slice z], db_part[z](M) =
// colsum(A[slice z]) with xhat = (x - mean) * rstd formed while staging x.
template <int D>
__global__ __launch_bounds__(256) void gemm_tn_xhat_kernel(
    const float* __restrict__ A, const float* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ part, float* __restrict__ db_part,
    int R, int M, int N) {
  gemm_tn_sel<true, D>(A, x, mean, rstd, nullptr, part, nullptr, db_part, R,
                       M, N, 0, blockIdx.x, blockIdx.y, blockIdx.z,
                       gridDim.z);
}

// out[e] += sum_z part[z][e]; db[m] += sum_z db_part[z][m] — fixed z
// order (deterministic reduce, no atomics).
// 64 output elements per workgroup; the 4 waves each sum a fixed
// quarter of the z slices (coalesced across elements) and combine
// through LDS in fixed order - deterministic, 4x the wave parallelism
// of a thread-per-element loop (see tn_reduce_bf16_kernel).
__device__ __forceinline__ void tn_reduce_body(
    const float* __restrict__ part, float* __restrict__ out, long elems,
    const float* __restrict__ db_part, float* __restrict__ db, long m_elems,
    int z, int accumulate, long block) {
  __shared__ float ps[4][64];
  const int el = threadIdx.x & 63;
  const int zg = threadIdx.x >> 6;
  const long e = block * 64 + el;
  const int zchunk = (z + 3) / 4;
  const int zbeg = zg * zchunk;
  const int zend = min(zbeg + zchunk, z);
  float s = 0.0f;
  if (e < elems) {
    for (int c = zbeg; c < zend; ++c) s += part[(long)c * elems + e];
  } else if (e < elems + m_elems) {
    const long m = e - elems;
    for (int c = zbeg; c < zend; ++c) s += db_part[(long)c * m_elems + m];
  }
  ps[zg][el] = s;
  __syncthreads();
  if (zg == 0) {
    const float t = ((ps[0][el] + ps[1][el]) + (ps[2][el] + ps[3][el]));
    if (e < elems) {
      out[e] = (accumulate ? out[e] : 0.0f) + t;
    } else if (e < elems + m_elems) {
      const long m = e - elems;
      db[m] = (accumulate ? db[m] : 0.0f) + t;
    }
  }
}

__global__ __launch_bounds__(256) void tn_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ out, long elems,
    const float* __restrict__ db_part, float* __restrict__ db, long m_elems,
    int z, int accumulate) {
  tn_reduce_body(part, out, elems, db_part, db, m_elems, z, accumulate,
                 blockIdx.x);
}

// the reduce of gemm_tn_pair_kernel: problem 0's blocks, then problem 1's
__global__ __launch_bounds__(256) void tn_reduce_pair_kernel(
    TnProblem p0, TnProblem p1, int M, int has_db, int z, int accumulate) {
  const long m_elems = has_db ? M : 0;
  const long e0 = (long)M * p0.N;
  const int blocks0 = (int)((e0 + m_elems + 63) / 64);
  const bool second = (int)blockIdx.x >= blocks0;
  tn_reduce_body(second ? p1.part : p0.part, second ? p1.out : p0.out,
                 (long)M * (second ? p1.N : p0.N),
                 second ? p1.db_part : p0.db_part, second ? p1.db : p0.db,
                 m_elems, z, accumulate,
                 second ? (int)blockIdx.x - blocks0 : (int)blockIdx.x);
}

// tn_reduce_pair_kernel for a short list of problems, each with its own M
// and N: problem 0's blocks, then problem 1's, ... Every element's sum is
// tn_reduce_body's, i.e. that of the problem's own tn_reduce launch.
#define TN_LIST_MAX 4
struct TnReduceItem {
  const float* part;
  float* out;
  const float* db_part;
  float* db;  // null: no bias gradient
  int M;
  int N;
};
struct TnReduceList {
  TnReduceItem it[TN_LIST_MAX];
  int n;
};
static inline long tn_reduce_blocks(const TnReduceItem& q) {
  return ((long)q.M * q.N + (q.db ? q.M : 0) + 63) / 64;
}
__global__ __launch_bounds__(256) void tn_reduce_list_kernel(
    TnReduceList L, int z, int accumulate) {
  long block = blockIdx.x;
  int i = 0;
  // constant indices and select chains throughout: indexing the by-value
  // struct with a run-time i could put it in scratch
#pragma unroll
  for (int j = 0; j + 1 < TN_LIST_MAX; ++j) {
    const long nb = ((long)L.it[j].M * L.it[j].N +
                     (L.it[j].db ? L.it[j].M : 0) + 63) / 64;
    if (i == j && j + 1 < L.n && block >= nb) {
      block -= nb;
      i = j + 1;
    }
  }
  TnReduceItem q = L.it[0];
#pragma unroll
  for (int j = 1; j < TN_LIST_MAX; ++j)
    if (i == j) q = L.it[j];
  tn_reduce_body(q.part, q.out, (long)q.M * q.N, q.db_part, q.db,
                 q.db ? q.M : 0, z, accumulate, block);
}

// Finish of the dxln-free LayerNorm + W1x backward. With
// G = dzx^T @ xhat (slices part[z](C,C)) and gb = colsum(dzx) (slices
// db_part[z](C)), both from gemm_tn_xhat_kernel:
//   g(b1x)[j]   = gb[j]
//   g(W1x)[j,c] = gamma[c] * G[j,c] + beta[c] * gb[j]
//   g(ln_b)[c]  = sum_j gb[j] * W1x[j,c]
//   g(ln_g)[c]  = sum_j W1x[j,c] * G[j,c]
// One workgroup per 8 columns c; thread (jl = tid/8, tid%8) walks
// rows j = jl, jl+128, ... summing the z slices in fixed order, then the
// 128 row-lane partials of each column combine in a fixed halving tree
// through LDS: deterministic, no atomics.
#define LWF_COLS 8
#define LWF_ROWL 128
__global__ __launch_bounds__(1024) void ln_w1x_finish_kernel(
    const float* __restrict__ part, const float* __restrict__ db_part,
    const float* __restrict__ W, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ gW,
    float* __restrict__ gb1, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int C, int nz) {
  __shared__ float sg[LWF_ROWL][LWF_COLS + 1];
  __shared__ float sb[LWF_ROWL][LWF_COLS + 1];
  const int cl = threadIdx.x & (LWF_COLS - 1);
  const int jl = threadIdx.x / LWF_COLS;
  const int c = blockIdx.x * LWF_COLS + cl;
  const bool live = c < C;
  const float gm = live ? gamma[c] : 0.0f;
  const float bt = live ? beta[c] : 0.0f;
  const long cc = (long)C * C;
  float ag = 0.0f, ab = 0.0f;
  for (int j = jl; j < C; j += LWF_ROWL) {
    // slices in groups of 8: the group's 16 loads issue together
    // (branch-free: indices clamped into range, the adds guarded), the
    // sums still run in ascending z
    const float* pj = part + (long)j * C + min(c, C - 1);
    float G = 0.0f, gbj = 0.0f;
    for (int z0 = 0; z0 < nz; z0 += 8) {
      float pv[8], pd[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int z = min(z0 + u, nz - 1);
        pv[u] = pj[z * cc];
        pd[u] = db_part[(long)z * C + j];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (z0 + u < nz) {
          G += pv[u];
          gbj += pd[u];
        }
      }
    }
    if (live) {
      const float w = W[(long)j * C + c];
      gW[(long)j * C + c] = fmaf(gm, G, bt * gbj);
      ag = fmaf(w, G, ag);
      ab = fmaf(gbj, w, ab);
    }
    if (blockIdx.x == 0 && cl == 0) gb1[j] = gbj;
  }
  sg[jl][cl] = ag;
  sb[jl][cl] = ab;
  __syncthreads();
  for (int h = LWF_ROWL / 2; h > 0; h >>= 1) {
    if (jl < h) {
      sg[jl][cl] += sg[jl + h][cl];
      sb[jl][cl] += sb[jl + h][cl];
    }
    __syncthreads();
  }
  if (jl == 0 && live) {
    dgamma[c] = sg[0][cl];
    dbeta[c] = sb[0][cl];
  }
}

// out(C) (+)= sum_r A(R,C): grid (ceil(C/64), ceil(R/CS_ROWS)); 256
// threads = 4 waves striping the row chunk, LDS-reduced, one atomicAdd
// per column per WG (out is a pre-zeroed grad slot).
#define CS_ROWS 256
__global__ __launch_bounds__(256) void colsum_kernel(
    const float* __restrict__ A, float* __restrict__ out, int R, int C) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int rbeg = blockIdx.y * CS_ROWS;
  const int rend = min(rbeg + CS_ROWS, R);
  float s = 0.0f;
  if (c < C) {
    for (int r = rbeg + w; r < rend; r += 4) s += A[(long)r * C + c];
  }
  part[w][lane] = s;
  __syncthreads();
  if (w == 0 && c < C) {
    const float v = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
    atomicAdd(&out[c], v);
  }
}

// dZ = dY * lrelu'(Y) elementwise, where Y is the post-activation output
// (slope 0.01 preserves sign, so Y's sign recovers the pre-activation's).
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(
    const float* __restrict__ dY, const float* __restrict__ Y,
    float* __restrict__ dZ, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < total) dZ[idx] = dY[idx] * lrelu_grad_from_out_(Y[idx]);
}

// variant -> global prefetch distance of the pipelined kernels (0: the
// original kernel, -1: no such variant). Measured at the benchmark's tail
// shapes (profiles/f32_gemm.md): gemm_nn 1 and 2 tiles ahead are equal
// within 3 %, gemm_tn is fastest 2 ahead (4 ahead is slower again).
#define NN_DIST 1
#define TN_DIST 2
static inline int nn_distance(int variant) {
  return variant == 0 ? 0 : variant == 1 ? NN_DIST : -1;
}
static inline int tn_distance(int variant) {
  return variant == 0 ? 0 : variant == 1 ? TN_DIST : -1;
}

extern "C" {

hipError_t fv_gemm_nt(const float* A, const float* W, const float* bias,
                      float* out, int R, int Ci, int Co, float alpha,
                      int accumulate, int act_lrelu, hipStream_t stream) {
  int flags = (accumulate ? 1 : 0) | (act_lrelu ? 2 : 0) | (bias ? 4 : 0);
  dim3 grid((Co + BC - 1) / BC, (R + BR - 1) / BR);
  hipLaunchKernelGGL(gemm_nt_kernel, grid, dim3(256), 0, stream,
                     A, W, bias, out, R, Ci, Co, alpha, flags);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_gemm_nn(const float* A, const float* B, const float* bias,
                      float* out, int R, int Ci, int Co, float alpha,
                      int accumulate, int act_lrelu, const float* lrelu_bwd_of,
                      int variant, hipStream_t stream) {
  // variant 0: gemm_nn_kernel; 1: gemm_nn_pipe_kernel (bit-identical)
  variant = nn_distance(variant);
  if (variant < 0) return hipErrorInvalidValue;
  int flags = (accumulate ? 1 : 0) | (act_lrelu ? 2 : 0) | (bias ? 4 : 0) |
              (lrelu_bwd_of ? 8 : 0);
  dim3 grid((Co + BC - 1) / BC, (R + BR - 1) / BR);
  if (R < 1 || Ci < 1 || Co < 1) variant = 0;  // the pipe kernel's clamps
  if (variant)
    hipLaunchKernelGGL((gemm_nn_pipe_kernel<NN_DIST, false>), grid, dim3(256), 0,
                       stream, A, B, bias, lrelu_bwd_of, out, nullptr, nullptr,
                       nullptr, nullptr, R, Ci, Co, alpha, flags);
  else
    hipLaunchKernelGGL(gemm_nn_kernel, grid, dim3(256), 0, stream,
                       A, B, bias, lrelu_bwd_of, out, R, Ci, Co, alpha, flags);
  HIP_CHECK_LAST();
  return hipSuccess;
}

// LayerNorm parameter-gradient partials straight from the dxln GEMM:
// part = what fv_ln_bwd_params' first kernel writes for
// dxln = alpha * (A(R,Ci) @ B(Ci,C)), without storing dxln; follow with
// fv_ln_bwd_reduce. Valid only where fv_ln_bwd_params works on 64-row
// blocks, gemm_nn's tile height (fv_ln_bwd_rows); otherwise *ran = 0 and
// nothing is launched (the caller runs gemm_nn and ln_bwd_params).
hipError_t fv_gemm_nn_ln(const float* A, const float* B, const float* x,
                         const float* mean, const float* rstd, float* part,
                         long R, int Ci, int C, float alpha, int* ran,
                         hipStream_t stream) {
  *ran = 0;
  if (R < 1 || R > 0x7fffffffL || Ci < 1 || C < 1) return hipSuccess;
  if (fv_ln_bwd_rows(R, C) != BR) return hipSuccess;
  dim3 grid((C + BC - 1) / BC, (unsigned)((R + BR - 1) / BR));
  if (grid.y > 65535u) return hipSuccess;
  hipLaunchKernelGGL((gemm_nn_pipe_kernel<NN_DIST, true>), grid, dim3(256), 0,
                     stream, A, B, nullptr, nullptr, nullptr, x, mean, rstd,
                     part, (int)R, Ci, C, alpha, 0);
  HIP_CHECK_LAST();
  *ran = 1;
  return hipSuccess;
}

hipError_t fv_gemm_tn(const float* A, const float* B, float* out,
                      float* part, float* db, float* db_part,
                      int R, int M, int N, int r_chunks,
                      int accumulate, int variant, int reduce,
                      hipStream_t stream) {
  // r_chunks > 1 is a request to chunk the R-reduction; the launcher
  // picks the actual split (>=512 rows per chunk, <=32 slices).
  // variant 0: the original loop; 1: the pipelined one (bit-identical).
  // reduce = 0: leave the slices in part/db_part for fv_tn_reduce_list.
  variant = tn_distance(variant);
  if (variant < 0) return hipErrorInvalidValue;
  if (r_chunks < 1) r_chunks = 1;
  if (!part) r_chunks = 1;
  if (r_chunks > 1) {
    r_chunks = (R + 511) / 512;
    if (r_chunks > 32) r_chunks = 32;
    if (r_chunks < 1) r_chunks = 1;
  }
  if (r_chunks > 1 && db && !db_part) r_chunks = 1;  // need partial space
  dim3 grid((M + TM - 1) / TM, (N + TN_ - 1) / TN_, r_chunks);
#define TN_LAUNCH(D)                                                       \
  hipLaunchKernelGGL(gemm_tn_kernel<D>, grid, dim3(256), 0, stream, A, B, \
                     out, part, db, db_part, R, M, N, accumulate)
  if (variant) TN_LAUNCH(TN_DIST);
  else TN_LAUNCH(0);
#undef TN_LAUNCH
  HIP_CHECK_LAST();
  if (r_chunks > 1 && reduce) {
    const long elems = (long)M * N;
    const long m_elems = db ? M : 0;
    dim3 rgrid((unsigned)((elems + m_elems + 63) / 64));
    hipLaunchKernelGGL(tn_reduce_kernel, rgrid, dim3(256), 0, stream,
                       part, out, elems, db_part, db, m_elems, r_chunks,
                       accumulate);
    HIP_CHECK_LAST();
  }
  return hipSuccess;
}

// Whh/Wih-style pair: out0(M,N0) = A0^T @ B0, out1(M,N1) = A1^T @ B1 over
// a common R, bias grads db0/db1(M) optional (both or neither). Same
// slice rule and per-element summation order as two fv_gemm_tn calls;
// one GEMM launch + (when sliced) one reduce launch.
hipError_t fv_gemm_tn_pair(const float* A0, const float* B0, float* out0,
                           float* part0, float* db0, float* db_part0, int N0,
                           const float* A1, const float* B1, float* out1,
                           float* part1, float* db1, float* db_part1, int N1,
                           int R, int M, int r_chunks, int accumulate,
                           int variant, int reduce, hipStream_t stream) {
  variant = tn_distance(variant);
  if (variant < 0) return hipErrorInvalidValue;
  if (r_chunks < 1) r_chunks = 1;
  if (!part0 || !part1) r_chunks = 1;
  if (r_chunks > 1) {
    r_chunks = (R + 511) / 512;
    if (r_chunks > 32) r_chunks = 32;
    if (r_chunks < 1) r_chunks = 1;
  }
  if (r_chunks > 1 && db0 && !(db_part0 && db_part1)) r_chunks = 1;
  const TnProblem p0 = {A0, B0, out0, part0, db0, db_part0, N0};
  const TnProblem p1 = {A1, B1, out1, part1, db1, db_part1, N1};
  const int mtiles = (M + TM - 1) / TM;
  const int tiles = mtiles * ((N0 + TN_ - 1) / TN_ + (N1 + TN_ - 1) / TN_);
#define TN_LAUNCH(D)                                                     \
  hipLaunchKernelGGL(gemm_tn_pair_kernel<D>, dim3(tiles, 1, r_chunks),  \
                     dim3(256), 0, stream, p0, p1, R, M, accumulate)
  if (variant) TN_LAUNCH(TN_DIST);
  else TN_LAUNCH(0);
#undef TN_LAUNCH
  HIP_CHECK_LAST();
  if (r_chunks > 1 && reduce) {
    const long m_elems = db0 ? M : 0;
    const long b0 = ((long)M * N0 + m_elems + 63) / 64;
    const long b1 = ((long)M * N1 + m_elems + 63) / 64;
    hipLaunchKernelGGL(tn_reduce_pair_kernel, dim3((unsigned)(b0 + b1)),
                       dim3(256), 0, stream, p0, p1, M, db0 ? 1 : 0, r_chunks,
                       accumulate);
    HIP_CHECK_LAST();
  }
  return hipSuccess;
}

// number of R slices fv_gemm_tn_xhat writes (the fv_gemm_tn rule:
// >= 512 rows per slice, <= 32 slices)
int fv_tn_xhat_slices(int R) {
  int z = (R + 511) / 512;
  if (z > 32) z = 32;
  if (z < 1) z = 1;
  return z;
}

// part[z](M,N) = A(R,M)[slice z]^T @ xhat(R,N)[slice z], db_part[z](M) =
// colsum(A[slice z]); never reduced here (ln_w1x_finish sums the slices).
hipError_t fv_gemm_tn_xhat(const float* A, const float* x, const float* mean,
                           const float* rstd, float* part, float* db_part,
                           int R, int M, int N, int variant,
                           hipStream_t stream) {
  variant = tn_distance(variant);
  if (variant < 0) return hipErrorInvalidValue;
  dim3 grid((M + TM - 1) / TM, (N + TN_ - 1) / TN_, fv_tn_xhat_slices(R));
#define TN_LAUNCH(D)                                                      \
  hipLaunchKernelGGL(gemm_tn_xhat_kernel<D>, grid, dim3(256), 0, stream, \
                     A, x, mean, rstd, part, db_part, R, M, N)
  if (variant) TN_LAUNCH(TN_DIST);
  else TN_LAUNCH(0);
#undef TN_LAUNCH
  HIP_CHECK_LAST();
  return hipSuccess;
}

// One reduce launch for n <= 4 sliced TN problems that share the slice
// count z (gemm_tn / gemm_tn_pair calls with reduce = 0 over a common R):
// out_i(M_i,N_i) (+)= sum_z part_i[z], db_i(M_i) (+)= sum_z db_part_i[z]
// where db_i is not null. Each element's sum is the one the problem's own
// reduce launch forms. z <= 1: the GEMMs wrote out/db themselves, nothing
// is launched.
hipError_t fv_tn_reduce_list(int n, const float* const* part,
                             float* const* out, const float* const* db_part,
                             float* const* db, const int* M, const int* N,
                             int z, int accumulate, hipStream_t stream) {
  if (n < 1 || n > TN_LIST_MAX) return hipErrorInvalidValue;
  if (z <= 1) return hipSuccess;
  TnReduceList L = {};
  L.n = n;
  long blocks = 0;
  for (int i = 0; i < n; ++i) {
    L.it[i] = {part[i], out[i], db_part[i], db[i], M[i], N[i]};
    blocks += tn_reduce_blocks(L.it[i]);
  }
  hipLaunchKernelGGL(tn_reduce_list_kernel, dim3((unsigned)blocks), dim3(256),
                     0, stream, L, z, accumulate);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_ln_w1x_finish(const float* part, const float* db_part,
                            const float* W1x, const float* gamma,
                            const float* beta, float* gW1x, float* gb1x,
                            float* dgamma, float* dbeta, int C, int nz,
                            hipStream_t stream) {
  hipLaunchKernelGGL(ln_w1x_finish_kernel,
                     dim3((C + LWF_COLS - 1) / LWF_COLS), dim3(1024), 0,
                     stream, part, db_part, W1x, gamma, beta, gW1x, gb1x,
                     dgamma, dbeta, C, nz);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_colsum(const float* A, float* out, int R, int C, int r_chunks,
                     hipStream_t stream) {
  (void)r_chunks;
  dim3 grid((C + 63) / 64, (R + CS_ROWS - 1) / CS_ROWS);
  hipLaunchKernelGGL(colsum_kernel, grid, dim3(256), 0, stream, A, out, R, C);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_lrelu_bwd(const float* dY, const float* Y, float* dZ, long total,
                        hipStream_t stream) {
  long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(lrelu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     stream, dY, Y, dZ, total);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
