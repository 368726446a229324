// Feature-extractor front kernels: LayerNorm forward + parameter backward,
// and the fused fp32 head (LayerNorm + C->C projection + GRU input
// projection in one launch). Outside the fused head the two projections
// are gemm_nt calls; the GRU recurrence is gru.hip.

#include "common.h"
#include "launchers.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;

// x(R,C) -> xln = gamma * (x-mean)*rstd + beta; one wave per row batch.
// Saves mean & rstd per row for the backward recompute.
#define LNF_ROWS 4
__global__ __launch_bounds__(256) void ln_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ xln,
    __bf16* __restrict__ xln_bf, unsigned char* __restrict__ xln_f8,
    int f8_ld,
    float* __restrict__ mean, float* __restrict__ rstd,
    long R, int C, float eps) {
  const int wid = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  // LNF_ROWS sequential rows per wave: 1-row waves left the kernel
  // launch/dispatch-bound (52k tiny workgroups at A-share, 96.6 us);
  // 4 rows amortize the workgroup and the gamma/beta loads -> 58.9 us,
  // bit-identical (scripts/probe/ln_probe.hip A/B).
  const long row0 = ((long)blockIdx.x * 4 + wid) * LNF_ROWS;
  const int c4 = lane * 4;

  // gamma/beta for this lane's main chunk, loaded once per wave
  float gv[4], bvv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c4 + i;
    gv[i] = (c < C) ? gamma[c] : 0.0f;
    bvv[i] = (c < C) ? beta[c] : 0.0f;
  }

  for (int r = 0; r < LNF_ROWS; ++r) {
    const long row = row0 + r;
    if (row >= R) return;
    const float* xr = x + row * C;

    // single pass, vectorized: lane l owns the f32x4 chunk at 4*l (plus
    // a strided tail for C > 256); the row stays in registers for the
    // normalize write — one HBM read of x instead of three
    // variance uses the TWO-PASS form sum((x-mu)^2) over the
    // register-resident row (a second wave reduce, no extra memory
    // traffic): the single-pass E[x^2]-mu^2 form cancels
    // catastrophically in fp32 when |mean| >> std — plausible for
    // un-normalized financial features.
    float xv[8];
    float s = 0.0f;
    if (c4 + 4 <= C) {
      const f32x4 v = *(const f32x4*)&xr[c4];
      xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
#pragma unroll
      for (int i = 0; i < 4; ++i) s += xv[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c4 + i;
        const float xx = (c < C) ? xr[c] : 0.0f;
        xv[i] = xx;
        s += xx;
      }
    }
    int tail = 0;
    for (int c = 256 + lane; c < C; c += 64, ++tail) {  // C > 256
      const float xx = xr[c];
      if (tail < 4) xv[4 + tail] = xx;
      s += xx;
    }
    s = wave_reduce_sum(s);
    s = __shfl(s, 0, 64);
    const float mu = s / C;
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (c4 + i < C) {
        const float d = xv[i] - mu;
        sq = fmaf(d, d, sq);
      }
    }
    tail = 0;
    for (int c = 256 + lane; c < C; c += 64, ++tail) {
      const float d = ((tail < 4) ? xv[4 + tail] : xr[c]) - mu;
      sq = fmaf(d, d, sq);
    }
    sq = wave_reduce_sum(sq);
    sq = __shfl(sq, 0, 64);
    const float var = fmaxf(sq / C, 0.0f);
    const float rs = rsqrtf(var + eps);

    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    float* o = xln ? xln + row * C : nullptr;
    __bf16* ob = xln_bf ? xln_bf + row * C : nullptr;
    unsigned char* o8 = xln_f8 ? xln_f8 + row * (long)f8_ld : nullptr;
    if (c4 + 4 <= C && (C & 1) == 0) {
      // vectorized main chunk (even C only: odd C breaks the 4B/8B
      // row-base alignment): the compiler cannot prove better than
      // element alignment for the bf16/fp8 rows, so pack explicitly
      // (f32 rows are 8B-aligned, bf16 4B, fp8 4B via the 128-padded
      // stride — all hold for every even C and padded f8_ld)
      float vv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        vv[i] = fmaf((xv[i] - mu) * rs, gv[i], bvv[i]);
      if (o) {
        *(float2*)&o[c4] = make_float2(vv[0], vv[1]);
        *(float2*)&o[c4 + 2] = make_float2(vv[2], vv[3]);
      }
      if (ob) {
        union { unsigned int u; __bf16 h[2]; } p0, p1;
        p0.h[0] = (__bf16)vv[0]; p0.h[1] = (__bf16)vv[1];
        p1.h[0] = (__bf16)vv[2]; p1.h[1] = (__bf16)vv[3];
        *(unsigned int*)&ob[c4] = p0.u;
        *(unsigned int*)&ob[c4 + 2] = p1.u;
      }
      if (o8) {
        unsigned int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(vv[0], vv[1], lo, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(vv[2], vv[3], hi, false);
        *(unsigned int*)&o8[c4] = (lo & 0xffffu) | (hi << 16);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c4 + i;
        if (c >= C) break;
        const float v_ = fmaf((xv[i] - mu) * rs, gv[i], bvv[i]);
        if (o) o[c] = v_;
        if (ob) ob[c] = (__bf16)v_;
        if (o8) {
          unsigned int u = 0;
          u = __builtin_amdgcn_cvt_pk_fp8_f32(v_, 0.0f, u, false);
          o8[c] = (unsigned char)(u & 0xff);
        }
      }
    }
    tail = 0;
    for (int c = 256 + lane; c < C; c += 64, ++tail) {
      const float xx = (tail < 4) ? xv[4 + tail] : xr[c];
      const float v_ = fmaf((xx - mu) * rs, gamma[c], beta[c]);
      if (o) o[c] = v_;
      if (ob) ob[c] = (__bf16)v_;
      if (o8) {
        unsigned int u = 0;
        u = __builtin_amdgcn_cvt_pk_fp8_f32(v_, 0.0f, u, false);
        o8[c] = (unsigned char)(u & 0xff);
      }
    }
  }
}

// Fused fp32 extractor head: one workgroup per SR-row strip of x runs
//   LayerNorm -> xp = lrelu(xln @ W1x^T + b1x) -> gi = xp @ Wih^T + bih
// with the strip resident in LDS, replacing ln_fwd + two gemm_nt launches.
// Every output is bit-identical to that sequence (docs/KERNELS.md):
//   - the per-row LayerNorm arithmetic is ln_fwd_kernel's, expression for
//     expression (lane l owns columns 4l..4l+3, same wave reductions);
//   - each output element accumulates k-groups 0, 1, 2, ... ascending into
//     one accumulator that starts at +0, lane fk = lane >> 4 supplying
//     k = 4*group + fk for both operands (gemm_nt_kernel's mapping), over
//     the same number of groups (k padded to a multiple of 32);
//   - every padded position (k >= C, rows >= R, output columns >= Co) is
//     exactly 0.0 in BOTH operands, and padded rows/columns are not stored.
// LDS: strip[SR][KP + 2] (xln, then overwritten by xp once GEMM 1's k loop
// is done) + wbuf[2][16 * max(ct1, ct2)][34], the double-buffered weight
// k-tile over all output columns. Row strides are == 2 (mod 32) dwords, so
// a fragment read (16 rows x 2 k per half-wave) touches 32 distinct banks.
// Wave w owns row tile w % RT and column tiles w / RT, w / RT + 4 / RT, ...
#define EH_BK 32
#define EH_WLD (EH_BK + 2)
#define EH_CT_MAX 16  // column tiles per GEMM: C <= 256 and G <= 256

// f32x4 at element (4-byte) alignment: rows of x and of the weights
// start wherever C puts them
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// wave_reduce_sum + broadcast of lane 0's total, for N independent values
// at once: each value sees wave_reduce_sum's additions in its order, the N
// cross-lane chains overlap instead of running one after the other.
template <int N>
DEVINL void eh_wave_sum_bcast(float (&v)[N]) {
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] += __shfl_down(v[q], off, 64);
  }
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = __shfl(v[q], 0, 64);
}

// One k-tile (8 k-groups) of NT output tiles. The fragments of k-groups
// 2p+2, 2p+3 are read from LDS before the MFMAs of groups 2p, 2p+1 issue,
// so the reads' latency hides under them; each accumulator still sees
// its k-groups in ascending order.
template <int NT>
DEVINL void eh_mma_ktile(const float* a_ptr, const float* w_ptr, int w_step,
                         f32x4* acc) {
  float a[2][2], b[2][NT][2];
  auto frag = [&](int buf, int kk) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      a[buf][h] = a_ptr[kk + 4 * h];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[buf][j][h] = w_ptr[j * w_step + kk + 4 * h];
    }
  };
  frag(0, 0);
#pragma unroll
  for (int p = 0; p < EH_BK / 8; ++p) {
    if (p + 1 < EH_BK / 8) frag((p + 1) & 1, (p + 1) * 8);
    __builtin_amdgcn_sched_barrier(0);  // keep the reads above the MFMAs
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            a[p & 1][h], b[p & 1][j][h], acc[j], 0, 0, 0);
    }
  }
}

// nt is wave-uniform: pick the instantiation with exactly nt tiles
template <int NT, int NTMAX>
DEVINL void eh_mma_sel(const float* a_ptr, const float* w_ptr, int w_step,
                       int nt, f32x4* acc) {
  if (nt == NT) {
    eh_mma_ktile<NT>(a_ptr, w_ptr, w_step, acc);
  } else if constexpr (NT < NTMAX) {
    eh_mma_sel<NT + 1, NTMAX>(a_ptr, w_ptr, w_step, nt, acc);
  }
}

template <int SR>
__global__ __launch_bounds__(256) void extractor_head_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ W1x,
    const float* __restrict__ b1x, const float* __restrict__ Wih,
    const float* __restrict__ bih, float* __restrict__ xln,
    float* __restrict__ mean, float* __restrict__ rstd,
    float* __restrict__ xp, float* __restrict__ gi,
    long R, int C, int G, float eps) {
  extern __shared__ __attribute__((aligned(16))) float eh_smem[];
  constexpr int RT = SR / 16;           // row tiles per strip
  constexpr int WPR = 4 / RT;           // waves sharing one row tile
  constexpr int NTMAX = EH_CT_MAX / WPR;  // column tiles per wave
  constexpr int LROWS = SR / 4;         // LayerNorm rows per wave

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int fi = lane & 15;
  const int fk = lane >> 4;
  const long r0 = (long)blockIdx.x * SR;

  const int KP = (C + EH_BK - 1) & ~(EH_BK - 1);
  const int SLD = KP + 2;
  const int ktiles = KP / EH_BK;
  const int ct1 = (C + 15) >> 4;
  const int ct2 = (G + 15) >> 4;
  float* strip = eh_smem;
  float* wbuf = eh_smem + SR * SLD;
  const int wbuf_sz = 16 * max(ct1, ct2) * EH_WLD;

  // weight staging: thread -> (row = tid/8 + 32u, k quad = 4 * (tid%8)),
  // one 16-byte load per 32 rows of the k-tile; a partial last k-tile
  // loads element by element. Row and k are clamped into range for the
  // loads, and the clamped positions become the exact zeros of the
  // padding only at the LDS store: nothing between the loads' issue and
  // the MFMAs uses a loaded value, so the loads fly under the MFMAs.
  const int s_row0 = tid >> 3;
  const int s_k = (tid & 7) * 4;
  f32x4 pw[EH_CT_MAX / 2];
  int p_co = 0;  // the staged weight's row count
  int p_gk = 0;  // the staged quad's first k
  auto stage_regs = [&](const float* __restrict__ W, int Co, int cop,
                        int k0) {
    const int gk = k0 + s_k;
    p_co = Co;
    p_gk = gk;
    if (k0 + EH_BK <= C) {  // wave-uniform: every k-tile but a partial last
#pragma unroll
      for (int u = 0; u < EH_CT_MAX / 2; ++u) {
        if (32 * u < cop) {  // wave-uniform
          const unsigned row = (unsigned)min(s_row0 + 32 * u, Co - 1);
          pw[u] = *(const f32x4u*)&W[row * (unsigned)C + gk];
        } else {
          pw[u] = f32x4{0, 0, 0, 0};
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < EH_CT_MAX / 2; ++u) {
        if (32 * u < cop) {
          const unsigned row = (unsigned)min(s_row0 + 32 * u, Co - 1);
          const float* src = W + row * (unsigned)C;
#pragma unroll
          for (int i = 0; i < 4; ++i) pw[u][i] = src[min(gk + i, C - 1)];
        } else {
          pw[u] = f32x4{0, 0, 0, 0};
        }
      }
    }
  };
  auto regs_to_lds = [&](int buf, int cop) {
    float* wb = wbuf + buf * wbuf_sz;
#pragma unroll
    for (int u = 0; u < EH_CT_MAX / 2; ++u) {
      const int row = s_row0 + 32 * u;
      if (row < cop) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          v[i] = (row < p_co && p_gk + i < C) ? pw[u][i] : 0.0f;
        float* d = &wb[row * EH_WLD + s_k];
        *(float2*)&d[0] = make_float2(v.x, v.y);
        *(float2*)&d[2] = make_float2(v.z, v.w);
      }
    }
  };

  // W1x's first k-tile flies under the LayerNorm
  stage_regs(W1x, C, ct1 * 16, 0);

  // ---- LayerNorm: ln_fwd_kernel's row arithmetic, LROWS rows per wave.
  // The rows go through each step together (one wave per SIMD here, so
  // the two wave reductions per row would otherwise be LROWS serial
  // cross-lane latency chains); per row the operations and their order
  // are ln_fwd_kernel's. Rows >= R compute on zeros and store nothing.
  {
    const int c4 = lane * 4;
    float gv[4], bvv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c4 + i;
      gv[i] = (c < C) ? gamma[c] : 0.0f;
      bvv[i] = (c < C) ? beta[c] : 0.0f;
    }
    float xv[LROWS][4];
#pragma unroll
    for (int q = 0; q < LROWS; ++q) {
      const long row = r0 + wv * LROWS + q;
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[q][i] = 0.0f;
      if (row < R) {
        const float* xr = x + row * C;
        if (c4 + 4 <= C) {
          const f32x4 v = *(const f32x4u*)&xr[c4];
          xv[q][0] = v.x; xv[q][1] = v.y; xv[q][2] = v.z; xv[q][3] = v.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (c4 + i < C) xv[q][i] = xr[c4 + i];
        }
      }
    }
    float mu[LROWS], rs[LROWS];
#pragma unroll
    for (int q = 0; q < LROWS; ++q) {
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) s += xv[q][i];
      mu[q] = s;
    }
    eh_wave_sum_bcast<LROWS>(mu);
#pragma unroll
    for (int q = 0; q < LROWS; ++q) {
      mu[q] = mu[q] / C;
      float sq = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (c4 + i < C) {
          const float d = xv[q][i] - mu[q];
          sq = fmaf(d, d, sq);
        }
      }
      rs[q] = sq;
    }
    eh_wave_sum_bcast<LROWS>(rs);
#pragma unroll
    for (int q = 0; q < LROWS; ++q) {
      const int lr = wv * LROWS + q;
      const long row = r0 + lr;
      const float var = fmaxf(rs[q] / C, 0.0f);
      const float rq = rsqrtf(var + eps);
      float vv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      if (row < R) {
        if (lane == 0) {
          mean[row] = mu[q];
          rstd[row] = rq;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c4 + i < C)
            vv[i] = fmaf((xv[q][i] - mu[q]) * rq, gv[i], bvv[i]);
        if (xln) {
          float* o = xln + row * C;
          if (c4 + 4 <= C && (C & 1) == 0) {
            *(float2*)&o[c4] = make_float2(vv[0], vv[1]);
            *(float2*)&o[c4 + 2] = make_float2(vv[2], vv[3]);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (c4 + i < C) o[c4 + i] = vv[i];
          }
        }
      }
      // the strip's k pad (columns C..KP-1) and rows >= R are exact zeros
      if (c4 < KP) {
        float* sp = &strip[lr * SLD + c4];
        *(float2*)&sp[0] = make_float2(vv[0], vv[1]);
        *(float2*)&sp[2] = make_float2(vv[2], vv[3]);
      }
    }
  }
  regs_to_lds(0, ct1 * 16);

  // ---- the two GEMMs as one sequence of 2 * ktiles weight k-tiles
  const int rt = wv % RT;
  const int ctw = wv / RT;  // first column tile of this wave
  const int nt1 = ct1 > ctw ? (ct1 - ctw + WPR - 1) / WPR : 0;
  const int nt2 = ct2 > ctw ? (ct2 - ctw + WPR - 1) / WPR : 0;
  const float* a_row = &strip[(rt * 16 + fi) * SLD + fk];
  const int w_off = (ctw * 16 + fi) * EH_WLD + fk;
  const int w_step = WPR * 16 * EH_WLD;

  f32x4 acc[NTMAX];
#pragma unroll
  for (int j = 0; j < NTMAX; ++j) acc[j] = f32x4{0, 0, 0, 0};

  const int steps = 2 * ktiles;
  for (int s = 0; s < steps; ++s) {
    // tile s is visible in wbuf[s & 1], and every wave is done with the
    // compute of tile s - 1, so wbuf[(s + 1) & 1] may be overwritten
    __syncthreads();
    const bool more = s + 1 < steps;
    const bool next2 = s + 1 >= ktiles;
    if (more) {
      if (next2) stage_regs(Wih, G, ct2 * 16, (s + 1 - ktiles) * EH_BK);
      else stage_regs(W1x, C, ct1 * 16, (s + 1) * EH_BK);
    }
    const bool second = s >= ktiles;
    const int k0 = (second ? s - ktiles : s) * EH_BK;
    eh_mma_sel<1, NTMAX>(a_row + k0, wbuf + (s & 1) * wbuf_sz + w_off,
                         w_step, second ? nt2 : nt1, acc);
    if (more) regs_to_lds((s + 1) & 1, (next2 ? ct2 : ct1) * 16);

    if (s == ktiles - 1) {
      // GEMM 1 epilogue (gemm_nt's order: + bias, LeakyReLU): xp goes to
      // memory and over the xln strip, once every wave has read xln
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NTMAX; ++j) {
        if (j < nt1) {
          const int gc = (ctw + j * WPR) * 16 + fi;
          if (gc < C) {
            const float bj = b1x[gc];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
              const int lr = rt * 16 + fk * 4 + rr;
              const long gr = r0 + lr;
              float v = acc[j][rr];
              v += bj;
              v = lrelu_(v);
              if (gr < R) xp[gr * C + gc] = v;
              strip[lr * SLD + gc] = (gr < R) ? v : 0.0f;
            }
          }
        }
        acc[j] = f32x4{0, 0, 0, 0};
      }
    }
  }

  // ---- GEMM 2 epilogue: + bias
#pragma unroll
  for (int j = 0; j < NTMAX; ++j) {
    if (j < nt2) {
      const int gc = (ctw + j * WPR) * 16 + fi;
      if (gc < G) {
        const float bj = bih[gc];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const long gr = r0 + rt * 16 + fk * 4 + rr;
          if (gr < R) gi[gr * G + gc] = acc[j][rr] + bj;
        }
      }
    }
  }
}

// Parameter grads only (x is input data, no dx needed):
//   dgamma[c] = sum_r dxln[r][c] * xhat[r][c],  dbeta[c] = sum_r dxln[r][c]
// xhat recomputed from x, mean, rstd. Grid: (ceil(C/64), ceil(R/LNB_ROWS));
// 4 waves stripe the row chunk, LDS-reduced, one atomicAdd per column/WG.
// rows per block chosen by the launcher: enough blocks to fill the
// chip, few enough that the one-atomic-per-column-per-block flush stays
// cheap at large R
// per-(row-chunk) partials, layout part[yblock][2C] ([dgamma C][dbeta C]),
// reduced in fixed yblock order by ln_bwd_reduce_kernel (deterministic).
__global__ __launch_bounds__(256) void ln_bwd_params_kernel(
    const float* __restrict__ x, const float* __restrict__ dxln,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ part, long R, int C,
    int rows_per_block) {
  __shared__ float pg[4][64];
  __shared__ float pb[4][64];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const long rbeg = (long)blockIdx.y * rows_per_block;
  const long rend = min(rbeg + (long)rows_per_block, R);
  float dg = 0.0f, db = 0.0f;
  if (c < C) {
    for (long r = rbeg + w; r < rend; r += 4) {
      const float g = dxln[r * C + c];
      const float xh = (x[r * C + c] - mean[r]) * rstd[r];
      dg = fmaf(g, xh, dg);
      db += g;
    }
  }
  pg[w][lane] = dg;
  pb[w][lane] = db;
  __syncthreads();
  if (w == 0 && c < C) {
    // TRANSPOSED partial layout part[e][yblock]: the reduce kernel then
    // reads each column's partials contiguously instead of strided
    part[(long)c * gridDim.y + blockIdx.y] =
        pg[0][lane] + pg[1][lane] + pg[2][lane] + pg[3][lane];
    part[((long)C + c) * gridDim.y + blockIdx.y] =
        pb[0][lane] + pb[1][lane] + pb[2][lane] + pb[3][lane];
  }
}

// One WAVE per output element: lane l sums partials l, l+64, ... then a
// fixed-tree wave reduction combines lanes. The schedule is a fixed
// function of (e, yblocks), so results stay bit-identical run to run.
// (The old thread-per-element form was 2-3 workgroups on 256 CUs, a
// ~55 us dependent-load chain at the very tail of the backward.)
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int yblocks, int C) {
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= 2 * C) return;
  const int lane = threadIdx.x & 63;
  const float* pe = part + (long)e * yblocks;
  float s0 = 0.f, s1 = 0.f;
  int z = lane;
  for (; z + 64 < yblocks; z += 128) {
    s0 += pe[z];
    s1 += pe[z + 64];
  }
  if (z < yblocks) s0 += pe[z];
  float s = wave_reduce_sum(s0 + s1);
  if (lane == 0) {
    if (e < C) dgamma[e] = s;
    else dbeta[e - C] = s;
  }
}

template <int SR>
static hipError_t eh_launch(const float* x, const float* gamma,
                            const float* beta, const float* W1x,
                            const float* b1x, const float* Wih,
                            const float* bih, float* xln, float* mean,
                            float* rstd, float* xp, float* gi, long R, int C,
                            int G, float eps, size_t lds,
                            hipStream_t stream) {
  static bool attr_set = false;  // dynamic LDS above the 64 KiB default
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(
        (const void*)extractor_head_fwd_kernel<SR>,
        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  dim3 grid((unsigned)((R + SR - 1) / SR));
  hipLaunchKernelGGL(extractor_head_fwd_kernel<SR>, grid, dim3(256), lds,
                     stream, x, gamma, beta, W1x, b1x, Wih, bih, xln, mean,
                     rstd, xp, gi, R, C, G, eps);
  HIP_CHECK_LAST();
  return hipSuccess;
}

// fv_ln_bwd_params' launch geometry. ~2000 blocks: the reduction is
// latency-bound per block (two global reads per row-iteration), so
// parallelism beats reduce thrift. Returns the row-chunk count.
static inline unsigned ln_bwd_geometry(long R, int C, long* rpb_out) {
  const int cblocks = (C + 63) / 64;
  long target_y = (2048 + cblocks - 1) / cblocks;
  long rpb = (R + target_y - 1) / target_y;
  if (rpb < 64) rpb = 64;
  if (rpb > 8192) rpb = 8192;
  *rpb_out = rpb;
  return (unsigned)((R + rpb - 1) / rpb);
}

extern "C" {

hipError_t fv_ln_fwd(const float* x, const float* gamma, const float* beta,
                     float* xln, void* xln_bf, void* xln_f8, int f8_ld,
                     float* mean, float* rstd,
                     long R, int C, float eps, hipStream_t stream) {
  const long wgrows = 4L * LNF_ROWS;
  dim3 grid((unsigned)((R + wgrows - 1) / wgrows));
  hipLaunchKernelGGL(ln_fwd_kernel, grid, dim3(256), 0, stream,
                     x, gamma, beta, xln, (__bf16*)xln_bf,
                     (unsigned char*)xln_f8, f8_ld, mean, rstd, R, C, eps);
  HIP_CHECK_LAST();
  return hipSuccess;
}

// LayerNorm + W1x projection + GRU input projection in one launch.
// Supported: 1 <= C <= 256 (ln_fwd's single-chunk row path; 16 column
// tiles), 1 <= G <= 256 (16 column tiles), and the strip plus the
// double-buffered weight k-tile within the 160 KiB of LDS:
//   4 * (strip * (ceil32(C) + 2) + 2 * 16 * ceil(max(C, G) / 16) * 34) B.
// strip: rows per workgroup, 16, 32 or 64; 0 = the default, 16. Outside the
// limits *ran = 0 and nothing is launched (the caller runs ln_fwd and the
// two gemm_nt calls instead). xln may be null.
hipError_t fv_extractor_head_fwd(const float* x, const float* gamma,
                                 const float* beta, const float* W1x,
                                 const float* b1x, const float* Wih,
                                 const float* bih, float* xln, float* mean,
                                 float* rstd, float* xp, float* gi, long R,
                                 int C, int G, float eps, int strip,
                                 int* ran, hipStream_t stream) {
  *ran = 0;
  if (strip == 0) strip = 16;  // fastest measured (profiles/f32_head.md)
  if (strip != 16 && strip != 32 && strip != 64) return hipErrorInvalidValue;
  if (R < 1 || C < 1 || C > 16 * EH_CT_MAX || G < 1 || G > 16 * EH_CT_MAX)
    return hipSuccess;
  if ((R + strip - 1) / strip > 0x7fffffffL) return hipSuccess;
  const int KP = (C + EH_BK - 1) & ~(EH_BK - 1);
  const int ctm = ((C > G ? C : G) + 15) / 16;
  const size_t lds = sizeof(float) * ((size_t)strip * (KP + 2) +
                                      2 * (size_t)16 * ctm * EH_WLD);
  if (lds > 160 * 1024) return hipSuccess;
  hipError_t e;
  if (strip == 16)
    e = eh_launch<16>(x, gamma, beta, W1x, b1x, Wih, bih, xln, mean, rstd, xp,
                      gi, R, C, G, eps, lds, stream);
  else if (strip == 32)
    e = eh_launch<32>(x, gamma, beta, W1x, b1x, Wih, bih, xln, mean, rstd, xp,
                      gi, R, C, G, eps, lds, stream);
  else
    e = eh_launch<64>(x, gamma, beta, W1x, b1x, Wih, bih, xln, mean, rstd, xp,
                      gi, R, C, G, eps, lds, stream);
  if (e == hipSuccess) *ran = 1;
  return e;
}

// row chunks of fv_ln_bwd_params; `part` holds 2C floats for each
int fv_ln_bwd_yblocks(long R, int C) {
  long rpb;
  return (int)ln_bwd_geometry(R, C, &rpb);
}

int fv_ln_bwd_rows(long R, int C) {
  long rpb;
  ln_bwd_geometry(R, C, &rpb);
  return (int)rpb;
}

hipError_t fv_ln_bwd_reduce(const float* part, float* dgamma, float* dbeta,
                            long R, int C, hipStream_t stream) {
  long rpb;
  const unsigned yblocks = ln_bwd_geometry(R, C, &rpb);
  hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((2 * C + 3) / 4),
                     dim3(256), 0, stream, part, dgamma, dbeta,
                     (int)yblocks, C);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_ln_bwd_params(const float* x, const float* dxln,
                            const float* mean, const float* rstd,
                            float* part, float* dgamma, float* dbeta,
                            long R, int C, int r_chunks,
                            hipStream_t stream) {
  (void)r_chunks;
  const int cblocks = (C + 63) / 64;
  long rpb;
  const unsigned yblocks = ln_bwd_geometry(R, C, &rpb);
  dim3 grid(cblocks, yblocks);
  hipLaunchKernelGGL(ln_bwd_params_kernel, grid, dim3(256), 0, stream,
                     x, dxln, mean, rstd, part, R, C, (int)rpb);
  HIP_CHECK_LAST();
  hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((2 * C + 3) / 4),
                     dim3(256), 0, stream, part, dgamma, dbeta,
                     (int)yblocks, C);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
