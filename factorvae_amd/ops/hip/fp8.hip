// fp8 (e4m3) forward path for the FactorVAE engine (gfx950) —
// BASELINE.json config 5: "fp8 weights+activations (CDNA4 fp8 MFMA)".
//
// Design: the FLOP-bound extractor forward GEMMs run on fp8 MFMA
// (v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulate) with e4m3 weights and
// activations; per-tensor weight scales (absmax -> 448 full-scale) are
// applied in the fp32 epilogue; activations are LN-normalized so they
// use unit scale. Backward runs on the bf16 kernels (the fp8 GEMMs also
// emit the bf16 activation copies backward needs). fp8 rows are padded
// to a multiple of 4 bytes so staging can use dword-coalesced loads.

#include "common.h"
#include "launchers.h"
#include <stdlib.h>

typedef __attribute__((ext_vector_type(4))) float f32x4;

#define FBR 64   // row tile
#define FBC 64   // col tile
#define FBK 64   // k tile (2 MFMA k-steps of 32)

union dw_f8 {
  unsigned int u;
  unsigned char b[4];
};

DEVINL unsigned char f32_to_e4m3(float x) {
  unsigned int v = 0;
  v = __builtin_amdgcn_cvt_pk_fp8_f32(x, 0.0f, v, false);
  return (unsigned char)(v & 0xff);
}

DEVINL float e4m3_to_f32(unsigned char b) {
  return __builtin_amdgcn_cvt_f32_fp8((unsigned int)b, 0);
}

// bounds-checked dword (4 fp8) load from a row-major padded matrix
DEVINL unsigned int load_dw_f8(const unsigned char* p, long row, int col0,
                               long nrows, int ncols, int ld) {
  if (row >= nrows) return 0u;
  const unsigned char* rp = p + row * (long)ld;
  if (col0 + 4 <= ncols) return *(const unsigned int*)(rp + col0);
  dw_f8 d;
  d.u = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    d.b[i] = (col0 + i < ncols) ? rp[col0 + i] : 0;
  return d.u;
}

// ---------------------------------------------------------------- NT
// out = act(alpha * sa*sb * (A(R,Ci)@W(Co,Ci)^T) + bias), A/W fp8 e4m3
// with padded leading dims lda/ldw (bytes). Outputs: fp32 and/or bf16
// and/or fp8 (fp8 out uses out scale so8, padded ldo).
__global__ __launch_bounds__(256) void gemm_nt_fp8_kernel(
    const unsigned char* __restrict__ A, const unsigned char* __restrict__ W,
    const float* __restrict__ bias, const float* __restrict__ inv_sw,
    float* __restrict__ out_f32, __bf16* __restrict__ out_bf16,
    unsigned char* __restrict__ out_fp8, int ldo,
    int R, int Ci, int Co, int lda, int ldw, float alpha, int flags) {
  __shared__ unsigned char As[2][FBR][FBK + 16];
  __shared__ unsigned char Ws[2][FBC][FBK + 16];

  const int r0 = blockIdx.x * FBR;
  const int c0 = blockIdx.y * FBC;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = tid >> 6;
  const int fi = lane & 15;
  const int fk = lane >> 4;       // k-group: 8 consecutive k each

  const int KD = FBK / 4;         // dwords per tile row (16)
  f32x4 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

  const int ktiles = (Ci + FBK - 1) / FBK;
  unsigned int pa[4], pw[4];

  auto stage_regs = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = tid + u * 256;
      const int row = idx / KD;
      const int cp = (idx % KD) * 4;
      pa[u] = load_dw_f8(A, (long)r0 + row, k0 + cp, R, Ci, lda);
      pw[u] = load_dw_f8(W, (long)c0 + row, k0 + cp, Co, Ci, ldw);
    }
  };
  auto regs_to_lds = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = tid + u * 256;
      const int row = idx / KD;
      const int cp = (idx % KD) * 4;
      *(unsigned int*)&As[buf][row][cp] = pa[u];
      *(unsigned int*)&Ws[buf][row][cp] = pw[u];
    }
  };

  stage_regs(0);
  regs_to_lds(0);

  for (int kt = 0; kt < ktiles; ++kt) {
    __syncthreads();
    if (kt + 1 < ktiles) stage_regs((kt + 1) * FBK);
    const int buf = kt & 1;
#pragma unroll
    for (int k32 = 0; k32 < FBK; k32 += 32) {
      const long a = *(const long*)&As[buf][wv * 16 + fi][k32 + fk * 8];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const long b = *(const long*)&Ws[buf][jt * 16 + fi][k32 + fk * 8];
        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, acc[jt],
                                                             0, 0, 0);
      }
    }
    if (kt + 1 < ktiles) {
      __syncthreads();
      regs_to_lds(1 - buf);
    }
  }

  const float sw = inv_sw ? *inv_sw : 1.0f;  // undo the weight scale
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    const int gc = c0 + jt * 16 + fi;
    if (gc >= Co) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int gr = r0 + wv * 16 + fk * 4 + rr;
      if (gr >= R) continue;
      float v = acc[jt][rr] * sw;
      if (flags & 4) v += bias[gc];
      v *= alpha;
      if (flags & 2) v = lrelu_(v);
      if (out_f32) out_f32[(long)gr * Co + gc] = v;
      if (out_bf16) out_bf16[(long)gr * Co + gc] = (__bf16)v;
      if (out_fp8) out_fp8[(long)gr * ldo + gc] = f32_to_e4m3(v);
    }
  }
}

// ------------------------------------------------- register-stationary
// MX-scaled NT (k <= 256): v_mfma_scale_f32_16x16x128_f8f6f4 at K=128 —
// the ONLY fp8 MFMA form that runs at the ~5 PF/s dense fp8 rate (the
// 16x16x32 form above runs at the bf16 rate; guide §4). Block scales
// are passed as unit (E8M0 bias 127): dequant stays the per-tensor fp32
// software scale in the epilogue, so numerics match the K=32 path
// exactly. Same wave-independent streaming structure as
// gemm_nt_bf16_rs: W block resident in registers, A rows ARE the
// fragments (32 k-contiguous fp8 bytes per lane), no LDS, no barriers.
// A and Wp must be row-padded to KP (multiple of 128) with ZEROS.
typedef __attribute__((ext_vector_type(8))) int i32x8;
#define FRSK 2  // max k128 groups (k <= 256)

// Extras for the fp8 DGRAD path (delayed per-tensor scaling):
// - inv_sa: the A operand's inverse scale (folded with inv_sw);
// - Y (flags bit3): multiply by lrelu'(Y) — fuses the activation
//   backward into the dgrad GEMM;
// - s_out: scale applied before the e4m3 out cast (the NEXT consumer's
//   operand scale);
// - amax_out: running |v| max of the true results, collected via
//   atomicMax (max is order-independent -> still deterministic); the
//   next step's scale_from_amax turns it into s/is.
template <int JT>
__global__ __launch_bounds__(256) void gemm_nt_fp8_rs_kernel(
    const unsigned char* __restrict__ A, const unsigned char* __restrict__ Wp,
    const float* __restrict__ bias, const float* __restrict__ inv_sw,
    const float* __restrict__ inv_sa, const __bf16* __restrict__ Y,
    const float* __restrict__ s_out, float* __restrict__ amax_out,
    float* __restrict__ out_f32, __bf16* __restrict__ out_bf16,
    unsigned char* __restrict__ out_fp8, int ldo, int R, int Ci, int Co,
    int KP, float alpha, int flags, int spw) {
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int fi = lane & 15;
  const int fk = lane >> 4;
  const int c0 = blockIdx.x * 64 + (JT == 2 ? (wv & 1) * 32 : 0);
  const int nk = KP >> 7;  // k128 groups

  i32x8 wfr[JT][FRSK];
#pragma unroll
  for (int jt = 0; jt < JT; ++jt) {
    const int gc = c0 + jt * 16 + fi;
#pragma unroll
    for (int k = 0; k < FRSK; ++k) {
      if (k < nk && gc < Co) {
        wfr[jt][k] = *(const i32x8*)&Wp[(long)gc * KP + k * 128 + fk * 32];
      } else {
        i32x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        wfr[jt][k] = z;
      }
    }
  }

  const int strips = (R + 15) >> 4;
  const int wslot = (JT == 2) ? (blockIdx.y * 2 + (wv >> 1))
                              : (blockIdx.y * 4 + wv);
  const int s0 = wslot * spw;
  const int s_end = min(s0 + spw, strips);
  if (s0 >= strips) return;

  auto loadA = [&](i32x8 (&fr)[FRSK], int s) {
    const long row = (long)s * 16 + fi;
    const bool live = row < R;
#pragma unroll
    for (int k = 0; k < FRSK; ++k) {
      if (k < nk && live) {
        fr[k] = *(const i32x8*)&A[row * KP + k * 128 + fk * 32];
      } else {
        i32x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        fr[k] = z;
      }
    }
  };
  float sw = inv_sw ? *inv_sw : 1.0f;
  if (inv_sa) sw *= *inv_sa;
  const float so = s_out ? *s_out : 1.0f;
  float amax_l = 0.0f;
  auto compute_store = [&](i32x8 (&fr)[FRSK], int s) {
    f32x4 acc[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) acc[jt] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < FRSK; ++k) {
      if (k < nk) {
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
          acc[jt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              fr[k], wfr[jt][k], acc[jt], 0, 0, 0, 127, 0, 127);
      }
    }
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
      const int gc = c0 + jt * 16 + fi;
      if (gc >= Co) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long gr = (long)s * 16 + fk * 4 + rr;
        if (gr >= R) continue;
        float v = acc[jt][rr] * sw;
        if (flags & 4) v += bias[gc];
        v *= alpha;
        if (flags & 2) v = lrelu_(v);
        if (flags & 8) {
          const float y = (float)Y[gr * Co + gc];
          v *= (y > 0.0f ? 1.0f : 0.01f);
        }
        if (amax_out) amax_l = fmaxf(amax_l, fabsf(v));
        if (out_f32) out_f32[gr * Co + gc] = v;
        if (out_bf16) out_bf16[gr * Co + gc] = (__bf16)v;
        if (out_fp8) out_fp8[gr * ldo + gc] = f32_to_e4m3(v * so);
      }
    }
  };

  i32x8 fr0[FRSK], fr1[FRSK];
  int s = s0;
  loadA(fr0, s);
  while (true) {
    if (s + 1 < s_end) loadA(fr1, s + 1);
    compute_store(fr0, s);
    if (++s >= s_end) break;
    if (s + 1 < s_end) loadA(fr0, s + 1);
    compute_store(fr1, s);
    if (++s >= s_end) break;
  }
  if (amax_out) {
    amax_l = wave_reduce_max(amax_l);
    if (lane == 0 && amax_l > 0.0f)
      atomicMax((int*)amax_out, __float_as_int(amax_l));
  }
}

// delayed-scaling bookkeeping for the two fp8 dgrad operands: turn the
// previous step's collected amax into (s = 448/amax, is = amax/448) and
// reset amax for this step's collection. One tiny launch per step.
__global__ void scale_from_amax2_kernel(
    float* __restrict__ amax1, float* __restrict__ s1, float* __restrict__ is1,
    float* __restrict__ amax2, float* __restrict__ s2,
    float* __restrict__ is2) {
  if (threadIdx.x == 0) {
    const float m1 = fmaxf(amax1[0], 1e-8f);
    s1[0] = 448.0f / m1;
    is1[0] = m1 / 448.0f;
    amax1[0] = 0.0f;
  } else if (threadIdx.x == 1) {
    const float m2 = fmaxf(amax2[0], 1e-8f);
    s2[0] = 448.0f / m2;
    is2[0] = m2 / 448.0f;
    amax2[0] = 0.0f;
  }
}

// dst_f8(R, ldp) = e4m3(src * s[0]) with fused running-amax collection
// of |src| (delayed scaling: s comes from the PREVIOUS step's amax).
__global__ __launch_bounds__(256) void cast_f32_fp8_damax_kernel(
    const float* __restrict__ src, unsigned char* __restrict__ dst,
    const float* __restrict__ s, float* __restrict__ amax_out, long rows,
    int cols, int ldp) {
  __shared__ float red[4];
  const float sc = s[0];
  float m = 0.0f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows * cols;
       i += (long)gridDim.x * 256) {
    const long r = i / cols;
    const int c = (int)(i % cols);
    const float v = src[i];
    m = fmaxf(m, fabsf(v));
    dst[r * (long)ldp + c] = f32_to_e4m3(v * sc);
  }
  m = wave_reduce_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m > 0.0f) atomicMax((int*)amax_out, __float_as_int(m));
  }
}

// transposed scaled cast: dstT(N, ldp) = e4m3(src(M,N)^T * scale[0])
__global__ __launch_bounds__(256) void cast_f32_fp8_scaled_t_kernel(
    const float* __restrict__ src, unsigned char* __restrict__ dstT,
    const float* __restrict__ scale, int M, int N, int ldp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long)M * N) {
    const int m = (int)(i / N), n = (int)(i % N);
    dstT[(long)n * ldp + m] = f32_to_e4m3(src[i] * scale[0]);
  }
}

// scale[0] = 448 / max(absmax(src), 1e-8): per-tensor e4m3 full-scale.
// Single workgroup (params are <=128k elements); deterministic.
__global__ __launch_bounds__(1024) void absmax_scale_kernel(
    const float* __restrict__ src, long n, float* __restrict__ scale,
    float* __restrict__ inv_scale) {
  __shared__ float red[16];
  float m = 0.0f;
  for (long i = threadIdx.x; i < n; i += 1024)
    m = fmaxf(m, fabsf(src[i]));
  m = wave_reduce_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    float mm = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) mm = fmaxf(mm, red[i]);
    mm = fmaxf(mm, 1e-8f);
    scale[0] = 448.0f / mm;
    inv_scale[0] = mm / 448.0f;
  }
}

// dst(rows, ldp bytes) = e4m3(src(rows, cols) * scale[0])
__global__ __launch_bounds__(256) void cast_f32_fp8_scaled_kernel(
    const float* __restrict__ src, unsigned char* __restrict__ dst,
    const float* __restrict__ scale, long rows, int cols, int ldp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long r = i / cols;
  const int c = (int)(i % cols);
  if (r < rows) {
    const float s = scale ? scale[0] : 1.0f;
    dst[r * (long)ldp + c] = f32_to_e4m3(src[r * (long)cols + c] * s);
  }
}

extern "C" {

hipError_t fv_gemm_nt_fp8(const void* A, const void* W, const float* bias,
                          const float* inv_sw, float* out_f32, void* out_bf16,
                          void* out_fp8, int ldo, int R, int Ci, int Co,
                          int lda, int ldw, float alpha, int act_lrelu,
                          int has_bias, hipStream_t stream) {
  int flags = (act_lrelu ? 2 : 0) | (has_bias ? 4 : 0);
  dim3 grid((R + FBR - 1) / FBR, (Co + FBC - 1) / FBC);
  hipLaunchKernelGGL(gemm_nt_fp8_kernel, grid, dim3(256), 0, stream,
                     (const unsigned char*)A, (const unsigned char*)W, bias,
                     inv_sw, out_f32, (__bf16*)out_bf16,
                     (unsigned char*)out_fp8, ldo, R, Ci, Co, lda, ldw,
                     alpha, flags);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_gemm_nt_fp8_rs(const void* A, const void* Wp,
                             const float* bias, const float* inv_sw,
                             const float* inv_sa, const void* Y,
                             const float* s_out, float* amax_out,
                             float* out_f32, void* out_bf16, void* out_fp8,
                             int ldo, int R, int Ci, int Co, int KP,
                             float alpha, int act_lrelu, int has_bias,
                             hipStream_t stream) {
  if (KP > 128 * FRSK || KP < Ci || (KP & 127)) return hipErrorInvalidValue;
  int flags = (act_lrelu ? 2 : 0) | (has_bias ? 4 : 0) | (Y ? 8 : 0);
  const int cblocks = (Co + 63) / 64;
  const int strips = (R + 15) / 16;
  // FV_RS_TGT: target wave count for the strip split (tuning knob;
  // default 4096 ~= 2 waves per SIMD slot)
  static int rs_tgt = 0;
  if (rs_tgt == 0) {
    const char* e = getenv("FV_RS_TGT");
    rs_tgt = (e && atoi(e) > 0) ? atoi(e) : 4096;
  }
  static int rs_jt = 0;
  if (rs_jt == 0) {
    const char* e2 = getenv("FV_RS_JT");
    rs_jt = (e2 && atoi(e2) == 4) ? 4 : 2;  // JT=2 measured faster
  }
  const int wps = (rs_jt == 2) ? 2 : 4;
  int spw = (strips * cblocks) / rs_tgt;
  if (spw < 1) spw = 1;
  const int yblocks = (strips + spw * wps - 1) / (spw * wps);
  dim3 grid(cblocks, yblocks);
  if (rs_jt == 2)
    hipLaunchKernelGGL(gemm_nt_fp8_rs_kernel<2>, grid, dim3(256), 0, stream,
                       (const unsigned char*)A, (const unsigned char*)Wp,
                       bias, inv_sw, inv_sa, (const __bf16*)Y, s_out,
                       amax_out, out_f32, (__bf16*)out_bf16,
                       (unsigned char*)out_fp8, ldo, R, Ci, Co, KP, alpha,
                       flags, spw);
  else
    hipLaunchKernelGGL(gemm_nt_fp8_rs_kernel<4>, grid, dim3(256), 0, stream,
                       (const unsigned char*)A, (const unsigned char*)Wp,
                       bias, inv_sw, inv_sa, (const __bf16*)Y, s_out,
                       amax_out, out_f32, (__bf16*)out_bf16,
                       (unsigned char*)out_fp8, ldo, R, Ci, Co, KP, alpha,
                       flags, spw);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_scale_from_amax2(float* amax1, float* s1, float* is1,
                               float* amax2, float* s2, float* is2,
                               hipStream_t stream) {
  hipLaunchKernelGGL(scale_from_amax2_kernel, dim3(1), dim3(64), 0, stream,
                     amax1, s1, is1, amax2, s2, is2);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_cast_f32_fp8_damax(const float* src, void* dst, const float* s,
                                 float* amax_out, long rows, int cols,
                                 int ldp, hipStream_t stream) {
  long blocks = (rows * cols + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(cast_f32_fp8_damax_kernel, dim3((unsigned)blocks),
                     dim3(256), 0, stream, src, (unsigned char*)dst, s,
                     amax_out, rows, cols, ldp);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_cast_f32_fp8_scaled_t(const float* src, void* dstT,
                                    const float* scale, int M, int N,
                                    int ldp, hipStream_t stream) {
  dim3 grid((unsigned)(((long)M * N + 255) / 256));
  hipLaunchKernelGGL(cast_f32_fp8_scaled_t_kernel, grid, dim3(256), 0,
                     stream, src, (unsigned char*)dstT, scale, M, N, ldp);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_absmax_scale(const float* src, long n, float* scale,
                           float* inv_scale, hipStream_t stream) {
  hipLaunchKernelGGL(absmax_scale_kernel, dim3(1), dim3(1024), 0, stream,
                     src, n, scale, inv_scale);
  HIP_CHECK_LAST();
  return hipSuccess;
}

hipError_t fv_cast_f32_fp8_scaled(const float* src, void* dst,
                                  const float* scale, long rows, int cols,
                                  int ldp, hipStream_t stream) {
  const long total = rows * cols;
  dim3 grid((unsigned)((total + 255) / 256));
  hipLaunchKernelGGL(cast_f32_fp8_scaled_kernel, grid, dim3(256), 0, stream,
                     src, (unsigned char*)dst, scale, rows, cols, ldp);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
