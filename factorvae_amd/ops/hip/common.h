// Common device helpers for the FactorVAE CDNA4 (gfx950) kernels.
// Plain HIP, fp32 compute. Wave width on CDNA4 is 64 (not 32).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#define WAVE 64
#define DEVINL __device__ __forceinline__

DEVINL float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

// fast tanh via __expf (same fast-math family as sigmoidf_ above; the
// libm tanhf lowers to a multi-branch ocml path that dominates the
// GRU's per-step latency chain). Computed on |x| so the exp never
// overflows; ~2 ulp of __expf, well inside the GRU parity tolerances.
DEVINL float tanhf_(float x) {
  const float ax = fabsf(x);
  const float t = __expf(-2.0f * ax);
  const float r = (1.0f - t) / (1.0f + t);
  return copysignf(r, x);
}

// softplus matching torch.nn.functional.softplus (beta=1, threshold=20)
DEVINL float softplusf_(float x) {
  return x > 20.0f ? x : log1pf(__expf(x));
}
// d/dx softplus = sigmoid(x); for x>20 torch's threshold makes it identity (grad 1)
DEVINL float softplus_gradf_(float x) {
  return x > 20.0f ? 1.0f : sigmoidf_(x);
}

// fp32 -> OCP e4m3 (saturating), shared by the fp8 kernels
DEVINL unsigned char f32_to_e4m3_(float x) {
  unsigned int v = 0;
  v = __builtin_amdgcn_cvt_pk_fp8_f32(x, 0.0f, v, false);
  return (unsigned char)(v & 0xff);
}

DEVINL float lrelu_(float x) { return x > 0.0f ? x : 0.01f * x; }
DEVINL float lrelu_grad_from_out_(float y) { return y > 0.0f ? 1.0f : 0.01f; }

// full-wave reduction (64 lanes)
DEVINL float wave_reduce_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;  // valid in lane 0
}
DEVINL float wave_reduce_max(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
  return v;
}

// block reduction over up to 1024 threads; result valid in thread 0.
// `scratch` must hold >= blockDim.x/64 floats. Includes trailing barrier so
// scratch can be reused after a broadcast read.
template <typename Op>
DEVINL float block_reduce(float v, float* scratch, Op op, float init) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, 64));
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = init;
  if (wid == 0) {
    float x = (lane < nw) ? scratch[lane] : init;
    for (int off = 32; off > 0; off >>= 1) x = op(x, __shfl_down(x, off, 64));
    if (lane == 0) scratch[0] = x;
  }
  __syncthreads();
  r = scratch[0];
  __syncthreads();
  return r;
}

struct SumOp { DEVINL float operator()(float a, float b) const { return a + b; } };
struct MaxOp { DEVINL float operator()(float a, float b) const { return fmaxf(a, b); } };

DEVINL float block_reduce_sum(float v, float* scratch) {
  return block_reduce(v, scratch, SumOp{}, 0.0f);
}
DEVINL float block_reduce_max(float v, float* scratch) {
  return block_reduce(v, scratch, MaxOp{}, -INFINITY);
}

// a + b as its own rounding step: never contracted with a multiply that
// produced a or b. Used where the original sequence stored the product
// to memory and added to it in a later kernel.
DEVINL float add_rn_(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// The four KL input-gradients of one factor, exactly loss_fused_kernel's
// expressions (loss.hip), for consumers that form them in place. Compiled
// without contraction: loss_fused_kernel rounds both squares of
// fs*fs + dmu*dmu before it adds them (the compiler pairs the two
// multiplies into one packed instruction there), and nothing else in
// these expressions has a multiply feeding an add.
struct KlGrad {
  float dfmu, dfsig_c, dpmu, dpsig_c;
};
DEVINL KlGrad kl_grad_(float fm, float fs, float pm, float ps, float gscale) {
#pragma clang fp contract(off)
  const float dmu = fm - pm;
  const float ps2 = ps * ps;
  KlGrad g;
  g.dfmu = gscale * dmu / ps2;
  g.dfsig_c = gscale * (-1.0f / fs + fs / ps2);
  g.dpmu = gscale * (-dmu / ps2);
  g.dpsig_c = gscale * (1.0f / ps - (fs * fs + dmu * dmu) / (ps2 * ps));
  return g;
}

// One lane's share of dec_bwd_reduce_kernel's fixed-order sum over the
// nblk block partials of one element: lane l takes partials l, l+64, ...
// into two accumulators; wave_reduce_sum of the result is the element's sum.
DEVINL float dec_part_lane_sum_(const float* __restrict__ pe, int nblk,
                                int lane) {
  float s0 = 0.f, s1 = 0.f;
  int z = lane;
  for (; z + 64 < nblk; z += 128) {
    s0 += pe[z];
    s1 += pe[z + 64];
  }
  if (z < nblk) s0 += pe[z];
  return s0 + s1;
}

#define HIP_CHECK_LAST()                                  \
  do {                                                      \
    hipError_t e_ = hipGetLastError();                      \
    if (e_ != hipSuccess) return e_;                        \
  } while (0)
