// The fused middle of the training step (FV_MID_FUSE, docs/KERNELS.md):
// kernels that ran side by side on two streams, because they do not depend
// on each other, as ONE launch each. A workgroup picks its role from its
// block index and runs that kernel's body (attn_mid.h, enc_mid.h,
// dec_mid.h) with the role-local index, so every element is computed by
// the separate kernels' own lines and comes out bit-identical.
//
//   mid_fwd  grid K + M      blocks 0..K-1    attn_fused_fwd_lat, head k
//                            blocks K..K+M-1  enc_fused_fwd_lat, portfolio m
//   mid_bwd  grid K + nblk   blocks 0..K-1    attn_fused_bwd_lat<KLG>, head k
//                            the rest         dec_fwd_bwd, block b - K of
//                                             nblk = fv_dec_nblk(N)
//
// The attention roles come first: they are the longer ones and the
// dispatcher hands out workgroups in index order.
//
// No role reads what the other role of the same launch writes:
//   mid_fwd  attention reads h, qk, cb, mask and the prior's parameters and
//            writes a, sd, guard, u, ctx, hm2, pmu, psig_pre, psig, psig_c;
//            the encoder reads h, y and its own parameters and writes
//            scores, a_enc, yp, fmu, fsig_pre, fsig, fsig_c and done.
//   mid_bwd  attention reads the forward's saved tensors above plus fmu,
//            fsig_c (mid_fwd's, a launch earlier) and writes dpmu, dpsig_c,
//            dz2, du, ds, dc, hpart and its parameter gradients; the
//            decoder reads h, fmu, fsig_c, eps, y and its own parameters
//            and writes recon, a1, beta, asig_pre, sigma, drecon, dh, dz1,
//            dbeta and its partials.
// No workgroup waits for another one. The only cross-workgroup protocol is
// the encoder's: the last of its M workgroups to arrive at the `done`
// counter goes on to the heads tail and resets the counter.
//
// The launch's dynamic LDS is the larger role's; the static __shared__ of
// both bodies (a few hundred bytes) coexists with it. VGPRs are the larger
// role's as well; at one workgroup per CU (the LDS footprint) that costs
// no occupancy.

#include "common.h"
#include "launchers.h"
#include "stage.h"
#include "attn_mid.h"
#include "dec_mid.h"
#include "enc_mid.h"

struct AttnFwdArgs {
  const float *h, *qk, *cb, *mask, *Wv, *bv, *Wl, *bl, *wmu, *bmu, *wsig,
      *bsig;
  float *a, *sd;
  int* guard;
  float *u, *ctx, *hm2, *pmu, *psig_pre, *psig, *psig_c;
  int N, K, H;
  float alpha, keep_inv;
};

struct EncFwdArgs {
  const float *h, *Wenc, *benc, *y;
  float *scores, *a, *yp;
  const float *Wmu, *bmu, *Wsig, *bsig;
  float *fmu, *fsig_pre, *fsig, *fsig_c;
  int* done;
  int K, N, M, H, img_floats;
};

struct AttnBwdArgs {
  const float *psig, *psig_pre, *hm2, *wmu, *wsig, *Wl, *h, *a, *sd, *mask;
  const int* guard;
  const float *u, *Wv, *q, *Wk, *bk;
  float *dz2, *du, *ds, *dc, *dWv, *dbv, *dq, *dWk, *dbk, *hpart;
  int N, K, H;
  float alpha, keep_inv;
  const float *kl_fmu, *kl_fsig_c, *kl_pmu, *kl_psig_c;
  float kl_gscale;
  float *dpmu, *dpsig_c;
};

struct DecArgs {
  const float *h, *W1, *b1, *wmu, *bmu, *wsig, *bsig, *Wb, *bb, *fmu,
      *fsig_c, *eps, *y;
  float *recon, *a1, *beta, *asig_pre, *sigma, *drecon, *dh, *dz1, *dbeta,
      *part;
  int N, K, H, iters, nblk;
  float gscale;
};

__global__ __launch_bounds__(256) void mid_fwd_kernel(AttnFwdArgs A,
                                                      EncFwdArgs E) {
  const int b = blockIdx.x;  // the role is uniform over the workgroup
  if (b < A.K)
    attn_fused_fwd_lat_body<true>(
        A.h, A.qk, A.cb, A.mask, A.Wv, A.bv, A.Wl, A.bl, A.wmu, A.bmu, A.wsig,
        A.bsig, A.a, A.sd, A.guard, A.u, A.ctx, A.hm2, A.pmu, A.psig_pre,
        A.psig, A.psig_c, A.N, A.K, A.H, A.alpha, A.keep_inv, b);
  else
    enc_fused_fwd_lat_body(E.h, E.Wenc, E.benc, E.y, E.scores, E.a, E.yp,
                           E.Wmu, E.bmu, E.Wsig, E.bsig, E.fmu, E.fsig_pre,
                           E.fsig, E.fsig_c, E.done, E.K, E.N, E.M, E.H,
                           E.img_floats, b - A.K);
}

__global__ __launch_bounds__(256) void mid_bwd_kernel(AttnBwdArgs A,
                                                      DecArgs D) {
  const int b = blockIdx.x;  // the role is uniform over the workgroup
  if (b < A.K)
    attn_fused_bwd_lat_body<true, true>(
        A.dpmu, A.dpsig_c, A.psig, A.psig_pre, A.hm2, A.wmu, A.wsig, A.Wl,
        A.h, A.a, A.sd, A.mask, A.guard, A.u, A.Wv, A.q, A.Wk, A.bk, A.dz2,
        A.du, A.ds, A.dc, A.dWv, A.dbv, A.dq, A.dWk, A.dbk, A.hpart, A.N, A.K,
        A.H, A.alpha, A.keep_inv, A.kl_fmu, A.kl_fsig_c, A.kl_pmu,
        A.kl_psig_c, A.kl_gscale, A.dpmu, A.dpsig_c, b);
  else
    dec_fwd_bwd_body(D.h, D.W1, D.b1, D.wmu, D.bmu, D.wsig, D.bsig, D.Wb,
                     D.bb, D.fmu, D.fsig_c, D.eps, D.y, D.recon, D.a1, D.beta,
                     D.asig_pre, D.sigma, D.drecon, D.dh, D.dz1, D.dbeta,
                     D.part, D.N, D.K, D.H, D.iters, D.gscale, b - A.K,
                     D.nblk);
}

// Dynamic plus static LDS of a launch stays within the CU's 160 KiB
#define MID_LDS_MAX (160 * 1024)
#define MID_LDS_STATIC 512

// what both roles of either launch accept: the latency-oriented variants
// (two rows per thread), the chain's N, H a multiple of 4 for the encoder's
// register rows, and the decoder's K
static inline bool mid_shape_ok(int N, int K, int M, int H) {
  return N >= 1 && N <= 384 && H >= 4 && H <= 64 && (H & 3) == 0 && K >= 1 &&
         K <= 128 && M >= 1;
}

// dynamic LDS above the 64 KiB default is opted into once per kernel; the
// runtime refuses a dynamic limit that, with the kernel's static LDS, would
// pass the CU's 160 KiB
static hipError_t mid_lds_opt_in(const void* kernel, bool* set) {
  if (*set) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(
      kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
      MID_LDS_MAX - MID_LDS_STATIC);
  if (e == hipSuccess) *set = true;
  return e;
}

extern "C" {

hipError_t fv_mid_fwd(
    const float* h, const float* qk, const float* cb, const float* mask,
    const float* Wv, const float* bv, const float* Wl, const float* bl,
    const float* wmu_p, const float* bmu_p, const float* wsig_p,
    const float* bsig_p, float* a_att, float* sd, int* guard, float* u,
    float* ctx, float* hm2, float* pmu, float* psig_pre, float* psig,
    float* psig_c, const float* Wenc, const float* benc, const float* y,
    float* scores, float* a_enc, float* yp, const float* Wmu_e,
    const float* bmu_e, const float* Wsig_e, const float* bsig_e, float* fmu,
    float* fsig_pre, float* fsig, float* fsig_c, int* done, int N, int K,
    int M, int H, float alpha, float keep_inv, int* ran, hipStream_t s) {
  *ran = 0;
  if (!mid_shape_ok(N, K, M, H)) return hipSuccess;
  // the two roles' footprints, as fv_attn_fused_fwd / fv_enc_fused_fwd
  // size them for the latency-oriented kernels
  const size_t lds_att = ((size_t)N * (H + 1) + N + 8 + 256 + 5 * 64 +
                          (size_t)H * (H + 1)) * sizeof(float);
  const size_t hs = (size_t)M + (size_t)2 * K * (M + 1);
  const size_t lds_enc = (hs + 8 + 64) * sizeof(float);
  const size_t lds = lds_att > lds_enc ? lds_att : lds_enc;
  if (lds + MID_LDS_STATIC > MID_LDS_MAX) return hipSuccess;
  static bool attr_set = false;
  hipError_t e = mid_lds_opt_in((const void*)mid_fwd_kernel, &attr_set);
  if (e != hipSuccess) return e;
  const AttnFwdArgs A = {h,  qk,  cb,   mask,     Wv,   bv,     Wl, bl,
                         wmu_p, bmu_p, wsig_p, bsig_p, a_att, sd, guard, u,
                         ctx, hm2, pmu, psig_pre, psig, psig_c, N,  K,
                         H,  alpha, keep_inv};
  const EncFwdArgs E = {h,    Wenc,   benc,     y,    scores, a_enc,
                        yp,   Wmu_e,  bmu_e,    Wsig_e, bsig_e, fmu,
                        fsig_pre, fsig, fsig_c, done, K,      N,
                        M,    H,      (int)hs};
  hipLaunchKernelGGL(mid_fwd_kernel, dim3(K + M), dim3(256), lds, s, A, E);
  HIP_CHECK_LAST();
  *ran = 1;
  return hipSuccess;
}

hipError_t fv_mid_bwd(
    const float* psig, const float* psig_pre, const float* hm2,
    const float* wmu_p, const float* wsig_p, const float* Wl, const float* h,
    const float* a_att, const float* sd, const float* mask, const int* guard,
    const float* u, const float* Wv, const float* q, const float* Wk,
    const float* bk, float* dz2, float* du, float* ds, float* dc, float* dWv,
    float* dbv, float* dq, float* dWk, float* dbk, float* hpart,
    const float* fmu, const float* fsig_c, const float* pmu,
    const float* psig_c, float* dpmu, float* dpsig_c, const float* W1,
    const float* b1, const float* wmu_d, const float* bmu_d,
    const float* wsig_d, const float* bsig_d, const float* Wb,
    const float* bb, const float* eps, const float* y, float* recon,
    float* a1, float* beta, float* asig_pre, float* sigma, float* drecon,
    float* dh, float* dz1, float* dbeta, float* part, int N, int K, int H,
    float alpha, float keep_inv, float gscale, int* ran, hipStream_t s) {
  *ran = 0;
  if (!mid_shape_ok(N, K, 1, H)) return hipSuccess;
  // fv_attn_fused_bwd's latency-oriented footprint and fv_dec_fwd_bwd's
  const size_t lds_att = ((size_t)N * (H + 1) + (size_t)H * (H + 1) + N + 8 +
                          256 + 7 * 64) * sizeof(float);
  const size_t lds_dec = dec_fwd_bwd_lds(K, H);
  const size_t lds = lds_att > lds_dec ? lds_att : lds_dec;
  if (lds + MID_LDS_STATIC > MID_LDS_MAX) return hipSuccess;
  static bool attr_set = false;
  hipError_t e = mid_lds_opt_in((const void*)mid_bwd_kernel, &attr_set);
  if (e != hipSuccess) return e;
  int iters, nblk;
  dec_bwd_geometry(N, &iters, &nblk);
  const AttnBwdArgs A = {psig, psig_pre, hm2,   wmu_p,  wsig_p, Wl,  h,
                         a_att, sd,      mask,  guard,  u,      Wv,  q,
                         Wk,   bk,       dz2,   du,     ds,     dc,  dWv,
                         dbv,  dq,       dWk,   dbk,    hpart,  N,   K,
                         H,    alpha,    keep_inv, fmu, fsig_c, pmu, psig_c,
                         gscale, dpmu,   dpsig_c};
  const DecArgs D = {h,     W1,    b1,    wmu_d,    bmu_d, wsig_d, bsig_d,
                     Wb,    bb,    fmu,   fsig_c,   eps,   y,      recon,
                     a1,    beta,  asig_pre, sigma, drecon, dh,    dz1,
                     dbeta, part,  N,     K,        H,     iters,  nblk,
                     gscale};
  hipLaunchKernelGGL(mid_bwd_kernel, dim3(K + nblk), dim3(256), lds, s, A, D);
  HIP_CHECK_LAST();
  *ran = 1;
  return hipSuccess;
}

}  // extern "C"
