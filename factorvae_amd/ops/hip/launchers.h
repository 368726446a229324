// Prototypes of every extern "C" launcher, declared once. Each .hip file
// includes this header, so a definition that disagrees with its prototype
// fails to compile; bindings.cpp calls the launchers through it.
// A declaration file and nothing else.
#pragma once

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

// ---- gemm.hip ---------------------------------------------------------
hipError_t fv_gemm_nt(const float* A, const float* W, const float* bias,
                      float* out, int R, int Ci, int Co, float alpha,
                      int accumulate, int act_lrelu, hipStream_t stream);
hipError_t fv_gemm_nn(const float* A, const float* B, const float* bias,
                      float* out, int R, int Ci, int Co, float alpha,
                      int accumulate, int act_lrelu, const float* lrelu_bwd_of,
                      int variant, hipStream_t stream);
// the dxln GEMM with fv_ln_bwd_params' partials as its only output; *ran = 0
// (nothing launched) unless fv_ln_bwd_rows(R, C) is 64
hipError_t fv_gemm_nn_ln(const float* A, const float* B, const float* x,
                         const float* mean, const float* rstd, float* part,
                         long R, int Ci, int C, float alpha, int* ran,
                         hipStream_t stream);
hipError_t fv_gemm_tn(const float* A, const float* B, float* out, float* part,
                      float* db, float* db_part, int R, int M, int N,
                      int r_chunks, int accumulate, int variant, int reduce,
                      hipStream_t stream);
hipError_t fv_gemm_tn_pair(const float* A0, const float* B0, float* out0,
                           float* part0, float* db0, float* db_part0, int N0,
                           const float* A1, const float* B1, float* out1,
                           float* part1, float* db1, float* db_part1, int N1,
                           int R, int M, int r_chunks, int accumulate,
                           int variant, int reduce, hipStream_t stream);
hipError_t fv_tn_reduce_list(int n, const float* const* part,
                             float* const* out, const float* const* db_part,
                             float* const* db, const int* M, const int* N,
                             int z, int accumulate, hipStream_t stream);
// number of R slices fv_gemm_tn_xhat writes
int fv_tn_xhat_slices(int R);
hipError_t fv_gemm_tn_xhat(const float* A, const float* x, const float* mean,
                           const float* rstd, float* part, float* db_part,
                           int R, int M, int N, int variant,
                           hipStream_t stream);
hipError_t fv_ln_w1x_finish(const float* part, const float* db_part,
                            const float* W1x, const float* gamma,
                            const float* beta, float* gW1x, float* gb1x,
                            float* dgamma, float* dbeta, int C, int nz,
                            hipStream_t stream);
hipError_t fv_colsum(const float* A, float* out, int R, int C, int r_chunks,
                     hipStream_t stream);
hipError_t fv_lrelu_bwd(const float* dY, const float* Y, float* dZ, long total,
                        hipStream_t stream);

// ---- gemm_bf16.hip ----------------------------------------------------
hipError_t fv_gemm_nt_bf16(const void* A, const void* W, const float* bias,
                           float* out_f32, void* out_bf16, int R, int Ci,
                           int Co, float alpha, int accumulate, int act_lrelu,
                           hipStream_t stream);
hipError_t fv_gemm_nn_bf16(const void* A, const void* B, const float* bias,
                           float* out_f32, void* out_bf16, const void* Y,
                           int R, int Ci, int Co, float alpha, int accumulate,
                           int act_lrelu, hipStream_t stream);
hipError_t fv_gemm_tn_bf16(const void* A, const void* B, float* out,
                           float* part, float* db, float* db_part, int R,
                           int M, int N, int r_chunks, int accumulate,
                           hipStream_t stream);
hipError_t fv_gemm_nt_bf16_rs(const void* A, const void* Wp, const float* bias,
                              float* out_f32, void* out_bf16, const void* Y,
                              int R, int Ci, int Co, int KP, float alpha,
                              int act_lrelu, hipStream_t stream);
hipError_t fv_cast_shadows(const float* s1, void* d1, void* d1t, int M1,
                           int N1, int KPn1, int KPm1, const float* s2,
                           void* d2, void* d2t, int M2, int N2, int KPn2,
                           int KPm2, const float* s3, void* d3, long n3,
                           hipStream_t stream);
hipError_t fv_wgrad_reduce(const float* part, float* out, long elems,
                           const float* db_part, float* db, long m_elems,
                           int z, int accumulate, hipStream_t stream);
hipError_t fv_cast_f32_bf16(const float* src, void* dst, long n,
                            hipStream_t stream);
hipError_t fv_lrelu_bwd_bf16(const void* dY, const void* Y, void* dZ,
                             long total, hipStream_t stream);

// ---- fp8.hip ----------------------------------------------------------
hipError_t fv_gemm_nt_fp8(const void* A, const void* W, const float* bias,
                          const float* inv_sw, float* out_f32, void* out_bf16,
                          void* out_fp8, int ldo, int R, int Ci, int Co,
                          int lda, int ldw, float alpha, int act_lrelu,
                          int has_bias, hipStream_t stream);
hipError_t fv_gemm_nt_fp8_rs(const void* A, const void* Wp, const float* bias,
                             const float* inv_sw, const float* inv_sa,
                             const void* Y, const float* s_out,
                             float* amax_out, float* out_f32, void* out_bf16,
                             void* out_fp8, int ldo, int R, int Ci, int Co,
                             int KP, float alpha, int act_lrelu, int has_bias,
                             hipStream_t stream);
hipError_t fv_scale_from_amax2(float* amax1, float* s1, float* is1,
                               float* amax2, float* s2, float* is2,
                               hipStream_t stream);
hipError_t fv_cast_f32_fp8_damax(const float* src, void* dst, const float* s,
                                 float* amax_out, long rows, int cols, int ldp,
                                 hipStream_t stream);
hipError_t fv_cast_f32_fp8_scaled_t(const float* src, void* dstT,
                                    const float* scale, int M, int N, int ldp,
                                    hipStream_t stream);
hipError_t fv_absmax_scale(const float* src, long n, float* scale,
                           float* inv_scale, hipStream_t stream);
hipError_t fv_cast_f32_fp8_scaled(const float* src, void* dst,
                                  const float* scale, long rows, int cols,
                                  int ldp, hipStream_t stream);

// ---- extractor.hip ----------------------------------------------------
hipError_t fv_ln_fwd(const float* x, const float* gamma, const float* beta,
                     float* xln, void* xln_bf, void* xln_f8, int f8_ld,
                     float* mean, float* rstd, long R, int C, float eps,
                     hipStream_t stream);
hipError_t fv_extractor_head_fwd(const float* x, const float* gamma,
                                 const float* beta, const float* W1x,
                                 const float* b1x, const float* Wih,
                                 const float* bih, float* xln, float* mean,
                                 float* rstd, float* xp, float* gi, long R,
                                 int C, int G, float eps, int strip, int* ran,
                                 hipStream_t stream);
// row chunks of fv_ln_bwd_params; `part` holds 2C floats for each
int fv_ln_bwd_yblocks(long R, int C);
// rows per row chunk of fv_ln_bwd_params
int fv_ln_bwd_rows(long R, int C);
hipError_t fv_ln_bwd_params(const float* x, const float* dxln,
                            const float* mean, const float* rstd, float* part,
                            float* dgamma, float* dbeta, long R, int C,
                            int r_chunks, hipStream_t stream);
// the second kernel of fv_ln_bwd_params alone: dgamma, dbeta from the
// partials of fv_ln_bwd_yblocks(R, C) row chunks
hipError_t fv_ln_bwd_reduce(const float* part, float* dgamma, float* dbeta,
                            long R, int C, hipStream_t stream);

// ---- gru.hip ----------------------------------------------------------
// variant 1: at H == 64, fp32 outputs only and N <= fv_gru_wave_max_n() the
// wave-per-stock kernels of gru_wave.hip; 0: the kernels from before them.
// Both give the same bits.
hipError_t fv_gru_fwd(const float* gi, const float* Whh, const float* bhh,
                      float* h_final, float* h_seq, float* h_prev,
                      float* gates4, int N, int T, int H, int variant,
                      hipStream_t stream);
hipError_t fv_gru_fwd_infer(const float* gi, const float* Whh,
                            const float* bhh, float* h_final, int N, int T,
                            int H, int variant, hipStream_t stream);
hipError_t fv_gru_bwd(const float* dh_final, const float* h_prev,
                      const float* gates4, const float* Whh, float* dgi,
                      float* dgh, void* dgi_bf, void* dgh_bf, int N, int T,
                      int H, int variant, hipStream_t stream);
// fv_dh_combine and fv_gru_bwd in one launch where fv_gru_bwd would take the
// wave kernel (fp32 outputs); otherwise *fused = 0 and nothing is launched
hipError_t fv_gru_bwd_combine(float* dh, const float* ds, const float* qk,
                              const float* a, const float* du,
                              const float* dscores, const float* Wenc, int K,
                              int M, const float* h_prev, const float* gates4,
                              const float* Whh, float* dgi, float* dgh, int N,
                              int T, int H, int variant, int* fused,
                              hipStream_t stream);
// The gather forms of the inference recurrences (gru_gather.h): gi_rows is
// (U,3H), idx (N,T) int32, and step t of stock n reads row idx[n*T + t]; an
// index outside [0,U) reads nothing and makes that stock's h_final NaN.
hipError_t fv_gru_fwd_infer_gather(const float* gi_rows, int U,
                                   const int* idx, const float* Whh,
                                   const float* bhh, float* h_final, int N,
                                   int T, int H, int variant,
                                   hipStream_t stream);

// ---- gru_wave.hip -----------------------------------------------------
// largest N at which fv_gru_fwd / _infer / _bwd take the wave kernels
int fv_gru_wave_max_n(void);
hipError_t fv_gru_fwd_wave_f32(const float* gi, const float* Whh,
                               const float* bhh, float* h_final, float* h_seq,
                               float* h_prev, float* gates4, int N, int T,
                               int H, hipStream_t stream);
hipError_t fv_gru_fwd_wave_f32_infer(const float* gi, const float* Whh,
                                     const float* bhh, float* h_final, int N,
                                     int T, int H, hipStream_t stream);
hipError_t fv_gru_fwd_wave_f32_infer_gather(const float* gi_rows, int U,
                                            const int* idx, const float* Whh,
                                            const float* bhh, float* h_final,
                                            int N, int T, int H,
                                            hipStream_t stream);
hipError_t fv_gru_bwd_wave_f32(const float* dh_final, const float* h_prev,
                               const float* gates4, const float* Whh,
                               float* dgi, float* dgh, int N, int T, int H,
                               hipStream_t stream);
hipError_t fv_gru_bwd_wave_f32_combine(float* dh, const float* ds,
                                       const float* qk, const float* a,
                                       const float* du, const float* dscores,
                                       const float* Wenc, int K, int M,
                                       const float* h_prev,
                                       const float* gates4, const float* Whh,
                                       float* dgi, float* dgh, int N, int T,
                                       int H, hipStream_t stream);

// ---- gru_mfma.hip -----------------------------------------------------
// number of workgroups fv_gru_bwd_mfma launches, one wgrad partial each
int fv_gru_wgrad_blocks(int N);
hipError_t fv_gru_fwd_mfma(const float* gi, const void* whh_bf,
                           const float* bhh, float* h_final, float* h_seq,
                           float* h_prev, float* gates4, int N, int T, int H,
                           hipStream_t stream);
hipError_t fv_gru_fwd_mfma_f32(const float* gi, const float* Whh,
                               const float* bhh, float* h_final, float* h_seq,
                               float* h_prev, float* gates4, int N, int T,
                               int H, hipStream_t stream);
hipError_t fv_gru_fwd_mfma_infer(const float* gi, const void* whh_bf,
                                 const float* bhh, float* h_final, int N,
                                 int T, int H, hipStream_t stream);
hipError_t fv_gru_fwd_mfma_f32_infer(const float* gi, const float* Whh,
                                     const float* bhh, float* h_final, int N,
                                     int T, int H, hipStream_t stream);
hipError_t fv_gru_fwd_mfma_infer_gather(const float* gi_rows, int U,
                                        const int* idx, const void* whh_bf,
                                        const float* bhh, float* h_final,
                                        int N, int T, int H,
                                        hipStream_t stream);
hipError_t fv_gru_fwd_mfma_f32_infer_gather(const float* gi_rows, int U,
                                            const int* idx, const float* Whh,
                                            const float* bhh, float* h_final,
                                            int N, int T, int H,
                                            hipStream_t stream);
hipError_t fv_gru_bwd_mfma_f32(const float* dh_final, const float* h_prev,
                               const float* gates4, const float* Whh,
                               float* dgi, float* dgh, int N, int T, int H,
                               hipStream_t stream);
hipError_t fv_gru_bwd_mfma(const float* dh_final, const float* h_prev,
                           const float* gates4, const void* whh_bf, float* dgi,
                           float* dgh, void* dgi_bf, void* dgh_bf,
                           void* dgi_f8, int ld8, const float* s_dgi,
                           float* amax_dgi, float* whh_part, float* bhh_part,
                           int N, int T, int H, hipStream_t stream);

// ---- encoder.hip ------------------------------------------------------
hipError_t fv_enc_bwd_fused(const float* dfmu, const float* dfsig_c,
                            const float* fsig, const float* fsig_pre,
                            const float* yp, const float* Wmu,
                            const float* Wsig, const float* a, const float* y,
                            float* dscores, float* dWmu, float* dbmu,
                            float* dWsig, float* dbsig, int N, int M, int K,
                            hipStream_t s);
hipError_t fv_enc_bwd_mid(const float* part, const float* fmu,
                          const float* fsig_c, const float* pmu,
                          const float* psig_c, const float* fsig,
                          const float* fsig_pre, const float* yp,
                          const float* Wmu, const float* Wsig, const float* a,
                          const float* y, float* dscores, float* dWmu,
                          float* dbmu, float* dWsig, float* dbsig, float* dfmu,
                          float* dfsig_c, int nblk, int N, int M, int K,
                          float gscale, hipStream_t s);
hipError_t fv_enc_fused_fwd(const float* h, const float* Wenc,
                            const float* benc, const float* y, float* scores,
                            float* a, float* yp, const float* Wmu,
                            const float* bmu, const float* Wsig,
                            const float* bsig, float* fmu, float* fsig_pre,
                            float* fsig, float* fsig_c, int* done, int K,
                            int N, int M, int H, int variant, hipStream_t s);
hipError_t fv_enc_softmax_fwd(const float* scores, const float* y, float* a,
                              float* yp, int N, int M, hipStream_t stream);
hipError_t fv_enc_softmax_bwd(const float* dyp, const float* a, const float* y,
                              float* dscores, int N, int M,
                              hipStream_t stream);
hipError_t fv_enc_heads_fwd(const float* yp, const float* Wmu,
                            const float* bmu, const float* Wsig,
                            const float* bsig, float* fmu, float* fsig_pre,
                            float* fsig, float* fsig_c, int M, int K,
                            hipStream_t stream);
hipError_t fv_enc_heads_bwd(const float* dfmu, const float* dfsig_c,
                            const float* fsig, const float* fsig_pre,
                            const float* yp, const float* Wmu,
                            const float* Wsig, float* dyp, float* dWmu,
                            float* dbmu, float* dWsig, float* dbsig, int M,
                            int K, hipStream_t stream);

// ---- attention.hip ----------------------------------------------------
hipError_t fv_dh_combine(float* dh, const float* ds, const float* qk,
                         const float* a, const float* du, const float* dscores,
                         const float* Wenc, int N, int K, int M, int H,
                         hipStream_t s);
hipError_t fv_attn_fused_bwd(const float* dpmu, const float* dpsig_c,
                             const float* psig, const float* psig_pre,
                             const float* hm2, const float* wmu,
                             const float* wsig, const float* Wl,
                             const float* h, const float* a, const float* sd,
                             const float* mask, const int* guard,
                             const float* u, const float* Wv, const float* q,
                             const float* Wk, const float* bk, float* dz2,
                             float* du, float* ds, float* dc, float* dWv,
                             float* dbv, float* dq, float* dWk, float* dbk,
                             float* hpart, float* dwmu, float* dbmu,
                             float* dwsig, float* dbsig, int N, int K, int H,
                             float alpha, float keep_inv, int variant,
                             const float* kl_fmu, const float* kl_fsig_c,
                             const float* kl_pmu, const float* kl_psig_c,
                             float kl_gscale, hipStream_t s);
// the reduce fv_attn_fused_bwd / fv_pred_mlp_bwd end with, on its own
hipError_t fv_pred_head_reduce(const float* hpart, float* dwmu, float* dbmu,
                               float* dwsig, float* dbsig, int K, int H,
                               hipStream_t s);
hipError_t fv_attn_fused_fwd(const float* h, const float* qk, const float* cb,
                             const float* mask, const float* Wv,
                             const float* bv, const float* Wl, const float* bl,
                             const float* wmu, const float* bmu,
                             const float* wsig, const float* bsig, float* a,
                             float* sd, int* guard, float* u, float* ctx,
                             float* hm2, float* pmu, float* psig_pre,
                             float* psig, float* psig_c, int N, int K, int H,
                             float alpha, float keep_inv, int variant,
                             hipStream_t s);
hipError_t fv_attn_qk_fwd(const float* q, const float* Wk, const float* bk,
                          float* qk, float* c, int K, int H, hipStream_t s);
hipError_t fv_attn_softmax_fwd(const float* sc, const float* mask, float* a,
                               float* sd, int* guard, int N, int K,
                               float keep_inv, hipStream_t s);
hipError_t fv_attn_ctx_fwd(const float* u, const float* Wv, const float* bv,
                           const int* guard, float* ctx, int K, int H,
                           hipStream_t s);
hipError_t fv_attn_head_bwd(const float* dctx, const float* u, const float* Wv,
                            const int* guard, float* du, float* dWv,
                            float* dbv, int K, int H, hipStream_t s);
hipError_t fv_attn_softmax_bwd(const float* da, const float* a,
                               const float* sd, const float* mask,
                               const int* guard, float* ds, float* dc, int N,
                               int K, float keep_inv, float alpha,
                               hipStream_t s);
hipError_t fv_attn_qk_bwd(const float* dqk, const float* dc, const float* q,
                          const float* Wk, const float* bk, float* dq,
                          float* dWk, float* dbk, int K, int H, hipStream_t s);
hipError_t fv_pred_mlp_fwd(const float* ctx, const float* Wl, const float* bl,
                           const float* wmu, const float* bmu,
                           const float* wsig, const float* bsig, float* hm2,
                           float* pmu, float* psig_pre, float* psig,
                           float* psig_c, int K, int H, hipStream_t s);
hipError_t fv_pred_mlp_bwd(const float* dpmu, const float* dpsig_c,
                           const float* psig, const float* psig_pre,
                           const float* hm2, const float* wmu,
                           const float* wsig, float* dz2, float* hpart,
                           float* dwmu, float* dbmu, float* dwsig,
                           float* dbsig, int K, int H, hipStream_t s);

// ---- decoder.hip ------------------------------------------------------
// number of workgroups the decoder backward launches for N rows; each
// writes one (2K + 2H + 2)-float partial
int fv_dec_nblk(int N);
hipError_t fv_dec_fwd_bwd(const float* h, const float* W1, const float* b1,
                          const float* wmu, const float* bmu,
                          const float* wsig, const float* bsig,
                          const float* Wb, const float* bb, const float* fmu,
                          const float* fsig_c, const float* eps,
                          const float* y, float* recon, float* a1, float* beta,
                          float* asig_pre, float* sigma, float* drecon,
                          float* dh, float* dz1, float* dbeta, float* part,
                          int N, int K, int H, float gscale, hipStream_t s);
hipError_t fv_dec_bwd_reduce_heads(const float* part, float* dwmu,
                                   float* dbmu, float* dwsig, float* dbsig,
                                   int N, int K, int H, hipStream_t s);
hipError_t fv_dec_fwd(const float* h, const float* W1, const float* b1,
                      const float* wmu, const float* bmu, const float* wsig,
                      const float* bsig, const float* Wb, const float* bb,
                      const float* fmu, const float* fsig_c, const float* eps,
                      float* recon, float* a1, float* beta, float* asig_pre,
                      float* sigma, int N, int K, int H, hipStream_t s);
hipError_t fv_dec_bwd(const float* drecon, const float* h, const float* a1,
                      const float* beta, const float* asig_pre,
                      const float* sigma, const float* eps, const float* fmu,
                      const float* fsig_c, const float* W1, const float* wmu,
                      const float* wsig, const float* Wb, float* dh,
                      float* dz1, float* dbeta, float* part, float* dfmu,
                      float* dfsig_c, float* dwmu, float* dbmu, float* dwsig,
                      float* dbsig, int N, int K, int H, hipStream_t s);

// ---- mid_fuse.hip (the fused middle, docs/KERNELS.md) ------------------
// fv_attn_fused_fwd and fv_enc_fused_fwd (with the heads) as one launch;
// fv_attn_fused_bwd's kernel (KL-gradient form, without its
// pred_head_reduce) and fv_dec_fwd_bwd as one launch. Latency-oriented
// variants only: N <= 384, H <= 64 a multiple of 4, K <= 128, LDS within
// 160 KiB. Otherwise *ran = 0 and nothing is launched.
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
    int M, int H, float alpha, float keep_inv, int* ran, hipStream_t s);
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
    float alpha, float keep_inv, float gscale, int* ran, hipStream_t s);

// ---- loss.hip ---------------------------------------------------------
hipError_t fv_loss_fused(const float* recon, const float* y, const float* fmu,
                         const float* fsig_c, const float* pmu,
                         const float* psig_c, float* loss, float* mse,
                         float* kl, float* drecon, float* dfmu,
                         float* dfsig_c, float* dpmu, float* dpsig_c, int N,
                         int K, float gscale, hipStream_t s);
hipError_t fv_loss_scalars(const float* recon, const float* y,
                           const float* fmu, const float* fsig_c,
                           const float* pmu, const float* psig_c, float* loss,
                           float* mse, float* kl, int N, int K, hipStream_t s);

// ---- predict.hip (batched multi-day scoring) --------------------------
hipError_t fv_attn_seg_fwd(const float* h, const int* seg_off, const float* qk,
                           const float* cb, const float* Wv, const float* bv,
                           const float* Wl, const float* bl, const float* wmu,
                           const float* bmu, const float* wsig,
                           const float* bsig, float* pmu, float* psig_c,
                           int* guard, int total, int D, int max_n, int K,
                           int H, float alpha, hipStream_t s);
hipError_t fv_dec_seg_fwd(const float* h, const int* seg_off, const float* W1,
                          const float* b1, const float* wmu, const float* bmu,
                          const float* wsig, const float* bsig,
                          const float* Wb, const float* bb, const float* fmu,
                          const float* fsig_c, const float* eps, float* mu,
                          float* sigma, float* sample, float* beta,
                          float* svar, int N, int D, int K, int H,
                          hipStream_t s);

// ---- posterior.hip ----------------------------------------------------
hipError_t fv_enc_seg_fwd(const float* h, const int* seg_off,
                          const float* Wenc, const float* benc,
                          const float* y, float* yp, int total, int D,
                          int max_n, int M, int H, hipStream_t s);
hipError_t fv_enc_seg_heads(const float* yp, const float* Wmu,
                            const float* bmu, const float* Wsig,
                            const float* bsig, float* fmu, float* fsig_c,
                            int D, int M, int K, hipStream_t s);
hipError_t fv_loss_seg(const float* recon, const float* y, const int* seg_off,
                       const float* fmu, const float* fsig_c,
                       const float* pmu, const float* psig_c, float* loss,
                       float* mse, float* kl, int total, int D, int K,
                       hipStream_t s);

// ---- risk.hip (factor risk model of the prior decoder) -----------------
hipError_t fv_risk_seg(const float* beta, const float* svar, const float* mu,
                       const float* w, const int* seg_off, const float* pmu,
                       const float* psig_c, float* stats, float* exposure,
                       float* factor_var, float* mcr, int total, int D, int K,
                       hipStream_t s);
hipError_t fv_risk_solve_seg(const float* beta, const float* svar,
                             const int* seg_off, const float* psig_c,
                             const float* b, float* x, int* info,
                             float* norms, int total, int D, int K, int R,
                             hipStream_t s);

// ---- metrics.hip ------------------------------------------------------
hipError_t fv_daily_ic_seg(const float* pred, long ld, const float* label,
                           const int* seg_off, double* stats, int* count,
                           int total, int D, int P, int max_n, int topk,
                           hipStream_t s);

// ---- adam.hip ---------------------------------------------------------
hipError_t fv_step_inc(int* step_t, hipStream_t s);
hipError_t fv_adam(float* p, const float* g, float* m, float* v,
                   const int* step_t, long total, float lr0, float eta_min,
                   float t_max, float beta1, float beta2, float eps,
                   hipStream_t s);

#ifdef __cplusplus
}
#endif
