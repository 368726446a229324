// Phase split of the fused attention / encoder kernels, original and
// latency-oriented, at one shape (default: the benchmark's N=300, H=64,
// K=20, M=128). The kernel files are compiled into this program with
// MID_STAMP defined, so thread 0 of workgroup 0 (the encoder's heads
// tail: thread 0 of the last workgroup) writes wall_clock64() (100 MHz)
// into a debug buffer at each phase boundary. The extension itself is
// built without the stamps.
//
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 \
//          scripts/probe/mid_phases.hip -o scripts/probe/mid_phases
// Run:   scripts/probe/mid_phases [N H K M]
// Prints, per kernel and variant, the median over the launches of each
// phase's length in us, and the event-timed time per launch of a
// back-to-back loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define MID_NSTAMP 8
__device__ long long mid_stamps[MID_NSTAMP];
#define MID_STAMP(i)                                               \
  do {                                                             \
    if (blockIdx.x == 0 && threadIdx.x == 0)                       \
      mid_stamps[i] = (long long)wall_clock64();                   \
  } while (0)
#define MID_STAMP_LAST(i)                                          \
  do {                                                             \
    if (threadIdx.x == 0) mid_stamps[i] = (long long)wall_clock64(); \
  } while (0)

#include "../../factorvae_amd/ops/hip/attention.hip"
#include "../../factorvae_amd/ops/hip/encoder.hip"

#define CK(x)                                                          \
  do {                                                                 \
    hipError_t e_ = (x);                                               \
    if (e_ != hipSuccess) {                                            \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__,                \
              hipGetErrorString(e_));                                  \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static float rnd() {  // uniform in [-1, 1)
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((rng_state >> 40) & 0xFFFFFF) / 8388608.0f - 1.0f;
}

static float* dev(size_t n, float scale) {
  std::vector<float> hst(n);
  for (auto& v : hst) v = rnd() * scale;
  float* d;
  CK(hipMalloc(&d, n * sizeof(float)));
  CK(hipMemcpy(d, hst.data(), n * sizeof(float), hipMemcpyHostToDevice));
  return d;
}

template <typename F>
static void measure(const char* name, int variant, const char* const* phase,
                    int nphase, F launch) {
  const int reps = 50;
  std::vector<std::vector<double>> len(nphase);
  for (int r = 0; r < reps; ++r) {
    launch();
    CK(hipDeviceSynchronize());
    long long st[MID_NSTAMP];
    CK(hipMemcpyFromSymbol(st, HIP_SYMBOL(mid_stamps), sizeof(st)));
    if (r < 10) continue;  // warm-up
    for (int p = 0; p < nphase; ++p)
      len[p].push_back((double)(st[p + 1] - st[p]) * 0.01);
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int loop = 200;
  CK(hipEventRecord(e0, 0));
  for (int r = 0; r < loop; ++r) launch();
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  float ms = 0.0f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  printf("%-14s variant %d: %6.2f us per launch back to back; phases:", name,
         variant, ms * 1000.0f / loop);
  double tot = 0.0;
  for (int p = 0; p < nphase; ++p) {
    std::sort(len[p].begin(), len[p].end());
    const double med = len[p][len[p].size() / 2];
    tot += med;
    printf("  %s %.2f", phase[p], med);
  }
  printf("  (sum %.2f)\n", tot);
}

int main(int argc, char** argv) {
  const int N = argc > 4 ? atoi(argv[1]) : 300;
  const int H = argc > 4 ? atoi(argv[2]) : 64;
  const int K = argc > 4 ? atoi(argv[3]) : 20;
  const int M = argc > 4 ? atoi(argv[4]) : 128;
  if (N < 1 || N > 384 || H < 1 || H > 64 || K < 1 || K > 256 || M < 1 ||
      M > 1024) {
    fprintf(stderr, "shape outside 1<=N<=384, H<=64, K<=256, M<=1024\n");
    return 1;
  }
  const float sH = 1.0f / sqrtf((float)H), sM = 1.0f / sqrtf((float)M);
  const float alpha = 1.0f / sqrtf((float)H + 1e-6f), keep_inv = 1.0f / 0.9f;
  printf("N=%d H=%d K=%d M=%d\n", N, H, K, M);

  float *h = dev((size_t)N * H, 1.0f), *qk = dev((size_t)K * H, sH),
        *cb = dev(K, 1.0f), *Wv = dev((size_t)K * H * H, sH),
        *bv = dev((size_t)K * H, 1.0f), *Wl = dev((size_t)H * H, sH),
        *bl = dev(H, 1.0f), *wmu = dev(H, sH), *bmu = dev(1, 1.0f),
        *wsig = dev(H, sH), *bsig = dev(1, 1.0f), *q = dev((size_t)K * H, 1.0f),
        *Wk = dev((size_t)K * H * H, sH), *bk = dev((size_t)K * H, 1.0f),
        *dpmu = dev(K, 1.0f), *dpsig_c = dev(K, 1.0f);
  std::vector<float> mh((size_t)N * K);
  for (auto& v : mh) v = rnd() > -0.8f ? 1.0f : 0.0f;
  float* mask;
  CK(hipMalloc(&mask, mh.size() * sizeof(float)));
  CK(hipMemcpy(mask, mh.data(), mh.size() * sizeof(float),
               hipMemcpyHostToDevice));
  // outputs (content irrelevant before the first launch)
  float *a = dev((size_t)N * K, 0.f), *sd = dev((size_t)N * K, 0.f),
        *u = dev((size_t)K * H, 0.f), *ctx = dev((size_t)K * H, 0.f),
        *hm2 = dev((size_t)K * H, 0.f), *pmu = dev(K, 0.f),
        *psig_pre = dev(K, 0.f), *psig = dev(K, 0.f), *psig_c = dev(K, 0.f);
  int* guard;
  CK(hipMalloc(&guard, K * sizeof(int)));
  float *dz2 = dev((size_t)K * H, 0.f), *du = dev((size_t)K * H, 0.f),
        *ds = dev((size_t)N * K, 0.f), *dc = dev(K, 0.f),
        *dWv = dev((size_t)K * H * H, 0.f), *dbv = dev((size_t)K * H, 0.f),
        *dq = dev((size_t)K * H, 0.f), *dWk = dev((size_t)K * H * H, 0.f),
        *dbk = dev((size_t)K * H, 0.f),
        *hpart = dev((size_t)K * (2 * H + 2), 0.f), *dwmu = dev(H, 0.f),
        *dbmu = dev(1, 0.f), *dwsig = dev(H, 0.f), *dbsig = dev(1, 0.f);
  // encoder
  float *Wenc = dev((size_t)M * H, sH), *benc = dev(M, 1.0f),
        *y = dev(N, 1.0f), *scores = dev((size_t)N * M, 0.f),
        *ae = dev((size_t)N * M, 0.f), *yp = dev(M, 0.f),
        *Wmu = dev((size_t)K * M, sM), *bmue = dev(K, 1.0f),
        *Wsig = dev((size_t)K * M, sM), *bsige = dev(K, 1.0f),
        *fmu = dev(K, 0.f), *fsig_pre = dev(K, 0.f), *fsig = dev(K, 0.f),
        *fsig_c = dev(K, 0.f);
  int* done;
  CK(hipMalloc(&done, sizeof(int)));
  CK(hipMemset(done, 0, sizeof(int)));

  static const char* const fwd_ph[] = {"stage", "scores+softmax", "u", "ctx",
                                       "hm2", "heads"};
  static const char* const bwd_ph[] = {"stage", "mlp+dctx", "dWv+du",
                                       "da+ds", "dqk", "dWk+dq"};
  static const char* const enc_ph[] = {"stage", "scores+softmax+yp",
                                       "handoff wait", "heads tail"};
  for (int variant = 0; variant < 2; ++variant) {
    measure("attn_fused_fwd", variant, fwd_ph, 6, [&] {
      CK(fv_attn_fused_fwd(h, qk, cb, mask, Wv, bv, Wl, bl, wmu, bmu, wsig,
                           bsig, a, sd, guard, u, ctx, hm2, pmu, psig_pre,
                           psig, psig_c, N, K, H, alpha, keep_inv, variant,
                           0));
    });
  }
  for (int variant = 0; variant < 2; ++variant) {
    measure("attn_fused_bwd", variant, bwd_ph, 6, [&] {
      CK(fv_attn_fused_bwd(dpmu, dpsig_c, psig, psig_pre, hm2, wmu, wsig, Wl,
                           h, a, sd, mask, guard, u, Wv, q, Wk, bk, dz2, du,
                           ds, dc, dWv, dbv, dq, dWk, dbk, hpart, dwmu, dbmu,
                           dwsig, dbsig, N, K, H, alpha, keep_inv, variant,
                           nullptr, nullptr, nullptr, nullptr, 1.0f, 0));
    });
  }
  for (int variant = 0; variant < 2; ++variant) {
    // "handoff wait": from workgroup 0's yp to the last workgroup's
    // barrier; it can be negative when workgroup 0 is itself the last
    measure("enc_fused_fwd", variant, enc_ph, 4, [&] {
      CK(fv_enc_fused_fwd(h, Wenc, benc, y, scores, ae, yp, Wmu, bmue, Wsig,
                          bsige, fmu, fsig_pre, fsig, fsig_c, done, K, N, M,
                          H, variant, 0));
    });
  }
  CK(hipDeviceSynchronize());
  printf("done\n");
  return 0;
}
