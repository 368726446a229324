// Per-day ranking metrics of the batched scoring workspace.
//
//   daily_ic_seg_kernel: one workgroup per (day, prediction column) of the
//     packed layout predict.hip uses (seg_off[D+1] row offsets). Writes
//     stats[d][p] = {ic, rank_ic, long_ret, short_ret} (float64) and
//     count[d][p] = number of valid rows (int32); every output element is
//     written, empty and refused days included.
//
// A row is valid when its prediction and its label are both finite; all
// statistics run over the valid rows only.
//   ic       Pearson correlation, two-pass float64.
//   rank_ic  Pearson correlation of the 1-based average ranks (ties share
//            the mean of their positions; -0.0 ties +0.0), centred on the
//            exact mean (n+1)/2.
//   long/short  mean label of the k = min(topk, n) rows with the highest /
//            lowest prediction; among equal predictions the higher row
//            index counts as higher (the order of the sorted keys).
//
// Ranks come from a bitonic sort of 64-bit keys in LDS:
//   key = ordered_u32(value) << 32 | local row index, all ones for invalid
//   rows and padding (no finite value maps to an all-ones high word).
// A sorted position's tie group is [lo, hi) = the first position whose
// high word is >= / > its own (two binary searches); its rank is
// (lo + hi + 1) / 2, exact in fp32 up to 8192.5.
//
// Every reduction is ordered by segment-local indices only (256-thread
// strided partials, wave shuffle tree, fixed 4-wave tree), no atomics: a
// day's four numbers do not depend on its position in the batch or on its
// neighbours.
//
// LDS map (bytes): keys[NP] u64 | rank_p[max_n] f32 | rank_l[max_n] f32 |
//   red[4][IC_RED] f64, NP = next_pow2(max_n). max_n <= 8192 gives
//   64 KB + 32 KB + 32 KB + 192 B, inside SEG_LDS_MAX of predict.hip.

#include "common.h"
#include "launchers.h"

#define IC_MAX_N 8192
#define IC_RED 6
#define IC_LDS_MAX (144 * 1024)

typedef unsigned long long u64;

// order-preserving float -> uint map; -0.0 is canonicalised to +0.0 first
DEVINL unsigned ordered_u32(float v) {
  unsigned u = (v == 0.0f) ? 0u : __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEVINL bool finitef_(float v) {
  return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
}

// float64 twin of block_reduce for R sums at once, 256 threads. The result
// is left in v[] of every thread. Fixed order: wave shuffle tree, then
// (w0 + w1) + (w2 + w3).
template <int R>
DEVINL void block_reduce_sum_f64(double (&v)[R], double* red) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    double x = v[r];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    if (lane == 0) red[wid * IC_RED + r] = x;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r)
    v[r] = (red[r] + red[IC_RED + r]) + (red[2 * IC_RED + r] + red[3 * IC_RED + r]);
  __syncthreads();
}

// keys of one column of the day: v[i] for valid rows, all ones otherwise
DEVINL void ic_build_keys(u64* keys, const float* __restrict__ v,
                          const float* __restrict__ a,
                          const float* __restrict__ b, int N, int np,
                          int tid) {
  for (int i = tid; i < np; i += 256) {
    u64 key = ~0ull;
    if (i < N && finitef_(a[i]) && finitef_(b[i]))
      key = ((u64)ordered_u32(v[i]) << 32) | (unsigned)i;
    keys[i] = key;
  }
  __syncthreads();
}

// ascending bitonic sort of np (a power of two >= 2) keys. Thread q owns
// the pair (i, i | j) with i = q with a zero inserted at bit log2(j). The
// 32 lanes of a ds_read_b64 group then hold 32 "low" elements out of 64,
// two per bank for j <= 16; lanes 16-31 read their high element first
// (and lanes 8-15 of each 16-lane ds_write_b64 group write it first), which
// puts every lane of a group on its own bank in all steps.
DEVINL void ic_bitonic_sort(u64* keys, int np, int tid) {
  const bool rd_hi_first = (tid & 16) != 0;
  const bool wr_hi_first = (tid & 8) != 0;
  for (int k = 2; k <= np; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = tid; q < (np >> 1); q += 256) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
        const int l = i | j;
        const u64 kf = keys[rd_hi_first ? l : i];
        const u64 ks = keys[rd_hi_first ? i : l];
        const u64 a = rd_hi_first ? ks : kf;  // keys[i]
        const u64 b = rd_hi_first ? kf : ks;  // keys[l]
        const bool up = (i & k) == 0;
        if ((a > b) == up) {
          // swap: i takes b, l takes a
          keys[wr_hi_first ? l : i] = wr_hi_first ? a : b;
          keys[wr_hi_first ? i : l] = wr_hi_first ? b : a;
        }
      }
      __syncthreads();
    }
  }
}

// first position in [0, n) whose key is >= bound (n when none)
DEVINL int ic_lower_bound(const u64* keys, int n, u64 bound) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < bound) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// average ranks of the sorted valid keys, scattered to rank[row]
DEVINL void ic_ranks(const u64* keys, float* rank, int nv, int tid) {
  for (int pos = tid; pos < nv; pos += 256) {
    const u64 key = keys[pos];
    const u64 hw = key >> 32;  // <= 0xff7fffff for a finite value
    const int lo = ic_lower_bound(keys, nv, hw << 32);
    const int hi = ic_lower_bound(keys, nv, (hw + 1) << 32);
    rank[(unsigned)key] = 0.5f * (float)(lo + hi + 1);
  }
}

__global__ __launch_bounds__(256) void daily_ic_seg_kernel(
    const float* __restrict__ pred, long ld, const float* __restrict__ label,
    const int* __restrict__ seg_off, double* __restrict__ stats,
    int* __restrict__ count, int total, int topk, int max_n, int NP) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u64* keys = (u64*)smem;                       // [NP]
  float* rank_p = (float*)(keys + NP);          // [max_n]
  const int rcap = (max_n + 1) & ~1;            // keeps red 8-byte aligned
  float* rank_l = rank_p + rcap;                // [max_n]
  double* red = (double*)(rank_l + rcap);       // [4][IC_RED]

  const int d = blockIdx.x;
  const int p = blockIdx.y;
  const int P = gridDim.y;
  const int tid = threadIdx.x;
  const long oi = (long)d * P + p;
  double* st = stats + oi * 4;

  const int r0 = seg_off[d];
  const int N = seg_off[d + 1] - r0;
  if (N == 0 || N < 0 || r0 < 0 || r0 > total - N || N > max_n) {
    // empty day: count 0. A segment outside the packed buffer or the
    // launch's LDS plan is never read: count -1. Stats NaN in both cases.
    if (tid == 0) {
      count[oi] = (N == 0) ? 0 : -1;
      st[0] = st[1] = st[2] = st[3] = (double)NAN;
    }
    return;
  }
  const float* x = pred + (long)p * ld + r0;
  const float* y = label + r0;
  int np = 2;
  while (np < N) np <<= 1;  // workgroup-uniform, <= NP

  // ---- valid count and the means of the valid rows
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < N; i += 256) {
    const float xv = x[i], yv = y[i];
    if (finitef_(xv) && finitef_(yv)) {
      acc[0] += 1.0;
      acc[1] += (double)xv;
      acc[2] += (double)yv;
    }
  }
  block_reduce_sum_f64<3>(acc, red);
  const int nv = (int)acc[0];
  const double mx = acc[1] / acc[0];
  const double my = acc[2] / acc[0];

  // ---- predictions: sort, ranks, both ends of the order
  ic_build_keys(keys, x, x, y, N, np, tid);
  ic_bitonic_sort(keys, np, tid);
  ic_ranks(keys, rank_p, nv, tid);
  const int k = min(topk, nv);
  double ls[2] = {0.0, 0.0};
  for (int j = tid; j < k; j += 256) {
    ls[0] += (double)y[(unsigned)keys[nv - 1 - j]];
    ls[1] += (double)y[(unsigned)keys[j]];
  }
  block_reduce_sum_f64<2>(ls, red);  // its barriers also fence the key reads

  // ---- labels: same keys buffer
  ic_build_keys(keys, y, x, y, N, np, tid);
  ic_bitonic_sort(keys, np, tid);
  ic_ranks(keys, rank_l, nv, tid);
  __syncthreads();

  // ---- centred sums of values and of ranks
  const double mr = 0.5 * (double)(nv + 1);
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < N; i += 256) {
    const float xv = x[i], yv = y[i];
    if (finitef_(xv) && finitef_(yv)) {
      const double dx = (double)xv - mx, dy = (double)yv - my;
      const double rx = (double)rank_p[i] - mr, ry = (double)rank_l[i] - mr;
      s[0] += dx * dx;
      s[1] += dy * dy;
      s[2] += dx * dy;
      s[3] += rx * rx;
      s[4] += ry * ry;
      s[5] += rx * ry;
    }
  }
  block_reduce_sum_f64<6>(s, red);

  if (tid == 0) {
    count[oi] = nv;
    const bool ok = nv >= 2;
    st[0] = (ok && s[0] > 0.0 && s[1] > 0.0) ? s[2] / sqrt(s[0] * s[1])
                                             : (double)NAN;
    st[1] = (ok && s[3] > 0.0 && s[4] > 0.0) ? s[5] / sqrt(s[3] * s[4])
                                             : (double)NAN;
    st[2] = (k > 0) ? ls[0] / (double)k : (double)NAN;
    st[3] = (k > 0) ? ls[1] / (double)k : (double)NAN;
  }
}

extern "C" {

// pred: P rows of `total` floats, row stride ld; label: total floats;
// seg_off: D+1 row offsets. max_n: the longest day of the launch's plan
// (sizes LDS; the kernel refuses a longer one). stats (D,P,4) f64 and
// count (D,P) i32 are fully written.
hipError_t fv_daily_ic_seg(const float* pred, long ld, const float* label,
                           const int* seg_off, double* stats, int* count,
                           int total, int D, int P, int max_n, int topk,
                           hipStream_t s) {
  if (P <= 0 || P > 65535 || max_n > IC_MAX_N || max_n < 0 || topk < 0 ||
      total < 0)
    return hipErrorInvalidValue;
  if (D <= 0) return hipSuccess;
  int NP = 2;
  while (NP < max_n) NP <<= 1;
  const size_t lds = (size_t)NP * 8 + 2 * (size_t)((max_n + 1) & ~1) * 4 +
                     4 * IC_RED * sizeof(double);
  if (lds > IC_LDS_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(daily_ic_seg_kernel, dim3(D, P), dim3(256), lds, s, pred,
                     ld, label, seg_off, stats, count, total, topk, max_n, NP);
  HIP_CHECK_LAST();
  return hipSuccess;
}

}  // extern "C"
