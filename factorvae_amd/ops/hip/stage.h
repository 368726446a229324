// Staging helpers of the latency-oriented fused kernels (attention.hip,
// encoder.hip): a thread's share of a small row-major matrix is loaded
// into registers with every load in flight at once, and written to a
// padded LDS image without a divide in the loop.
#pragma once

#include "common.h"

// Phase stamps of the fused attention / encoder kernels, for
// scripts/probe/mid_phases.hip only, which defines both macros before it
// includes the kernel files. The extension is built without them: here
// they expand to nothing. MID_STAMP marks a phase boundary in workgroup 0,
// MID_STAMP_LAST one in whichever workgroup runs the encoder's heads tail.
#ifndef MID_STAMP
#define MID_STAMP(i)
#define MID_STAMP_LAST(i)
#endif

// Cursor of one thread walking a row-major (R,H) matrix in fixed element
// steps: one divide at construction, an add and a compare per step.
struct RowCol {
  int row, col, drow, dcol, H;
  DEVINL RowCol(int e0, int step, int H_) : H(H_) {
    row = e0 / H_;
    col = e0 - row * H_;
    drow = step / H_;
    dcol = step - drow * H_;
  }
  DEVINL void next() {
    row += drow;
    col += dcol;
    if (col >= H) {
      col -= H;
      ++row;
    }
  }
};

// A register tile holds NT floats per thread of a 256-thread workgroup,
// so one round covers 256*NT elements. QUAD (H % 4 == 0): the thread owns
// NT/4 runs of four consecutive elements, run i starting at element
// 4*(tid + 256*i); a run never crosses a row. Otherwise element
// tid + 256*i. Loads past `total` are clamped to the last element (they
// are issued unconditionally, so nothing waits between them) and dropped
// at the store.
template <bool QUAD, int NT>
DEVINL void tile_load(float (&v)[NT], const float* __restrict__ src,
                      int total, int tid) {
  if (QUAD) {
    const int nq = total >> 2;
    if ((reinterpret_cast<size_t>(src) & 15) == 0) {
      const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
      for (int i = 0; i < NT / 4; ++i) {
        const float4 t = s4[min(tid + i * 256, nq - 1)];
        v[4 * i] = t.x;
        v[4 * i + 1] = t.y;
        v[4 * i + 2] = t.z;
        v[4 * i + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NT / 4; ++i) {
        const float* s = src + 4 * min(tid + i * 256, nq - 1);
        v[4 * i] = s[0];
        v[4 * i + 1] = s[1];
        v[4 * i + 2] = s[2];
        v[4 * i + 3] = s[3];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < NT; ++i) v[i] = src[min(tid + i * 256, total - 1)];
  }
}

DEVINL RowCol tile_cursor(bool quad, int tid, int H) {
  return quad ? RowCol(4 * tid, 1024, H) : RowCol(tid, 256, H);
}

// Write a tile into an LDS image with row stride SH (H+1: the row chains
// and the column reads of the kernels are bank-conflict free with it; the
// four stores of a run land in four different banks, rows of one wave in
// banks shifted by one). `rc` is advanced by one round.
template <bool QUAD, int NT>
DEVINL void tile_store_lds(float* dst, const float (&v)[NT], int total,
                           int tid, RowCol& rc, int SH) {
  if (QUAD) {
#pragma unroll
    for (int i = 0; i < NT / 4; ++i) {
      if (4 * (tid + i * 256) < total) {
        float* d = dst + rc.row * SH + rc.col;
        d[0] = v[4 * i];
        d[1] = v[4 * i + 1];
        d[2] = v[4 * i + 2];
        d[3] = v[4 * i + 3];
      }
      rc.next();
    }
  } else {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      if (tid + i * 256 < total) dst[rc.row * SH + rc.col] = v[i];
      rc.next();
    }
  }
}

// out[e] = rowv[row(e)] * colv[col(e)] over a tile's elements of an
// (H,H) matrix (the outer-product weight gradients), 16-byte stores where
// the destination allows.
template <bool QUAD, int NT>
DEVINL void tile_outer_store(float* __restrict__ out, const float* rowv,
                             const float* colv, int total, int tid, int H) {
  RowCol rc = tile_cursor(QUAD, tid, H);
  if (QUAD) {
    const bool al = (reinterpret_cast<size_t>(out) & 15) == 0;
#pragma unroll
    for (int i = 0; i < NT / 4; ++i) {
      const int e = 4 * (tid + i * 256);
      if (e < total) {
        const float r = rowv[rc.row];
        float4 o;
        o.x = r * colv[rc.col];
        o.y = r * colv[rc.col + 1];
        o.z = r * colv[rc.col + 2];
        o.w = r * colv[rc.col + 3];
        if (al) {
          *reinterpret_cast<float4*>(out + e) = o;
        } else {
          out[e] = o.x;
          out[e + 1] = o.y;
          out[e + 2] = o.z;
          out[e + 3] = o.w;
        }
      }
      rc.next();
    }
  } else {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int e = tid + i * 256;
      if (e < total) out[e] = rowv[rc.row] * colv[rc.col];
      rc.next();
    }
  }
}

// Stage a row-major (R,H) matrix into an LDS image of row stride H+1,
// NT floats per thread per round (all of a round's loads in flight).
template <bool QUAD, int NT>
DEVINL void stage_rows_lds(float* dst, const float* __restrict__ src, int R,
                           int H, int tid) {
  const int total = R * H;
  RowCol rc = tile_cursor(QUAD, tid, H);
  for (int base = 0; base < total; base += 256 * NT) {
    float v[NT];
    tile_load<QUAD, NT>(v, src + base, total - base, tid);
    tile_store_lds<QUAD, NT>(dst, v, total - base, tid, rc, H + 1);
  }
}

// 64-lane sums of NJ independent values at once: per value exactly
// wave_reduce_sum's tree (valid in lane 0), but the NJ shuffles of a level
// are issued together, so their latencies overlap instead of adding up.
template <int NJ>
DEVINL void wave_reduce_sum_n(float (&v)[NJ]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float t[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) t[j] = __shfl_down(v[j], off, 64);
#pragma unroll
    for (int j = 0; j < NJ; ++j) v[j] += t[j];
  }
}
