// Gathered gate inputs of the inference GRU recurrences (GATHER = true).
//
// The dense kernels read step t of stock n at gi + (n*T + t)*3H. The gather
// forms read gi_rows + idx[n*T + t]*3H instead: gi_rows is (U, 3H), idx is
// (N, T) int32. An index outside [0, U) is a missing row: nothing is read
// and the step's 3H gate inputs are quiet NaN, so the stock's h turns NaN
// through the arithmetic, as it does on the dense path behind a NaN x row.
#pragma once

#include "common.h"

// a, b, c = the r, z, n gate inputs of hidden unit j from row ix of rows
DEVINL void gather3_(const float* __restrict__ rows, int ix, int U, int H,
                     int j, float& a, float& b, float& c) {
  a = b = c = __builtin_nanf("");
  if ((unsigned)ix < (unsigned)U) {
    const float* g = rows + (long)ix * 3 * H;
    a = g[j];
    b = g[H + j];
    c = g[2 * H + j];
  }
}

// The T row numbers of one stock for a wave that walks its time steps: 64
// at a time, one per lane, so the number of a later step is a register read
// and the gate-input loads it addresses can be issued a step ahead. at(j)
// is wave-uniform; j must not decrease between calls.
struct WaveIdx {
  const int* p;
  int T, v;
  // T <= 0: no index is read and every at() is missing
  DEVINL void init(const int* idx_row, int T_, int lane) {
    p = idx_row;
    T = T_;
    v = lane < T ? p[lane] : -1;
  }
  DEVINL int at(int j, int lane) {
    if (j > 0 && (j & 63) == 0) v = j + lane < T ? p[j + lane] : -1;
    return __builtin_amdgcn_readlane(v, j & 63);
  }
};
