// The uniform cell grid in Morton (z-curve) order that tl_outlier.hip and tl_change.hip search: the grid, the key of a cell, and the row
// range of a cell of the key-sorted array.  A cell of the grid coarsened s times (cell edge h * 2^s) is the contiguous key range
// [m << 3s, (m + 1) << 3s), so one sort serves every coarsening.
#pragma once
#include "tl_common.h"

constexpr int kMortonBits = 21;                        // cells per axis: 2^21

struct Grid {
  double lo[3]; double h;
  int dims[3];                                         // cells per axis at level 0
};

// bits of v (21 used) spread to every third position
__host__ __device__ __forceinline__ uint64_t spread3(uint64_t v) {
  v &= 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}
__device__ __forceinline__ uint64_t morton(int x, int y, int z) { return spread3((uint64_t)x) << 2 | spread3((uint64_t)y) << 1 | spread3((uint64_t)z); }

// first row in [0, n) whose key is >= key (n when none); keys are below 2^63, key may be 2^63
__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ keys, int64_t n, uint64_t key) {
  int64_t a = 0, b = n;
  while (a < b) { const int64_t m = (a + b) >> 1; if ((uint64_t)keys[m] < key) a = m + 1; else b = m; }
  return a;
}

// lane l < 27: the row range of the level-s cell (qc + offset l) of the sorted array; empty outside the grid and for lanes >= 27
__device__ __forceinline__ void cell_range(const int64_t* __restrict__ keys, int64_t n, const Grid& g, const int qc[3], int s, int lane,
                                           int64_t* start, int64_t* end) {
  *start = 0; *end = 0;
  if (lane >= 27) return;
  const int d[3] = {lane / 9 - 1, (lane / 3) % 3 - 1, lane % 3 - 1};
  int c[3];
  for (int a = 0; a < 3; ++a) {
    c[a] = (qc[a] >> s) + d[a];
    if (c[a] < 0 || c[a] > ((g.dims[a] - 1) >> s)) return;
  }
  const uint64_t m = morton(c[0], c[1], c[2]);
  *start = lower_bound(keys, n, m << (3 * s));
  *end = lower_bound(keys, n, (m + 1) << (3 * s));       // s = 21: m = 0 and 1 << 63 is above every key
}

static inline bool make_grid(const double lo[3], const int32_t dims[3], double h, Grid* g) {
  if (!lo || !dims || !(h > 0.0)) return false;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > (1 << kMortonBits)) return false;
    g->lo[a] = lo[a]; g->dims[a] = dims[a];
  }
  g->h = h;
  return true;
}
