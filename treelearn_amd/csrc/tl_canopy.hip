// Canopy height model of a cloud: the highest height above ground per cell, pits and holes mended from the neighbours' median, tree tops
// as window maxima, and height statistics per cell of a coarser metrics grid (the semantics are the project's own,
// restated in numpy in tests/canopy_restatement.py).
// tl_chm_max:     tl_dtm_min's shape with the other sign: one pass over the rows, cell index, the highest h per cell as a 64-bit atomicMax
//   on the order-preserving u64 image of the f64 bits, rows per cell.  Lanes of a wave whose consecutive rows share a cell form a run; the
//   run's maximum is taken with shuffles and its first lane issues one atomicAdd for the whole run, and one atomicMax where the cell's key
//   as it reads it is still lower.
// tl_chm_owner:   a second pass: a row whose h is its cell's maximum offers its label to an integer atomicMax.
// tl_chm_pits, tl_chm_tops: one thread per cell, each reads one grid and writes another.
// tl_canopy_keys: the metrics-grid cell of every row.  tl_grid_metrics: one workgroup per metrics cell over its range of ascending heights:
//   the counts are differences of binary searches, only the two sums walk the range.
// Every formula is f64 in plain operators under the pragma below (no contraction into fma).  Maxima and counts are integer atomics; sums
// run in fixed per-thread strides and a fixed tree over values whose order does not depend on the order of the rows.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr uint64_t kSign = 1ull << 63;
constexpr int kMaxSide = 32768;
constexpr int64_t kMaxCells = (int64_t)1 << 26;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr int kMaxLayers = 256;
constexpr int kMaxPercentiles = 16;

// order-preserving u64 image of a double: a < b  <=>  enc(a) < enc(b); no finite value (nor an infinity) maps to 0, the empty cell
__device__ __forceinline__ uint64_t enc(double z) {
  const uint64_t b = (uint64_t)__double_as_longlong(z);
  return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double dec(uint64_t k) { return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k)); }

// the cell of a row, or -1 with *bad set: a non-finite x, y or h, or a row outside the grid.  A NaN h: -1, *bad untouched.
template <typename T>
__device__ __forceinline__ int64_t cell_of(const T* __restrict__ pts, int64_t ld, int64_t i, double h, double cell, double ix0, double iy0, int nx,
                                           int ny, bool* bad) {
  const double x = (double)pts[i * ld], y = (double)pts[i * ld + 1];
  const double fx = floor(x / cell) - ix0, fy = floor(y / cell) - iy0;
  const bool inside = fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny;   // (NaN fails every comparison)
  if (h != h) {
    if (!inside) *bad = true;
    return -1;
  }
  if (!inside || !(fabs(h) <= kDblMax)) { *bad = true; return -1; }
  return (int64_t)fy * nx + (int64_t)fx;
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_chm_max(const T* __restrict__ pts, int64_t ld, const double* __restrict__ hag, int64_t n, double cell,
                                                    double ix0, double iy0, int nx, int ny, unsigned long long* __restrict__ keys,
                                                    int32_t* __restrict__ count, int32_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  // block-uniform trip count: every lane takes part in the wave shuffles, lanes past n and rows without a height carry cell -1
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    int64_t c = -1;
    unsigned long long k = 0ull;
    bool no_ground = false;
    if (i < n) {
      const double h = hag[i] + 0.0;                                 // -0.0 -> 0.0
      bool bad = false;
      c = cell_of(pts, ld, i, h, cell, ix0, iy0, nx, ny, &bad);
      if (bad) flags[0] = 1;
      no_ground = h != h;
      if (c >= 0) k = enc(h);
    }
    const uint64_t nans = __ballot(no_ground);
    if (lane == 0 && nans) atomicAdd(flags + 1, (int32_t)__popcll((unsigned long long)nans));
    const int64_t prev = __shfl_up(c, 1);
    const bool head = lane == 0 || prev != c;
    const uint64_t heads = __ballot(head);
    const uint64_t above = heads & ~((2ull << lane) - 1ull);         // heads after this lane (lane 63: none)
    const int end = above ? __ffsll((unsigned long long)above) - 1 : 64;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                               // suffix maximum inside the run: after the step, lanes [l, min(l + 2o, end))
      const unsigned long long other = __shfl_down(k, o);
      if (lane + o < end && other > k) k = other;
    }
    if (head && c >= 0) {
      if (keys[c] < k) atomicMax(keys + c, k);                       // (keys only grow: a stale read costs an atomic, never a maximum)
      atomicAdd(count + c, end - lane);
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_chm_owner(const T* __restrict__ pts, int64_t ld, const double* __restrict__ hag,
                                                      const int64_t* __restrict__ labels, int64_t n, double cell, double ix0, double iy0, int nx,
                                                      int ny, const unsigned long long* __restrict__ keys, int32_t* __restrict__ owner,
                                                      int32_t* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double h = hag[i] + 0.0;
    bool bad = false;
    const int64_t c = cell_of(pts, ld, i, h, cell, ix0, iy0, nx, ny, &bad);
    if (c < 0 || keys[c] != enc(h)) continue;
    const int64_t l = labels[i];
    if (l > 2147483647ll || l < -2147483648ll) { *err = 1; continue; }
    if (l >= 0) atomicMax(owner + c, (int32_t)l);
  }
}

__global__ void __launch_bounds__(kBlock) k_chm_pits(const unsigned long long* __restrict__ keys, int nx, int ny, double pit_depth, int min_nb,
                                                     double* __restrict__ top, double* __restrict__ chm, uint8_t* __restrict__ state) {
  const int64_t cells = (int64_t)nx * ny;
  for (int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x; id < cells; id += (int64_t)gridDim.x * kBlock) {
    const int j = (int)(id / nx), i = (int)(id - (int64_t)j * nx);
    unsigned long long v[8];                                         // the neighbours' images, ascending: the order of the values
    int k = 0;
    for (int dj = -1; dj <= 1; ++dj)
      for (int di = -1; di <= 1; ++di) {
        const int jj = j + dj, ii = i + di;
        if ((di == 0 && dj == 0) || jj < 0 || jj >= ny || ii < 0 || ii >= nx) continue;
        const unsigned long long q = keys[(int64_t)jj * nx + ii];
        if (q == 0ull) continue;
        int s = k++;
        while (s > 0 && v[s - 1] > q) { v[s] = v[s - 1]; --s; }
        v[s] = q;
      }
    double m = __builtin_nan("");
    if (k > 0) m = (k & 1) ? dec(v[k / 2]) : (dec(v[k / 2 - 1]) + dec(v[k / 2])) / 2.0;
    const unsigned long long kp = keys[id];
    const bool enough = k >= min_nb;
    if (kp != 0ull) {
      const double t = dec(kp);
      const bool pit = enough && m - t > pit_depth;
      top[id] = t;
      chm[id] = pit ? m : t;
      state[id] = pit ? 2 : 1;
    } else {
      top[id] = __builtin_nan("");
      chm[id] = enough ? m : __builtin_nan("");
      state[id] = enough ? 3 : 0;
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_chm_tops(const double* __restrict__ chm, int nx, int ny, int window, double min_height,
                                                     uint8_t* __restrict__ mask) {
  const int64_t cells = (int64_t)nx * ny;
  for (int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x; id < cells; id += (int64_t)gridDim.x * kBlock) {
    const double c = chm[id];
    bool is_top = c == c && c >= min_height;
    if (is_top) {
      const int j = (int)(id / nx), i = (int)(id - (int64_t)j * nx);
      const int j0 = j - window < 0 ? 0 : j - window, j1 = j > ny - 1 - window ? ny - 1 : j + window;
      const int i0 = i - window < 0 ? 0 : i - window, i1 = i > nx - 1 - window ? nx - 1 : i + window;
      for (int jj = j0; jj <= j1 && is_top; ++jj)
        for (int ii = i0; ii <= i1; ++ii) {
          const int64_t q = (int64_t)jj * nx + ii;
          const double o = chm[q];                                   // (a NaN compares false both ways)
          if (o > c || (o == c && q < id)) { is_top = false; break; }
        }
    }
    mask[id] = is_top ? 1 : 0;
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_canopy_keys(const T* __restrict__ pts, int64_t ld, const double* __restrict__ hag, int64_t n, double cell,
                                                        double ix0, double iy0, int nx, int ny, int64_t* __restrict__ keys,
                                                        int32_t* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    bool bad = false;
    keys[i] = cell_of(pts, ld, i, hag[i], cell, ix0, iy0, nx, ny, &bad);
    if (bad) *err = 1;
  }
}

struct Percentiles { double q[kMaxPercentiles]; };

// the sum of part[0 .. 256) by a fixed pairwise tree; every thread of the workgroup calls it and gets the sum
__device__ __forceinline__ double tree_sum(double* part, double mine) {
  part[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + o];
    __syncthreads();
  }
  const double s = part[0];
  __syncthreads();
  return s;
}

__global__ void __launch_bounds__(kBlock) k_grid_metrics(const double* __restrict__ sorted_h, const int64_t* __restrict__ start, double cutoff,
                                                         Percentiles pq, int np, double layer, int L, double* __restrict__ metrics,
                                                         int32_t* __restrict__ counts, int32_t* __restrict__ layers, int32_t* __restrict__ n_clipped) {
  __shared__ int64_t first[kMaxLayers + 2];                          // the first row of layer l, of the vegetation, of the clipped rows
  __shared__ double part[kBlock];
  const int64_t cellid = blockIdx.x;
  const int64_t a = start[cellid], b = start[cellid + 1];
  const int64_t r = b - a;
  const int tid = threadIdx.x;
  const double ceiling = (double)L * layer;
  // the heights ascend, so the layer of a row, h > cutoff and h >= ceiling never step back along the range: every count is the distance
  // between two first rows, each found by one thread's binary search with the predicate as it is stated -- no histogram
  for (int job = tid; job < L + 2; job += kBlock) {
    int64_t lo = a, hi = b;
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      const double h = sorted_h[mid] + 0.0;
      bool reached;
      if (job == L) reached = h > cutoff;
      else if (job == L + 1) reached = h >= ceiling;
      else {
        double l = 0.0;
        if (!(h < 0.0)) {
          const double f = floor(h / layer);
          l = f < (double)(L - 1) ? f : (double)(L - 1);
        }
        reached = l >= (double)job;
      }
      if (reached) hi = mid; else lo = mid + 1;
    }
    first[job] = lo;
  }
  __syncthreads();
  const int64_t m = b - first[L];
  for (int l = tid; l < L; l += kBlock) layers[cellid * L + l] = (int32_t)((l + 1 < L ? first[l + 1] : b) - first[l]);
  if (tid == 0 && b > first[L + 1]) atomicAdd(n_clipped, (int32_t)(b - first[L + 1]));
  const double* __restrict__ v = sorted_h + (b - m);                 // ascending: the vegetation rows are the last m
  double s = 0.0;
  for (int64_t i = tid; i < m; i += kBlock) s = s + (v[i] + 0.0);
  const double mean = tree_sum(part, s) / (double)m;                 // (0 / 0 = NaN for m = 0)
  double s2 = 0.0;
  for (int64_t i = tid; i < m; i += kBlock) {
    const double d = (v[i] + 0.0) - mean;
    s2 = s2 + d * d;
  }
  const double var = tree_sum(part, s2) / (double)m;
  const int W = 4 + np;
  double* __restrict__ out = metrics + cellid * W;
  const double nan = __builtin_nan("");
  if (tid == 0) {
    counts[cellid * 2] = (int32_t)r;
    counts[cellid * 2 + 1] = (int32_t)m;
    out[0] = r > 0 ? (double)m / (double)r : nan;
    out[1] = r > 0 ? sorted_h[b - 1] + 0.0 : nan;
    out[2] = m > 0 ? mean : nan;
    out[3] = m > 0 ? sqrt(var) : nan;
  }
  if (tid < np) {
    double p = nan;
    if (m > 0) {
      const double pos = (pq.q[tid] / 100.0) * (double)(m - 1);
      const double lo = floor(pos);
      const double t = pos - lo;
      const int64_t i0 = (int64_t)lo, i1 = i0 + 1 < m - 1 ? i0 + 1 : m - 1;
      const double v0 = v[i0] + 0.0, v1 = v[i1] + 0.0;
      p = v0 + (v1 - v0) * t;
    }
    out[4 + tid] = p;
  }
}

bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }
bool is_finite(double v) { return v >= -kDblMax && v <= kDblMax; }
bool grid_ok(int nx, int ny) { return nx >= 0 && ny >= 0 && nx <= kMaxSide && ny <= kMaxSide && (int64_t)nx * ny <= kMaxCells; }
bool index_ok(int64_t i0) { return i0 > -((int64_t)1 << 52) && i0 < ((int64_t)1 << 52); }           // exact as a double
bool rows_ok(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* h, double cell, int64_t ix0, int64_t iy0, int nx, int ny) {
  if (!pts || !h || n < 0 || ld < 2 || (dtype_f64 != 0 && dtype_f64 != 1)) return false;
  if (!(cell > 0.0) || !is_finite(cell) || !grid_ok(nx, ny) || !index_ok(ix0) || !index_ok(iy0)) return false;
  if (n > 0 && (int64_t)nx * ny == 0) return false;
  return aligned(pts, dtype_f64 ? 8 : 4) && aligned(h, 8);
}
}  // namespace

extern "C" int tl_chm_max(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* h, double cell, int64_t ix0, int64_t iy0, int nx,
                          int ny, uint64_t* keys, int32_t* count, int32_t* flags, tl_stream_t stream) {
  if (!rows_ok(pts, dtype_f64, ld, n, h, cell, ix0, iy0, nx, ny) || !keys || !count || !flags) return TL_ERR_ARG;
  if (!aligned(keys, 8) || !aligned(count, 4) || !aligned(flags, 4)) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (cells == 0) return TL_OK;
  if (hipMemsetAsync(keys, 0, (size_t)cells * sizeof(uint64_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (hipMemsetAsync(count, 0, (size_t)cells * sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (n == 0) return TL_OK;
  unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
  if (dtype_f64)
    k_chm_max<double><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const double*>(pts), ld, h, n, cell, (double)ix0, (double)iy0, nx, ny, k, count,
                                                           flags);
  else
    k_chm_max<float><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const float*>(pts), ld, h, n, cell, (double)ix0, (double)iy0, nx, ny, k, count,
                                                          flags);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_chm_owner(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* h, const int64_t* labels, double cell, int64_t ix0,
                            int64_t iy0, int nx, int ny, const uint64_t* keys, int32_t* owner, int32_t* err, tl_stream_t stream) {
  if (!rows_ok(pts, dtype_f64, ld, n, h, cell, ix0, iy0, nx, ny) || !labels || !keys || !owner || !err) return TL_ERR_ARG;
  if (!aligned(labels, 8) || !aligned(keys, 8) || !aligned(owner, 4) || !aligned(err, 4)) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny;
  if (cells == 0) return TL_OK;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(owner, 0xff, (size_t)cells * sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (n == 0) return TL_OK;
  const unsigned long long* k = reinterpret_cast<const unsigned long long*>(keys);
  if (dtype_f64)
    k_chm_owner<double><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const double*>(pts), ld, h, labels, n, cell, (double)ix0, (double)iy0, nx, ny,
                                                             k, owner, err);
  else
    k_chm_owner<float><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const float*>(pts), ld, h, labels, n, cell, (double)ix0, (double)iy0, nx, ny, k,
                                                            owner, err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_chm_pits(const uint64_t* keys, int nx, int ny, double pit_depth, int pit_min_neighbours, double* top, double* chm,
                           uint8_t* state, tl_stream_t stream) {
  if (!keys || !top || !chm || !state || !grid_ok(nx, ny) || pit_min_neighbours < 1 || pit_min_neighbours > 9) return TL_ERR_ARG;
  if (!(pit_depth >= 0.0) || !is_finite(pit_depth) || !aligned(keys, 8) || !aligned(top, 8) || !aligned(chm, 8) || top == chm) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny;
  if (cells == 0) return TL_OK;
  k_chm_pits<<<tl_grid(cells, kBlock), kBlock, 0, tl_s(stream)>>>(reinterpret_cast<const unsigned long long*>(keys), nx, ny, pit_depth,
                                                                 pit_min_neighbours, top, chm, state);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_chm_tops(const double* chm, int nx, int ny, int window, double min_height, uint8_t* mask, tl_stream_t stream) {
  if (!chm || !mask || !grid_ok(nx, ny) || window < 1 || !is_finite(min_height) || !aligned(chm, 8)) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny;
  if (cells == 0) return TL_OK;
  if (window > kMaxSide) window = kMaxSide;                          // (no grid is wider)
  k_chm_tops<<<tl_grid(cells, kBlock), kBlock, 0, tl_s(stream)>>>(chm, nx, ny, window, min_height, mask);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_canopy_keys(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* h, double cell, int64_t ix0, int64_t iy0, int nx,
                              int ny, int64_t* keys, int32_t* err, tl_stream_t stream) {
  if (!rows_ok(pts, dtype_f64, ld, n, h, cell, ix0, iy0, nx, ny) || !keys || !err || !aligned(keys, 8) || !aligned(err, 4)) return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  hipStream_t s = tl_s(stream);
  if (dtype_f64)
    k_canopy_keys<double><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const double*>(pts), ld, h, n, cell, (double)ix0, (double)iy0, nx, ny, keys,
                                                               err);
  else
    k_canopy_keys<float><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const float*>(pts), ld, h, n, cell, (double)ix0, (double)iy0, nx, ny, keys,
                                                              err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_grid_metrics(const double* sorted_h, int64_t n, const int64_t* start, int64_t cells, double cutoff, const double* percentiles,
                               int n_percentiles, double layer, int L, double* metrics, int32_t* counts, int32_t* layers, int32_t* n_clipped,
                               tl_stream_t stream) {
  if (!sorted_h || !start || !percentiles || !metrics || !counts || !layers || !n_clipped || n < 0 || cells < 0 || cells > kMaxCells)
    return TL_ERR_ARG;
  if (n_percentiles < 1 || n_percentiles > kMaxPercentiles || L < 1 || L > kMaxLayers || !(layer > 0.0) || !is_finite(layer) || !is_finite(cutoff))
    return TL_ERR_ARG;
  if (!aligned(sorted_h, 8) || !aligned(start, 8) || !aligned(metrics, 8) || !aligned(counts, 4) || !aligned(layers, 4) || !aligned(n_clipped, 4))
    return TL_ERR_ARG;
  Percentiles pq = {};
  for (int i = 0; i < n_percentiles; ++i) {
    if (!(percentiles[i] >= 0.0 && percentiles[i] <= 100.0)) return TL_ERR_ARG;
    pq.q[i] = percentiles[i];
  }
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(n_clipped, 0, sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (cells == 0) return TL_OK;
  k_grid_metrics<<<(unsigned)cells, kBlock, 0, s>>>(sorted_h, start, cutoff, pq, n_percentiles, layer, L, metrics, counts, layers, n_clipped);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
