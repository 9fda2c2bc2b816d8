// Terrain model of a labelled cloud: a raster of ground heights (DTM), and the ground under any point (the semantics are
// the project's own, restated in numpy in tests/terrain_restatement.py).
// tl_dtm_min:    one pass over the rows: cell index, candidate test (label 0, or every row without labels), candidates per cell and
//   the lowest candidate z per cell, as a 64-bit atomicMin on the order-preserving u64 image of the f64 bits.  Lanes of a wave whose
//   consecutive rows share a cell form a run (inputs come spatially sorted); the run's minimum is taken with shuffles and its first lane
//   issues one atomicMin and one integer atomicAdd for the whole run, as tl_eval_contingency does for its counts.
// tl_dtm_filter: one thread per cell, against the raw minima: a cell is rejected when a neighbour within `window` cells lies lower than
//   the slope bound allows.  tl_dtm_fill: one thread per cell without a ground value: the first ring radius that meets a ground cell,
//   then the inverse-square-distance mean of that window's ground cells in row-major order.  Both read one grid and write another.
// tl_dtm_sample: one thread per row: bilinear ground between the four nearest cell centres, or the containing cell where one of the
//   four is NaN; writes the ground and / or z - ground.
// Every formula is f64 in plain operators under the pragma below (no contraction into fma), so every predicate sees the value numpy
// sees.  Minima and counts are integer atomics, sums run in one thread in a fixed order: two runs give the same bits, whatever the
// order of the rows.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr uint64_t kEmpty = ~0ull;            // no finite double maps to it
constexpr uint64_t kSign = 1ull << 63;
constexpr int kMaxSide = 32768;
constexpr int64_t kMaxCells = (int64_t)1 << 26;

// order-preserving u64 image of a double: a < b  <=>  enc(a) < enc(b) (finite values; -0.0 sorts below +0.0)
__device__ __forceinline__ uint64_t enc(double z) {
  const uint64_t b = (uint64_t)__double_as_longlong(z);
  return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double dec(uint64_t k) { return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k)); }

template <typename T>
__global__ void __launch_bounds__(kBlock) k_dtm_min(const T* __restrict__ pts, int64_t ld, const int64_t* __restrict__ labels, int64_t n, double cell,
                                                    double ix0, double iy0, int nx, int ny, unsigned long long* __restrict__ keys,
                                                    int32_t* __restrict__ count, int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  // block-uniform trip count: every lane takes part in the wave shuffles, lanes past n and non-candidates carry cell -1
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    int64_t c = -1;
    unsigned long long k = kEmpty;
    if (i < n) {
      const double x = (double)pts[i * ld], y = (double)pts[i * ld + 1], z = (double)pts[i * ld + 2];
      const double fx = floor(x / cell) - ix0, fy = floor(y / cell) - iy0;
      if (fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny && fabs(z) <= 1.7976931348623157e308) {
        if (!labels || labels[i] == 0) { c = (int64_t)fy * nx + (int64_t)fx; k = enc(z); }
      } else {
        *err = 1;                                                // (NaN fails every comparison; a row outside the grid is refused, not written)
      }
    }
    const int64_t prev = __shfl_up(c, 1);
    const bool head = lane == 0 || prev != c;
    const uint64_t heads = __ballot(head);
    const uint64_t above = heads & ~((2ull << lane) - 1ull);     // heads after this lane (lane 63: none)
    const int end = above ? __ffsll((unsigned long long)above) - 1 : 64;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                           // suffix minimum inside the run: after the step, lanes [l, min(l + 2o, end))
      const unsigned long long other = __shfl_down(k, o);
      if (lane + o < end && other < k) k = other;
    }
    if (head && c >= 0) {
      atomicMin(keys + c, k);
      atomicAdd(count + c, end - lane);
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_dtm_filter(const unsigned long long* __restrict__ keys, int nx, int ny, double cell, double max_slope,
                                                       double step_tol, int window, double* __restrict__ zmin, uint8_t* __restrict__ state) {
  const int64_t cells = (int64_t)nx * ny;
  for (int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x; id < cells; id += (int64_t)gridDim.x * kBlock) {
    const unsigned long long kp = keys[id];
    if (kp == kEmpty) { zmin[id] = __builtin_nan(""); state[id] = 0; continue; }
    const int j = (int)(id / nx), i = (int)(id - (int64_t)j * nx);
    const double zp = dec(kp);
    const int j0 = j - window < 0 ? 0 : j - window, j1 = j + window > ny - 1 ? ny - 1 : j + window;
    const int i0 = i - window < 0 ? 0 : i - window, i1 = i + window > nx - 1 ? nx - 1 : i + window;
    bool rejected = false;
    for (int jj = j0; jj <= j1 && !rejected; ++jj)
      for (int ii = i0; ii <= i1; ++ii) {
        const unsigned long long kq = keys[(int64_t)jj * nx + ii];
        if (kq == kEmpty || (jj == j && ii == i)) continue;
        const int64_t di = ii - i, dj = jj - j;
        const double d = cell * sqrt((double)(di * di + dj * dj));
        if (zp - dec(kq) > max_slope * d + step_tol) { rejected = true; break; }
      }
    zmin[id] = zp;
    state[id] = rejected ? 2 : 1;
  }
}

__global__ void __launch_bounds__(kBlock) k_dtm_fill(const double* __restrict__ zmin, const uint8_t* __restrict__ state_in, int nx, int ny,
                                                     int fill_radius, double* __restrict__ z, uint8_t* __restrict__ state) {
  const int64_t cells = (int64_t)nx * ny;
  for (int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x; id < cells; id += (int64_t)gridDim.x * kBlock) {
    const uint8_t s = state_in[id];
    if (s == 1) { z[id] = zmin[id]; state[id] = 1; continue; }
    const int j = (int)(id / nx), i = (int)(id - (int64_t)j * nx);
    // the first ring that holds a ground cell; rings beyond the farthest grid edge are empty
    int reach = i > nx - 1 - i ? i : nx - 1 - i;
    const int reach_y = j > ny - 1 - j ? j : ny - 1 - j;
    reach = reach > reach_y ? reach : reach_y;
    if (reach > fill_radius) reach = fill_radius;
    int rho = 0;
    for (int r = 1; r <= reach && !rho; ++r) {
      const int i0 = i - r < 0 ? 0 : i - r, i1 = i + r > nx - 1 ? nx - 1 : i + r;
      const int j0 = j - r < 0 ? 0 : j - r, j1 = j + r > ny - 1 ? ny - 1 : j + r;
      if (j - r >= 0)
        for (int ii = i0; ii <= i1 && !rho; ++ii) if (state_in[(int64_t)(j - r) * nx + ii] == 1) rho = r;
      if (j + r <= ny - 1)
        for (int ii = i0; ii <= i1 && !rho; ++ii) if (state_in[(int64_t)(j + r) * nx + ii] == 1) rho = r;
      if (i - r >= 0)
        for (int jj = j0; jj <= j1 && !rho; ++jj) if (state_in[(int64_t)jj * nx + (i - r)] == 1) rho = r;
      if (i + r <= nx - 1)
        for (int jj = j0; jj <= j1 && !rho; ++jj) if (state_in[(int64_t)jj * nx + (i + r)] == 1) rho = r;
    }
    if (!rho) { z[id] = __builtin_nan(""); state[id] = s; continue; }
    const int i0 = i - rho < 0 ? 0 : i - rho, i1 = i + rho > nx - 1 ? nx - 1 : i + rho;
    const int j0 = j - rho < 0 ? 0 : j - rho, j1 = j + rho > ny - 1 ? ny - 1 : j + rho;
    double sw = 0.0, swz = 0.0;
    for (int jj = j0; jj <= j1; ++jj)                            // row-major: the order of the restatement
      for (int ii = i0; ii <= i1; ++ii) {
        const int64_t q = (int64_t)jj * nx + ii;
        if (state_in[q] != 1) continue;
        const int64_t di = ii - i, dj = jj - j;
        const double w = 1.0 / (double)(di * di + dj * dj);
        swz = swz + w * zmin[q];
        sw = sw + w;
      }
    z[id] = swz / sw;
    state[id] = s == 0 ? 3 : 4;
  }
}

// index of floor(v) clamped to 0 .. n - 1 (v finite)
__device__ __forceinline__ int clamp_index(double v, int n) { return v < 0.0 ? 0 : v > (double)(n - 1) ? n - 1 : (int)v; }

template <typename T>
__global__ void __launch_bounds__(kBlock) k_dtm_sample(const T* __restrict__ pts, int64_t ld, int64_t n, const double* __restrict__ grid, double cell,
                                                       double ix0, double iy0, int nx, int ny, double* __restrict__ ground,
                                                       double* __restrict__ hag) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += (int64_t)gridDim.x * kBlock) {
    const double x = (double)pts[r * ld], y = (double)pts[r * ld + 1];
    double g = __builtin_nan("");
    if (nx > 0 && ny > 0 && fabs(x) <= 1.7976931348623157e308 && fabs(y) <= 1.7976931348623157e308) {
      const double u = x / cell - (ix0 + 0.5), v = y / cell - (iy0 + 0.5);
      const double fu = floor(u), fv = floor(v);
      const double fx = u - fu, fy = v - fv;
      const int a0 = clamp_index(fu, nx), a1 = clamp_index(fu + 1.0, nx), b0 = clamp_index(fv, ny), b1 = clamp_index(fv + 1.0, ny);
      const double g00 = grid[(int64_t)b0 * nx + a0], g10 = grid[(int64_t)b0 * nx + a1];
      const double g01 = grid[(int64_t)b1 * nx + a0], g11 = grid[(int64_t)b1 * nx + a1];
      if (g00 == g00 && g10 == g10 && g01 == g01 && g11 == g11) {
        g = (g00 * (1.0 - fx) + g10 * fx) * (1.0 - fy) + (g01 * (1.0 - fx) + g11 * fx) * fy;
      } else {
        const int ci = clamp_index(floor(x / cell) - ix0, nx), cj = clamp_index(floor(y / cell) - iy0, ny);
        g = grid[(int64_t)cj * nx + ci];
      }
    }
    if (ground) ground[r] = g;
    if (hag) hag[r] = (double)pts[r * ld + 2] - g;
  }
}

bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }
bool grid_ok(int nx, int ny) { return nx >= 0 && ny >= 0 && nx <= kMaxSide && ny <= kMaxSide && (int64_t)nx * ny <= kMaxCells; }
bool index_ok(int64_t i0) { return i0 > -((int64_t)1 << 52) && i0 < ((int64_t)1 << 52); }           // exact as a double
}  // namespace

extern "C" int tl_dtm_min(const void* pts, int dtype_f64, int64_t ld, int64_t n, const int64_t* labels, double cell, int64_t ix0, int64_t iy0,
                          int nx, int ny, uint64_t* keys, int32_t* n_candidates, int32_t* err, tl_stream_t stream) {
  if (!pts || !keys || !n_candidates || !err || n < 0 || ld < 3 || (dtype_f64 != 0 && dtype_f64 != 1)) return TL_ERR_ARG;
  if (!(cell > 0.0) || !(cell <= 1.7976931348623157e308) || !grid_ok(nx, ny) || !index_ok(ix0) || !index_ok(iy0)) return TL_ERR_ARG;
  if (!aligned(pts, dtype_f64 ? 8 : 4) || !aligned(labels, 8) || !aligned(keys, 8) || !aligned(n_candidates, 4) || !aligned(err, 4)) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny;
  if (n > 0 && cells == 0) return TL_ERR_ARG;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(err, 0, sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (cells == 0) return TL_OK;
  if (hipMemsetAsync(keys, 0xff, (size_t)cells * sizeof(uint64_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (hipMemsetAsync(n_candidates, 0, (size_t)cells * sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (n == 0) return TL_OK;
  unsigned long long* k = reinterpret_cast<unsigned long long*>(keys);
  if (dtype_f64)
    k_dtm_min<double><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const double*>(pts), ld, labels, n, cell, (double)ix0, (double)iy0, nx, ny, k,
                                                           n_candidates, err);
  else
    k_dtm_min<float><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const float*>(pts), ld, labels, n, cell, (double)ix0, (double)iy0, nx, ny, k,
                                                          n_candidates, err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_dtm_filter(const uint64_t* keys, int nx, int ny, double cell, double max_slope, double step_tol, int window, double* zmin,
                             uint8_t* state, tl_stream_t stream) {
  if (!keys || !zmin || !state || !grid_ok(nx, ny) || window < 0 || window > kMaxSide) return TL_ERR_ARG;
  if (!(cell > 0.0) || !(cell <= 1.7976931348623157e308) || !(max_slope >= 0.0) || !(step_tol >= 0.0)) return TL_ERR_ARG;
  if (!aligned(keys, 8) || !aligned(zmin, 8)) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny;
  if (cells == 0) return TL_OK;
  k_dtm_filter<<<tl_grid(cells, kBlock), kBlock, 0, tl_s(stream)>>>(reinterpret_cast<const unsigned long long*>(keys), nx, ny, cell, max_slope, step_tol,
                                                                   window, zmin, state);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_dtm_fill(const double* zmin, const uint8_t* state_in, int nx, int ny, int fill_radius, double* z, uint8_t* state,
                           tl_stream_t stream) {
  if (!zmin || !state_in || !z || !state || !grid_ok(nx, ny) || fill_radius < 0 || fill_radius > kMaxSide) return TL_ERR_ARG;
  if (!aligned(zmin, 8) || !aligned(z, 8) || zmin == z || state_in == state) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny;
  if (cells == 0) return TL_OK;
  k_dtm_fill<<<tl_grid(cells, kBlock), kBlock, 0, tl_s(stream)>>>(zmin, state_in, nx, ny, fill_radius, z, state);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_dtm_sample(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* z, double cell, int64_t ix0, int64_t iy0, int nx,
                             int ny, double* ground, double* hag, tl_stream_t stream) {
  if (!pts || (!ground && !hag) || n < 0 || ld < (hag ? 3 : 2) || (dtype_f64 != 0 && dtype_f64 != 1)) return TL_ERR_ARG;
  if (!(cell > 0.0) || !(cell <= 1.7976931348623157e308) || !grid_ok(nx, ny) || !index_ok(ix0) || !index_ok(iy0)) return TL_ERR_ARG;
  if ((int64_t)nx * ny > 0 && !z) return TL_ERR_ARG;
  if (!aligned(pts, dtype_f64 ? 8 : 4) || !aligned(z, 8) || !aligned(ground, 8) || !aligned(hag, 8)) return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  if ((int64_t)nx * ny == 0) { nx = 0; ny = 0; }
  if (dtype_f64)
    k_dtm_sample<double><<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(static_cast<const double*>(pts), ld, n, z, cell, (double)ix0, (double)iy0, nx,
                                                                         ny, ground, hag);
  else
    k_dtm_sample<float><<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(static_cast<const float*>(pts), ld, n, z, cell, (double)ix0, (double)iy0, nx, ny,
                                                                        ground, hag);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
