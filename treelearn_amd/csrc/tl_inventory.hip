// Per-tree inventory of a labelled cloud: position, height, stem diameter at breast height, crown cells (the semantics are
// restated in numpy in tests/inventory_restatement.py).
// tl_inventory_gather: the rows of the tree labels, widened to f64 and written in label order, so that a tree is one contiguous range.
// tl_tree_inventory:   one workgroup per tree, four trips over its range: (a) the four lowest / highest z -> z_low, z_top; (b) the base
//   sums -> position; (c) the slice moments -> one lane solves the 3 x 3 system of the algebraic circle fit; (d) the residual sum.
// tl_tree_ground:      one workgroup per tree, trips (c) and (d) again with the terrain's ground under the tree in place of z_low.
// tl_crown_keys / tl_crown_count: one packed (tree, cell x, cell y) key per row; distinct keys per tree counted on the sorted keys.
// Every formula is f64 in plain operators under the pragma below (no contraction into fma), so every predicate sees the value numpy
// sees.  Sums go registers -> wave shuffles -> LDS in a fixed order and counts are integers: two runs give the same bits.
#include "tl_circle_fit.h"

#pragma clang fp contract(off)

namespace {
constexpr int kCols = 10;                    // z_low, z_top, height, x, y, z, dbh, dbh_x, dbh_y, dbh_rmse
constexpr int kGroundCols = 7;               // z_ground, height_ag, base_gap, dbh_ag, dbh_ag_x, dbh_ag_y, dbh_ag_rmse
constexpr int kCellBits = 21;                // cell index + 2^20 in 0 .. 2^21 - 1; tree id in the 21 bits above both
constexpr int64_t kCellHalf = (int64_t)1 << (kCellBits - 1);

template <typename T>
__global__ void __launch_bounds__(kBlock) k_inventory_gather(const T* __restrict__ pts, int64_t ld, const int64_t* __restrict__ order, int64_t n_src,
                                                             int64_t n, double* __restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    const int64_t i = order[j];
    const bool ok = (uint64_t)i < (uint64_t)n_src;
    const double nan = __builtin_nan("");
    out[3 * j] = ok ? (double)pts[i * ld] : nan;
    out[3 * j + 1] = ok ? (double)pts[i * ld + 1] : nan;
    out[3 * j + 2] = ok ? (double)pts[i * ld + 2] : nan;
  }
}

// the four smallest values seen, ascending, duplicates kept
__device__ __forceinline__ void low4_insert(double (&t)[4], double v) {
  if (!(v < t[3])) return;
  int k = 3;
  while (k > 0 && v < t[k - 1]) { t[k] = t[k - 1]; --k; }
  t[k] = v;
}

__global__ void __launch_bounds__(kBlock) k_tree_inventory(const double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ start,
                                                           double slice_height, double half_thickness, double r2max, int64_t min_points,
                                                           double* __restrict__ table, int64_t* __restrict__ counts) {
  __shared__ double s_ext[kBlock * 8];       // per thread: four lowest, four highest (negated) z
  __shared__ double s_red[kWaves * 9];
  __shared__ double s_par[5];
  __shared__ int s_ok;
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  int64_t lo = start[t], hi = start[t + 1];
  if (lo < 0 || hi > n || lo > hi) { lo = 0; hi = 0; }        // a malformed range reads nothing
  const int64_t rows = hi - lo;
  double* out = table + t * kCols;
  const double nan = __builtin_nan("");
  if (rows == 0) {                                             // block-uniform
    if (tid < kCols) out[tid] = nan;
    if (tid == 0) { counts[2 * t] = 0; counts[2 * t + 1] = 0; }
    return;
  }

  // (a) rank 3 from below and from above (duplicates counted) for more than 11 rows, else the extremes
  double lo4[4], hi4[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { lo4[k] = __builtin_inf(); hi4[k] = __builtin_inf(); }
  for (int64_t j = lo + tid; j < hi; j += kBlock) {
    const double z = xyz[3 * j + 2];
    low4_insert(lo4, z);
    low4_insert(hi4, -z);                                      // (negation is exact: the four largest z)
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { s_ext[tid * 8 + k] = lo4[k]; s_ext[tid * 8 + 4 + k] = hi4[k]; }
  __syncthreads();
  if (tid == 0 || tid == 64) {                                 // one lane of wave 0 merges the lows, one of wave 1 the highs
    const int side = tid == 0 ? 0 : 4;
    double a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = __builtin_inf();
    for (int th = 0; th < kBlock; ++th)
#pragma unroll
      for (int k = 0; k < 4; ++k) low4_insert(a, s_ext[th * 8 + side + k]);
    const double v = rows > 11 ? a[3] : a[0];
    s_par[side ? 1 : 0] = side ? -v : v;
  }
  __syncthreads();
  const double z_low = s_par[0], z_top = s_par[1];

  // (b) position: mean of the base rows
  double px, py, pz;
  {
    const double thr = z_low + 0.5;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t j = lo + tid; j < hi; j += kBlock) {
      const double z = xyz[3 * j + 2];
      if (z <= thr) { v[0] = v[0] + xyz[3 * j]; v[1] = v[1] + xyz[3 * j + 1]; v[2] = v[2] + z; v[3] = v[3] + 1.0; }
    }
    block_sum<4>(v, s_red);                                    // (every thread holds the sums: the rank-3 row is a base row, v[3] >= 1)
    px = v[0] / v[3]; py = v[1] / v[3]; pz = v[2] / v[3];
  }

  // (c) slice moments and fit, (d) residuals
  double cnt, rss;
  const Fit f = slice_circle(xyz, lo, hi, px, py, z_low + slice_height, half_thickness, r2max, min_points, s_red, s_par + 2, &s_ok, cnt, rss);
  if (tid == 0) {
    out[0] = z_low; out[1] = z_top; out[2] = z_top - z_low;
    out[3] = px; out[4] = py; out[5] = pz;
    out[6] = f.ok ? 2.0 * f.r : nan;
    out[7] = f.ok ? f.cx + px : nan;
    out[8] = f.ok ? f.cy + py : nan;
    out[9] = f.ok ? sqrt(rss / cnt) : nan;
    counts[2 * t] = rows;
    counts[2 * t + 1] = (int64_t)cnt;
  }
}

// The slice fit of every tree once more, with the ground under the tree (z_ground, sampled from the terrain at the tree's position)
// in place of z_low.  table: tl_tree_inventory's.  out f64[n_trees, 7] = z_ground, height_ag, base_gap, dbh_ag, dbh_ag_x, dbh_ag_y,
// dbh_ag_rmse; out_n i64[n_trees] = dbh_ag_n.
__global__ void __launch_bounds__(kBlock) k_tree_ground(const double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ start,
                                                        const double* __restrict__ table, const double* __restrict__ z_ground, double slice_height,
                                                        double half_thickness, double r2max, int64_t min_points, double* __restrict__ out,
                                                        int64_t* __restrict__ out_n) {
  __shared__ double s_red[kWaves * 9];
  __shared__ double s_fit[3];
  __shared__ int s_ok;
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  int64_t lo = start[t], hi = start[t + 1];
  if (lo < 0 || hi > n || lo > hi) { lo = 0; hi = 0; }        // a malformed range reads nothing
  const double nan = __builtin_nan("");
  const double zg = z_ground[t];
  double* o = out + t * kGroundCols;
  if (hi == lo || !(zg == zg)) {                               // block-uniform: no rows, or no terrain under the tree
    if (tid < kGroundCols) o[tid] = nan;
    if (tid == 0) out_n[t] = 0;
    return;
  }
  const double z_low = table[t * kCols], z_top = table[t * kCols + 1], px = table[t * kCols + 3], py = table[t * kCols + 4];
  double cnt, rss;
  const Fit f = slice_circle(xyz, lo, hi, px, py, zg + slice_height, half_thickness, r2max, min_points, s_red, s_fit, &s_ok, cnt, rss);
  if (tid == 0) {
    o[0] = zg; o[1] = z_top - zg; o[2] = z_low - zg;
    o[3] = f.ok ? 2.0 * f.r : nan;
    o[4] = f.ok ? f.cx + px : nan;
    o[5] = f.ok ? f.cy + py : nan;
    o[6] = f.ok ? sqrt(rss / cnt) : nan;
    out_n[t] = (int64_t)cnt;
  }
}

__global__ void __launch_bounds__(kBlock) k_crown_keys(const double* __restrict__ xyz, const int64_t* __restrict__ label, int64_t n, double cell,
                                                       int64_t* __restrict__ keys, int32_t* __restrict__ err) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    const double fx = floor(xyz[3 * j] / cell), fy = floor(xyz[3 * j + 1] / cell);
    const int64_t l = label[j];
    const double lim = (double)kCellHalf;
    int64_t key = 0;
    if (fx >= -lim && fx < lim && fy >= -lim && fy < lim && l >= 1 && l < ((int64_t)1 << kCellBits))
      key = (l << (2 * kCellBits)) | (((int64_t)fx + kCellHalf) << kCellBits) | ((int64_t)fy + kCellHalf);
    else
      *err = 1;                                                // (NaN fails every comparison)
    keys[j] = key;
  }
}

__global__ void __launch_bounds__(kBlock) k_crown_count(const int64_t* __restrict__ keys, int64_t n, int64_t n_trees, int64_t* __restrict__ cells) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    const int64_t k = keys[j];
    if (j > 0 && keys[j - 1] == k) continue;
    const int64_t t = (k >> (2 * kCellBits)) - 1;
    if (t >= 0 && t < n_trees) atomicAdd(reinterpret_cast<unsigned long long*>(cells + t), 1ull);
  }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
}  // namespace

extern "C" int tl_inventory_gather(const void* pts, int dtype_f64, int64_t ld, int64_t n_src, const int64_t* order, int64_t n, double* out_xyz,
                                   tl_stream_t stream) {
  if (!pts || !order || !out_xyz || n < 0 || n_src < 0 || ld < 3 || (dtype_f64 != 0 && dtype_f64 != 1)) return TL_ERR_ARG;
  if (!aligned8(order) || !aligned8(out_xyz) || (reinterpret_cast<uintptr_t>(pts) & (dtype_f64 ? 7 : 3))) return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  if (dtype_f64)
    k_inventory_gather<double><<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(static_cast<const double*>(pts), ld, order, n_src, n, out_xyz);
  else
    k_inventory_gather<float><<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(static_cast<const float*>(pts), ld, order, n_src, n, out_xyz);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_tree_inventory(const double* sorted_xyz, int64_t n, const int64_t* start, int64_t n_trees, double slice_height,
                                 double slice_thickness, double dbh_max_radius, int64_t dbh_min_points, double* table, int64_t* counts,
                                 tl_stream_t stream) {
  if (!sorted_xyz || !start || !table || !counts || n < 0 || n_trees < 0 || n_trees >= ((int64_t)1 << 31)) return TL_ERR_ARG;
  if (!aligned8(sorted_xyz) || !aligned8(start) || !aligned8(table) || !aligned8(counts)) return TL_ERR_ARG;
  if (!(slice_thickness > 0.0) || !(dbh_max_radius > 0.0) || !(slice_height == slice_height) || dbh_min_points < 0) return TL_ERR_ARG;
  if (n_trees == 0) return TL_OK;
  k_tree_inventory<<<(unsigned)n_trees, kBlock, 0, tl_s(stream)>>>(sorted_xyz, n, start, slice_height, slice_thickness / 2.0,
                                                                    dbh_max_radius * dbh_max_radius, dbh_min_points, table, counts);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_tree_ground(const double* sorted_xyz, int64_t n, const int64_t* start, int64_t n_trees, const double* table,
                              const double* z_ground, double slice_height, double slice_thickness, double dbh_max_radius, int64_t dbh_min_points,
                              double* ground_table, int64_t* ground_n, tl_stream_t stream) {
  if (!sorted_xyz || !start || !table || !z_ground || !ground_table || !ground_n || n < 0 || n_trees < 0 || n_trees >= ((int64_t)1 << 31))
    return TL_ERR_ARG;
  if (!aligned8(sorted_xyz) || !aligned8(start) || !aligned8(table) || !aligned8(z_ground) || !aligned8(ground_table) || !aligned8(ground_n))
    return TL_ERR_ARG;
  if (!(slice_thickness > 0.0) || !(dbh_max_radius > 0.0) || !(slice_height == slice_height) || dbh_min_points < 0) return TL_ERR_ARG;
  if (n_trees == 0) return TL_OK;
  k_tree_ground<<<(unsigned)n_trees, kBlock, 0, tl_s(stream)>>>(sorted_xyz, n, start, table, z_ground, slice_height, slice_thickness / 2.0,
                                                                 dbh_max_radius * dbh_max_radius, dbh_min_points, ground_table, ground_n);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_crown_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, double cell, int64_t* keys, int32_t* err,
                             tl_stream_t stream) {
  if (!sorted_xyz || !sorted_label || !keys || !err || n < 0 || !(cell > 0.0)) return TL_ERR_ARG;
  if (!aligned8(sorted_xyz) || !aligned8(sorted_label) || !aligned8(keys) || (reinterpret_cast<uintptr_t>(err) & 3)) return TL_ERR_ARG;
  if (hipMemsetAsync(err, 0, sizeof(int32_t), tl_s(stream)) != hipSuccess) return TL_ERR_LAUNCH;
  if (n == 0) return TL_OK;
  k_crown_keys<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(sorted_xyz, sorted_label, n, cell, keys, err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_crown_count(const int64_t* sorted_keys, int64_t n, int64_t n_trees, int64_t* cells, tl_stream_t stream) {
  if (!sorted_keys || !cells || n < 0 || n_trees < 0 || n_trees >= ((int64_t)1 << kCellBits)) return TL_ERR_ARG;
  if (!aligned8(sorted_keys) || !aligned8(cells)) return TL_ERR_ARG;
  if (n_trees == 0) return TL_OK;
  if (hipMemsetAsync(cells, 0, (size_t)n_trees * sizeof(int64_t), tl_s(stream)) != hipSuccess) return TL_ERR_LAUNCH;
  if (n == 0) return TL_OK;
  k_crown_count<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(sorted_keys, n, n_trees, cells);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
