// Statistical and radius outlier removal on the device: the two open3d filters SampleGenerator applies to every training crop and
// every inference tile (tree_learn/util/data_preparation.py:281-287,446-454; helpers sor_filter / rad_filter at :589-614).
//
//   tl_outlier_keys   cell keys of the points on a uniform grid, in Morton (z-curve) bit order
//   tl_knn_mean_dist  mean distance to the min(k, n) nearest points, the point itself included     <- remove_statistical_outlier
//   tl_sor_keep       cloud mean / standard deviation of those means, threshold, keep mask          <- remove_statistical_outlier
//   tl_radius_count   points strictly inside the ball of radius r                                   <- remove_radius_outlier
//
// open3d is not part of the reference tree: the semantics are restated in DESIGN §15 and that restatement is the specification.
// Exactness: all arithmetic is f64, d2 = (dx*dx + dy*dy) + dz*dz in that order under the pragma below (no fma contraction), sqrt is
// correctly rounded, the k smallest distances are added in ascending order one after the other.  The k smallest VALUES of a point are
// a property of the cloud, so `avg` does not depend on the grid, the launch geometry or the row order.
//
// Search form: the caller sorts the points by Morton key (one torch sort).  A cell of the grid coarsened s times (cell edge h * 2^s) is
// then the contiguous key range [m << 3s, (m + 1) << 3s) of the sorted array, so ONE sort serves every coarsening.  One wavefront works
// on one query: lanes 0..26 each find the row range of one of the 27 cells around the query's cell (two binary searches, all 27 in
// flight together), then the 64 lanes stride over the candidate rows.  When the k-th best distance is not yet below the edge of the
// current cells -- what any point outside the 27 cells is at least away -- the walk restarts one level coarser; at most 21 levels, the
// last of which is the whole grid, so it ends for a point tens of metres from every other.  The k best distances live one per lane,
// ascending by lane (k <= 64 = the wave width: no per-lane list, a handful of registers); a candidate below the k-th best is inserted
// with one ballot, one popcount and one lane shift.
#include "tl_common.h"
#include "tl_morton.h"                                 // the grid, the Morton key, the 27-cell range search

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kMaxK = 64;
constexpr int kChunk = 2048;                           // rows per partial of the two cloud sums (fixed: the sums do not depend on the grid)
constexpr double kInf = 1e300;

__device__ __forceinline__ int cell_of(double p, double lo, double h) { return (int)floor((p - lo) / h); }

__global__ void __launch_bounds__(kBlock) k_keys(const double* __restrict__ xyz, int64_t n, Grid g, int64_t* __restrict__ keys, int32_t* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    int c[3]; bool bad = false;
    for (int a = 0; a < 3; ++a) {
      const double q = floor((xyz[i * 3 + a] - g.lo[a]) / g.h);
      bad |= !(q >= 0.0 && q < (double)g.dims[a]);     // also a NaN coordinate
      c[a] = bad ? 0 : (int)q;
    }
    if (bad) { *err = 1; keys[i] = 0; continue; }
    keys[i] = (int64_t)morton(c[0], c[1], c[2]);
  }
}

__device__ __forceinline__ double dist2(const double* __restrict__ xyz, int64_t j, double x, double y, double z) {
  const double dx = xyz[j * 3] - x, dy = xyz[j * 3 + 1] - y, dz = xyz[j * 3 + 2] - z;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ int max_level(const Grid& g) {
  const int m = max(max(g.dims[0], g.dims[1]), g.dims[2]) - 1;
  int s = 0;
  while ((m >> s) > 0) ++s;
  return s;                                              // the first level at which the grid is one cell
}

// one wavefront per query row of the sorted array
__global__ void __launch_bounds__(kBlock) k_knn_mean(const double* __restrict__ xyz, const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                     int64_t n, Grid g, int k, double* __restrict__ avg) {
  const int lane = threadIdx.x & 63;
  const int kk = (int)(n < k ? n : k);
  const int top = max_level(g);
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * kWaves;
  for (int64_t q = w0; q < n; q += stride) {             // q is the same in all 64 lanes
    const double x = xyz[q * 3], y = xyz[q * 3 + 1], z = xyz[q * 3 + 2];
    const int qc[3] = {cell_of(x, g.lo[0], g.h), cell_of(y, g.lo[1], g.h), cell_of(z, g.lo[2], g.h)};
    double best = kInf;                                  // this lane's entry of the ascending list
    for (int s = 0;; ++s) {
      best = kInf;                                       // a coarser level sees the finer level's rows again: start over
      double tau = kInf;                                 // the kk-th best so far
      int64_t cs, ce;
      cell_range(keys, n, g, qc, s, lane, &cs, &ce);
      for (int c = 0; c < 27; ++c) {
        const int64_t a = __shfl(cs, c), e = __shfl(ce, c);
        for (int64_t j0 = a; j0 < e; j0 += 64) {
          const int64_t j = j0 + lane;
          const double d = j < e ? dist2(xyz, j, x, y, z) : kInf;
          uint64_t m = __ballot(d < tau);
          while (m) {
            const int b = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const double dv = __shfl(d, b);
            if (dv < tau) {                              // tau may have dropped since the ballot
              const int pos = __popcll(__ballot(best <= dv));          // best ascends with the lane: a prefix
              const double up = __shfl_up(best, 1);
              best = lane < pos ? best : (lane == pos ? dv : up);
              tau = __shfl(best, kk - 1);
            }
          }
        }
      }
      // a row outside the 27 cells is at least one cell edge away along some axis (0.999: the cell index is a rounded quotient)
      const double reach = 0.999 * g.h * (double)(1ll << s);
      if (tau < reach * reach || s >= top) break;
    }
    const double dist = sqrt(best);                      // llvm.sqrt.f64: correctly rounded
    double sum = 0.0;
    for (int t = 0; t < kk; ++t) sum += __shfl(dist, t);  // ascending, one after the other
    if (lane == 0) avg[perm[q]] = sum / (double)kk;
  }
}

// one wavefront per query row; h >= r, so the ball lies inside the 27 cells of level 0
__global__ void __launch_bounds__(kBlock) k_radius_count(const double* __restrict__ xyz, const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                         int64_t n, Grid g, double r2, int32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * kWaves;
  for (int64_t q = w0; q < n; q += stride) {
    const double x = xyz[q * 3], y = xyz[q * 3 + 1], z = xyz[q * 3 + 2];
    const int qc[3] = {cell_of(x, g.lo[0], g.h), cell_of(y, g.lo[1], g.h), cell_of(z, g.lo[2], g.h)};
    int64_t cs, ce;
    cell_range(keys, n, g, qc, 0, lane, &cs, &ce);
    int cnt = 0;
    for (int c = 0; c < 27; ++c) {
      const int64_t a = __shfl(cs, c), e = __shfl(ce, c);
      for (int64_t j0 = a; j0 < e; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool in = j < e && dist2(xyz, j, x, y, z) < r2;           // THE comparison of the radius filter: strict
        cnt += __popcll(__ballot(in));
      }
    }
    if (lane == 0) count[perm[q]] = cnt;
  }
}

// ---- the two cloud sums: partials over fixed chunks of kChunk rows, every reduction a fixed tree -> the same bits for any grid
__device__ __forceinline__ double block_sum(double v) {
  __shared__ double sh[kBlock];
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int off = kBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  return sh[0];
}
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int64_t nparts) {
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < nparts; i += kBlock) v += part[i];
  return block_sum(v);
}
__device__ __forceinline__ double cloud_mean(const double* __restrict__ part, int64_t nparts, int64_t n) { return sum_partials(part, nparts) / (double)n; }

__global__ void __launch_bounds__(kBlock) k_sum_parts(const double* __restrict__ avg, int64_t n, int64_t nparts, double* __restrict__ part) {
  for (int64_t p = blockIdx.x; p < nparts; p += gridDim.x) {
    double v = 0.0;
    for (int t = 0; t < kChunk / kBlock; ++t) {
      const int64_t i = p * kChunk + t * kBlock + threadIdx.x;
      if (i < n && avg[i] > 0.0) v += avg[i];
    }
    v = block_sum(v);
    if (threadIdx.x == 0) part[p] = v;
  }
}
__global__ void __launch_bounds__(kBlock) k_sq_parts(const double* __restrict__ avg, int64_t n, int64_t nparts, const double* __restrict__ part,
                                                     double* __restrict__ sq) {
  const double mean = cloud_mean(part, nparts, n);
  for (int64_t p = blockIdx.x; p < nparts; p += gridDim.x) {
    double v = 0.0;
    for (int t = 0; t < kChunk / kBlock; ++t) {
      const int64_t i = p * kChunk + t * kBlock + threadIdx.x;
      if (i < n && avg[i] > 0.0) { const double d = avg[i] - mean; v += d * d; }
    }
    v = block_sum(v);
    if (threadIdx.x == 0) sq[p] = v;
  }
}
__global__ void __launch_bounds__(kBlock) k_keep(const double* __restrict__ avg, int64_t n, int64_t nparts, const double* __restrict__ part,
                                                 const double* __restrict__ sq, double ratio, uint8_t* __restrict__ keep, double* __restrict__ thr_out) {
  const double mean = cloud_mean(part, nparts, n);
  const double sd = sqrt(sum_partials(sq, nparts) / (double)(n - 1));
  const double thr = mean + ratio * sd;
  if (blockIdx.x == 0 && threadIdx.x == 0) *thr_out = thr;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) keep[i] = avg[i] > 0.0 && avg[i] < thr;
}
__global__ void k_keep_none(uint8_t* __restrict__ keep, int64_t n, double* __restrict__ thr_out) {
  if (threadIdx.x == 0) *thr_out = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) keep[i] = 0;
}

unsigned wave_grid(int64_t n) {                          // one wavefront per row, at most 256 CUs x 8 blocks
  int64_t b = tl_cdiv(n, kWaves);
  if (b > 256 * 8) b = 256 * 8;
  return (unsigned)b;
}

}  // namespace

extern "C" {

int tl_outlier_keys(const double* xyz, int64_t n, const double lo[3], double h, const int32_t dims[3], int64_t* keys, int32_t* err,
                    tl_stream_t stream) {
  Grid g;
  if (!xyz || !keys || !err || n <= 0) return TL_ERR_ARG;
  if (!make_grid(lo, dims, h, &g)) return TL_ERR_UNSUPPORTED;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(err, 0, sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  k_keys<<<tl_grid(n, kBlock), kBlock, 0, s>>>(xyz, n, g, keys, err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_knn_mean_dist(const double* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n, const double lo[3], double h,
                     const int32_t dims[3], int k, double* avg, tl_stream_t stream) {
  Grid g;
  if (!xyz_sorted || !keys_sorted || !perm || !avg || n <= 0) return TL_ERR_ARG;
  if (k < 1 || k > kMaxK || !make_grid(lo, dims, h, &g)) return TL_ERR_UNSUPPORTED;
  k_knn_mean<<<wave_grid(n), kBlock, 0, tl_s(stream)>>>(xyz_sorted, keys_sorted, perm, n, g, k, avg);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int64_t tl_sor_ws_doubles(int64_t n) { return 2 * tl_cdiv(n > 0 ? n : 1, kChunk); }

int tl_sor_keep(const double* avg, int64_t n, double std_ratio, uint8_t* keep, double* thr, double* ws, tl_stream_t stream) {
  if (!avg || !keep || !thr || !ws || n <= 0) return TL_ERR_ARG;
  hipStream_t s = tl_s(stream);
  if (n == 1) {                                          // the standard deviation divides by n - 1: nothing is kept
    k_keep_none<<<1, 64, 0, s>>>(keep, n, thr);
    TL_CHECK_LAUNCH();
    return TL_OK;
  }
  const int64_t nparts = tl_cdiv(n, kChunk);
  const unsigned gp = (unsigned)(nparts < 256 * 8 ? nparts : 256 * 8);
  k_sum_parts<<<gp, kBlock, 0, s>>>(avg, n, nparts, ws);
  k_sq_parts<<<gp, kBlock, 0, s>>>(avg, n, nparts, ws, ws + nparts);
  k_keep<<<tl_grid(n, kBlock), kBlock, 0, s>>>(avg, n, nparts, ws, ws + nparts, std_ratio, keep, thr);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_radius_count(const double* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t n, const double lo[3], double h,
                    const int32_t dims[3], double radius, int32_t* count, tl_stream_t stream) {
  Grid g;
  if (!xyz_sorted || !keys_sorted || !perm || !count || n <= 0 || !(radius > 0.0)) return TL_ERR_ARG;
  if (!make_grid(lo, dims, h, &g)) return TL_ERR_UNSUPPORTED;
  if (h < radius * 1.0001) return TL_ERR_ARG;            // the 27 cells must hold the ball (margin: the cell index is a rounded quotient)
  k_radius_count<<<wave_grid(n), kBlock, 0, tl_s(stream)>>>(xyz_sorted, keys_sorted, perm, n, g, radius * radius, count);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

}  // extern "C"
