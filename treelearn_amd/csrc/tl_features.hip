// Geometric point features on the device: the full eigen-feature set of the radius neighbourhood that the
// reference delegates to jakteristics 0.5.1 (compute_features(points, search_radius, feature_names=[...]),
// tree_learn/util/data_preparation.py:82-88).  jakteristics is absent from the reference tree and from this image: the
// definitions are restated here (parity unpinned, as for tl_verticality) and checked against tests/features_restatement.py.
//
// Input as for tl_verticality: points sorted by a (radius)-sized cell key with z fastest, so the points of one (x, y) COLUMN of cells
// are one run of the sorted array, ascending in z-cell.  The unit of work is a PIECE: up to 64 consecutive points of one column inside
// one aligned 64-block of the sorted array, one wave, one point per lane (a piece starts wherever the column changes or the index is a
// multiple of 64 -- a rule local to each index, so the table is one compaction).  With z-cells zmin..zmax in the piece, all its points
// share 9 candidate ranges: per (dx, dy) column the cells zmin-1 .. zmax+1, contiguous in the sorted array.  The wave finds them once
// (lanes 0..17, one binary search each), then stages every range through LDS in chunks of kChunk candidates: coalesced f64 loads of the
// next chunk are in flight while every lane walks the current one with broadcast LDS reads.  No lane searches or reads global memory
// per candidate.  A neighbour is a staged point with d^2 <= r^2 (the ranges hold at least the 27 cells around every point of the
// piece; what they hold beyond lies further than r).  Each lane adds its neighbours in the order of the sorted array -- ascending x
// column, then y column, then position -- in f64 relative to itself, under fp contract(off) with plain operators: the result is defined
// by the source order, does not depend on how points fall into pieces, and is the same bits on every run.
//
// Per point: sample covariance (n - 1), all three eigenpairs by cyclic Jacobi in f64, l1 >= l2 >= l3 clamped at 0, every
// eigenvector oriented by z >= 0 (then y >= 0, then x >= 0).  Fewer than 3 neighbours: NaN in every column but
// number_of_neighbors.  Only the requested columns are computed and stored.
//
// tl_eigen_features_scales: the same at 1 to 4 ascending radii in one launch.  The cells are those of the largest radius;
// one walk over the staged candidates feeds a count and nine sums per scale (k_eigen_features_scales<S>, accumulators in registers).
// Every scale's row is, bit for bit, the row of tl_eigen_features on the same sorted arrays at that radius.  The covariance, eigen3 and
// the column switch exist once (feature_row) for both kernels.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBits = 21;
constexpr int64_t kMask = (1ll << kBits) - 1;
constexpr int kChunk = 128;                         // candidates per LDS chunk: 3 KiB, two buffers
constexpr int kLoads = kChunk * 3 / 64;             // f64 loads per lane and chunk

struct FeatCols { int32_t id[TL_FEAT_COUNT]; int32_t F; };

enum : int {
  kEigenvalueSum = 0, kOmnivariance, kEigenentropy, kAnisotropy, kPlanarity, kLinearity, kPCA1, kPCA2, kSurfaceVariation, kSphericity,
  kVerticality, kNx, kNy, kNz, kNumberOfNeighbors, kEigenvalue1, kEigenvalue2, kEigenvalue3, kEigenvector1x
};

__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

__device__ __forceinline__ double pick3(const double v[3], int m) { return m == 0 ? v[0] : (m == 1 ? v[1] : v[2]); }
__device__ __forceinline__ double xlnx(double l) { return l > 0.0 ? l * log(l) : 0.0; }

// All eigenpairs of a symmetric 3x3 matrix by cyclic Jacobi (the sweep of tl_verticality's smallest_evec_z, here without contraction):
// lam[k] descending and clamped at 0, vec[k] = unit eigenvector of lam[k], oriented.
__device__ void eigen3(double a00, double a01, double a02, double a11, double a12, double a22, double lam[3], double vec[3][3]) {
  double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    if (off <= 1e-300 || off <= 1e-18 * (fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]))) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
      }
  }
  const double d[3] = {A[0][0], A[1][1], A[2][2]};
  int o0 = 0, o1 = 1, o2 = 2;                       // a stable three-element sort, descending
  if (pick3(d, o0) < pick3(d, o1)) { const int t = o0; o0 = o1; o1 = t; }
  if (pick3(d, o1) < pick3(d, o2)) { const int t = o1; o1 = o2; o2 = t; }
  if (pick3(d, o0) < pick3(d, o1)) { const int t = o0; o0 = o1; o1 = t; }
  const int o[3] = {o0, o1, o2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double l = pick3(d, o[k]);
    lam[k] = l > 0.0 ? l : 0.0;
    double x = pick3(V[0], o[k]), y = pick3(V[1], o[k]), z = pick3(V[2], o[k]);
    const bool flip = z < 0.0 || (z == 0.0 && (y < 0.0 || (y == 0.0 && x < 0.0)));
    if (flip) { x = -x; y = -y; z = -z; }
    vec[k][0] = x; vec[k][1] = y; vec[k][2] = z;
  }
}

// One output row from the neighbourhood sums of one point at one radius: the covariance, eigen3 and the column switch.  The one copy
// that k_eigen_features and k_eigen_features_scales share.
__device__ __forceinline__ void feature_row(int64_t cnt, double s0, double s1, double s2, double s00, double s01, double s02, double s11,
                                            double s12, double s22, const FeatCols& cols, float* __restrict__ o) {
  if (cnt < 3) {
    for (int c = 0; c < cols.F; ++c) o[c] = cols.id[c] == kNumberOfNeighbors ? (float)cnt : __builtin_nanf("");
    return;
  }
  const double inv_n = 1.0 / (double)cnt, inv = 1.0 / (double)(cnt - 1);
  double l[3], e[3][3];
  eigen3((s00 - s0 * s0 * inv_n) * inv, (s01 - s0 * s1 * inv_n) * inv, (s02 - s0 * s2 * inv_n) * inv,
         (s11 - s1 * s1 * inv_n) * inv, (s12 - s1 * s2 * inv_n) * inv, (s22 - s2 * s2 * inv_n) * inv, l, e);
  const double l1 = l[0], l2 = l[1], l3 = l[2], s = l1 + l2 + l3;
  for (int c = 0; c < cols.F; ++c) {
    double v;
    switch (cols.id[c]) {
      case kEigenvalueSum: v = s; break;
      case kOmnivariance: v = cbrt(l1 * l2 * l3); break;
      case kEigenentropy: v = -(xlnx(l1) + xlnx(l2) + xlnx(l3)); break;
      case kAnisotropy: v = (l1 - l3) / l1; break;
      case kPlanarity: v = (l2 - l3) / l1; break;
      case kLinearity: v = (l1 - l2) / l1; break;
      case kPCA1: v = l1 / s; break;
      case kPCA2: v = l2 / s; break;
      case kSurfaceVariation: v = l3 / s; break;
      case kSphericity: v = l3 / l1; break;
      case kVerticality: v = 1.0 - fabs(e[2][2]); break;
      case kNx: v = e[2][0]; break;
      case kNy: v = e[2][1]; break;
      case kNz: v = e[2][2]; break;
      case kNumberOfNeighbors: v = (double)cnt; break;
      case kEigenvalue1: v = l1; break;
      case kEigenvalue2: v = l2; break;
      case kEigenvalue3: v = l3; break;
      default: {
        const int k = cols.id[c] - kEigenvector1x;                 // 0..8, checked by the launcher
        const int a = k / 3, d = k - 3 * a;
        v = a == 0 ? pick3(e[0], d) : (a == 1 ? pick3(e[1], d) : pick3(e[2], d));
      }
    }
    o[c] = (float)v;
  }
}

__global__ void __launch_bounds__(64) k_eigen_features(const double* __restrict__ xyz, const int64_t* __restrict__ keys, int64_t n, double r2,
                                                       int64_t nx, int64_t ny, const int64_t* __restrict__ piece_start, int64_t n_pieces,
                                                       FeatCols cols, float* __restrict__ out) {
  __shared__ double buf[2][kChunk * 3];
  __shared__ int64_t rng[18];                       // [r][lo, hi) of the 9 (dx, dy) columns, x-major
  const int lane = threadIdx.x;
  const int64_t w = blockIdx.x;
  if (w >= n_pieces) return;
  const int64_t start = piece_start[w];
  if (start < 0 || start >= n) return;              // (uniform: nothing in a table can send the wave out of the arrays)
  const int64_t key = keys[start], col = key >> kBits;
  const int64_t cx = key >> (2 * kBits), cy = (key >> kBits) & kMask;
  const int64_t blk_end = ((start >> 6) + 1) << 6 < n ? ((start >> 6) + 1) << 6 : n;     // a piece stays inside its aligned 64-block
  const int64_t i = start + lane;
  const bool valid = i < blk_end && (keys[i < blk_end ? i : start] >> kBits) == col;       // (a prefix of the lanes: the array is sorted)
  const int nvalid = __popcll(__ballot(valid));
  if (lane < 18) {
    const int r = lane >> 1;
    const int64_t x = cx - 1 + r / 3, y = cy - 1 + r % 3;
    const int64_t zmin = key & kMask, zmax = keys[start + nvalid - 1] & kMask;
    const int64_t z0 = zmin > 0 ? zmin - 1 : 0, z1 = zmax < kMask ? zmax + 1 : kMask;
    int64_t v = 0;                                  // a column outside the plot: the empty range [0, 0)
    if (x >= 0 && x <= nx && y >= 0 && y <= ny) {
      const int64_t kb = (x << (2 * kBits)) | (y << kBits);
      v = lower_bound(keys, n, (lane & 1) ? (kb | z1) + 1 : (kb | z0));
    }
    rng[lane] = v;
  }
  __syncthreads();
  const int64_t ip = valid ? i : start;
  const double px = xyz[ip * 3], py = xyz[ip * 3 + 1], pz = xyz[ip * 3 + 2];

  // the chunks of the 9 ranges, in order
  int r = -1; int64_t off = 0, hi = 0;
  auto next = [&](int64_t& c_off, int& c_cnt) -> bool {
    while (off >= hi) { if (++r >= 9) return false; off = rng[2 * r]; hi = rng[2 * r + 1]; }
    c_off = off; c_cnt = (int)((hi - off) < (int64_t)kChunk ? (hi - off) : (int64_t)kChunk); off += c_cnt;
    return true;
  };
  double reg[kLoads];
  auto fetch = [&](int64_t c_off, int c_cnt) {
    const double* __restrict__ src = xyz + c_off * 3;
#pragma unroll
    for (int k = 0; k < kLoads; ++k) { const int idx = k * 64 + lane; reg[k] = idx < c_cnt * 3 ? src[idx] : 0.0; }
  };

  double s0 = 0, s1 = 0, s2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
  int64_t cnt = 0;
  int64_t c_off = 0; int c_cnt = 0, b = 0;
  bool have = next(c_off, c_cnt);
  if (have) fetch(c_off, c_cnt);
  while (have) {
    double* cur = buf[b];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) cur[k * 64 + lane] = reg[k];
    __syncthreads();
    const int m = c_cnt;
    have = next(c_off, c_cnt);
    if (have) fetch(c_off, c_cnt);                  // in flight while the lanes walk the current chunk
    for (int j = 0; j < m; ++j) {
      const double dx = cur[3 * j] - px, dy = cur[3 * j + 1] - py, dz = cur[3 * j + 2] - pz;
      if (dx * dx + dy * dy + dz * dz <= r2) {
        ++cnt; s0 += dx; s1 += dy; s2 += dz;
        s00 += dx * dx; s01 += dx * dy; s02 += dx * dz; s11 += dy * dy; s12 += dy * dz; s22 += dz * dz;
      }
    }
    b ^= 1;
  }
  if (!valid) return;

  feature_row(cnt, s0, s1, s2, s00, s01, s02, s11, s12, s22, cols, out + i * (int64_t)cols.F);
}

// S radii in one walk.  The cells are those of the LARGEST radius, so the 9 ranges hold every candidate of every scale; the
// work split, the staging and the order of the additions are those of k_eigen_features.  Scale k keeps its own count and nine sums and
// takes a candidate when the same d^2 <= r_k^2: its row is, bit for bit, what k_eigen_features gives on the same sorted arrays with
// radius r_k.  The accumulators are indexed by the unrolled k only (registers, no scratch).
struct FeatRadii2 { double v[TL_FEAT_MAX_SCALES]; };
struct FeatSums { double s0, s1, s2, s00, s01, s02, s11, s12, s22; int64_t cnt; };

template <int S>
__global__ void __launch_bounds__(64) k_eigen_features_scales(const double* __restrict__ xyz, const int64_t* __restrict__ keys, int64_t n,
                                                              FeatRadii2 r2, int64_t nx, int64_t ny, const int64_t* __restrict__ piece_start,
                                                              int64_t n_pieces, FeatCols cols, float* __restrict__ out) {
  __shared__ double buf[2][kChunk * 3];
  __shared__ int64_t rng[18];                       // [r][lo, hi) of the 9 (dx, dy) columns, x-major
  const int lane = threadIdx.x;
  const int64_t w = blockIdx.x;
  if (w >= n_pieces) return;
  const int64_t start = piece_start[w];
  if (start < 0 || start >= n) return;              // (uniform: nothing in a table can send the wave out of the arrays)
  const int64_t key = keys[start], col = key >> kBits;
  const int64_t cx = key >> (2 * kBits), cy = (key >> kBits) & kMask;
  const int64_t blk_end = ((start >> 6) + 1) << 6 < n ? ((start >> 6) + 1) << 6 : n;     // a piece stays inside its aligned 64-block
  const int64_t i = start + lane;
  const bool valid = i < blk_end && (keys[i < blk_end ? i : start] >> kBits) == col;       // (a prefix of the lanes: the array is sorted)
  const int nvalid = __popcll(__ballot(valid));
  if (lane < 18) {
    const int r = lane >> 1;
    const int64_t x = cx - 1 + r / 3, y = cy - 1 + r % 3;
    const int64_t zmin = key & kMask, zmax = keys[start + nvalid - 1] & kMask;
    const int64_t z0 = zmin > 0 ? zmin - 1 : 0, z1 = zmax < kMask ? zmax + 1 : kMask;
    int64_t v = 0;                                  // a column outside the plot: the empty range [0, 0)
    if (x >= 0 && x <= nx && y >= 0 && y <= ny) {
      const int64_t kb = (x << (2 * kBits)) | (y << kBits);
      v = lower_bound(keys, n, (lane & 1) ? (kb | z1) + 1 : (kb | z0));
    }
    rng[lane] = v;
  }
  __syncthreads();
  const int64_t ip = valid ? i : start;
  const double px = xyz[ip * 3], py = xyz[ip * 3 + 1], pz = xyz[ip * 3 + 2];

  // the chunks of the 9 ranges, in order
  int r = -1; int64_t off = 0, hi = 0;
  auto next = [&](int64_t& c_off, int& c_cnt) -> bool {
    while (off >= hi) { if (++r >= 9) return false; off = rng[2 * r]; hi = rng[2 * r + 1]; }
    c_off = off; c_cnt = (int)((hi - off) < (int64_t)kChunk ? (hi - off) : (int64_t)kChunk); off += c_cnt;
    return true;
  };
  double reg[kLoads];
  auto fetch = [&](int64_t c_off, int c_cnt) {
    const double* __restrict__ src = xyz + c_off * 3;
#pragma unroll
    for (int k = 0; k < kLoads; ++k) { const int idx = k * 64 + lane; reg[k] = idx < c_cnt * 3 ? src[idx] : 0.0; }
  };

  FeatSums a[S];
#pragma unroll
  for (int k = 0; k < S; ++k) a[k] = FeatSums{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int64_t c_off = 0; int c_cnt = 0, b = 0;
  bool have = next(c_off, c_cnt);
  if (have) fetch(c_off, c_cnt);
  while (have) {
    double* cur = buf[b];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) cur[k * 64 + lane] = reg[k];
    __syncthreads();
    const int m = c_cnt;
    have = next(c_off, c_cnt);
    if (have) fetch(c_off, c_cnt);                  // in flight while the lanes walk the current chunk
    for (int j = 0; j < m; ++j) {
      const double dx = cur[3 * j] - px, dy = cur[3 * j + 1] - py, dz = cur[3 * j + 2] - pz;
      const double d2 = dx * dx + dy * dy + dz * dz;
      if (d2 <= r2.v[S - 1]) {                      // (the radii ascend: outside the largest is outside all)
        const double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
#pragma unroll
        for (int k = 0; k < S; ++k)
          if (d2 <= r2.v[k]) {
            ++a[k].cnt; a[k].s0 += dx; a[k].s1 += dy; a[k].s2 += dz;
            a[k].s00 += xx; a[k].s01 += xy; a[k].s02 += xz; a[k].s11 += yy; a[k].s12 += yz; a[k].s22 += zz;
          }
      }
    }
    b ^= 1;
  }
  if (!valid) return;

#pragma unroll
  for (int k = 0; k < S; ++k)
    feature_row(a[k].cnt, a[k].s0, a[k].s1, a[k].s2, a[k].s00, a[k].s01, a[k].s02, a[k].s11, a[k].s12, a[k].s22, cols,
                out + (i * S + k) * (int64_t)cols.F);
}

template <int S>
void launch_scales(const double* xyz, const int64_t* keys, int64_t n, const FeatRadii2& r2, const int64_t* extent2, const int64_t* piece_start,
                   int64_t n_pieces, const FeatCols& fc, float* out, tl_stream_t stream) {
  k_eigen_features_scales<S><<<(unsigned)n_pieces, 64, 0, tl_s(stream)>>>(xyz, keys, n, r2, extent2[0], extent2[1], piece_start, n_pieces, fc, out);
}

}  // namespace

extern "C" {

int tl_eigen_features(const double* xyz_sorted, const int64_t* sorted_keys, int64_t n, double radius, const int64_t* extent2,
                      const int64_t* piece_start, int64_t n_pieces, const int32_t* cols, int F, float* out, tl_stream_t stream) {
  if (!xyz_sorted || !sorted_keys || !extent2 || !piece_start || !cols || !out || n <= 0 || n_pieces <= 0 || !(radius > 0)) return TL_ERR_ARG;
  if (F < 1 || F > TL_FEAT_COUNT || n_pieces > n || n_pieces > 0x7fffffffll) return TL_ERR_ARG;
  if (extent2[0] < 0 || extent2[0] > kMask || extent2[1] < 0 || extent2[1] > kMask) return TL_ERR_ARG;
  FeatCols fc;
  fc.F = F;
  for (int c = 0; c < TL_FEAT_COUNT; ++c) {
    fc.id[c] = c < F ? cols[c] : 0;
    if (c < F && (cols[c] < 0 || cols[c] >= TL_FEAT_COUNT)) return TL_ERR_ARG;
  }
  k_eigen_features<<<(unsigned)n_pieces, 64, 0, tl_s(stream)>>>(xyz_sorted, sorted_keys, n, radius * radius, extent2[0], extent2[1],
                                                                piece_start, n_pieces, fc, out);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_eigen_features_scales(const double* xyz_sorted, const int64_t* sorted_keys, int64_t n, const double* radii, int S, const int64_t* extent2,
                             const int64_t* piece_start, int64_t n_pieces, const int32_t* cols, int F, float* out, tl_stream_t stream) {
  if (!xyz_sorted || !sorted_keys || !radii || !extent2 || !piece_start || !cols || !out || n <= 0 || n_pieces <= 0) return TL_ERR_ARG;
  if (S < 1 || S > TL_FEAT_MAX_SCALES || F < 1 || F > TL_FEAT_COUNT || n_pieces > n || n_pieces > 0x7fffffffll) return TL_ERR_ARG;
  if (extent2[0] < 0 || extent2[0] > kMask || extent2[1] < 0 || extent2[1] > kMask) return TL_ERR_ARG;
  FeatRadii2 r2;
  for (int k = 0; k < TL_FEAT_MAX_SCALES; ++k) {
    const double r = radii[k < S ? k : S - 1];
    if (!(r > 0.0 && r < __builtin_inf()) || (k > 0 && k < S && !(r > radii[k - 1]))) return TL_ERR_ARG;      // (NaN fails)
    r2.v[k] = r * r;
  }
  FeatCols fc;
  fc.F = F;
  for (int c = 0; c < TL_FEAT_COUNT; ++c) {
    fc.id[c] = c < F ? cols[c] : 0;
    if (c < F && (cols[c] < 0 || cols[c] >= TL_FEAT_COUNT)) return TL_ERR_ARG;
  }
  switch (S) {
    case 1: launch_scales<1>(xyz_sorted, sorted_keys, n, r2, extent2, piece_start, n_pieces, fc, out, stream); break;
    case 2: launch_scales<2>(xyz_sorted, sorted_keys, n, r2, extent2, piece_start, n_pieces, fc, out, stream); break;
    case 3: launch_scales<3>(xyz_sorted, sorted_keys, n, r2, extent2, piece_start, n_pieces, fc, out, stream); break;
    default: launch_scales<4>(xyz_sorted, sorted_keys, n, r2, extent2, piece_start, n_pieces, fc, out, stream); break;
  }
  TL_CHECK_LAUNCH();
  return TL_OK;
}

}  // extern "C"
