// Two epochs of one plot on the device: the hot path of rigid registration (ICP), cloud-to-cloud distances and tree matching.
//
//   tl_cross_nn     nearest reference point of every query, the query moved by a rigid transform on the fly, capped by a distance
//   tl_rigid_sums   the 17 sums one ICP step needs, over the accepted pairs, as a fixed tree
//
// The semantics are the project's own; tests/change_restatement.py states them in numpy and that restatement is the specification.
// Exactness: all arithmetic is f64 under the pragma below (no fma contraction), f32 queries are widened first.
//   moved query   x'_a = ((T[a][0]*x + T[a][1]*y) + T[a][2]*z) + T[a][3]
//   distance      d2 = (dx*dx + dy*dy) + dz*dz
// so nn and d2 are properties of the two clouds and the transform: they do not depend on the grid, the launch geometry or the row order
// of the reference (ties in d2 go to the smaller ORIGINAL reference row).
//
// Search form: the reference is binned and Morton-sorted exactly as tl_outlier.hip's clouds are (tl_outlier_keys + one torch sort,
// csrc/tl_morton.h).  One wavefront works on one query: lanes 0..26 each find the row range of one of the 27 cells around the moved
// query's cell, the 64 lanes stride over the candidate rows, the wave reduces the (d2, original row) minimum with a xor butterfly.  The
// cell edge is at least 1.0001 * max_dist, so every candidate below max_dist lies in those 27 cells.  A moved query may lie anywhere: its
// cell index is clamped in f64 to -2 .. dims + 1 before it becomes an integer (at -2 and dims + 1 none of the 27 cells is inside the grid).
//
// Sums: rows in fixed chunks of 2048 in query-row order; within a chunk the halving tree s[i] += s[i + stride], stride 1024 .. 1, missing
// rows holding +0.0; the chunk partials are reduced by the same tree, 2048 at a time, until one is left.  256 threads: thread t owns rows
// t + 256 k (strides 1024, 512, 256 are per-thread adds), strides 128 and 64 go through LDS, strides 32 .. 1 are a xor butterfly in the
// first wavefront.  No atomics: the same bits on every run and for any launch geometry.
#include "tl_common.h"
#include "tl_morton.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kChunk = 2048;                           // rows per partial (fixed: the sums do not depend on the launch)
constexpr int kTerms = 17;
constexpr int64_t kNone = INT64_MAX;

struct Xf { double t[12]; };                           // row-major 3 x 4

__device__ __forceinline__ void move_point(const Xf& T, double x, double y, double z, double p[3]) {
  for (int a = 0; a < 3; ++a) p[a] = ((T.t[4 * a] * x + T.t[4 * a + 1] * y) + T.t[4 * a + 2] * z) + T.t[4 * a + 3];
}

// cell index of a finite coordinate, clamped in f64: -2 and dim + 1 stand for everything farther out
__device__ __forceinline__ int clamped_cell(double p, double lo, double h, int dim) {
  double c = floor((p - lo) / h);
  c = !(c >= -2.0) ? -2.0 : c;
  c = c > (double)(dim + 1) ? (double)(dim + 1) : c;
  return (int)c;
}

__device__ __forceinline__ bool closer(double d, int64_t i, double bd, int64_t bi) { return d < bd || (d == bd && i < bi); }

// one wavefront per query row
template <typename F>
__global__ void __launch_bounds__(kBlock) k_cross_nn(const double* __restrict__ xyz, const int64_t* __restrict__ keys, const int64_t* __restrict__ perm,
                                                     int64_t nr, Grid g, const F* __restrict__ q, int64_t ld, int64_t nq, Xf T, double r2,
                                                     int64_t* __restrict__ nn, double* __restrict__ d2) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), stride = (int64_t)gridDim.x * kWaves;
  for (int64_t i = w0; i < nq; i += stride) {            // i is the same in all 64 lanes
    double p[3];
    move_point(T, (double)q[i * ld], (double)q[i * ld + 1], (double)q[i * ld + 2], p);
    double bd = HUGE_VAL; int64_t bi = kNone;
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
      const int qc[3] = {clamped_cell(p[0], g.lo[0], g.h, g.dims[0]), clamped_cell(p[1], g.lo[1], g.h, g.dims[1]),
                         clamped_cell(p[2], g.lo[2], g.h, g.dims[2])};
      int64_t cs, ce;
      cell_range(keys, nr, g, qc, 0, lane, &cs, &ce);
      for (int c = 0; c < 27; ++c) {
        const int64_t a = __shfl(cs, c), e = __shfl(ce, c);
        for (int64_t j = a + lane; j < e; j += 64) {
          const double dx = xyz[j * 3] - p[0], dy = xyz[j * 3 + 1] - p[1], dz = xyz[j * 3 + 2] - p[2];
          const double d = (dx * dx + dy * dy) + dz * dz;
          if (d < r2) {                                  // THE comparison of the cap: strict
            const int64_t o = perm[j];
            if (closer(d, o, bd, bi)) { bd = d; bi = o; }
          }
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(bd, off); const int64_t oi = __shfl_xor(bi, off);
        if (closer(od, oi, bd, bi)) { bd = od; bi = oi; }
      }
    }
    if (lane == 0) { nn[i] = bi == kNone ? -1 : bi; d2[i] = bi == kNone ? HUGE_VAL : bd; }
  }
}

__global__ void __launch_bounds__(kBlock) k_no_neighbour(int64_t nq, int64_t* __restrict__ nn, double* __restrict__ d2) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nq; i += (int64_t)gridDim.x * kBlock) { nn[i] = -1; d2[i] = HUGE_VAL; }
}

// ---- the halving tree over one chunk of 2048 items of 17 values; `item(i, o)` fills o[17] (+0.0 for a missing item)
template <typename Item>
__device__ __forceinline__ void chunk_tree(int64_t first, Item item, double* __restrict__ out) {
  __shared__ double sh[kTerms][kBlock / 2];
  const int t = threadIdx.x;
  double w[2][kTerms];
  for (int h = 0; h < 2; ++h) {                          // h = 0: rows t + 256 {0, 4, 2, 6}, h = 1: rows t + 256 {1, 5, 3, 7}
    double u[2][kTerms];
    for (int e = 0; e < 2; ++e) {
      const int k = h + 2 * e;                           // stride 1024: row k with row k + 4
      double r0[kTerms], r1[kTerms];
      item(first + t + kBlock * k, r0);
      item(first + t + kBlock * (k + 4), r1);
      for (int m = 0; m < kTerms; ++m) u[e][m] = r0[m] + r1[m];
    }
    for (int m = 0; m < kTerms; ++m) w[h][m] = u[0][m] + u[1][m];        // stride 512
  }
  double v[kTerms];
  for (int m = 0; m < kTerms; ++m) v[m] = w[0][m] + w[1][m];             // stride 256
  __syncthreads();                                       // (the LDS of a previous chunk has been read)
  if (t >= 128) for (int m = 0; m < kTerms; ++m) sh[m][t - 128] = v[m];
  __syncthreads();
  if (t < 128) for (int m = 0; m < kTerms; ++m) v[m] += sh[m][t];        // stride 128
  __syncthreads();
  if (t >= 64 && t < 128) for (int m = 0; m < kTerms; ++m) sh[m][t - 64] = v[m];
  __syncthreads();
  if (t < 64) {
    for (int m = 0; m < kTerms; ++m) {
      v[m] += sh[m][t];                                  // stride 64
      for (int off = 32; off > 0; off >>= 1) v[m] += __shfl_xor(v[m], off);      // strides 32 .. 1: lane i < off adds lane i + off
      if (t == 0) out[m] = v[m];
    }
  }
}

template <typename F>
__global__ void __launch_bounds__(kBlock) k_rigid_rows(const F* __restrict__ q, int64_t ld, int64_t nq, Xf T, const int64_t* __restrict__ nn,
                                                       const double* __restrict__ d2, const double* __restrict__ ref, int64_t nr, double cx, double cy,
                                                       double cz, double reject2, int64_t nparts, double* __restrict__ part) {
  auto item = [&](int64_t i, double* o) {
    for (int m = 0; m < kTerms; ++m) o[m] = 0.0;
    if (i >= nq) return;
    const int64_t j = nn[i]; const double d = d2[i];
    if (!(j >= 0 && j < nr && d < reject2)) return;
    double p[3];
    move_point(T, (double)q[i * ld], (double)q[i * ld + 1], (double)q[i * ld + 2], p);
    const double a[3] = {p[0] - cx, p[1] - cy, p[2] - cz};
    const double b[3] = {ref[j * 3] - cx, ref[j * 3 + 1] - cy, ref[j * 3 + 2] - cz};
    o[0] = 1.0;
    for (int r = 0; r < 3; ++r) { o[1 + r] = a[r]; o[4 + r] = b[r]; }
    for (int r = 0; r < 3; ++r) for (int s = 0; s < 3; ++s) o[7 + 3 * r + s] = a[r] * b[s];
    o[16] = d;
  };
  for (int64_t p = blockIdx.x; p < nparts; p += gridDim.x) chunk_tree(p * kChunk, item, part + p * kTerms);
}

__global__ void __launch_bounds__(kBlock) k_rigid_level(const double* __restrict__ in, int64_t n, int64_t nparts, double* __restrict__ part) {
  auto item = [&](int64_t i, double* o) {
    for (int m = 0; m < kTerms; ++m) o[m] = i < n ? in[i * kTerms + m] : 0.0;
  };
  for (int64_t p = blockIdx.x; p < nparts; p += gridDim.x) chunk_tree(p * kChunk, item, part + p * kTerms);
}

bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }

bool query_ok(const void* q, int dtype_f64, int64_t ld, int64_t nq) {
  return q && (dtype_f64 == 0 || dtype_f64 == 1) && ld >= 3 && nq >= 0 && nq < ((int64_t)1 << 40) && ld < ((int64_t)1 << 20) &&
         aligned(q, dtype_f64 ? 8 : 4);
}

bool load_transform(const double* T, Xf* x) {
  static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (T && !aligned(T, 8)) return false;
  for (int k = 0; k < 12; ++k) x->t[k] = T ? T[k] : eye[k];
  return true;
}

unsigned wave_grid(int64_t n) {                          // one wavefront per row, at most 256 CUs x 8 blocks
  int64_t b = tl_cdiv(n, kWaves);
  if (b > 256 * 8) b = 256 * 8;
  return (unsigned)b;
}

unsigned part_grid(int64_t nparts) { return (unsigned)(nparts < 256 * 8 ? nparts : 256 * 8); }

}  // namespace

extern "C" {

int tl_cross_nn(const double* xyz_sorted, const int64_t* keys_sorted, const int64_t* perm, int64_t nr, const double lo[3], double h,
                const int32_t dims[3], const void* q, int dtype_f64, int64_t ld, int64_t nq, const double* T, double max_dist, int64_t* nn,
                double* d2, tl_stream_t stream) {
  Xf x;
  if (!query_ok(q, dtype_f64, ld, nq) || !nn || !d2 || !aligned(nn, 8) || !aligned(d2, 8) || !load_transform(T, &x)) return TL_ERR_ARG;
  if (nr < 0 || nr >= ((int64_t)1 << 40) || !(max_dist > 0.0) || !(max_dist <= 1e150)) return TL_ERR_ARG;
  if (nr > 0 && (!xyz_sorted || !keys_sorted || !perm || !aligned(xyz_sorted, 8) || !aligned(keys_sorted, 8) || !aligned(perm, 8))) return TL_ERR_ARG;
  Grid g = {};
  if (nr > 0) {
    if (!make_grid(lo, dims, h, &g)) return TL_ERR_UNSUPPORTED;
    if (!isfinite(h) || !isfinite(lo[0]) || !isfinite(lo[1]) || !isfinite(lo[2])) return TL_ERR_ARG;
    if (h < max_dist * 1.0001) return TL_ERR_ARG;        // the 27 cells must hold the ball (margin: the cell index is a rounded quotient)
  }
  if (nq == 0) return TL_OK;
  hipStream_t s = tl_s(stream);
  if (nr == 0) {
    k_no_neighbour<<<tl_grid(nq, kBlock), kBlock, 0, s>>>(nq, nn, d2);
  } else if (dtype_f64) {
    k_cross_nn<double><<<wave_grid(nq), kBlock, 0, s>>>(xyz_sorted, keys_sorted, perm, nr, g, static_cast<const double*>(q), ld, nq, x,
                                                        max_dist * max_dist, nn, d2);
  } else {
    k_cross_nn<float><<<wave_grid(nq), kBlock, 0, s>>>(xyz_sorted, keys_sorted, perm, nr, g, static_cast<const float*>(q), ld, nq, x,
                                                       max_dist * max_dist, nn, d2);
  }
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int64_t tl_rigid_sums_ws_doubles(int64_t nq) {
  int64_t n = nq > 0 ? nq : 1, total = 0;
  do { n = tl_cdiv(n, kChunk); total += n; } while (n > 1);
  return kTerms * total;
}

int tl_rigid_sums(const void* q, int dtype_f64, int64_t ld, int64_t nq, const double* T, const int64_t* nn, const double* d2, const double* ref,
                  int64_t nr, const double c[3], double reject2, double* sums, double* ws, tl_stream_t stream) {
  Xf x;
  if (!query_ok(q, dtype_f64, ld, nq) || !nn || !d2 || !c || !sums || !ws || !load_transform(T, &x)) return TL_ERR_ARG;
  if (!aligned(nn, 8) || !aligned(d2, 8) || !aligned(ref, 8) || !aligned(sums, 8) || !aligned(ws, 8)) return TL_ERR_ARG;
  if (nr < 0 || nr >= ((int64_t)1 << 40) || (nr > 0 && !ref) || !(reject2 >= 0.0)) return TL_ERR_ARG;
  if (!isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2])) return TL_ERR_ARG;
  hipStream_t s = tl_s(stream);
  if (nq == 0) {                                         // a tree over nothing but padding
    if (hipMemsetAsync(sums, 0, kTerms * sizeof(double), s) != hipSuccess) return TL_ERR_LAUNCH;
    return TL_OK;
  }
  int64_t nparts = tl_cdiv(nq, kChunk);
  double* out = nparts == 1 ? sums : ws;
  if (dtype_f64)
    k_rigid_rows<double><<<part_grid(nparts), kBlock, 0, s>>>(static_cast<const double*>(q), ld, nq, x, nn, d2, ref, nr, c[0], c[1], c[2], reject2,
                                                              nparts, out);
  else
    k_rigid_rows<float><<<part_grid(nparts), kBlock, 0, s>>>(static_cast<const float*>(q), ld, nq, x, nn, d2, ref, nr, c[0], c[1], c[2], reject2,
                                                             nparts, out);
  TL_CHECK_LAUNCH();
  while (nparts > 1) {                                   // the same tree over the partials, 2048 at a time
    const double* in = out;
    const int64_t n = nparts;
    nparts = tl_cdiv(n, kChunk);
    out = nparts == 1 ? sums : out + n * kTerms;
    k_rigid_level<<<part_grid(nparts), kBlock, 0, s>>>(in, n, nparts, out);
    TL_CHECK_LAUNCH();
  }
  return TL_OK;
}

}  // extern "C"
