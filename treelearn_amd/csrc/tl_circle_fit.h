// The circle fit that the inventory and the stem profiles share: the workgroup sum, the Kasa solve and the slice fit
// of one contiguous row range, for workgroups of kBlock threads.  Internal to tl_inventory.hip and tl_stem.hip; tl_wood.hip
// takes the Kasa solve and the wavefront sum.  Every formula is f64 in plain operators under the pragma below (no contraction into fma).
#pragma once
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

// Sum of K per-thread values over the workgroup, the same in every thread: xor butterfly inside a wave, then the wave sums added in
// wave order.  A fixed tree: the result depends on the values and their thread, not on timing.  s: kWaves * K doubles.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* __restrict__ s) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] = v[k] + __shfl_xor(v[k], o);
  __syncthreads();                           // the previous use of s has been read
  if ((tid & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) s[(tid >> 6) * K + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = s[k];
    for (int w = 1; w < kWaves; ++w) a = a + s[w * K + k];
    v[k] = a;
  }
}

// Sum of K per-lane values over one wavefront, the same in every lane: the xor butterfly alone.  No LDS, no barrier: the waves of a
// workgroup may call it independently (csrc/tl_wood.hip: one wave per node).
template <int K>
__device__ __forceinline__ void wave_sum(double (&v)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] = v[k] + __shfl_xor(v[k], o);
}

struct Fit { double cx, cy, r; int ok; };

// Kasa circle fit from the nine moments: Gaussian elimination with partial pivoting (first largest entry of the column).
__device__ Fit kasa_solve(const double (&m)[9], double cnt) {
  // m: Suu Suv Svv Su Sv Suw Svw Sw (m[8], the count, comes as cnt)
  double A[3][3] = {{m[0], m[1], m[3]}, {m[1], m[2], m[4]}, {m[3], m[4], cnt}};
  double b[3] = {m[5], m[6], m[7]};
  Fit f{0.0, 0.0, 0.0, 0};
  double big = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) big = fabs(A[i][j]) > big ? fabs(A[i][j]) : big;
  const double tol = 1e-12 * big;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int p = k;
#pragma unroll
    for (int i = k + 1; i < 3; ++i)
      if (fabs(A[i][k]) > fabs(A[p][k])) p = i;
    if (fabs(A[p][k]) < tol) return f;
#pragma unroll
    for (int i = k + 1; i < 3; ++i)
      if (i == p) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double t = A[k][j]; A[k][j] = A[i][j]; A[i][j] = t; }
        const double t = b[k]; b[k] = b[i]; b[i] = t;
      }
#pragma unroll
    for (int i = k + 1; i < 3; ++i) {
      const double g = A[i][k] / A[k][k];
#pragma unroll
      for (int j = k + 1; j < 3; ++j) A[i][j] = A[i][j] - g * A[k][j];
      b[i] = b[i] - g * b[k];
    }
  }
  const double x2 = b[2] / A[2][2];
  const double x1 = (b[1] - A[1][2] * x2) / A[1][1];
  const double x0 = ((b[0] - A[0][1] * x1) - A[0][2] * x2) / A[0][0];
  f.cx = x0 / 2.0;
  f.cy = x1 / 2.0;
  const double rr = (x2 + f.cx * f.cx) + f.cy * f.cy;
  if (!(rr > 0.0)) return f;
  f.r = sqrt(rr);
  f.ok = 1;
  return f;
}

// Trips (c) and (d) over the rows lo .. hi of one tree, by the whole workgroup: the moments of the slice rows (zc - half_thickness <= z <
// zc + half_thickness, within r2max of (px, py) horizontally), one lane solves the 3 x 3 system and broadcasts the circle through
// s_fit (3 doubles) and s_ok, then the residual sum.  Every thread returns the same fit, cnt (slice rows) and rss.  s_red: kWaves * 9.
__device__ __forceinline__ Fit slice_circle(const double* __restrict__ xyz, int64_t lo, int64_t hi, double px, double py, double zc,
                                            double half_thickness, double r2max, int64_t min_points, double* __restrict__ s_red,
                                            double* __restrict__ s_fit, int* __restrict__ s_ok, double& cnt, double& rss) {
  const int tid = threadIdx.x;
  const double z0 = zc - half_thickness, z1 = zc + half_thickness;
  double m[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // Suu Suv Svv Su Sv Suw Svw Sw count
  for (int64_t j = lo + tid; j < hi; j += kBlock) {
    const double z = xyz[3 * j + 2];
    if (!(z >= z0 && z < z1)) continue;
    const double u = xyz[3 * j] - px, v = xyz[3 * j + 1] - py;
    const double w = u * u + v * v;
    if (!(w < r2max)) continue;
    m[0] = m[0] + u * u; m[1] = m[1] + u * v; m[2] = m[2] + v * v; m[3] = m[3] + u; m[4] = m[4] + v;
    m[5] = m[5] + u * w; m[6] = m[6] + v * w; m[7] = m[7] + w; m[8] = m[8] + 1.0;
  }
  block_sum<9>(m, s_red);
  cnt = m[8];                                                  // an exact integer: fewer than 2^53 rows
  if (tid == 0) {                                              // one lane solves the 3 x 3 system
    Fit g{0.0, 0.0, 0.0, 0};
    if (cnt >= (double)min_points && cnt > 0.0) g = kasa_solve(m, cnt);
    s_fit[0] = g.cx; s_fit[1] = g.cy; s_fit[2] = g.r; *s_ok = g.ok;
  }
  __syncthreads();
  const Fit f{s_fit[0], s_fit[1], s_fit[2], *s_ok};
  // residuals of the fitted circle over the slice rows
  double e[1] = {0.0};
  if (f.ok) {
    for (int64_t j = lo + tid; j < hi; j += kBlock) {
      const double z = xyz[3 * j + 2];
      if (!(z >= z0 && z < z1)) continue;
      const double u = xyz[3 * j] - px, v = xyz[3 * j + 1] - py;
      if (!(u * u + v * v < r2max)) continue;
      const double du = u - f.cx, dv = v - f.cy;
      const double d = sqrt(du * du + dv * dv) - f.r;
      e[0] = e[0] + d * d;
    }
  }
  block_sum<1>(e, s_red);
  rss = e[0];
  return f;
}
}  // namespace
