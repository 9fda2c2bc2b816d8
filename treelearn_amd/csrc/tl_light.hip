// Light under the canopy: a bit grid of the occupied voxels of a cloud and a ray march through it that counts, per origin and zenith ring,
// how the rays of a direction table end (the semantics are the project's own, restated in numpy in
// tests/light_restatement.py).
// tl_light_voxels: one pass over the rows: the voxel of a row by the terrain's rule in three axes, its bit by an integer atomicOr into
//   u32 words along x, and with labels the largest label of the voxel by an integer atomicMax.  A lane reads the word (the owner) first
//   and issues the atomic only where it would still change something: bits only get set and owners only grow, so a stale read costs an
//   atomic, never a result.
// tl_light_march: one wave serves 64 consecutive directions of one origin; the waves of the launch stride over (origin, chunk of 64
//   directions) pairs, which covers many origins x a few hundred directions and one origin x 10^5 directions alike.  A lane walks its ray
//   voxel by voxel: the time to the next plane of every axis is recomputed from the integer index each time it changes, never
//   accumulated, so the voxel sequence is a pure function of the indices.  Exit codes are combined per wave: for every ring present among
//   the lanes, one ballot and popcount per code and one integer atomicAdd by the ring's first lane.
// Every formula is f64 in plain operators under the pragma below (no contraction into fma); the only atomics are integer ones, so every
// output has the same bits for any row order and any order of the waves.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kMaxSide = 8192;
constexpr int64_t kMaxVoxels = (int64_t)1 << 31;
constexpr int64_t kMaxOwned = (int64_t)1 << 28;
constexpr int kMaxRings = 1 << 16;
constexpr double kDblMax = 1.7976931348623157e308;

struct Grid {
  double v, i0[3];
  int n[3];
  int wx;                                                            // u32 words per x row of occ
};

template <typename T>
__global__ void __launch_bounds__(kBlock) k_light_voxels(const T* __restrict__ pts, int64_t ld, int64_t n, const int64_t* __restrict__ labels, Grid g,
                                                         unsigned int* __restrict__ occ, int32_t* __restrict__ owner, int32_t* __restrict__ err) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double x = (double)pts[i * ld], y = (double)pts[i * ld + 1], z = (double)pts[i * ld + 2];
    const double fx = floor(x / g.v) - g.i0[0], fy = floor(y / g.v) - g.i0[1], fz = floor(z / g.v) - g.i0[2];
    const bool inside = fx >= 0.0 && fx < (double)g.n[0] && fy >= 0.0 && fy < (double)g.n[1] && fz >= 0.0 && fz < (double)g.n[2];   // (NaN fails)
    if (!inside) { *err = 1; continue; }
    const int ix = (int)fx;
    const int64_t row = (int64_t)fz * g.n[1] + (int64_t)fy;
    unsigned int* w = occ + row * g.wx + (ix >> 5);
    const unsigned int bit = 1u << (ix & 31);
    if (!(*w & bit)) atomicOr(w, bit);
    if (labels) {
      const int64_t l = labels[i];
      if (l > 2147483647ll || l < -2147483648ll) { *err = 1; continue; }
      int32_t* o = owner + row * g.n[0] + ix;
      if (l >= 0 && *o < (int32_t)l) atomicMax(o, (int32_t)l);
    }
  }
}

// the time at which the ray o + t d meets the plane that bounds voxel index i of an axis on the side it moves to (s != 0)
__device__ __forceinline__ double plane_time(double i0, int i, int s, double v, double o, double d) {
  return ((i0 + (double)(i + (s > 0 ? 1 : 0))) * v - o) / d;
}

__global__ void __launch_bounds__(kBlock) k_light_march(const double* __restrict__ origins, const int32_t* __restrict__ skip, int64_t P,
                                                        const double* __restrict__ dirs, const int32_t* __restrict__ ring, int64_t D, int R,
                                                        const unsigned int* __restrict__ occ, const int32_t* __restrict__ owner, Grid g,
                                                        double max_range, int min_hits, int32_t* __restrict__ counts,
                                                        int32_t* __restrict__ status, uint8_t* __restrict__ code_out, double* __restrict__ first_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t chunks = D > 0 ? (D + kWave - 1) / kWave : 1;
  const int64_t jobs = P * chunks;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
  const int max_steps = g.n[0] + g.n[1] + g.n[2];
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  for (int64_t job = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave); job < jobs; job += waves) {   // wave-uniform
    const int64_t p = job / chunks, d = (job - p * chunks) * kWave + lane;
    const double o[3] = {origins[p * 3], origins[p * 3 + 1], origins[p * 3 + 2]};
    int i[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double f = floor(o[a] / g.v) - g.i0[a];
      inside = inside && f >= 0.0 && f < (double)g.n[a];                 // (a NaN origin is outside)
      i[a] = inside ? (int)f : 0;
    }
    if (job == p * chunks && lane == 0) status[p] = inside ? 0 : 1;
    const bool live = d < D;
    int code = -1, r = -1;
    double first = nan;
    if (live && inside) {
      const int sk = (skip && owner) ? skip[p] : -1;
      r = ring[d];
      if (r < 0 || r >= R) r = -1;                                       // (the host checks the table; a ring outside it is counted nowhere)
      double dv[3], t[3];
      int s[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        dv[a] = dirs[d * 3 + a];
        s[a] = dv[a] > 0.0 ? 1 : (dv[a] < 0.0 ? -1 : 0);
        t[a] = s[a] != 0 ? plane_time(g.i0[a], i[a], s[a], g.v, o[a], dv[a]) : inf;
      }
      int hits = 0;
      code = 2;                                                          // (only a walk that runs out of steps keeps this; none does)
      for (int step = 0; step < max_steps; ++step) {
        int a = 0;
        if (t[1] < t[0]) a = 1;
        if (t[2] < t[a]) a = 2;                                          // ties go to x, then y, then z
        const double t_enter = t[a];
        if (t_enter > max_range) { code = 2; break; }
        // (t_enter is finite here, so s[a] != 0)
        const int sa = a == 0 ? s[0] : (a == 1 ? s[1] : s[2]);
        const int ia = (a == 0 ? i[0] : (a == 1 ? i[1] : i[2])) + sa;
        const int na = a == 0 ? g.n[0] : (a == 1 ? g.n[1] : g.n[2]);
        if (ia < 0 || ia >= na) { code = (a == 2 && sa > 0) ? 1 : 3; break; }
        if (a == 0) { i[0] = ia; t[0] = plane_time(g.i0[0], ia, sa, g.v, o[0], dv[0]); }
        else if (a == 1) { i[1] = ia; t[1] = plane_time(g.i0[1], ia, sa, g.v, o[1], dv[1]); }
        else { i[2] = ia; t[2] = plane_time(g.i0[2], ia, sa, g.v, o[2], dv[2]); }
        const int64_t row = (int64_t)i[2] * g.n[1] + i[1];
        if ((occ[row * g.wx + (i[0] >> 5)] >> (i[0] & 31)) & 1u) {
          if (sk < 0 || owner[row * g.n[0] + i[0]] != sk) {
            if (++hits >= min_hits) { code = 0; first = t_enter; break; }
          }
        }
      }
    }
    if (live) {
      if (code_out) code_out[p * D + d] = inside ? (uint8_t)code : (uint8_t)255;
      if (first_out) first_out[p * D + d] = first;
    }
    // per ring present among the lanes: one ballot and popcount per exit code, added by the ring's first lane
    uint64_t todo = __ballot(r >= 0);
    while (todo) {                                                       // wave-uniform
      const int lead = __ffsll((unsigned long long)todo) - 1;
      const int r0 = __shfl(r, lead);
      const bool mine = r == r0;
      const uint64_t same = __ballot(mine);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint64_t m = __ballot(mine && code == c);
        if (lane == lead && m) atomicAdd(counts + ((p * R + r0) * 4 + c), (int32_t)__popcll((unsigned long long)m));
      }
      todo &= ~same;
    }
  }
}

bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }
bool is_finite(double v) { return v >= -kDblMax && v <= kDblMax; }
bool index_ok(int64_t i0) { return i0 > -((int64_t)1 << 52) && i0 < ((int64_t)1 << 52); }           // exact as a double
bool grid_ok(double voxel, int64_t ix0, int64_t iy0, int64_t iz0, int nx, int ny, int nz, bool owned) {
  if (!(voxel > 0.0) || !is_finite(voxel) || !index_ok(ix0) || !index_ok(iy0) || !index_ok(iz0)) return false;
  if (nx < 0 || ny < 0 || nz < 0 || nx > kMaxSide || ny > kMaxSide || nz > kMaxSide) return false;
  return (int64_t)nx * ny * nz <= (owned ? kMaxOwned : kMaxVoxels);
}
Grid grid_of(double voxel, int64_t ix0, int64_t iy0, int64_t iz0, int nx, int ny, int nz) {
  Grid g;
  g.v = voxel;
  g.i0[0] = (double)ix0; g.i0[1] = (double)iy0; g.i0[2] = (double)iz0;
  g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
  g.wx = (nx + 31) / 32;
  return g;
}
}  // namespace

extern "C" int tl_light_voxels(const void* pts, int dtype_f64, int64_t ld, int64_t n, const int64_t* labels, double voxel, int64_t ix0, int64_t iy0,
                               int64_t iz0, int nx, int ny, int nz, uint32_t* occ, int32_t* owner, int32_t* err, tl_stream_t stream) {
  if (!pts || !occ || !err || n < 0 || ld < 3 || (dtype_f64 != 0 && dtype_f64 != 1) || (labels != nullptr) != (owner != nullptr)) return TL_ERR_ARG;
  if (!grid_ok(voxel, ix0, iy0, iz0, nx, ny, nz, owner != nullptr)) return TL_ERR_ARG;
  if (!aligned(pts, dtype_f64 ? 8 : 4) || !aligned(labels, 8) || !aligned(occ, 4) || !aligned(owner, 4) || !aligned(err, 4)) return TL_ERR_ARG;
  const int64_t cells = (int64_t)nx * ny * nz;
  if (n > 0 && cells == 0) return TL_ERR_ARG;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(err, 0, sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (cells == 0) return TL_OK;
  const Grid g = grid_of(voxel, ix0, iy0, iz0, nx, ny, nz);
  if (hipMemsetAsync(occ, 0, (size_t)nz * ny * g.wx * sizeof(uint32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (owner && hipMemsetAsync(owner, 0xff, (size_t)cells * sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (n == 0) return TL_OK;
  if (dtype_f64)
    k_light_voxels<double><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const double*>(pts), ld, n, labels, g, occ, owner, err);
  else
    k_light_voxels<float><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const float*>(pts), ld, n, labels, g, occ, owner, err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_light_march(const double* origins, const int32_t* skip, int64_t n_origins, const double* dirs, const int32_t* ring, int64_t n_dirs,
                              int n_rings, const uint32_t* occ, const int32_t* owner, double voxel, int64_t ix0, int64_t iy0, int64_t iz0, int nx,
                              int ny, int nz, double max_range, int min_hits, int32_t* counts, int32_t* status, uint8_t* code, double* first,
                              tl_stream_t stream) {
  if (!origins || !dirs || !ring || !occ || !counts || !status || n_origins < 0 || n_dirs < 0) return TL_ERR_ARG;
  if (n_rings < 1 || n_rings > kMaxRings || min_hits < 1 || !(max_range > 0.0) || !is_finite(max_range)) return TL_ERR_ARG;
  if (!grid_ok(voxel, ix0, iy0, iz0, nx, ny, nz, owner != nullptr)) return TL_ERR_ARG;
  if (n_origins > ((int64_t)1 << 40) / n_rings || (n_dirs > 0 && n_origins > ((int64_t)1 << 46) / n_dirs)) return TL_ERR_ARG;
  if (!aligned(origins, 8) || !aligned(skip, 4) || !aligned(dirs, 8) || !aligned(ring, 4) || !aligned(occ, 4) || !aligned(owner, 4) ||
      !aligned(counts, 4) || !aligned(status, 4) || !aligned(first, 8))
    return TL_ERR_ARG;
  if (n_origins > 0 && (int64_t)nx * ny * nz == 0) return TL_ERR_ARG;    // origins without a grid
  if (n_origins == 0) return TL_OK;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(counts, 0, (size_t)n_origins * n_rings * 4 * sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  const int64_t chunks = n_dirs > 0 ? (n_dirs + kWave - 1) / kWave : 1;   // (an empty table: one wave per origin writes its status)
  k_light_march<<<tl_grid(n_origins * chunks * kWave, kBlock), kBlock, 0, s>>>(origins, skip, n_origins, dirs, ring, n_dirs, n_rings, occ, owner,
                                                                              grid_of(voxel, ix0, iy0, iz0, nx, ny, nz), max_range, min_hits, counts,
                                                                              status, code, first);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
