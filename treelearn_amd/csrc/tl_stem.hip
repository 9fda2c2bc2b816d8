// Stem profiles of the trees of a labelled cloud: a circle per horizontal slab along the stem, tracked bottom-up, and from the accepted
// circles the stem volume, the diameter at breast height, the lean and the taper (the semantics are restated in numpy in
// tests/stem_restatement.py).
// tl_stem_keys:    one thread per gathered row: the corridor test and the slab of the row -> key = tree * S + slab, or the sentinel
//   n_trees * S.  One stable sort of the keys (the caller's) then makes every slab of every tree one contiguous range.
// tl_stem_profile: one workgroup per tree walks its slabs upwards; each step is the slice fit of tl_circle_fit.h on the slab's own range
//   around the last accepted centre; thread 0 applies the acceptance rule, keeps the walk's state in LDS and computes the summary.
// Every formula is f64 in plain operators under the pragma below (no contraction into fma).  Sums go registers -> wave shuffles -> LDS in
// a fixed order and counts are integers: two runs give the same bits.
#include "tl_circle_fit.h"

#pragma clang fp contract(off)

namespace {
constexpr int kTreeCols = 4;                 // px, py, z_ref, z_top
constexpr int kProfileCols = 5;              // h, x, y, r, rmse
constexpr int kSummaryCols = 6;              // stem_base_h, stem_top_h, stem_volume, dbh_stem, stem_lean, stem_taper
constexpr double kPi = 3.141592653589793;

struct StemArgs {                            // tl_stem_params with the derived values, by value to the kernels
  double first_height, step, half_thickness, corridor2, start_radius, search_factor, search_margin, max_rmse, min_radius, max_radius,
      max_growth, dbh_height;
  int64_t max_slices, min_points, max_misses;
};

// slab k of a tree of height H above its reference exists when k < max_slices and h_k <= H (h_k does not decrease with k; NaN H: none)
__device__ __forceinline__ bool slab_exists(const StemArgs& a, int64_t k, double H, double& h) {
  h = a.first_height + (double)k * a.step;
  return k >= 0 && k < a.max_slices && h <= H;
}

__global__ void __launch_bounds__(kBlock) k_stem_keys(const double* __restrict__ xyz, const int64_t* __restrict__ label, int64_t n,
                                                      const double* __restrict__ tree, int64_t n_trees, int64_t S, StemArgs a,
                                                      int64_t* __restrict__ keys) {
  const int64_t sentinel = n_trees * S;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    int64_t key = sentinel;
    const int64_t t = label[j] - 1;
    if (t >= 0 && t < n_trees) {
      const double px = tree[t * kTreeCols], py = tree[t * kTreeCols + 1], zr = tree[t * kTreeCols + 2], zt = tree[t * kTreeCols + 3];
      const double H = zt - zr;
      const double z = xyz[3 * j + 2];
      const double u = xyz[3 * j] - px, v = xyz[3 * j + 1] - py;
      const double w = u * u + v * v;
      const double q = ((z - zr) - (a.first_height - a.half_thickness)) / a.step;
      if (w < a.corridor2 && q > -2.0 && q < (double)(a.max_slices + 1)) {      // (NaN fails; q is in range before it becomes an integer)
        const int64_t k0 = (int64_t)floor(q);
        for (int64_t k = k0 - 1; k <= k0 + 1; ++k) {
          double h;
          if (!slab_exists(a, k, H, h) || k >= S) continue;
          const double zc = zr + h;
          if (z >= zc - a.half_thickness && z < zc + a.half_thickness) { key = t * S + k; break; }
        }
      }
    }
    keys[j] = key;
  }
}

__global__ void __launch_bounds__(kBlock) k_stem_profile(const double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ slab_start,
                                                         const double* __restrict__ tree, int64_t S, StemArgs a, double* __restrict__ profile,
                                                         int64_t* __restrict__ pcount, double* __restrict__ summary,
                                                         int64_t* __restrict__ slices) {
  __shared__ double s_red[kWaves * 9];
  __shared__ double s_fit[3];
  __shared__ int s_ok;
  __shared__ double s_walk[4];               // centre x, y, search radius, last accepted radius
  __shared__ int s_state[2];                 // consecutive misses, stopped
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const double nan = __builtin_nan("");
  const double zr = tree[t * kTreeCols + 2];
  const double H = tree[t * kTreeCols + 3] - zr;
  double* prof = profile + t * S * kProfileCols;
  int64_t* pc = pcount + t * S * 2;
  if (tid == 0) {
    s_walk[0] = tree[t * kTreeCols]; s_walk[1] = tree[t * kTreeCols + 1]; s_walk[2] = a.start_radius; s_walk[3] = nan;
    s_state[0] = 0; s_state[1] = 0;
  }
  for (int64_t k = 0; k < S; ++k) {
    double h;
    const bool exists = slab_exists(a, k, H, h);                   // block-uniform
    __syncthreads();                                               // the walk's state after slab k - 1
    const double cx = s_walk[0], cy = s_walk[1], R = s_walk[2];
    const bool stopped = s_state[1] != 0;
    double* o = prof + k * kProfileCols;
    if (!exists || stopped) {                                      // block-uniform: beyond the tree's last slab, or not visited
      if (tid == 0) {
        o[0] = exists ? h : nan; o[1] = nan; o[2] = nan; o[3] = nan; o[4] = nan;
        pc[2 * k] = 0; pc[2 * k + 1] = 0;
      }
      continue;
    }
    int64_t lo = slab_start[t * S + k], hi = slab_start[t * S + k + 1];
    if (lo < 0 || hi > n || lo > hi) { lo = 0; hi = 0; }          // a malformed range reads nothing
    double cnt, rss;
    const Fit f = slice_circle(xyz, lo, hi, cx, cy, zr + h, a.half_thickness, R * R, a.min_points, s_red, s_fit, &s_ok, cnt, rss);
    if (tid == 0) {
      const double r_prev = s_walk[3];
      const double rmse = f.ok ? sqrt(rss / cnt) : nan;
      const bool accepted = f.ok && rmse <= a.max_rmse && f.r >= a.min_radius && f.r <= a.max_radius &&
                            (!(r_prev == r_prev) || f.r <= a.max_growth * r_prev);
      o[0] = h;
      pc[2 * k] = (int64_t)cnt;
      if (accepted) {
        const double x = f.cx + cx, y = f.cy + cy;
        o[1] = x; o[2] = y; o[3] = f.r; o[4] = rmse;
        pc[2 * k + 1] = 1;
        s_walk[0] = x; s_walk[1] = y; s_walk[2] = a.search_factor * f.r + a.search_margin; s_walk[3] = f.r;
        s_state[0] = 0;
      } else {
        o[1] = nan; o[2] = nan; o[3] = nan; o[4] = nan;
        pc[2 * k + 1] = 2;
        const int misses = s_state[0] + 1;
        s_state[0] = misses;
        if (misses >= a.max_misses) s_state[1] = 1;
      }
    }
  }
  if (tid != 0) return;

  // the summary, by the one lane that wrote the profile, over the accepted slabs in ascending k
  double* sm = summary + t * kSummaryCols;
  int64_t m = 0, first = -1, last = -1;
  double sh = 0.0, sd = 0.0;
  for (int64_t k = 0; k < S; ++k)
    if (pc[2 * k + 1] == 1) {
      if (first < 0) first = k;
      last = k;
      ++m;
      sh = sh + prof[k * kProfileCols];
      sd = sd + 2.0 * prof[k * kProfileCols + 3];
    }
  slices[t] = m;
  if (m == 0) {
#pragma unroll
    for (int c = 0; c < kSummaryCols; ++c) sm[c] = nan;
    return;
  }
  const double h_first = prof[first * kProfileCols], h_last = prof[last * kProfileCols];
  const double r0 = prof[first * kProfileCols + 3];
  double V = (kPi * (r0 * r0)) * h_first;
  double dbh = nan;
  bool have_dbh = false;
  int64_t i = first;
  for (int64_t j = first + 1; j <= last; ++j) {
    if (pc[2 * j + 1] != 1) continue;
    const double hi_ = prof[i * kProfileCols], hj = prof[j * kProfileCols];
    const double ri = prof[i * kProfileCols + 3], rj = prof[j * kProfileCols + 3];
    V = V + ((kPi / 3.0) * (hj - hi_)) * ((ri * ri + ri * rj) + rj * rj);
    if (!have_dbh && hi_ <= a.dbh_height && a.dbh_height <= hj) {
      dbh = 2.0 * (ri + (rj - ri) * ((a.dbh_height - hi_) / (hj - hi_)));
      have_dbh = true;
    }
    i = j;
  }
  sm[0] = h_first; sm[1] = h_last; sm[2] = V; sm[3] = dbh;
  if (m < 2) { sm[4] = nan; sm[5] = nan; return; }
  const double dx = prof[last * kProfileCols + 1] - prof[first * kProfileCols + 1];
  const double dy = prof[last * kProfileCols + 2] - prof[first * kProfileCols + 2];
  sm[4] = atan2(sqrt(dx * dx + dy * dy), h_last - h_first) * (180.0 / kPi);
  const double hm = sh / (double)m, dm = sd / (double)m;
  double num = 0.0, den = 0.0;
  for (int64_t k = first; k <= last; ++k)
    if (pc[2 * k + 1] == 1) {
      const double eh = prof[k * kProfileCols] - hm, ed = 2.0 * prof[k * kProfileCols + 3] - dm;
      num = num + eh * ed;
      den = den + eh * eh;
    }
  sm[5] = num / den;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// the constraints of the parameter table; NaN fails every one of them
bool params_ok(const tl_stem_params* p) {
  if (!p) return false;
  const double inf = __builtin_inf();
  if (!(p->first_height > 0.0 && p->first_height < inf) || !(p->step > 0.0 && p->step < inf)) return false;
  if (!(p->thickness > 0.0 && p->thickness <= p->step)) return false;
  if (p->max_slices < 1 || p->max_slices > 256) return false;
  if (!(p->corridor > 0.0 && p->corridor < inf) || !(p->start_radius > 0.0 && p->start_radius < inf)) return false;
  if (!(p->search_factor >= 1.0 && p->search_factor < inf) || !(p->search_margin >= 0.0 && p->search_margin < inf)) return false;
  if (p->min_points < 3 || !(p->max_rmse > 0.0)) return false;
  if (!(p->min_radius > 0.0 && p->min_radius <= p->max_radius && p->max_radius < inf)) return false;
  if (!(p->max_growth >= 1.0) || p->max_misses < 1 || p->max_misses >= ((int64_t)1 << 31)) return false;
  if (!(p->dbh_height > 0.0 && p->dbh_height < inf)) return false;
  return true;
}

StemArgs stem_args(const tl_stem_params* p) {
  return StemArgs{p->first_height, p->step, p->thickness / 2.0, p->corridor * p->corridor, p->start_radius, p->search_factor, p->search_margin,
                  p->max_rmse, p->min_radius, p->max_radius, p->max_growth, p->dbh_height, p->max_slices, p->min_points, p->max_misses};
}
}  // namespace

extern "C" int tl_stem_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, const double* tree, int64_t n_trees, int64_t S,
                            const tl_stem_params* params, int64_t* keys, tl_stream_t stream) {
  if (!sorted_xyz || !sorted_label || !tree || !keys || n < 0 || n_trees < 0 || n_trees >= ((int64_t)1 << 31) || S < 0) return TL_ERR_ARG;
  if (!aligned8(sorted_xyz) || !aligned8(sorted_label) || !aligned8(tree) || !aligned8(keys)) return TL_ERR_ARG;
  if (!params_ok(params) || S > params->max_slices) return TL_ERR_ARG;
  if (n == 0 || n_trees == 0 || S == 0) return TL_OK;
  k_stem_keys<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(sorted_xyz, sorted_label, n, tree, n_trees, S, stem_args(params), keys);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_stem_profile(const double* stem_xyz, int64_t n, const int64_t* slab_start, const double* tree, int64_t n_trees, int64_t S,
                               const tl_stem_params* params, double* profile, int64_t* pcount, double* summary, int64_t* slices,
                               tl_stream_t stream) {
  if (!stem_xyz || !slab_start || !tree || !profile || !pcount || !summary || !slices || n < 0 || n_trees < 0 ||
      n_trees >= ((int64_t)1 << 31) || S < 0)
    return TL_ERR_ARG;
  if (!aligned8(stem_xyz) || !aligned8(slab_start) || !aligned8(tree) || !aligned8(profile) || !aligned8(pcount) || !aligned8(summary) ||
      !aligned8(slices))
    return TL_ERR_ARG;
  if (!params_ok(params) || S > params->max_slices) return TL_ERR_ARG;
  if (n_trees == 0 || S == 0) return TL_OK;
  k_stem_profile<<<(unsigned)n_trees, kBlock, 0, tl_s(stream)>>>(stem_xyz, n, slab_start, tree, S, stem_args(params), profile, pcount, summary,
                                                                  slices);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
