// Crown structure of the trees of a labelled cloud on a grid of cell x cell x layer: where the crown begins, the voxels it fills, the
// cells it projects onto the ground, their centroid and the crown radius in eight directions (the semantics are restated in
// numpy in tests/crown_restatement.py).
// tl_crown_voxel_keys: one thread per gathered row: key = tree (21 bits) | ix_rel (13) | iy_rel (13) | layer (8), or the sentinel above
//   every real key.  One sort of the keys (the caller's) makes every tree one contiguous range, the rows of one xy column adjacent in it
//   and the layers ascending inside the column.
// tl_crown_structure:  one workgroup per tree, two trips over its keys: (a) rows and distinct keys per layer into LDS counters, then one
//   lane finds the widest layer and walks down to the crown base; (b) the last key of every xy column is the column's highest layer: at
//   or above the base the column is a projection cell -> count, integer index sums, the largest squared distance per sector.
// Every formula is f64 in plain operators under the pragma below (no contraction into fma).  Counts and sums are integers and the
// maxima are exact, reduced registers -> xor butterfly -> wave order in LDS: the same bits run to run and for any row order.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTreeCols = 4;                 // px, py, z_ref, z_top
constexpr int kSummaryCols = 11;             // base_h, length, ratio, widest_h, volume, proj_area, x, y, offset, radius_max, radius_mean
constexpr int kMaxLayers = 256;
constexpr int kLayerBits = 8, kCellBits = 13, kTreeBits = 21;
constexpr int kTreeShift = kLayerBits + 2 * kCellBits;               // 34
constexpr int64_t kCellHalf = (int64_t)1 << (kCellBits - 1);         // 4096
constexpr int64_t kCellMask = ((int64_t)1 << kCellBits) - 1;
constexpr int64_t kSentinel = (int64_t)1 << (kTreeShift + kTreeBits);

// layers of a tree of height H above its reference: min(floor(H / layer) + 1, max_layers), none unless H >= 0 (the range is decided on
// the f64 value)
__device__ __forceinline__ int tree_layers(double H, double layer, int64_t max_layers) {
  if (!(H >= 0.0)) return 0;
  const double q = floor(H / layer) + 1.0;
  return q < (double)max_layers ? (int)q : (int)max_layers;
}

// floor(p / cell) of a tree position as an integer; 0 for a value no cell index can be near (such a tree has no real key)
__device__ __forceinline__ int64_t base_cell(double p, double cell) {
  const double f = floor(p / cell);
  return f > -1e15 && f < 1e15 ? (int64_t)f : 0;
}

__global__ void __launch_bounds__(kBlock) k_crown_voxel_keys(const double* __restrict__ xyz, const int64_t* __restrict__ label, int64_t n,
                                                             const double* __restrict__ tree, int64_t n_trees, tl_crown_params a,
                                                             int64_t* __restrict__ keys, int32_t* __restrict__ err) {
  const double inf = __builtin_inf();
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    int64_t key = kSentinel;
    const int64_t t = label[j] - 1;
    if (t >= 0 && t < n_trees) {
      const double x = xyz[3 * j], y = xyz[3 * j + 1], z = xyz[3 * j + 2];
      if (!(fabs(x) < inf && fabs(y) < inf && fabs(z) < inf)) {
        *err = 1;
      } else {
        const double px = tree[t * kTreeCols], py = tree[t * kTreeCols + 1], zr = tree[t * kTreeCols + 2], zt = tree[t * kTreeCols + 3];
        const int Lt = tree_layers(zt - zr, a.layer, a.max_layers);
        const double l = floor((z - zr) / a.layer);
        if (l >= 0.0 && l < (double)Lt) {                                        // (NaN fails)
          const double rx = (floor(x / a.cell) - floor(px / a.cell)) + (double)kCellHalf;
          const double ry = (floor(y / a.cell) - floor(py / a.cell)) + (double)kCellHalf;
          const double lim = (double)(2 * kCellHalf);
          if (rx >= 0.0 && rx < lim && ry >= 0.0 && ry < lim)
            key = (t << kTreeShift) | ((int64_t)rx << (kLayerBits + kCellBits)) | ((int64_t)ry << kLayerBits) | (int64_t)l;
          else
            *err = 1;
        }
      }
    }
    keys[j] = key;
  }
}

__global__ void __launch_bounds__(kBlock) k_crown_structure(const int64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ kstart,
                                                            const double* __restrict__ tree, int64_t L, tl_crown_params a,
                                                            double* __restrict__ summary, int64_t* __restrict__ counts,
                                                            double* __restrict__ prof_h, int64_t* __restrict__ pcount,
                                                            double* __restrict__ radii) {
  __shared__ unsigned s_n[kMaxLayers], s_cells[kMaxLayers];
  __shared__ int s_walk[2];                  // l_b (-1: no crown), l_w
  __shared__ long long s_vox;
  __shared__ long long s_sum[kWaves * 3];
  __shared__ double s_w[kWaves * 8];
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  const double nan = __builtin_nan("");
  int64_t lo = kstart[t], hi = kstart[t + 1];
  if (lo < 0 || hi > n || lo > hi) { lo = 0; hi = 0; }          // a malformed range reads nothing
  const double px = tree[t * kTreeCols], py = tree[t * kTreeCols + 1];
  const double H = tree[t * kTreeCols + 3] - tree[t * kTreeCols + 2];
  const int Lt = tree_layers(H, a.layer, a.max_layers);
  s_n[tid] = 0u; s_cells[tid] = 0u;                              // (kBlock == kMaxLayers)
  __syncthreads();

  // (a) rows and distinct voxels per layer
  for (int64_t j = lo + tid; j < hi; j += kBlock) {
    const int64_t key = keys[j];
    const int l = (int)(key & (kMaxLayers - 1));
    atomicAdd(&s_n[l], 1u);
    if (j == lo || keys[j - 1] != key) atomicAdd(&s_cells[l], 1u);
  }
  __syncthreads();
  for (int64_t l = tid; l < L; l += kBlock) {
    const bool in = l < Lt;
    prof_h[t * L + l] = in ? (double)l * a.layer : nan;
    pcount[(t * L + l) * 2] = in ? (int64_t)s_n[l] : 0;
    pcount[(t * L + l) * 2 + 1] = in ? (int64_t)s_cells[l] : 0;
  }
  if (tid == 0) {                                                // the widest layer and the walk down to the crown base
    int l_min = 0;
    while (l_min < (int)a.max_layers && (double)l_min * a.layer < a.min_height) ++l_min;
    int64_t cmax = 0;
    int l_w = -1;
    for (int l = l_min; l < Lt; ++l)
      if ((int64_t)s_cells[l] > cmax) { cmax = s_cells[l]; l_w = l; }
    int l_b = l_w;
    int64_t vox = 0;
    if (l_w >= 0) {
      int64_t gap = 0;
      for (int l = l_w - 1; l >= l_min; --l) {
        if ((int64_t)s_cells[l] * 100 >= a.base_percent * cmax) { l_b = l; gap = 0; }
        else if (++gap > a.max_gap) break;
      }
      for (int l = l_b; l < Lt; ++l) vox += s_cells[l];
    }
    s_walk[0] = l_b; s_walk[1] = l_w; s_vox = vox;
  }
  __syncthreads();
  const int l_b = s_walk[0];
  if (l_b < 0) {                                                 // block-uniform: no crown
    if (tid < kSummaryCols) summary[t * kSummaryCols + tid] = nan;
    if (tid < 8) radii[t * 8 + tid] = nan;
    if (tid == 0) { counts[3 * t] = Lt; counts[3 * t + 1] = 0; counts[3 * t + 2] = 0; }
    return;
  }

  // (b) the projection cells: the xy columns whose highest layer is at or above the base
  const int64_t bx = base_cell(px, a.cell) - kCellHalf, by = base_cell(py, a.cell) - kCellHalf;
  long long acc[3] = {0, 0, 0};                                  // cells, sum ix, sum iy
  double wmax[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) wmax[s] = -1.0;                    // (w >= 0: below every real value)
  for (int64_t j = lo + tid; j < hi; j += kBlock) {
    const int64_t key = keys[j];
    if (j + 1 < hi && (keys[j + 1] >> kLayerBits) == (key >> kLayerBits)) continue;
    if ((int)(key & (kMaxLayers - 1)) < l_b) continue;
    const int64_t ix = ((key >> (kLayerBits + kCellBits)) & kCellMask) + bx, iy = ((key >> kLayerBits) & kCellMask) + by;
    acc[0] += 1; acc[1] += ix; acc[2] += iy;
    const double u = ((double)ix + 0.5) * a.cell - px, v = ((double)iy + 0.5) * a.cell - py;
    const double w = u * u + v * v;
    int s = 0;
    if (u > 0.0 && v >= 0.0) s = v < u ? 0 : 1;
    else if (u <= 0.0 && v > 0.0) s = -u < v ? 2 : 3;
    else if (u < 0.0 && v <= 0.0) s = -v < -u ? 4 : 5;
    else if (u >= 0.0 && v < 0.0) s = u < -v ? 6 : 7;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k == s && w > wmax[k]) wmax[k] = w;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    for (int o = 32; o > 0; o >>= 1) {
      const double other = __shfl_xor(wmax[k], o);
      wmax[k] = other > wmax[k] ? other : wmax[k];
    }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s_sum[(tid >> 6) * 3 + k] = acc[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) s_w[(tid >> 6) * 8 + k] = wmax[k];
  }
  __syncthreads();
  if (tid != 0) return;

  for (int w = 1; w < kWaves; ++w) {
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += s_sum[w * 3 + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) wmax[k] = s_w[w * 8 + k] > wmax[k] ? s_w[w * 8 + k] : wmax[k];
  }
  const int l_w = s_walk[1];
  const int64_t vox = s_vox;
  const double c = (double)acc[0];
  const double base_h = (double)l_b * a.layer;
  const double length = H - base_h;
  const double cx = (((double)acc[1] / c) + 0.5) * a.cell, cy = (((double)acc[2] / c) + 0.5) * a.cell;
  const double dx = cx - px, dy = cy - py;
  double rmax = 0.0, rsum = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double r = wmax[k] >= 0.0 ? sqrt(wmax[k]) : 0.0;
    radii[t * 8 + k] = r;
    rmax = r > rmax ? r : rmax;
    rsum = rsum + r;
  }
  double* sm = summary + t * kSummaryCols;
  sm[0] = base_h; sm[1] = length; sm[2] = length / H; sm[3] = ((double)l_w + 0.5) * a.layer;
  sm[4] = (double)vox * ((a.cell * a.cell) * a.layer);
  sm[5] = c * (a.cell * a.cell);
  sm[6] = cx; sm[7] = cy; sm[8] = sqrt(dx * dx + dy * dy);
  sm[9] = rmax; sm[10] = rsum / 8.0;
  counts[3 * t] = Lt; counts[3 * t + 1] = vox; counts[3 * t + 2] = acc[0];
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// the constraints of the parameter table; NaN fails every one of them
bool params_ok(const tl_crown_params* p) {
  if (!p) return false;
  const double inf = __builtin_inf();
  if (!(p->layer > 0.0 && p->layer < inf) || !(p->cell > 0.0 && p->cell < inf) || !(p->min_height >= 0.0 && p->min_height < inf)) return false;
  if (p->max_layers < 1 || p->max_layers > kMaxLayers || p->base_percent < 1 || p->base_percent > 100 || p->max_gap < 0) return false;
  return true;
}
}  // namespace

extern "C" int tl_crown_voxel_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, const double* tree, int64_t n_trees,
                                   const tl_crown_params* params, int64_t* keys, int32_t* err, tl_stream_t stream) {
  if (!sorted_xyz || !sorted_label || !tree || !keys || !err || n < 0 || n_trees < 0 || n_trees >= ((int64_t)1 << kTreeBits)) return TL_ERR_ARG;
  if (!aligned8(sorted_xyz) || !aligned8(sorted_label) || !aligned8(tree) || !aligned8(keys) || (reinterpret_cast<uintptr_t>(err) & 3))
    return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (n == 0 || n_trees == 0) return TL_OK;
  if (hipMemsetAsync(err, 0, sizeof(int32_t), tl_s(stream)) != hipSuccess) return TL_ERR_LAUNCH;
  k_crown_voxel_keys<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(sorted_xyz, sorted_label, n, tree, n_trees, *params, keys, err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_crown_structure(const int64_t* sorted_keys, int64_t n, const int64_t* kstart, const double* tree, int64_t n_trees, int64_t L,
                                  const tl_crown_params* params, double* summary, int64_t* counts, double* prof_h, int64_t* pcount, double* radii,
                                  tl_stream_t stream) {
  if (!sorted_keys || !kstart || !tree || !summary || !counts || !prof_h || !pcount || !radii || n < 0 || n_trees < 0 ||
      n_trees >= ((int64_t)1 << kTreeBits) || L < 0)
    return TL_ERR_ARG;
  if (!aligned8(sorted_keys) || !aligned8(kstart) || !aligned8(tree) || !aligned8(summary) || !aligned8(counts) || !aligned8(prof_h) ||
      !aligned8(pcount) || !aligned8(radii))
    return TL_ERR_ARG;
  if (!params_ok(params) || L > params->max_layers) return TL_ERR_ARG;
  if (n_trees == 0 || L == 0) return TL_OK;
  k_crown_structure<<<(unsigned)n_trees, kBlock, 0, tl_s(stream)>>>(sorted_keys, n, kstart, tree, L, *params, summary, counts, prof_h, pcount,
                                                                     radii);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
