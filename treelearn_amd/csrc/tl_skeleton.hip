// Branch structure of the trees of a labelled cloud on a grid of voxel^3: the geodesic distance of every voxel from the stem base along
// the tree's own voxels, the level sets of that distance cut into connected components (the skeleton nodes) and every node's parent
// (the semantics are restated in Python in tests/branches_restatement.py).  The branches are read off the small node table
// on the host (util/branches.py).
// tl_skel_voxel_keys: one thread per gathered row: key = tree (21 bits) | ix_rel (12) | iy_rel (12) | iz_rel (11), or -1.  One sort and
//   unique of the keys (the caller's) makes every tree one contiguous ascending range of distinct voxels: a voxel is its index there.
// tl_skel_distance:   one workgroup per tree.  Neighbours are found by binary search inside the tree's own range, so no edge leaves the
//   tree.  Every edge weighs >= 100, so the voxels whose tentative distance lies in [100 k, 100 k + 100) are final once every bucket
//   below k is done: one barrier-separated round per non-empty bucket, integer atomicMin into the later buckets.  The fixpoint is the
//   unique shortest-path distance whatever the order of the atomics.
// tl_skel_nodes:      one thread per voxel: unite it with its same-bin neighbours (tl_scan.h's union-find: the root is the smallest index,
//   which is the smallest key), then integer count, coordinate sums and the 64-bit minimum of (d << 32 | index) per root.
// tl_skel_links:      one thread per node (the roots, ordered by the caller): centroid from the integer sums, predecessor of the node's
//   first voxel -> parent node.
// Integers throughout; the only f64 arithmetic is floor(coordinate / voxel) and the centroid division, in plain operators under the pragma.
#include "tl_scan.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kDistBlock = 1024;             // one workgroup per tree: the largest tree sets the time of the stage
constexpr int kRotate = 37;                  // odd: the rotations of kDistBlock successive chunks are all different
constexpr int kTreeCols = 4;                 // px, py, z_ref, z_top
constexpr int kZBits = 11, kXYBits = 12, kTreeBits = 21;
constexpr int kYShift = kZBits, kXShift = kZBits + kXYBits, kTreeShift = kZBits + 2 * kXYBits;   // 11, 23, 35
constexpr int kHalf = 1 << (kXYBits - 1);    // 2048: ix_rel of the tree's own column
constexpr int kXYMask = (1 << kXYBits) - 1, kZMask = (1 << kZBits) - 1;
constexpr int kUnreached = 0x7fffffff;

// floor(p / voxel) of a tree position, and whether it is a number a voxel index can be near
__device__ __forceinline__ bool base_voxel(double p, double voxel, double* f) {
  *f = floor(p / voxel);
  return *f > -1e15 && *f < 1e15;           // (NaN fails)
}

// floor(sqrt(10000 * s)) for the squared lengths s = dx^2 + dy^2 + dz^2 a reach of 2 can give
__device__ __forceinline__ int edge_weight(int s) {
  switch (s) {
    case 1: return 100;
    case 2: return 141;
    case 3: return 173;
    case 4: return 200;
    case 5: return 223;
    case 6: return 244;
    case 8: return 282;
    case 9: return 300;
    default: return 346;                     // 12
  }
}

// f(index, dx^2 + dy^2 + dz^2) for every voxel of keys[lo, hi) within `reach` of `key` (not itself).  The z neighbours of one xy column
// are adjacent in key order: one lower bound per column, then a walk.
template <class F>
__device__ __forceinline__ void for_neighbours(const int64_t* __restrict__ keys, int64_t lo, int64_t hi, int64_t key, int reach, F f) {
  const int x = (int)(key >> kXShift) & kXYMask, y = (int)(key >> kYShift) & kXYMask, z = (int)key & kZMask;
  const int64_t tbase = (key >> kTreeShift) << kTreeShift;
  const int zlo = z - reach < 0 ? 0 : z - reach, zhi = z + reach > kZMask ? kZMask : z + reach;
  for (int dx = -reach; dx <= reach; ++dx) {
    const int xx = x + dx;
    if (xx < 0 || xx > kXYMask) continue;
    for (int dy = -reach; dy <= reach; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy > kXYMask) continue;
      const int64_t k0 = tbase | ((int64_t)xx << kXShift) | ((int64_t)yy << kYShift) | zlo, k1 = k0 + (zhi - zlo);
      int64_t a = lo, b = hi;
      while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (keys[mid] < k0) a = mid + 1; else b = mid;
      }
      for (; a < hi; ++a) {
        const int64_t ku = keys[a];
        if (ku > k1) break;
        const int dz = ((int)ku & kZMask) - z;
        const int s = dx * dx + dy * dy + dz * dz;
        if (s) f(a, s);
      }
    }
  }
}

__device__ __forceinline__ int load_d(const int* d, int64_t i) { return __hip_atomic_load(&d[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_d(int* d, int64_t i, int v) { __hip_atomic_store(&d[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(kBlock) k_skel_voxel_keys(const double* __restrict__ xyz, const int64_t* __restrict__ label, int64_t n,
                                                            const double* __restrict__ tree, int64_t n_trees, tl_skel_params a,
                                                            int64_t* __restrict__ keys, int32_t* __restrict__ err) {
  const double inf = __builtin_inf();
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    int64_t key = -1;
    const int64_t t = label[j] - 1;
    if (t >= 0 && t < n_trees) {
      const double x = xyz[3 * j], y = xyz[3 * j + 1], z = xyz[3 * j + 2];
      double fpx, fpy, fzr;
      if (!(fabs(x) < inf && fabs(y) < inf && fabs(z) < inf)) {
        *err = 1;
      } else if (base_voxel(tree[t * kTreeCols], a.voxel, &fpx) && base_voxel(tree[t * kTreeCols + 1], a.voxel, &fpy) &&
                 base_voxel(tree[t * kTreeCols + 2], a.voxel, &fzr)) {
        const double rz = floor(z / a.voxel) - fzr;
        if (rz >= 0.0) {                                                         // rows below the reference take no part
          const double rx = (floor(x / a.voxel) - fpx) + (double)kHalf, ry = (floor(y / a.voxel) - fpy) + (double)kHalf;
          if (rx >= 1.0 && rx <= (double)kXYMask && ry >= 1.0 && ry <= (double)kXYMask && rz < (double)kZMask)
            key = (t << kTreeShift) | ((int64_t)rx << kXShift) | ((int64_t)ry << kYShift) | (int64_t)rz;
          else
            *err = 1;
        }
      }
    }
    keys[j] = key;
  }
}

__global__ void __launch_bounds__(kDistBlock) k_skel_distance(const int64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ kstart,
                                                              tl_skel_params a, int* __restrict__ d, int32_t* __restrict__ rounds) {
  __shared__ int s_iz0;
  __shared__ int s_next[3];                  // the smallest pending bucket seen in round r, in slot r % 3
  const int tid = threadIdx.x;
  const int64_t t = blockIdx.x;
  int64_t lo = kstart[t], hi = kstart[t + 1];
  if (lo < 0 || hi > n || lo > hi) { lo = 0; hi = 0; }          // a malformed range touches nothing
  if (tid == 0) { rounds[t] = 0; s_iz0 = kUnreached; s_next[0] = s_next[1] = s_next[2] = kUnreached; }
  if (hi - lo > a.max_voxels) {                                  // block-uniform: too large, no skeleton
    for (int64_t v = lo + tid; v < hi; v += kDistBlock) d[v] = -1;
    return;
  }
  __syncthreads();
  const int reach = (int)a.reach, base_reach = (int)a.base_reach;

  // the sources: the lowest base_layers layers of the voxels within base_reach of the tree's own column
  auto near_base = [&](int64_t key) {
    const int rx = ((int)(key >> kXShift) & kXYMask) - kHalf, ry = ((int)(key >> kYShift) & kXYMask) - kHalf;
    return rx >= -base_reach && rx <= base_reach && ry >= -base_reach && ry <= base_reach;
  };
  for (int64_t v = lo + tid; v < hi; v += kDistBlock) {
    const int64_t key = keys[v];
    if (near_base(key)) atomicMin(&s_iz0, (int)key & kZMask);
  }
  __syncthreads();
  const int iz0 = s_iz0;
  if (iz0 == kUnreached) {                                       // block-uniform: nothing at the base, no skeleton
    for (int64_t v = lo + tid; v < hi; v += kDistBlock) d[v] = -1;
    return;
  }
  for (int64_t v = lo + tid; v < hi; v += kDistBlock) {
    const int64_t key = keys[v];
    store_d(d, v, near_base(key) && (int64_t)(((int)key & kZMask) - iz0) < a.base_layers ? 0 : kUnreached);
  }
  __threadfence();
  __syncthreads();

  int k = 0, r = 0;
  while (true) {
    int* nx = &s_next[r % 3];
    if (tid == 0) s_next[(r + 1) % 3] = kUnreached;              // last read two barriers ago
    int pending = kUnreached;                                    // the smallest bucket above k this thread saw or made
    // A bucket's voxels tend to sit at one place of many xy columns, a constant stride apart in key order: every chunk of kDistBlock
    // voxels is dealt to the threads rotated by another offset, so that such a front does not land on a few threads.
    int rot = tid;
    for (int64_t c = lo; c < hi; c += kDistBlock, rot += kRotate) {
      const int64_t v = c + (rot & (kDistBlock - 1));
      if (v >= hi) continue;
      const int dv = load_d(d, v);
      if (dv == kUnreached) continue;
      const int b = dv / 100;
      if (b > k) { pending = b < pending ? b : pending; continue; }   // (a later relaxation reports its own, smaller bucket)
      if (b < k) continue;
      for_neighbours(keys, lo, hi, keys[v], reach, [&](int64_t u, int s) {
        const int nd = dv + edge_weight(s);
        if (nd < load_d(d, u) && nd < atomicMin(&d[u], nd)) pending = nd / 100 < pending ? nd / 100 : pending;
      });
    }
    if (pending != kUnreached) atomicMin(nx, pending);
    __threadfence();
    __syncthreads();
    const int kn = *nx;
    ++r;
    if (kn == kUnreached) break;
    k = kn;
  }
  if (tid == 0) rounds[t] = r;
  for (int64_t v = lo + tid; v < hi; v += kDistBlock)
    if (load_d(d, v) == kUnreached) store_d(d, v, -1);
}

__global__ void __launch_bounds__(kBlock) k_skel_init(int64_t n, int* __restrict__ parent, unsigned long long* __restrict__ acc,
                                                      unsigned long long* __restrict__ vstar) {
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
    parent[v] = (int)v;
    acc[4 * v] = 0; acc[4 * v + 1] = 0; acc[4 * v + 2] = 0; acc[4 * v + 3] = 0;
    vstar[v] = ~0ull;
  }
}

// the range of the tree that owns `key`, clamped so that a malformed kstart reads nothing outside keys[0, n)
__device__ __forceinline__ bool tree_range(int64_t key, const int64_t* __restrict__ kstart, int64_t n_trees, int64_t n, int64_t* lo, int64_t* hi) {
  const int64_t t = key >> kTreeShift;
  if (t < 0 || t >= n_trees) return false;
  *lo = kstart[t]; *hi = kstart[t + 1];
  return *lo >= 0 && *hi <= n && *lo <= *hi;
}

__global__ void __launch_bounds__(kBlock) k_skel_unite(const int64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ kstart,
                                                       int64_t n_trees, tl_skel_params a, const int* __restrict__ d, int* __restrict__ parent) {
  const int step = 100 * (int)a.level;
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
    const int dv = d[v];
    int64_t lo, hi;
    if (dv < 0 || !tree_range(keys[v], kstart, n_trees, n, &lo, &hi)) continue;
    const int bin = dv / step;
    for_neighbours(keys, lo, hi, keys[v], (int)a.reach, [&](int64_t u, int) {
      if (u > v && d[u] >= 0 && d[u] / step == bin) tl_unite(parent, (int)v, (int)u);     // (every pair once, from its smaller index)
    });
  }
}

__global__ void __launch_bounds__(kBlock) k_skel_accumulate(const int64_t* __restrict__ keys, int64_t n, const int* __restrict__ d,
                                                            int* __restrict__ parent, unsigned long long* __restrict__ acc,
                                                            unsigned long long* __restrict__ vstar) {
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < n; v += (int64_t)gridDim.x * kBlock) {
    const int dv = d[v];
    if (dv < 0) continue;
    const int64_t key = keys[v];
    const int64_t r = tl_find_root(parent, (int)v);
    atomicAdd(&acc[4 * r], 1ull);
    atomicAdd(&acc[4 * r + 1], (unsigned long long)((key >> kXShift) & kXYMask));
    atomicAdd(&acc[4 * r + 2], (unsigned long long)((key >> kYShift) & kXYMask));
    atomicAdd(&acc[4 * r + 3], (unsigned long long)(key & kZMask));
    atomicMin(&vstar[r], ((unsigned long long)(unsigned)dv << 32) | (unsigned long long)v);
  }
}

__global__ void __launch_bounds__(kBlock) k_skel_links(const int64_t* __restrict__ keys, int64_t n, const int64_t* __restrict__ kstart,
                                                       const double* __restrict__ tree, int64_t n_trees, tl_skel_params a,
                                                       const int* __restrict__ d, int* __restrict__ parent, const unsigned long long* __restrict__ acc,
                                                       const unsigned long long* __restrict__ vstar, const int32_t* __restrict__ roots, int64_t n_nodes,
                                                       const int32_t* __restrict__ node_id, const int64_t* __restrict__ node_start,
                                                       double* __restrict__ xyz, int32_t* __restrict__ par, int32_t* __restrict__ bin,
                                                       int64_t* __restrict__ count) {
  const int step = 100 * (int)a.level;
  const double nan = __builtin_nan("");
  for (int64_t m = (int64_t)blockIdx.x * kBlock + threadIdx.x; m < n_nodes; m += (int64_t)gridDim.x * kBlock) {
    const int64_t r = roots[m];
    int64_t lo = 0, hi = 0;
    int64_t c = 0;
    int b = -1, p = -1;
    double cx = nan, cy = nan, cz = nan;
    if (r >= 0 && r < n && d[r] >= 0 && tree_range(keys[r], kstart, n_trees, n, &lo, &hi)) {
      const int64_t t = keys[r] >> kTreeShift;
      b = d[r] / step;
      c = (int64_t)acc[4 * r];
      double fpx, fpy, fzr;
      if (c > 0 && (base_voxel(tree[t * kTreeCols], a.voxel, &fpx) && base_voxel(tree[t * kTreeCols + 1], a.voxel, &fpy) &&
                    base_voxel(tree[t * kTreeCols + 2], a.voxel, &fzr))) {
        const int64_t sx = (int64_t)acc[4 * r + 1] + c * ((int64_t)fpx - kHalf), sy = (int64_t)acc[4 * r + 2] + c * ((int64_t)fpy - kHalf),
                      sz = (int64_t)acc[4 * r + 3] + c * (int64_t)fzr;
        cx = ((double)sx / (double)c + 0.5) * a.voxel;
        cy = ((double)sy / (double)c + 0.5) * a.voxel;
        cz = ((double)sz / (double)c + 0.5) * a.voxel;
      }
      const int64_t v = (int64_t)(vstar[r] & 0xffffffffull);
      if (b > 0 && v >= lo && v < hi) {
        const int dv = d[v];
        int64_t best = -1;
        for_neighbours(keys, lo, hi, keys[v], (int)a.reach, [&](int64_t u, int s) {
          if (d[u] >= 0 && d[u] + edge_weight(s) == dv && (best < 0 || u < best)) best = u;
        });
        if (best >= 0) p = (int)((int64_t)node_id[tl_find_root(parent, (int)best)] - node_start[t]);
      }
    }
    xyz[3 * m] = cx; xyz[3 * m + 1] = cy; xyz[3 * m + 2] = cz;
    par[m] = p; bin[m] = b; count[m] = c;
  }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
constexpr int64_t kMaxVoxels = ((int64_t)1 << 31) - 1;           // a voxel is an int index

// the constraints of the parameter table; NaN fails every one of them
bool params_ok(const tl_skel_params* p) {
  if (!p) return false;
  const double inf = __builtin_inf();
  if (!(p->voxel > 0.0 && p->voxel < inf) || !(p->min_branch >= 0.0 && p->min_branch < inf) || !(p->min_height >= 0.0 && p->min_height < inf))
    return false;
  if (p->reach < 1 || p->reach > 2 || p->base_reach < 0 || p->base_reach > 2047 || p->base_layers < 1 || p->level < 1 ||
      p->level > 1000000 || p->max_voxels < 1)
    return false;
  return true;
}
}  // namespace

extern "C" int tl_skel_voxel_keys(const double* sorted_xyz, const int64_t* sorted_label, int64_t n, const double* tree, int64_t n_trees,
                                  const tl_skel_params* params, int64_t* keys, int32_t* err, tl_stream_t stream) {
  if (!sorted_xyz || !sorted_label || !tree || !keys || !err || n < 0 || n_trees < 0 || n_trees >= ((int64_t)1 << kTreeBits)) return TL_ERR_ARG;
  if (!aligned8(sorted_xyz) || !aligned8(sorted_label) || !aligned8(tree) || !aligned8(keys) || !aligned4(err)) return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (n == 0 || n_trees == 0) return TL_OK;
  if (hipMemsetAsync(err, 0, sizeof(int32_t), tl_s(stream)) != hipSuccess) return TL_ERR_LAUNCH;
  k_skel_voxel_keys<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(sorted_xyz, sorted_label, n, tree, n_trees, *params, keys, err);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_skel_distance(const int64_t* voxel_keys, int64_t n, const int64_t* kstart, int64_t n_trees, const tl_skel_params* params,
                                int32_t* d, int32_t* rounds, tl_stream_t stream) {
  if (!voxel_keys || !kstart || !d || !rounds || n < 0 || n > kMaxVoxels || n_trees < 0 || n_trees >= ((int64_t)1 << kTreeBits)) return TL_ERR_ARG;
  if (!aligned8(voxel_keys) || !aligned8(kstart) || !aligned4(d) || !aligned4(rounds)) return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (n == 0 || n_trees == 0) return TL_OK;
  k_skel_distance<<<(unsigned)n_trees, kDistBlock, 0, tl_s(stream)>>>(voxel_keys, n, kstart, *params, d, rounds);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_skel_nodes(const int64_t* voxel_keys, int64_t n, const int64_t* kstart, int64_t n_trees, const tl_skel_params* params,
                             const int32_t* d, int32_t* parent, int64_t* acc, int64_t* vstar, tl_stream_t stream) {
  if (!voxel_keys || !kstart || !d || !parent || !acc || !vstar || n < 0 || n > kMaxVoxels || n_trees < 0 || n_trees >= ((int64_t)1 << kTreeBits))
    return TL_ERR_ARG;
  if (!aligned8(voxel_keys) || !aligned8(kstart) || !aligned4(d) || !aligned4(parent) || !aligned8(acc) || !aligned8(vstar)) return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (n == 0 || n_trees == 0) return TL_OK;
  unsigned long long* uacc = reinterpret_cast<unsigned long long*>(acc);
  unsigned long long* uvs = reinterpret_cast<unsigned long long*>(vstar);
  k_skel_init<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(n, parent, uacc, uvs);
  TL_CHECK_LAUNCH();
  k_skel_unite<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(voxel_keys, n, kstart, n_trees, *params, d, parent);
  TL_CHECK_LAUNCH();
  k_skel_accumulate<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(voxel_keys, n, d, parent, uacc, uvs);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_skel_links(const int64_t* voxel_keys, int64_t n, const int64_t* kstart, const double* tree, int64_t n_trees,
                             const tl_skel_params* params, const int32_t* d, int32_t* parent, const int64_t* acc, const int64_t* vstar,
                             const int32_t* roots, int64_t n_nodes, const int32_t* node_id, const int64_t* node_start, double* node_xyz,
                             int32_t* node_parent, int32_t* node_bin, int64_t* node_count, tl_stream_t stream) {
  if (!voxel_keys || !kstart || !tree || !d || !parent || !acc || !vstar || !roots || !node_id || !node_start || !node_xyz || !node_parent ||
      !node_bin || !node_count || n < 0 || n > kMaxVoxels || n_nodes < 0 || n_nodes > n || n_trees < 0 || n_trees >= ((int64_t)1 << kTreeBits))
    return TL_ERR_ARG;
  if (!aligned8(voxel_keys) || !aligned8(kstart) || !aligned8(tree) || !aligned4(d) || !aligned4(parent) || !aligned8(acc) || !aligned8(vstar) ||
      !aligned4(roots) || !aligned4(node_id) || !aligned8(node_start) || !aligned8(node_xyz) || !aligned4(node_parent) || !aligned4(node_bin) ||
      !aligned8(node_count))
    return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (n == 0 || n_trees == 0 || n_nodes == 0) return TL_OK;
  k_skel_links<<<tl_grid(n_nodes, kBlock), kBlock, 0, tl_s(stream)>>>(
      voxel_keys, n, kstart, tree, n_trees, *params, d, parent, reinterpret_cast<const unsigned long long*>(acc),
      reinterpret_cast<const unsigned long long*>(vstar), roots, n_nodes, node_id, node_start, node_xyz, node_parent, node_bin, node_count);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
