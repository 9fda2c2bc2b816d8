// Cylinder model of the trees of a labelled cloud: one circle fit per skeleton node, in the plane across the node's axis (the
// semantics are restated in Python in tests/wood_restatement.py).  The radii along the branches, the frusta and the columns are read off
// the node table on the host (util/wood.py).
// tl_wood_row_nodes: one thread per gathered row: the row's voxel key (tl_skel_voxel_keys') is looked up in the ascending array of distinct
//   voxels; a reached voxel (d >= 0) leads through the union-find forest of tl_skel_nodes to its node.  row_node = the node or -1.
// One stable sort of row_node and one searchsorted (the caller's) make every node a contiguous range of the permutation.
// tl_wood_fit:       one wavefront per node, four nodes per workgroup.  The axis (the parent -> node chord) and the plane basis come from
//   the node table; the lanes stride over the node's range for the nine moments, summed by a fixed xor butterfly; lane 0 solves and
//   broadcasts by shuffle; a second strided pass takes the residual.  No LDS, no atomics.
// Every formula is f64 in plain operators under the pragma (no contraction into fma).
#include "tl_circle_fit.h"
#include "tl_scan.h"

#pragma clang fp contract(off)

namespace {
constexpr int kNodesPerBlock = kWaves;       // one wave per node
constexpr int64_t kMaxVoxels = ((int64_t)1 << 31) - 1;           // a voxel and a node are int indices

__global__ void __launch_bounds__(kBlock) k_wood_row_nodes(const int64_t* __restrict__ row_keys, int64_t m, const int64_t* __restrict__ voxel_keys,
                                                           int64_t n_voxels, const int32_t* __restrict__ d, int32_t* __restrict__ uf_parent,
                                                           const int32_t* __restrict__ node_id, int64_t n_nodes, int32_t* __restrict__ row_node) {
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += (int64_t)gridDim.x * kBlock) {
    const int64_t key = row_keys[j];
    int32_t node = -1;
    if (key >= 0) {
      int64_t a = 0, b = n_voxels;
      while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (voxel_keys[mid] < key) a = mid + 1; else b = mid;
      }
      if (a < n_voxels && voxel_keys[a] == key && d[a] >= 0) {
        const int32_t id = node_id[tl_find_root(uf_parent, (int)a)];
        if (id >= 0 && id < n_nodes) node = id;
      }
    }
    row_node[j] = node;
  }
}

__global__ void __launch_bounds__(kBlock) k_wood_fit(const double* __restrict__ xyz, int64_t m, const int64_t* __restrict__ perm,
                                                     const int64_t* __restrict__ range_start, const double* __restrict__ node_xyz,
                                                     const int32_t* __restrict__ node_parent, const int64_t* __restrict__ node_start,
                                                     int64_t n_trees, int64_t n_nodes, tl_wood_params a, double* __restrict__ radius_fit,
                                                     int64_t* __restrict__ count, double* __restrict__ rmse_out, int32_t* __restrict__ state,
                                                     double* __restrict__ centre, double* __restrict__ axis) {
  const int lane = threadIdx.x & 63;
  const double nan = __builtin_nan("");
  for (int64_t i = (int64_t)blockIdx.x * kNodesPerBlock + (threadIdx.x >> 6); i < n_nodes; i += (int64_t)gridDim.x * kNodesPerBlock) {
    int64_t lo = range_start[i], hi = range_start[i + 1];
    if (lo < 0 || hi > m || lo > hi) { lo = 0; hi = 0; }          // a malformed range touches nothing
    // the node's tree (the last t with node_start[t] <= i) turns the local parent into a node index
    int64_t ta = 0, tb = n_trees;
    while (tb - ta > 1) {
      const int64_t mid = (ta + tb) >> 1;
      if (node_start[mid] <= i) ta = mid; else tb = mid;
    }
    const int32_t pl = node_parent[i];
    const int64_t p = pl >= 0 ? node_start[ta] + pl : -1;
    const double cx = node_xyz[3 * i], cy = node_xyz[3 * i + 1], cz = node_xyz[3 * i + 2];
    double ax = 0.0, ay = 0.0, az = 1.0;
    if (p >= 0 && p < n_nodes) {
      const double dx = cx - node_xyz[3 * p], dy = cy - node_xyz[3 * p + 1], dz = cz - node_xyz[3 * p + 2];
      const double seg = sqrt(dx * dx + dy * dy + dz * dz);
      if (seg > 0.0) { ax = dx / seg; ay = dy / seg; az = dz / seg; }
    }
    // the plane basis: e_k along the smallest |a_k| (the first among equals), w = a x e_k, e1 = w / |w|, e2 = a x e1
    int k = 0;
    if (fabs(ay) < fabs(ax)) k = 1;
    if (fabs(az) < (k ? fabs(ay) : fabs(ax))) k = 2;
    const double kx = k == 0 ? 1.0 : 0.0, ky = k == 1 ? 1.0 : 0.0, kz = k == 2 ? 1.0 : 0.0;
    const double wx = ay * kz - az * ky, wy = az * kx - ax * kz, wz = ax * ky - ay * kx;
    const double wn = sqrt(wx * wx + wy * wy + wz * wz);
    const double e1x = wx / wn, e1y = wy / wn, e1z = wz / wn;
    const double e2x = ay * e1z - az * e1y, e2y = az * e1x - ax * e1z, e2z = ax * e1y - ay * e1x;

    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // Suu Suv Svv Su Sv Suw Svw Sw count
    for (int64_t j = lo + lane; j < hi; j += 64) {
      const int64_t r = perm[j];
      if (r < 0 || r >= m) continue;
      const double qx = xyz[3 * r] - cx, qy = xyz[3 * r + 1] - cy, qz = xyz[3 * r + 2] - cz;
      const double u = qx * e1x + qy * e1y + qz * e1z, v = qx * e2x + qy * e2y + qz * e2z;
      const double w = u * u + v * v;
      s[0] = s[0] + u * u; s[1] = s[1] + u * v; s[2] = s[2] + v * v; s[3] = s[3] + u; s[4] = s[4] + v;
      s[5] = s[5] + u * w; s[6] = s[6] + v * w; s[7] = s[7] + w; s[8] = s[8] + 1.0;
    }
    wave_sum<9>(s);
    const double cnt = s[8];                                      // an exact integer: fewer than 2^53 rows
    const bool enough = cnt >= (double)a.min_points && cnt > 0.0;
    Fit f{0.0, 0.0, 0.0, 0};
    if (lane == 0 && enough) f = kasa_solve(s, cnt);              // one lane solves the 3 x 3 system
    f.cx = __shfl(f.cx, 0); f.cy = __shfl(f.cy, 0); f.r = __shfl(f.r, 0); f.ok = __shfl(f.ok, 0);
    double e[1] = {0.0};
    if (f.ok) {
      for (int64_t j = lo + lane; j < hi; j += 64) {
        const int64_t r = perm[j];
        if (r < 0 || r >= m) continue;
        const double qx = xyz[3 * r] - cx, qy = xyz[3 * r + 1] - cy, qz = xyz[3 * r + 2] - cz;
        const double u = qx * e1x + qy * e1y + qz * e1z, v = qx * e2x + qy * e2y + qz * e2z;
        const double du = u - f.cx, dv = v - f.cy;
        const double t = sqrt(du * du + dv * dv) - f.r;
        e[0] = e[0] + t * t;
      }
    }
    wave_sum<1>(e);
    if (lane == 0) {
      const double rmse = f.ok ? sqrt(e[0] / cnt) : nan;
      const bool accept = f.ok && f.r >= a.min_radius && f.r <= a.max_radius && rmse <= a.max_rmse && sqrt(f.cx * f.cx + f.cy * f.cy) <= f.r;
      radius_fit[i] = accept ? f.r : nan;
      count[i] = (int64_t)cnt;
      rmse_out[i] = accept ? rmse : nan;
      state[i] = !enough ? 0 : accept ? 1 : 2;
      centre[3 * i] = accept ? cx + f.cx * e1x + f.cy * e2x : nan;
      centre[3 * i + 1] = accept ? cy + f.cx * e1y + f.cy * e2y : nan;
      centre[3 * i + 2] = accept ? cz + f.cx * e1z + f.cy * e2z : nan;
      axis[3 * i] = ax; axis[3 * i + 1] = ay; axis[3 * i + 2] = az;
    }
  }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// the constraints of the parameter table; NaN fails every one of them
bool params_ok(const tl_wood_params* p) {
  if (!p) return false;
  const double inf = __builtin_inf();
  if (!(p->max_rmse >= 0.0 && p->max_rmse < inf) || !(fabs(p->max_radius) < inf) || !(p->min_radius >= 0.0 && p->min_radius < p->max_radius))
    return false;
  if (!(p->max_growth >= 1.0 && p->max_growth < inf) || !(p->dbh_height >= 0.0 && p->dbh_height < inf) || p->min_points < 3) return false;
  return true;
}
}  // namespace

extern "C" int tl_wood_row_nodes(const int64_t* row_keys, int64_t m, const int64_t* voxel_keys, int64_t n_voxels, const int32_t* d,
                                 int32_t* uf_parent, const int32_t* node_id, int64_t n_nodes, int32_t* row_node, tl_stream_t stream) {
  if (!row_keys || !voxel_keys || !d || !uf_parent || !node_id || !row_node || m < 0 || n_voxels < 0 || n_voxels > kMaxVoxels || n_nodes < 0 ||
      n_nodes > n_voxels)
    return TL_ERR_ARG;
  if (!aligned8(row_keys) || !aligned8(voxel_keys) || !aligned4(d) || !aligned4(uf_parent) || !aligned4(node_id) || !aligned4(row_node)) return TL_ERR_ARG;
  if (m == 0 || n_nodes == 0) return TL_OK;
  k_wood_row_nodes<<<tl_grid(m, kBlock), kBlock, 0, tl_s(stream)>>>(row_keys, m, voxel_keys, n_voxels, d, uf_parent, node_id, n_nodes, row_node);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_wood_fit(const double* sorted_xyz, int64_t m, const int64_t* perm, const int64_t* range_start, const double* node_xyz,
                           const int32_t* node_parent, const int64_t* node_start, int64_t n_trees, int64_t n_nodes, const tl_wood_params* params,
                           double* radius_fit, int64_t* count, double* rmse, int32_t* state, double* centre, double* axis, tl_stream_t stream) {
  if (!sorted_xyz || !perm || !range_start || !node_xyz || !node_parent || !node_start || !radius_fit || !count || !rmse || !state || !centre ||
      !axis || m < 0 || n_trees < 0 || n_nodes < 0 || n_nodes > kMaxVoxels)
    return TL_ERR_ARG;
  if (!aligned8(sorted_xyz) || !aligned8(perm) || !aligned8(range_start) || !aligned8(node_xyz) || !aligned4(node_parent) || !aligned8(node_start) ||
      !aligned8(radius_fit) || !aligned8(count) || !aligned8(rmse) || !aligned4(state) || !aligned8(centre) || !aligned8(axis))
    return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (m == 0 || n_nodes == 0 || n_trees == 0) return TL_OK;
  k_wood_fit<<<tl_grid(n_nodes, kNodesPerBlock), kBlock, 0, tl_s(stream)>>>(sorted_xyz, m, perm, range_start, node_xyz, node_parent, node_start,
                                                                            n_trees, n_nodes, *params, radius_fit, count, rmse, state, centre, axis);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
