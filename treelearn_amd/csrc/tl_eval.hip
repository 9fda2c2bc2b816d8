// Scoring a segmented forest against ground truth (reference tree_learn/util/eval.py, driven by tools/evaluation/evaluate.py).
// tl_eval_contingency: the pred x gt point-count table every detection matrix and the unpartitioned scores follow from (eval.py:7-25,
//   100-123); integer atomics, so the table is exact and deterministic.
// tl_eval_partition: per (gt, pred) pair, tp / fp / fn counts in radial (xy) or vertical (z) bands (eval.py:127-227), reading only the
//   points of the gt tree and of its prediction.  The per-point values that get binned are computed in fp64 in the reference's
//   operation order, written as plain operators under the pragma below: no contraction into fma (hipcc contracts across statements
//   by default, and the __d*_rn helpers are defined outside the pragma's reach), so every band predicate sees the value numpy sees.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kLdsBins = 16384;              // 64 KiB of int32 counters: the table is privatised per workgroup up to this size
constexpr int kMaxIntervals = 256;

// Wave-aggregated add: lanes with equal consecutive bins (spatially sorted inputs) form runs; the first lane of a run adds its length.
// Every lane of the wave must call this (bin < 0: nothing to add).
template <bool LDS>
__device__ __forceinline__ void add_runs(int bin, int* __restrict__ hist, int64_t* __restrict__ table) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(bin, 1);
  const bool head = lane == 0 || prev != bin;
  const uint64_t heads = __ballot(head);
  if (head && bin >= 0) {
    const uint64_t above = heads & ~((2ull << lane) - 1ull);     // heads after this lane (lane 63: none)
    const int end = above ? __ffsll((unsigned long long)above) - 1 : 64;
    const int len = end - lane;
    if (LDS) atomicAdd(hist + bin, len);
    else atomicAdd(reinterpret_cast<unsigned long long*>(table + bin), (unsigned long long)len);
  }
}

template <bool LDS>
__global__ void __launch_bounds__(kBlock) k_eval_contingency(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int64_t n,
                                                             int64_t n_pred, int64_t n_gt, int64_t non_tree, int64_t* __restrict__ table) {
  extern __shared__ int hist[];
  const int64_t ncols = n_gt + 1;
  const int nbins = (int)((n_pred + 1) * ncols);
  if (LDS) {
    for (int b = threadIdx.x; b < nbins; b += kBlock) hist[b] = 0;
    __syncthreads();
  }
  // block-uniform trip count: every lane takes part in the wave shuffles, lanes past n carry bin -1
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    int bin = -1;
    if (i < n) {
      const int64_t p = pred[i], g = gt[i];
      const int64_t r = p < 0 ? 0 : p + 1;
      const int64_t c = (g < 0 || g == non_tree) ? 0 : g + 1;
      if (r <= n_pred && c <= n_gt) bin = (int)(r * ncols + c);
    }
    add_runs<LDS>(bin, hist, table);
  }
  if (LDS) {
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += kBlock) {
      const int v = hist[b];
      if (v) atomicAdd(reinterpret_cast<unsigned long long*>(table + b), (unsigned long long)v);
    }
  }
}

// top-5 (descending, duplicates kept) of a thread's values
__device__ __forceinline__ void top5_insert(double (&t)[5], double v) {
  if (!(v > t[4])) return;
  int k = 4;
  while (k > 0 && v > t[k - 1]) { t[k] = t[k - 1]; --k; }
  t[k] = v;
}

struct Seg { int64_t lo, hi; };

__device__ __forceinline__ Seg segment(const int64_t* __restrict__ start, int64_t nseg, int64_t id, int64_t n) {
  Seg s{0, 0};
  if (id < 0 || id >= nseg) return s;
  const int64_t a = start[id], b = start[id + 1];
  if (a < 0 || b > n || a > b) return s;
  s.lo = a; s.hi = b;
  return s;
}

// One workgroup per (gt, pred) pair.
__global__ void __launch_bounds__(kBlock) k_eval_partition(const double* __restrict__ xyz, const int64_t* __restrict__ gt, const int64_t* __restrict__ pred,
                                                           int64_t n, const int64_t* __restrict__ gt_order, const int64_t* __restrict__ gt_start,
                                                           int64_t n_gt, const int64_t* __restrict__ pred_order, const int64_t* __restrict__ pred_start,
                                                           int64_t n_pred, const int64_t* __restrict__ pairs, const double* __restrict__ edges, int n_int,
                                                           int mode, int64_t* __restrict__ out_tp, int64_t* __restrict__ out_fp,
                                                           int64_t* __restrict__ out_fn, double* __restrict__ norm) {
  __shared__ double s_edges[kMaxIntervals + 1];
  __shared__ int s_tp[kMaxIntervals], s_fp[kMaxIntervals], s_fn[kMaxIntervals];
  __shared__ double s_a[kBlock], s_b[kBlock];
  __shared__ int s_f[kBlock];
  __shared__ double s_top[kBlock * 5];
  __shared__ double s_min[kBlock / 64];
  __shared__ double s_par[3];
  const int tid = threadIdx.x;
  const int64_t pair = blockIdx.x;
  const int64_t g = pairs[2 * pair], p = pairs[2 * pair + 1];
  const Seg gs = segment(gt_start, n_gt, g, n), ps = segment(pred_start, n_pred, p, n);
  for (int k = tid; k <= n_int; k += kBlock) s_edges[k] = edges[k];
  for (int k = tid; k < n_int; k += kBlock) { s_tp[k] = 0; s_fp[k] = 0; s_fn[k] = 0; }

  // minimum z of the gt tree (np.min: order-free)
  double zmin = __builtin_inf();
  for (int64_t j = gs.lo + tid; j < gs.hi; j += kBlock) {
    const int64_t i = gt_order[j];
    if ((uint64_t)i < (uint64_t)n) zmin = fmin(zmin, xyz[3 * i + 2]);
  }
  for (int o = 32; o > 0; o >>= 1) zmin = fmin(zmin, __shfl_xor(zmin, o));
  if ((tid & 63) == 0) s_min[tid >> 6] = zmin;
  __syncthreads();
  zmin = s_min[0];
  for (int w = 1; w < kBlock / 64; ++w) zmin = fmin(zmin, s_min[w]);

  // xy: tree position = np.mean(lowest_points, axis=0)[:2], lowest = z <= min_z + 0.30; numpy reduces axis 0 of the (n, 3) array row
  // after row, so the sum is sequential in point order (one thread, fed through LDS a chunk at a time), then divided by the count
  double px = 0.0, py = 0.0;
  if (mode == TL_EVAL_XY) {
    const double thr = zmin + 0.30;
    double sx = 0.0, sy = 0.0;
    int64_t cnt = 0;
    for (int64_t j0 = gs.lo; j0 < gs.hi; j0 += kBlock) {
      const int64_t j = j0 + tid;
      int f = 0;
      if (j < gs.hi) {
        const int64_t i = gt_order[j];
        if ((uint64_t)i < (uint64_t)n && xyz[3 * i + 2] <= thr) { f = 1; s_a[tid] = xyz[3 * i]; s_b[tid] = xyz[3 * i + 1]; }
      }
      s_f[tid] = f;
      __syncthreads();
      if (tid == 0) {
        const int m = (int)((gs.hi - j0) < kBlock ? (gs.hi - j0) : kBlock);
        for (int t = 0; t < m; ++t)
          if (s_f[t]) {
            if (cnt == 0) { sx = s_a[t]; sy = s_b[t]; }
            else { sx = sx + s_a[t]; sy = sy + s_b[t]; }
            ++cnt;
          }
      }
      __syncthreads();
    }
    if (tid == 0) { s_par[0] = sx / (double)cnt; s_par[1] = sy / (double)cnt; }
    __syncthreads();
    px = s_par[0]; py = s_par[1];
  }

  // regularised max: the 5th-largest tree value (sorted_inds[-5]); xy: distance to the position, z: raw z
  double t5[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) t5[k] = -__builtin_inf();
  for (int64_t j = gs.lo + tid; j < gs.hi; j += kBlock) {
    const int64_t i = gt_order[j];
    if ((uint64_t)i >= (uint64_t)n) continue;
    double v;
    if (mode == TL_EVAL_XY) {
      const double dx = xyz[3 * i] - px, dy = xyz[3 * i + 1] - py;
      v = sqrt(dx * dx + dy * dy);
    } else {
      v = xyz[3 * i + 2];
    }
    top5_insert(t5, v);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) s_top[tid * 5 + k] = t5[k];
  __syncthreads();
  if (tid == 0) {
    double a[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) a[k] = -__builtin_inf();
    for (int t = 0; t < kBlock * 5; ++t) top5_insert(a, s_top[t]);
    s_par[2] = a[4];
  }
  __syncthreads();
  const double regmax = s_par[2];
  const double denom = mode == TL_EVAL_XY ? regmax : regmax - zmin;     // z: (regularized_max - min z), once

  auto value = [&](int64_t i) -> double {
    if (mode == TL_EVAL_XY) {
      const double dx = xyz[3 * i] - px, dy = xyz[3 * i + 1] - py;
      return sqrt(dx * dx + dy * dy) / denom;
    }
    return (xyz[3 * i + 2] - zmin) / denom;
  };
  // gt points: tp if predicted p, else fn; pred-p points of another label: fp.  Each band tested on its own (>= lo && < hi).
  for (int64_t j = gs.lo + tid; j < gs.hi; j += kBlock) {
    const int64_t i = gt_order[j];
    if ((uint64_t)i >= (uint64_t)n) continue;
    const double v = value(i);
    int* c = pred[i] == p ? s_tp : s_fn;
    for (int k = 0; k < n_int; ++k)
      if (v >= s_edges[k] && v < s_edges[k + 1]) atomicAdd(c + k, 1);
  }
  for (int64_t j = ps.lo + tid; j < ps.hi; j += kBlock) {
    const int64_t i = pred_order[j];
    if ((uint64_t)i >= (uint64_t)n || gt[i] == g) continue;
    const double v = value(i);
    for (int k = 0; k < n_int; ++k)
      if (v >= s_edges[k] && v < s_edges[k + 1]) atomicAdd(s_fp + k, 1);
  }
  __syncthreads();
  for (int k = tid; k < n_int; k += kBlock) {
    out_tp[pair * n_int + k] = s_tp[k];
    out_fp[pair * n_int + k] = s_fp[k];
    out_fn[pair * n_int + k] = s_fn[k];
  }
  if (tid == 0) {
    if (mode == TL_EVAL_XY) { norm[3 * pair] = px; norm[3 * pair + 1] = py; norm[3 * pair + 2] = regmax; }
    else { norm[3 * pair] = zmin; norm[3 * pair + 1] = regmax; norm[3 * pair + 2] = 0.0; }
  }
}
}  // namespace

extern "C" int tl_eval_contingency(const int64_t* pred, const int64_t* gt, int64_t n, int64_t n_pred, int64_t n_gt, int64_t non_tree_label,
                                   int64_t* table, tl_stream_t stream) {
  if (!pred || !gt || !table || n < 0 || n >= ((int64_t)1 << 31) || n_pred < 0 || n_gt < 0) return TL_ERR_ARG;
  const int64_t nbins = (n_pred + 1) * (n_gt + 1);
  if (n_pred >= ((int64_t)1 << 31) || n_gt >= ((int64_t)1 << 31) || nbins >= ((int64_t)1 << 31)) return TL_ERR_ARG;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(table, 0, (size_t)nbins * sizeof(int64_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (n == 0) return TL_OK;
  if (nbins <= kLdsBins) {
    const unsigned grid = tl_grid(n, kBlock) < 1024 ? tl_grid(n, kBlock) : 1024u;
    k_eval_contingency<true><<<grid, kBlock, (size_t)nbins * sizeof(int), s>>>(pred, gt, n, n_pred, n_gt, non_tree_label, table);
  } else {
    k_eval_contingency<false><<<tl_grid(n, kBlock), kBlock, 0, s>>>(pred, gt, n, n_pred, n_gt, non_tree_label, table);
  }
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_eval_partition(const double* xyz, const int64_t* gt, const int64_t* pred, int64_t n, const int64_t* gt_order,
                                 const int64_t* gt_start, int64_t n_gt, const int64_t* pred_order, const int64_t* pred_start, int64_t n_pred,
                                 const int64_t* pairs, int64_t m, const double* edges, int n_edges, int mode, int64_t* tp, int64_t* fp,
                                 int64_t* fn, double* norm, tl_stream_t stream) {
  if (!xyz || !gt || !pred || !gt_order || !gt_start || !pred_order || !pred_start || !pairs || !edges || !tp || !fp || !fn || !norm)
    return TL_ERR_ARG;
  if (n < 0 || n_gt < 0 || n_pred < 0 || m < 0 || m >= ((int64_t)1 << 31) || n_edges < 2 || n_edges > kMaxIntervals + 1 ||
      (mode != TL_EVAL_XY && mode != TL_EVAL_Z))
    return TL_ERR_ARG;
  if (m == 0) return TL_OK;
  k_eval_partition<<<(unsigned)m, kBlock, 0, tl_s(stream)>>>(xyz, gt, pred, n, gt_order, gt_start, n_gt, pred_order, pred_start, n_pred, pairs,
                                                              edges, n_edges - 1, mode, tp, fp, fn, norm);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
