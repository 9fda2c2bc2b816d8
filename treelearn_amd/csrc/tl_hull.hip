// Points against the plot outline (reference tree_learn/util/pipeline.py:211-223 `get_coords_within_shape`, applied to the polygon of
// `get_hull` and to the ring buffer of `get_hull_buffer`, :226-275).  One u8 per point: bit 0 = strictly inside the closed ring
// (even-odd, half-open crossing test), bit 1 = closer to the ring than r.
//
// Pruning structures, built on the device from the ring alone (counts -> scan on the host side of the call -> fill):
//   slabs: horizontal bands; a slab lists the segments whose y-range, widened by `pad`, meets it.  The crossing test of a point only
//          reads its slab.
//   cells: a uniform grid over the ring's box widened by r + pad; a cell lists the segments whose distance from the cell centre is
//          below r + half the cell diagonal + pad (so every segment within r of any point of the cell); `covered` marks cells that lie
//          entirely within r - 2 pad of one listed segment (distance to a segment is convex: its maximum over a rectangle is at a corner).
// The per-point arithmetic is f64, written as plain operators in the order of include/treelearn_hip.h under the pragma below (no fma
// contraction), so both bits equal a numpy evaluation of the same formulas over ALL segments; the pruning only drops segments that
// cannot change the answer by more than `pad`, which the host sizes well above the rounding of the formulas.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;

__device__ __forceinline__ double seg_d2(double px, double py, double x1, double y1, double x2, double y2) {
  const double dx = x2 - x1, dy = y2 - y1;
  double t = ((px - x1) * dx + (py - y1) * dy) / (dx * dx + dy * dy);
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);                       // a NaN t (zero-length segment) stays NaN, as np.clip leaves it
  const double qx = x1 + t * dx, qy = y1 + t * dy;
  return (px - qx) * (px - qx) + (py - qy) * (py - qy);
}

__device__ __forceinline__ bool crosses(double px, double py, double x1, double y1, double x2, double y2) {
  if ((y1 > py) != (y2 > py)) {
    const double xi = x1 + (py - y1) * (x2 - x1) / (y2 - y1);
    return px < xi;
  }
  return false;
}

__device__ __forceinline__ int clampi(double f, int n) {           // floor(f) clamped to [0, n - 1]; NaN -> 0
  if (!(f >= 0.0)) return 0;
  if (f >= (double)n) return n - 1;
  return (int)floor(f);
}

// Segment k's cell rectangle [cx0, cx1] x [cy0, cy1] and slab range [s0, s1]; the same code feeds the count and the fill pass.
struct SegBox { int cx0, cx1, cy0, cy1, s0, s1; };

__device__ __forceinline__ SegBox seg_box(const double* __restrict__ ring, int64_t k, const tl_ring_grid& g) {
  const double x1 = ring[2 * k], y1 = ring[2 * k + 1], x2 = ring[2 * k + 2], y2 = ring[2 * k + 3];
  const double xmin = fmin(x1, x2), xmax = fmax(x1, x2), ymin = fmin(y1, y2), ymax = fmax(y1, y2);
  SegBox b;
  b.s0 = clampi((ymin - g.pad - g.slab_lo) / g.slab_h, g.nslab);
  b.s1 = clampi((ymax + g.pad - g.slab_lo) / g.slab_h, g.nslab);
  if (g.nx > 0) {
    const double reach = g.r + g.pad;
    b.cx0 = clampi((xmin - reach - g.lo[0]) / g.h, g.nx);
    b.cx1 = clampi((xmax + reach - g.lo[0]) / g.h, g.nx);
    b.cy0 = clampi((ymin - reach - g.lo[1]) / g.h, g.ny);
    b.cy1 = clampi((ymax + reach - g.lo[1]) / g.h, g.ny);
  } else {
    b.cx0 = 0; b.cx1 = -1; b.cy0 = 0; b.cy1 = -1;
  }
  return b;
}

__device__ __forceinline__ bool seg_near_cell(const double* __restrict__ ring, int64_t k, const tl_ring_grid& g, int cx, int cy) {
  const double ccx = g.lo[0] + ((double)cx + 0.5) * g.h, ccy = g.lo[1] + ((double)cy + 0.5) * g.h;
  const double reach = g.r + 0.70711 * g.h + 2.0 * g.pad;        // half diagonal = 0.7071067.. h
  const double d2 = seg_d2(ccx, ccy, ring[2 * k], ring[2 * k + 1], ring[2 * k + 2], ring[2 * k + 3]);
  return !(d2 >= reach * reach);                                 // NaN (zero-length segment): listed, harmlessly
}

template <bool FILL>
__global__ void __launch_bounds__(kBlock) k_ring_lists(const double* __restrict__ ring, int64_t nseg, tl_ring_grid g,
                                                       int64_t* __restrict__ cell_cnt, int64_t* __restrict__ slab_cnt,
                                                       int32_t* __restrict__ cell_seg, int32_t* __restrict__ slab_seg) {
  for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nseg; k += (int64_t)gridDim.x * kBlock) {
    const SegBox b = seg_box(ring, k, g);
    for (int s = b.s0; s <= b.s1; ++s) {
      const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(slab_cnt + s), 1ull);
      if (FILL) slab_seg[at] = (int32_t)k;
    }
    for (int cy = b.cy0; cy <= b.cy1; ++cy)
      for (int cx = b.cx0; cx <= b.cx1; ++cx) {
        if (!seg_near_cell(ring, k, g, cx, cy)) continue;
        const int64_t c = (int64_t)cy * g.nx + cx;
        const unsigned long long at = atomicAdd(reinterpret_cast<unsigned long long*>(cell_cnt + c), 1ull);
        if (FILL) cell_seg[at] = (int32_t)k;
      }
  }
}

__global__ void __launch_bounds__(kBlock) k_ring_covered(const double* __restrict__ ring, tl_ring_grid g, const int64_t* __restrict__ cell_start,
                                                         const int32_t* __restrict__ cell_seg, uint8_t* __restrict__ covered) {
  const int64_t ncells = (int64_t)g.nx * g.ny;
  for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * kBlock) {
    const int cx = (int)(c % g.nx), cy = (int)(c / g.nx);
    const double x0 = g.lo[0] + (double)cx * g.h, y0 = g.lo[1] + (double)cy * g.h;
    const double x1 = x0 + g.h, y1 = y0 + g.h;
    uint8_t cov = 0;
    if (g.cover_r2 > 0.0) {
      for (int64_t j = cell_start[c]; j < cell_start[c + 1] && !cov; ++j) {
        const int64_t k = cell_seg[j];
        const double ax = ring[2 * k], ay = ring[2 * k + 1], bx = ring[2 * k + 2], by = ring[2 * k + 3];
        cov = seg_d2(x0, y0, ax, ay, bx, by) < g.cover_r2 && seg_d2(x1, y0, ax, ay, bx, by) < g.cover_r2 &&
              seg_d2(x0, y1, ax, ay, bx, by) < g.cover_r2 && seg_d2(x1, y1, ax, ay, bx, by) < g.cover_r2;
      }
    }
    covered[c] = cov;
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_ring_classify(const T* __restrict__ pts, int64_t ld, int64_t n, const double* __restrict__ ring,
                                                          tl_ring_grid g, const int64_t* __restrict__ slab_start, const int32_t* __restrict__ slab_seg,
                                                          const int64_t* __restrict__ cell_start, const int32_t* __restrict__ cell_seg,
                                                          const uint8_t* __restrict__ covered, uint8_t* __restrict__ out) {
  const double r2 = g.r * g.r;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double px = (double)pts[i * ld], py = (double)pts[i * ld + 1];
    uint8_t bits = 0;
    const double fs = (py - g.slab_lo) / g.slab_h;
    if (fs >= 0.0 && fs < (double)g.nslab) {
      const int s = (int)floor(fs);
      int par = 0;
      for (int64_t j = slab_start[s]; j < slab_start[s + 1]; ++j) {
        const int64_t k = slab_seg[j];
        par ^= crosses(px, py, ring[2 * k], ring[2 * k + 1], ring[2 * k + 2], ring[2 * k + 3]) ? 1 : 0;
      }
      bits |= (uint8_t)par;
    }
    if (g.nx > 0) {
      const double fx = (px - g.lo[0]) / g.h, fy = (py - g.lo[1]) / g.h;
      if (fx >= 0.0 && fx < (double)g.nx && fy >= 0.0 && fy < (double)g.ny) {
        const int64_t c = (int64_t)floor(fy) * g.nx + (int64_t)floor(fx);
        bool near = covered[c] != 0;
        for (int64_t j = cell_start[c]; j < cell_start[c + 1] && !near; ++j) {
          const int64_t k = cell_seg[j];
          near = seg_d2(px, py, ring[2 * k], ring[2 * k + 1], ring[2 * k + 2], ring[2 * k + 3]) < r2;
        }
        if (near) bits |= 2;
      }
    }
    out[i] = bits;
  }
}

bool grid_ok(const tl_ring_grid* g) {
  if (!g || !(g->slab_h > 0.0) || g->nslab < 1 || !(g->r >= 0.0) || !(g->pad >= 0.0)) return false;
  if (g->nx < 0 || g->ny < 0 || (g->nx > 0) != (g->ny > 0)) return false;
  if (g->nx > 0 && !(g->h > 0.0)) return false;
  return (int64_t)g->nx * g->ny < ((int64_t)1 << 31);
}
}  // namespace

extern "C" int tl_ring_lists(const double* ring, int64_t V, const tl_ring_grid* grid, int64_t* cell_cnt, int64_t* slab_cnt, int32_t* cell_seg,
                             int32_t* slab_seg, tl_stream_t stream) {
  if (!ring || V < 2 || V >= ((int64_t)1 << 31) || !grid_ok(grid) || !slab_cnt || (grid->nx > 0 && !cell_cnt)) return TL_ERR_ARG;
  const bool fill = cell_seg != nullptr || slab_seg != nullptr;
  if (fill && (!slab_seg || (grid->nx > 0 && !cell_seg))) return TL_ERR_ARG;
  const int64_t nseg = V - 1;
  hipStream_t s = tl_s(stream);
  if (fill) k_ring_lists<true><<<tl_grid(nseg, kBlock), kBlock, 0, s>>>(ring, nseg, *grid, cell_cnt, slab_cnt, cell_seg, slab_seg);
  else k_ring_lists<false><<<tl_grid(nseg, kBlock), kBlock, 0, s>>>(ring, nseg, *grid, cell_cnt, slab_cnt, nullptr, nullptr);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_ring_covered(const double* ring, const tl_ring_grid* grid, const int64_t* cell_start, const int32_t* cell_seg, uint8_t* covered,
                               tl_stream_t stream) {
  if (!ring || !grid_ok(grid)) return TL_ERR_ARG;
  const int64_t ncells = (int64_t)grid->nx * grid->ny;
  if (ncells == 0) return TL_OK;
  if (!cell_start || !cell_seg || !covered) return TL_ERR_ARG;
  k_ring_covered<<<tl_grid(ncells, kBlock), kBlock, 0, tl_s(stream)>>>(ring, *grid, cell_start, cell_seg, covered);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_ring_classify(const void* pts, int dtype_f64, int64_t ld, int64_t n, const double* ring, const tl_ring_grid* grid,
                                const int64_t* slab_start, const int32_t* slab_seg, const int64_t* cell_start, const int32_t* cell_seg,
                                const uint8_t* covered, uint8_t* out, tl_stream_t stream) {
  if (!ring || !grid_ok(grid) || !slab_start || !slab_seg || n < 0 || ld < 2 || (n > 0 && (!pts || !out))) return TL_ERR_ARG;
  if (grid->nx > 0 && (!cell_start || !cell_seg || !covered)) return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  hipStream_t s = tl_s(stream);
  if (dtype_f64)
    k_ring_classify<double><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const double*>(pts), ld, n, ring, *grid, slab_start, slab_seg,
                                                                  cell_start, cell_seg, covered, out);
  else
    k_ring_classify<float><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const float*>(pts), ld, n, ring, *grid, slab_start, slab_seg,
                                                                 cell_start, cell_seg, covered, out);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
