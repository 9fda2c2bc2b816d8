// Random training crops on the device: the four numpy stages of SampleGenerator's random-crop half
// (tree_learn/util/data_preparation.py:136-172,209-230,264-289,571-586) on a plot resident in HBM.
//
//   occupancy marking   <- get_occupancy_grid, :154-166 (Python double loop over cells, all points scanned per cell)
//   hole filling        <- fill_holes, :571-586 (Python double loop)
//   candidate occupancy <- check_occupancy, :209-230 (candidates x cells boolean matrix)
//   crop extraction     <- save, :264-289 ((10 crops) x N boolean matrix over the whole plot per 10 crops)
//
// Exactness: f64 wherever the reference is f64, plain operators in the reference's order under the
// pragma below (no fma contraction), no division in the step search.  The reference's ±3 m view boxes
// (generate_views, :548-561) only preselect a superset of the rotated square and are not restated.
#include "tl_scan.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxCrops = 32;

// first k in [0, m) with steps[k] >= v (m when none): steps ascending, f64 compare of the widened f32 value
__device__ __forceinline__ int lower_bound(const double* __restrict__ steps, int m, double v) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (steps[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// :162-166: cell (i, j) is occupied when some point has steps[i] < x <= steps[i+1] and likewise in y
__global__ void __launch_bounds__(256) k_occ_mark(const float* __restrict__ xy, int64_t n, const double* __restrict__ xs, int X,
                                                  const double* __restrict__ ys, int Y, uint8_t* __restrict__ grid) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const double x = (double)xy[p * 2], y = (double)xy[p * 2 + 1];
    const int kx = lower_bound(xs, X + 1, x), ky = lower_bound(ys, Y + 1, y);
    if (kx >= 1 && kx <= X && ky >= 1 && ky <= Y) grid[(int64_t)(kx - 1) * Y + (ky - 1)] = 1;
  }
}

// :575-585, reading the unfilled grid only
__global__ void __launch_bounds__(256) k_fill(const uint8_t* __restrict__ raw, int X, int Y, int h, double min_pct, uint8_t* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= (int64_t)X * Y) return;
  if (raw[c]) { out[c] = 1; return; }
  const int i = (int)(c / Y), j = (int)(c % Y);
  const int i0 = i - min(h, i), i1 = i + min(h + 1, X - i), j0 = j - min(h, j), j1 = j + min(h + 1, Y - j);
  int cnt = 0;
  for (int a = i0; a < i1; ++a)
    for (int b = j0; b < j1; ++b) cnt += raw[(int64_t)a * Y + b] != 0;
  const double pct = (double)cnt / (double)((int64_t)(i1 - i0) * (j1 - j0));
  out[c] = pct >= min_pct;
}

// (s0, s1) @ Rinv.T with Rinv row-major {a, b, c, d}: u = s0 a + s1 b, v = s0 c + s1 d (invert_rotate_and_shift, :535-545)
__device__ __forceinline__ bool in_square(double s0, double s1, const double* __restrict__ r, double half, double* u, double* v) {
  *u = s0 * r[0] + s1 * r[1];
  *v = s0 * r[2] + s1 * r[3];
  return fabs(*u) <= half && fabs(*v) <= half;          // norm(ord=inf) <= size / 2; a NaN row is outside, as in numpy
}

// :217-228, one workgroup per candidate: grid-cell centres are f64, so the centring subtraction is f64 here
__global__ void __launch_bounds__(256) k_check(const double* __restrict__ cx, int X, const double* __restrict__ cy, int Y,
                                               const uint8_t* __restrict__ occ, const float* __restrict__ centre, const double* __restrict__ rinv,
                                               double half, double denom, double min_pct, double* __restrict__ sum, uint8_t* __restrict__ pass) {
  const int64_t k = blockIdx.x;
  const double ox = (double)centre[k * 2], oy = (double)centre[k * 2 + 1];
  const double* r = rinv + k * 4;
  uint32_t cnt = 0;
  for (int64_t c = threadIdx.x; c < (int64_t)X * Y; c += 256) {
    const int i = (int)(c / Y), j = (int)(c % Y);
    double u, v;
    if (occ[c] && in_square(cx[i] - ox, cy[j] - oy, r, half, &u, &v)) ++cnt;
  }
  uint32_t tot; tl_block_scan<4>(cnt, &tot);
  if (threadIdx.x == 0) {
    const double s = (double)tot;
    if (sum) sum[k] = s;
    if (pass) pass[k] = s / denom > min_pct;
  }
}

struct CropSet {
  float cen[kMaxCrops * 2];
  double r[kMaxCrops * 4];
};

// :270-276 for a batch of crops: the f32 xy minus the f32 centre (a float32 subtraction in numpy), widened by the rotation
__device__ __forceinline__ uint32_t crop_bits(const CropSet& cs, int nc, float x, float y, double half) {
  uint32_t bits = 0;
  for (int c = 0; c < nc; ++c) {
    const double s0 = (double)(x - cs.cen[c * 2]), s1 = (double)(y - cs.cen[c * 2 + 1]);
    double u, v;
    if (in_square(s0, s1, cs.r + c * 4, half, &u, &v)) bits |= 1u << c;
  }
  return bits;
}

__device__ __forceinline__ void load_set(CropSet& cs, const float* __restrict__ centre, const double* __restrict__ rinv, int nc) {
  for (int t = threadIdx.x; t < nc * 2; t += 256) cs.cen[t] = centre[t];
  for (int t = threadIdx.x; t < nc * 4; t += 256) cs.r[t] = rinv[t];
  __syncthreads();
}

// per block and crop: rows inside the crop -> part[c * nb + block]
__global__ void __launch_bounds__(256) k_crop_partials(const float* __restrict__ xyz, int64_t n, int nc, const float* __restrict__ centre,
                                                       const double* __restrict__ rinv, double half, int32_t* __restrict__ part, int64_t nb) {
  __shared__ CropSet cs;
  load_set(cs, centre, rinv, nc);
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t bits[kScanItems];
  for (int j = 0; j < kScanItems; ++j) {
    bits[j] = 0;
    if (base + j < n) bits[j] = crop_bits(cs, nc, xyz[(base + j) * 3], xyz[(base + j) * 3 + 1], half);
  }
  for (int c = 0; c < nc; ++c) {
    uint32_t s = 0;
    for (int j = 0; j < kScanItems; ++j) s += (bits[j] >> c) & 1u;
    uint32_t tot; tl_block_scan<4>(s, &tot);
    if (threadIdx.x == 0) part[c * nb + blockIdx.x] = (int32_t)tot;
  }
}

// :276-289: the kept rows in plot order, rotated xy rounded to f32 (astype(np.float32)), z as it is, label -> int32, features
__global__ void __launch_bounds__(256) k_crop_scatter(const float* __restrict__ xyz, const float* __restrict__ label, const float* __restrict__ feat,
                                                      int64_t n, int F, int nc, const float* __restrict__ centre, const double* __restrict__ rinv,
                                                      double half, const int32_t* __restrict__ part, int64_t nb, int64_t cap,
                                                      float* __restrict__ out_xyz, int32_t* __restrict__ out_label, float* __restrict__ out_feat) {
  __shared__ CropSet cs;
  load_set(cs, centre, rinv, nc);
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t bits[kScanItems];
  for (int j = 0; j < kScanItems; ++j) {
    bits[j] = 0;
    if (base + j < n) bits[j] = crop_bits(cs, nc, xyz[(base + j) * 3], xyz[(base + j) * 3 + 1], half);
  }
  for (int c = 0; c < nc; ++c) {
    uint32_t s = 0;
    for (int j = 0; j < kScanItems; ++j) s += (bits[j] >> c) & 1u;
    uint32_t tot; int64_t pos = (int64_t)tl_block_scan<4>(s, &tot) + (uint32_t)part[c * nb + blockIdx.x];
    for (int j = 0; j < kScanItems; ++j)
      if ((bits[j] >> c) & 1u) {
        const int64_t r = base + j;
        if (pos < cap) {
          const double s0 = (double)(xyz[r * 3] - cs.cen[c * 2]), s1 = (double)(xyz[r * 3 + 1] - cs.cen[c * 2 + 1]);
          double u, v; in_square(s0, s1, cs.r + c * 4, half, &u, &v);
          out_xyz[pos * 3] = (float)u; out_xyz[pos * 3 + 1] = (float)v; out_xyz[pos * 3 + 2] = xyz[r * 3 + 2];
          out_label[pos] = (int32_t)label[r];
          for (int f = 0; f < F; ++f) out_feat[pos * F + f] = feat[r * F + f];
        }
        ++pos;
      }
  }
}

}  // namespace

extern "C" {

int tl_crops_occupancy(const float* xy, int64_t n, const double* x_steps, int x_dim, const double* y_steps, int y_dim, uint8_t* grid,
                       tl_stream_t stream) {
  if (!xy || !x_steps || !y_steps || !grid || n <= 0 || x_dim <= 0 || y_dim <= 0) return TL_ERR_ARG;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(grid, 0, (size_t)x_dim * y_dim, s) != hipSuccess) return TL_ERR_LAUNCH;
  k_occ_mark<<<tl_grid(n, 256), 256, 0, s>>>(xy, n, x_steps, x_dim, y_steps, y_dim, grid);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_crops_fill(const uint8_t* raw, int x_dim, int y_dim, int how_far_fill, double min_percent_occupied_fill, uint8_t* filled,
                  tl_stream_t stream) {
  if (!raw || !filled || raw == filled || x_dim <= 0 || y_dim <= 0 || how_far_fill < 0) return TL_ERR_ARG;
  const int64_t cells = (int64_t)x_dim * y_dim;
  k_fill<<<(unsigned)tl_cdiv(cells, 256), 256, 0, tl_s(stream)>>>(raw, x_dim, y_dim, how_far_fill, min_percent_occupied_fill, filled);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_crops_check(const double* cell_x, int x_dim, const double* cell_y, int y_dim, const uint8_t* occupancy, const float* centres,
                   const double* rinv, int64_t n_candidates, double chunk_size, double denominator, double min_percent_occupied_choose,
                   double* sums, uint8_t* pass, tl_stream_t stream) {
  if (!cell_x || !cell_y || !occupancy || !centres || !rinv || (!sums && !pass) || x_dim <= 0 || y_dim <= 0 || n_candidates <= 0 ||
      n_candidates > 0x7fffffff)
    return TL_ERR_ARG;
  k_check<<<(unsigned)n_candidates, 256, 0, tl_s(stream)>>>(cell_x, x_dim, cell_y, y_dim, occupancy, centres, rinv, chunk_size / 2,
                                                             denominator, min_percent_occupied_choose, sums, pass);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int64_t tl_crops_ws_words(int64_t n, int n_crops) { return tl_cdiv(n, kScanTile) * (int64_t)n_crops + 1; }

int tl_crops_count(const float* xyz, int64_t n, int n_crops, const float* centres, const double* rinv, double chunk_size, int32_t* counts,
                   int32_t* ws, tl_stream_t stream) {
  if (!xyz || !centres || !rinv || !counts || !ws || n <= 0 || n_crops <= 0 || n_crops > kMaxCrops) return TL_ERR_ARG;
  if (n > (int64_t)INT32_MAX / n_crops) return TL_ERR_ARG;             // row offsets of the whole batch are int32
  const int64_t nb = tl_cdiv(n, kScanTile);
  hipStream_t s = tl_s(stream);
  k_crop_partials<<<(unsigned)nb, 256, 0, s>>>(xyz, n, n_crops, centres, rinv, chunk_size / 2, ws, nb);
  tl_launch_scan_parts(ws, nb, n_crops, counts, nullptr, s);       // crop-major: crop c's rows follow crop c-1's
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_crops_extract(const float* xyz, const float* label, const float* feat, int64_t n, int F, int n_crops, const float* centres,
                     const double* rinv, double chunk_size, const int32_t* ws, int64_t capacity, float* out_xyz, int32_t* out_label,
                     float* out_feat, tl_stream_t stream) {
  if (!xyz || !label || (F > 0 && (!feat || !out_feat)) || !centres || !rinv || !ws || !out_xyz || !out_label || n <= 0 || F < 0 ||
      n_crops <= 0 || n_crops > kMaxCrops || capacity <= 0 || n > (int64_t)INT32_MAX / n_crops)
    return TL_ERR_ARG;
  const int64_t nb = tl_cdiv(n, kScanTile);
  k_crop_scatter<<<(unsigned)nb, 256, 0, tl_s(stream)>>>(xyz, label, feat, n, F, n_crops, centres, rinv, chunk_size / 2, ws, nb, capacity,
                                                          out_xyz, out_label, out_feat);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

}  // extern "C"
