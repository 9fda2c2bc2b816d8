// Pictures of clouds and rasters: orthographic point splats with a depth test, rasters as depth-keyed pixels, and a shading pass that
// darkens a pixel by how far its neighbours stand in front of it (the semantics are the project's own, restated in numpy in
// tests/render_restatement.py).
// tl_splat:        one pass over the rows.  A row is projected through its view record, its f32 depth and its colour are packed into one
//   u64 key (order-preserving image of the depth in the high word, rgb in the low one) and every pixel of its k x k footprint inside the
//   row's viewport takes a 64-bit atomicMax where the key as the lane reads it is still lower (tl_chm_max's trick: keys only grow, a stale
//   read costs an atomic and never a pixel).  A row whose footprint misses its viewport stops before it reads its attribute.
// tl_raster_keys:  one thread per output pixel of a zoomed grid: the cell's value is the depth, its colour comes from a 256-entry ramp.
// tl_render_shade: one thread per pixel: decodes the key, reads the 8 neighbours at distance r, writes rgb u8 and optionally the depth.
// Every formula is f64 in plain operators under the pragma below (no contraction into fma), no transcendental function is called, and
// the only atomics are integer maxima: every output has the same bits for any row order.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kMaxSide = 16384;
constexpr int kMaxViews = 1 << 20;
constexpr int kViewLen = 18;
constexpr double kDblMax = 1.7976931348623157e308;
constexpr float kFltMax = 3.4028234663852886e38f;

// order-preserving u32 image of a float: a < b  <=>  enc(a) < enc(b); no finite value (nor an infinity) maps to 0, the empty pixel
__device__ __forceinline__ uint32_t enc32(float z) {
  const uint32_t b = __float_as_uint(z);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// index into a 256-entry ramp: floor((v - lo) / (hi - lo) * 255 + 0.5) clamped to 0 .. 255 (v is not NaN)
__device__ __forceinline__ int ramp_index(double v, double lo, double hi) {
  const double t = floor((v - lo) / (hi - lo) * 255.0 + 0.5);
  if (!(t >= 0.0)) return 0;
  return t > 255.0 ? 255 : (int)t;
}

// MODE 0: one colour; 1: labels i64 through a palette; 2: values A = float or double through a ramp; 3: rgb u8[n, 3]
template <typename T, int MODE, typename A>
__global__ void __launch_bounds__(kBlock) k_splat(const T* __restrict__ pts, int64_t ld, int64_t n, const int32_t* __restrict__ vid,
                                                  const double* __restrict__ views, int V, uint32_t rgb0, const A* __restrict__ attr,
                                                  const uint32_t* __restrict__ lut, int P, double lo, double hi, uint32_t nan_rgb, int k,
                                                  unsigned long long* __restrict__ keys, int W, int H, int32_t* __restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    int view = 0;
    if (vid) {
      view = vid[i];
      if (view < 0) continue;
      if (view >= V) { flags[0] = 1; continue; }
    }
    const double* __restrict__ m = views + (int64_t)view * kViewLen;
    const double x = (double)pts[i * ld], y = (double)pts[i * ld + 1], z = (double)pts[i * ld + 2];
    if (!(fabs(x) <= kDblMax) || !(fabs(y) <= kDblMax) || !(fabs(z) <= kDblMax)) { flags[0] = 1; continue; }
    const double qx = x - m[9], qy = y - m[10], qz = z - m[11];
    const double d = (m[6] * qx + m[7] * qy) + m[8] * qz;
    const float df = (float)(d + 0.0);                               // round to nearest even; -0.0 -> 0.0
    if (!(fabsf(df) <= kFltMax)) { flags[0] = 1; continue; }
    const double a = (m[0] * qx + m[1] * qy) + m[2] * qz;
    const double b = (m[3] * qx + m[4] * qy) + m[5] * qz;
    const double s = m[12], x0 = m[13], y0 = m[14], vw = m[15], vh = m[16];
    const double px = floor(a * s + (x0 + vw / 2.0));
    const double py = floor((y0 + vh / 2.0) - b * s);
    const double kl = (double)((k - 1) / 2), kh = (double)(k / 2);
    // the footprint px - kl .. px + kh against the viewport x0 .. x0 + vw - 1 and the canvas (a NaN fails every comparison)
    double xa = px - kl, xb = px + kh, ya = py - kl, yb = py + kh;
    const double vx1 = x0 + vw - 1.0, vy1 = y0 + vh - 1.0;
    if (!(xb >= x0) || !(xa <= vx1) || !(yb >= y0) || !(ya <= vy1)) continue;
    if (xa < x0) xa = x0;
    if (xb > vx1) xb = vx1;
    if (ya < y0) ya = y0;
    if (yb > vy1) yb = vy1;
    if (xa < 0.0) xa = 0.0;                                          // (a viewport lies inside the canvas; no store leaves it either way)
    if (ya < 0.0) ya = 0.0;
    if (xb > (double)(W - 1)) xb = (double)(W - 1);
    if (yb > (double)(H - 1)) yb = (double)(H - 1);
    if (!(xa <= xb) || !(ya <= yb)) continue;
    uint32_t rgb;
    if constexpr (MODE == 0) {
      rgb = rgb0;
    } else if constexpr (MODE == 1) {
      const int64_t l = attr[i];
      rgb = lut[l < 0 ? 0 : l == 0 ? 1 : 2 + (int)((l - 1) % (int64_t)(P - 2))];
    } else if constexpr (MODE == 2) {
      const double v = (double)attr[i];
      rgb = v != v ? nan_rgb : lut[ramp_index(v, lo, hi)];
    } else {
      rgb = (uint32_t)attr[i * 3] << 16 | (uint32_t)attr[i * 3 + 1] << 8 | (uint32_t)attr[i * 3 + 2];
    }
    const unsigned long long key = (unsigned long long)enc32(df) << 32 | (unsigned long long)(rgb & 0xFFFFFFu);
    const int ix0 = (int)xa, ix1 = (int)xb, iy0 = (int)ya, iy1 = (int)yb;
    for (int yy = iy0; yy <= iy1; ++yy)
      for (int xx = ix0; xx <= ix1; ++xx) {
        unsigned long long* p = keys + (int64_t)yy * W + xx;
#ifdef TL_RENDER_COUNT
        atomicAdd(flags + 2, 1);                                     // the counting build of tools/dev_render.py: pixels visited,
        if (*p < key) { atomicAdd(flags + 1, 1); atomicMax(p, key); }  // atomics issued
#else
        if (*p < key) atomicMax(p, key);
#endif
      }
  }
}

__global__ void __launch_bounds__(kBlock) k_raster_keys(const double* __restrict__ grid, int nx, int ny, int zoom, int x0, int y0,
                                                        const uint32_t* __restrict__ lut, double lo, double hi,
                                                        unsigned long long* __restrict__ keys, int W) {
  const int64_t ow = (int64_t)nx * zoom, total = ow * ny * zoom;
  for (int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x; id < total; id += (int64_t)gridDim.x * kBlock) {
    const int py = (int)(id / ow), px = (int)(id - (int64_t)py * ow);
    const double v = grid[(int64_t)(ny - 1 - py / zoom) * nx + px / zoom];
    unsigned long long key = 0ull;
    if (v == v) key = (unsigned long long)enc32((float)(v + 0.0)) << 32 | (unsigned long long)(lut[ramp_index(v, lo, hi)] & 0xFFFFFFu);
    keys[(int64_t)(y0 + py) * W + (x0 + px)] = key;
  }
}

__device__ __forceinline__ uint8_t shade_channel(uint32_t ch, double shade) {
  const double t = floor((double)ch * shade + 0.5);
  if (!(t >= 0.0)) return 0;
  return t > 255.0 ? 255 : (uint8_t)t;
}

__global__ void __launch_bounds__(kBlock) k_render_shade(const unsigned long long* __restrict__ keys, int W, int H, int r, double strength,
                                                         uint32_t background, uint8_t* __restrict__ out, float* __restrict__ depth) {
  const int64_t total = (int64_t)W * H;
  for (int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x; id < total; id += (int64_t)gridDim.x * kBlock) {
    const int y = (int)(id / W), x = (int)(id - (int64_t)y * W);
    const unsigned long long kc = keys[id];
    uint32_t rgb = background;
    double shade = 1.0;
    float df = __builtin_nanf("");
    if (kc != 0ull) {
      rgb = (uint32_t)kc & 0xFFFFFFu;
      df = dec32((uint32_t)(kc >> 32));
      const double dc = (double)df;
      double o = 0.0;
      for (int dy = -r; dy <= r; dy += r)
        for (int dx = -r; dx <= r; dx += r) {
          const int yy = y + dy, xx = x + dx;
          double c = 0.0;
          if ((dy != 0 || dx != 0) && yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const unsigned long long kn = keys[(int64_t)yy * W + xx];
            if (kn != 0ull) {
              const double diff = (double)dec32((uint32_t)(kn >> 32)) - dc;
              if (diff > 0.0) c = diff;                              // (a NaN, from two infinities, counts as 0)
            }
          }
          o = o + c;
        }
      o = o / 8.0;
      shade = 1.0 / (1.0 + strength * o);
    }
    out[id * 3] = shade_channel(rgb >> 16 & 0xFFu, shade);
    out[id * 3 + 1] = shade_channel(rgb >> 8 & 0xFFu, shade);
    out[id * 3 + 2] = shade_channel(rgb & 0xFFu, shade);
    if (depth) depth[id] = df;
  }
}

bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }
bool is_finite(double v) { return v >= -kDblMax && v <= kDblMax; }
bool canvas_ok(const void* keys, int W, int H) { return keys && aligned(keys, 8) && W >= 1 && H >= 1 && W <= kMaxSide && H <= kMaxSide; }

template <typename T, int MODE, typename A>
void launch_splat(const void* pts, int64_t ld, int64_t n, const int32_t* vid, const double* views, int V, uint32_t rgb, const void* attr,
                  const uint32_t* lut, int P, double lo, double hi, uint32_t nan_rgb, int k, uint64_t* keys, int W, int H, int32_t* flags,
                  hipStream_t s) {
  k_splat<T, MODE, A><<<tl_grid(n, kBlock), kBlock, 0, s>>>(static_cast<const T*>(pts), ld, n, vid, views, V, rgb, static_cast<const A*>(attr), lut, P,
                                                           lo, hi, nan_rgb, k, reinterpret_cast<unsigned long long*>(keys), W, H, flags);
}

template <typename T>
void splat_of_mode(int mode, int attr_f64, const void* pts, int64_t ld, int64_t n, const int32_t* vid, const double* views, int V, uint32_t rgb,
                   const void* attr, const uint32_t* lut, int P, double lo, double hi, uint32_t nan_rgb, int k, uint64_t* keys, int W, int H,
                   int32_t* flags, hipStream_t s) {
  if (mode == 0) launch_splat<T, 0, uint8_t>(pts, ld, n, vid, views, V, rgb, attr, lut, P, lo, hi, nan_rgb, k, keys, W, H, flags, s);
  else if (mode == 1) launch_splat<T, 1, int64_t>(pts, ld, n, vid, views, V, rgb, attr, lut, P, lo, hi, nan_rgb, k, keys, W, H, flags, s);
  else if (mode == 2 && attr_f64) launch_splat<T, 2, double>(pts, ld, n, vid, views, V, rgb, attr, lut, P, lo, hi, nan_rgb, k, keys, W, H, flags, s);
  else if (mode == 2) launch_splat<T, 2, float>(pts, ld, n, vid, views, V, rgb, attr, lut, P, lo, hi, nan_rgb, k, keys, W, H, flags, s);
  else launch_splat<T, 3, uint8_t>(pts, ld, n, vid, views, V, rgb, attr, lut, P, lo, hi, nan_rgb, k, keys, W, H, flags, s);
}
}  // namespace

extern "C" int tl_splat(const void* pts, int dtype_f64, int64_t ld, int64_t n, const int32_t* vid, const double* views, int n_views, int mode,
                        uint32_t rgb, const void* attr, int attr_f64, const uint32_t* lut, int n_lut, double lo, double hi, uint32_t nan_rgb,
                        int size, uint64_t* keys, int width, int height, int32_t* flags, tl_stream_t stream) {
  if (!pts || !views || !flags || !canvas_ok(keys, width, height) || n < 0 || ld < 3) return TL_ERR_ARG;
  if ((dtype_f64 != 0 && dtype_f64 != 1) || (attr_f64 != 0 && attr_f64 != 1) || n_views < 1 || n_views > kMaxViews) return TL_ERR_ARG;
  if (mode < 0 || mode > 3 || size < 1 || size > 9 || rgb > 0xFFFFFFu || nan_rgb > 0xFFFFFFu) return TL_ERR_ARG;
  if (!aligned(pts, dtype_f64 ? 8 : 4) || !aligned(views, 8) || !aligned(flags, 4) || (vid && !aligned(vid, 4))) return TL_ERR_ARG;
  if (mode != 0 && !attr) return TL_ERR_ARG;
  if (mode == 1 && (!lut || !aligned(lut, 4) || !aligned(attr, 8) || n_lut < 3)) return TL_ERR_ARG;
  if (mode == 2 && (!lut || !aligned(lut, 4) || !aligned(attr, attr_f64 ? 8 : 4) || n_lut != 256 || !is_finite(lo) || !is_finite(hi) || !(lo < hi)))
    return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  hipStream_t s = tl_s(stream);
  if (dtype_f64)
    splat_of_mode<double>(mode, attr_f64, pts, ld, n, vid, views, n_views, rgb, attr, lut, n_lut, lo, hi, nan_rgb, size, keys, width, height, flags, s);
  else
    splat_of_mode<float>(mode, attr_f64, pts, ld, n, vid, views, n_views, rgb, attr, lut, n_lut, lo, hi, nan_rgb, size, keys, width, height, flags, s);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_raster_keys(const double* grid, int nx, int ny, int zoom, int x0, int y0, const uint32_t* lut, double lo, double hi,
                              uint64_t* keys, int width, int height, tl_stream_t stream) {
  if (!grid || !lut || !canvas_ok(keys, width, height) || !aligned(grid, 8) || !aligned(lut, 4)) return TL_ERR_ARG;
  if (nx < 0 || ny < 0 || nx > kMaxSide || ny > kMaxSide || zoom < 1 || zoom > kMaxSide || x0 < 0 || y0 < 0) return TL_ERR_ARG;
  if (!is_finite(lo) || !is_finite(hi) || !(lo < hi)) return TL_ERR_ARG;
  if ((int64_t)x0 + (int64_t)nx * zoom > width || (int64_t)y0 + (int64_t)ny * zoom > height) return TL_ERR_ARG;
  const int64_t total = (int64_t)nx * zoom * ny * zoom;
  if (total == 0) return TL_OK;
  k_raster_keys<<<tl_grid(total, kBlock), kBlock, 0, tl_s(stream)>>>(grid, nx, ny, zoom, x0, y0, lut, lo, hi,
                                                                    reinterpret_cast<unsigned long long*>(keys), width);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_render_shade(const uint64_t* keys, int width, int height, int radius, double strength, uint32_t background, uint8_t* out,
                               float* depth, tl_stream_t stream) {
  if (!out || !canvas_ok(keys, width, height) || radius < 1 || radius > 16 || !(strength >= 0.0) || !is_finite(strength)) return TL_ERR_ARG;
  if (background > 0xFFFFFFu || (depth && !aligned(depth, 4))) return TL_ERR_ARG;
  if (static_cast<const void*>(out) == static_cast<const void*>(keys) || static_cast<const void*>(depth) == static_cast<const void*>(keys) ||
      static_cast<const void*>(depth) == static_cast<const void*>(out))
    return TL_ERR_ARG;
  k_render_shade<<<tl_grid((int64_t)width * height, kBlock), kBlock, 0, tl_s(stream)>>>(reinterpret_cast<const unsigned long long*>(keys), width, height,
                                                                                       radius, strength, background, out, depth);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
