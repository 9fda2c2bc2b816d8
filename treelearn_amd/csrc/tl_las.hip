// LAS point records on the device (the ASPRS layout and this project's reading / writing rules are restated in numpy in
// tests/las_restatement.py).
// tl_las_decode: raw records of any point format -> f64 rows x y z [label].  x = X * scale + offset, a multiply and then an add (the
//   pragma below keeps the compiler from contracting them); the label rule of the reference's load_data on the treeID extra dimension
//   and the classification.
// tl_las_encode: coordinates + labels (optionally gathered through `order`) -> the writer's 38-byte records (point format 3 + u32
//   treeID), X = rint((x - offset) / scale), and the extreme integers per segment with integer atomicMin / atomicMax (exact, the same
//   bits for any row order).  A row whose coordinate is not finite or whose quotient leaves i32 gets an all-zero record and sets *err.
// Records are only byte aligned (lengths are often odd), but 256 records always start on a multiple of 256 bytes.  Decoding has two paths:
//   plain:  one lane per record, byte loads of the fields it needs;
//   staged: a workgroup moves its tile of 256 records from HBM to LDS with 16-byte loads, and every lane takes its fields from LDS.  A
//           field at any byte offset is read as the two dwords that contain it, shifted: no unaligned LDS access.  Records longer than
//           kStagedMaxRec bytes only have the plain path.
// Measured on the 1.89 M-row tile: staged wins where the label is decoded (17+ bytes of a record are needed), plain where
// only x y z are (12 bytes): the library's choice follows that.  Encoding writes one lane per record with 16-bit stores (38 is even); a
// staged form of it (records assembled in LDS, written with 16-byte stores) was measured no faster and is not kept.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr int kStagedMaxRec = 128;            // 32 KB of LDS per workgroup at most
constexpr int kRec = 38;                      // the writer's record: point format 3 (34 bytes) + u32 treeID
constexpr int kEncodeBlocks = 1024;           // 4 per CU, each over a contiguous range of tiles
constexpr int kPathAuto = 0, kPathPlain = 1, kPathStaged = 2;

struct GlobalBytes {                          // a record in global memory, read byte by byte
  const uint8_t* p;
  __device__ __forceinline__ uint32_t u8(int off) const { return p[off]; }
  __device__ __forceinline__ uint32_t u16(int off) const { return (uint32_t)p[off] | ((uint32_t)p[off + 1] << 8); }
  __device__ __forceinline__ uint32_t u32(int off) const {
    return (uint32_t)p[off] | ((uint32_t)p[off + 1] << 8) | ((uint32_t)p[off + 2] << 16) | ((uint32_t)p[off + 3] << 24);
  }
};

struct LdsBytes {                             // a record inside the LDS tile: `base` is its byte offset from the dword array `w`
  const uint32_t* w;
  int base;
  __device__ __forceinline__ uint32_t u8(int off) const {
    const int a = base + off;
    return (w[a >> 2] >> ((a & 3) * 8)) & 0xffu;
  }
  __device__ __forceinline__ uint32_t u16(int off) const {
    const int a = base + off, sh = (a & 3) * 8;
    const uint32_t lo = w[a >> 2] >> sh;
    if (sh != 24) return lo & 0xffffu;                           // both bytes in one dword
    return (lo | (w[(a >> 2) + 1] << 8)) & 0xffffu;
  }
  __device__ __forceinline__ uint32_t u32(int off) const {
    const int a = base + off, sh = (a & 3) * 8;
    const uint32_t lo = w[a >> 2];
    if (sh == 0) return lo;
    const uint32_t hi = w[(a >> 2) + 1];
    return (lo >> sh) | (hi << (32 - sh));
  }
};

// the treeID extra dimension widened to f64, as numpy's assignment into a float64 array does (types 1 .. 10 of the extra-bytes VLR)
template <typename R>
__device__ __forceinline__ double read_tree_id(const R& r, int off, int type) {
  switch (type) {
    case 1: return (double)r.u8(off);
    case 2: return (double)(int8_t)r.u8(off);
    case 3: return (double)r.u16(off);                           // (never a byte at or beyond off + width: the field may end the buffer)
    case 4: return (double)(int16_t)r.u16(off);
    case 5: return (double)r.u32(off);
    case 6: return (double)(int32_t)r.u32(off);
    case 9: return (double)__uint_as_float(r.u32(off));
    default: break;
  }
  const uint64_t v = (uint64_t)r.u32(off) | ((uint64_t)r.u32(off + 4) << 32);
  if (type == 7) return (double)v;
  if (type == 8) return (double)(int64_t)v;
  return __longlong_as_double((long long)v);
}

struct DecodeParams {
  int rec_len, cls_off, cls_mask, tid_off, tid_type, cols;
  double scale[3], offset[3];
};

template <typename R>
__device__ __forceinline__ void decode_row(const R& r, const DecodeParams& P, double* __restrict__ out) {
  const int32_t X = (int32_t)r.u32(0), Y = (int32_t)r.u32(4), Z = (int32_t)r.u32(8);
  out[0] = (double)X * P.scale[0] + P.offset[0];
  out[1] = (double)Y * P.scale[1] + P.offset[1];
  out[2] = (double)Z * P.scale[2] + P.offset[2];
  if (P.cols == 4) {
    const double t = read_tree_id(r, P.tid_off, P.tid_type);
    const int cls = (int)(r.u8(P.cls_off) & (uint32_t)P.cls_mask);
    const bool tree = t != 0.0, non_tree = cls == 1 || cls == 2;
    out[3] = non_tree ? 0.0 : tree ? t : -1.0;                   // the non-tree classes are applied second, so they win
  }
}

__global__ void __launch_bounds__(kBlock) k_las_decode_plain(const uint8_t* __restrict__ rec, int64_t n, DecodeParams P, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    GlobalBytes r{rec + i * P.rec_len};
    decode_row(r, P, out + i * P.cols);
  }
}

__global__ void __launch_bounds__(kBlock) k_las_decode_staged(const uint8_t* __restrict__ rec, int64_t n, DecodeParams P, double* __restrict__ out) {
  extern __shared__ uint4 tile16[];                              // 256 * rec_len bytes rounded up to 16, + 16 (the second dword of a field)
  const int64_t tiles = (n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {      // block-uniform trip count: every lane reaches the barriers
    const int64_t row0 = t * kBlock;
    const int rows = (int)(n - row0 < kBlock ? n - row0 : kBlock);
    const int bytes = rows * P.rec_len;
    const uint8_t* src = rec + row0 * P.rec_len;                 // a multiple of 256 bytes from a base aligned to 16
    const int full = bytes >> 4;
    for (int c = threadIdx.x; c < full; c += kBlock) tile16[c] = reinterpret_cast<const uint4*>(src)[c];
    uint8_t* tile8 = reinterpret_cast<uint8_t*>(tile16);
    for (int b = (full << 4) + threadIdx.x; b < bytes; b += kBlock) tile8[b] = src[b];      // the last tile's tail: never read past the records
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      LdsBytes r{reinterpret_cast<const uint32_t*>(tile16), (int)threadIdx.x * P.rec_len};
      decode_row(r, P, out + (row0 + threadIdx.x) * P.cols);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- encode
struct EncodeParams {
  double scale[3], offset[3];
};

// the colour of a label: black for 0, else three bytes of an integer mix of its low 32 bits, each widened to 16 bits (b * 257)
__device__ __forceinline__ void label_rgb(int64_t label, uint32_t rgb[3]) {
  if (label == 0) { rgb[0] = rgb[1] = rgb[2] = 0; return; }
  uint32_t h = (uint32_t)(uint64_t)label * 2654435761u;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  rgb[0] = (h & 0xffu) * 257u;
  rgb[1] = ((h >> 8) & 0xffu) * 257u;
  rgb[2] = ((h >> 16) & 0xffu) * 257u;
}

// row j of the output: its 19 halfwords in h (all zero and false when the row cannot be written), its integers in q
template <typename T>
__device__ __forceinline__ bool encode_row(const T* __restrict__ pts, int64_t ld, int64_t n_src, const int64_t* __restrict__ labels,
                                           const int64_t* __restrict__ order, int64_t j, const EncodeParams& P, uint16_t h[19], int32_t q[3]) {
#pragma unroll
  for (int k = 0; k < 19; ++k) h[k] = 0;
  const int64_t s = order ? order[j] : j;
  if (s < 0 || s >= n_src) return false;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = ((double)pts[s * ld + a] - P.offset[a]) / P.scale[a];
    const double r = rint(v);                                    // round half to even
    ok = ok && r >= -2147483648.0 && r <= 2147483647.0;          // false for NaN
    q[a] = ok ? (int32_t)r : 0;
  }
  if (!ok) return false;
  const int64_t label = labels[s];
  uint32_t rgb[3];
  label_rgb(label, rgb);
  const uint32_t tid = (uint32_t)(uint64_t)label;
#pragma unroll
  for (int a = 0; a < 3; ++a) { h[2 * a] = (uint16_t)((uint32_t)q[a] & 0xffffu); h[2 * a + 1] = (uint16_t)((uint32_t)q[a] >> 16); }
  h[7] = (uint16_t)(0x09u | ((label == 0 ? 2u : 4u) << 8));      // byte 14: return 1 of 1; byte 15: classification
  h[14] = (uint16_t)rgb[0]; h[15] = (uint16_t)rgb[1]; h[16] = (uint16_t)rgb[2];             // bytes 12-13, 16-27 stay 0 (intensity .. GPS time)
  h[17] = (uint16_t)(tid & 0xffffu); h[18] = (uint16_t)(tid >> 16);
  return true;
}

// segment of output row j: the last s with start[s] <= j (start has n_seg + 1 ascending entries, start[n_seg] = n)
__device__ __forceinline__ int64_t segment_of(const int64_t* __restrict__ start, int64_t n_seg, int64_t j) {
  int64_t lo = 0, hi = n_seg;                                    // invariant: start[lo] <= j < start[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (start[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// ext[seg] = {min X, min Y, min Z, max X, max Y, max Z}.  Global atomics on one address serialise (measured: 11 ns each), so they are
// kept to a few per workgroup: a workgroup walks a contiguous range of tiles and holds the extremes of its current segment -- that of
// the tile's first row -- in LDS (s_ext); they go to the table when the segment changes and at the end.  The active lanes of a wave that
// share one segment (nearly always: segments are ranges of consecutive rows) first reduce with shuffles.  A row of another segment than
// the workgroup's current one (a tile across a boundary) goes to the table directly.
__device__ __forceinline__ void put_extremes(int64_t seg, int64_t seg_block, const int32_t lo[3], const int32_t hi[3], int32_t* s_ext,
                                             int32_t* __restrict__ ext) {
  if (seg == seg_block) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(s_ext + a, lo[a]); atomicMax(s_ext + 3 + a, hi[a]); }
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMin(ext + seg * 6 + a, lo[a]); atomicMax(ext + seg * 6 + 3 + a, hi[a]); }
  }
}

__device__ __forceinline__ void extremes(bool ok, int64_t seg, int64_t seg_block, const int32_t q[3], int32_t* s_ext, int32_t* __restrict__ ext) {
  const uint64_t act = __ballot(ok);
  if (!act) return;
  const int first = __ffsll((unsigned long long)act) - 1;
  const int64_t seg0 = __shfl(seg, first);
  int32_t lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { lo[a] = ok ? q[a] : 2147483647; hi[a] = ok ? q[a] : (-2147483647 - 1); }
  if (__all(!ok || seg == seg0)) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int32_t l2 = __shfl_xor(lo[a], o), h2 = __shfl_xor(hi[a], o);
        lo[a] = l2 < lo[a] ? l2 : lo[a];
        hi[a] = h2 > hi[a] ? h2 : hi[a];
      }
    if ((int)(threadIdx.x & 63) == first) put_extremes(seg0, seg_block, lo, hi, s_ext, ext);
  } else if (ok) {
    put_extremes(seg, seg_block, lo, hi, s_ext, ext);
  }
}

__device__ __forceinline__ int32_t ext_empty(int k) { return k < 3 ? 2147483647 : (-2147483647 - 1); }

__global__ void __launch_bounds__(kBlock) k_las_ext_init(int32_t* __restrict__ ext, int64_t n_seg) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_seg * 6; i += (int64_t)gridDim.x * kBlock) ext[i] = ext_empty((int)(i % 6));
}

template <typename T>
__global__ void __launch_bounds__(kBlock) k_las_encode(const T* __restrict__ pts, int64_t ld, int64_t n_src, const int64_t* __restrict__ labels,
                                                       const int64_t* __restrict__ order, int64_t n, EncodeParams P,
                                                       const int64_t* __restrict__ start, int64_t n_seg, uint8_t* __restrict__ rec,
                                                       int32_t* __restrict__ err, int32_t* __restrict__ ext) {
  __shared__ int32_t s_ext[6];
  const int64_t tiles = (n + kBlock - 1) / kBlock, per = (tiles + gridDim.x - 1) / gridDim.x;
  const int64_t t_begin = (int64_t)blockIdx.x * per, t_end = t_begin + per < tiles ? t_begin + per : tiles;
  if (threadIdx.x < 6) s_ext[threadIdx.x] = ext_empty(threadIdx.x);
  int64_t cur = -1;                                              // the segment s_ext belongs to (the same value in every thread)
  __syncthreads();
  for (int64_t t = t_begin; t < t_end; ++t) {                    // block-uniform trip count (barriers, wave shuffles)
    const int64_t row0 = t * kBlock, j = row0 + threadIdx.x;
    const int64_t seg_tile = start ? segment_of(start, n_seg, row0) : 0;
    const int64_t seg_end = start ? start[seg_tile + 1] : n;
    if (seg_tile != cur) {                                       // (every wave has passed the barrier that ends the previous tile)
      if (threadIdx.x < 6) {
        if (cur >= 0) { if (threadIdx.x < 3) atomicMin(ext + cur * 6 + threadIdx.x, s_ext[threadIdx.x]); else atomicMax(ext + cur * 6 + threadIdx.x, s_ext[threadIdx.x]); }
        s_ext[threadIdx.x] = ext_empty(threadIdx.x);
      }
      cur = seg_tile;
      __syncthreads();
    }
    uint16_t h[19];
    int32_t q[3] = {0, 0, 0};
    bool ok = false;
    if (j < n) {
      ok = encode_row(pts, ld, n_src, labels, order, j, P, h, q);
      if (!ok) *err = 1;
      uint16_t* d = reinterpret_cast<uint16_t*>(rec + j * kRec);          // rec is aligned to 16 and 38 is even
#pragma unroll
      for (int k = 0; k < 19; ++k) d[k] = h[k];
    }
    extremes(ok, !ok ? 0 : j < seg_end ? seg_tile : segment_of(start, n_seg, j), cur, q, s_ext, ext);
    __syncthreads();
  }
  if (cur >= 0 && threadIdx.x < 6) {
    if (threadIdx.x < 3) atomicMin(ext + cur * 6 + threadIdx.x, s_ext[threadIdx.x]); else atomicMax(ext + cur * 6 + threadIdx.x, s_ext[threadIdx.x]);
  }
}

bool aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(a - 1)) == 0; }
int type_width(int type) {
  static const int w[11] = {0, 1, 1, 2, 2, 4, 4, 8, 8, 4, 8};
  return type >= 1 && type <= 10 ? w[type] : 0;
}
bool finite3(const double* v) { return fabs(v[0]) <= 1.7976931348623157e308 && fabs(v[1]) <= 1.7976931348623157e308 && fabs(v[2]) <= 1.7976931348623157e308; }
}  // namespace

extern "C" int tl_las_decode(const uint8_t* records, int64_t n, int32_t record_length, int32_t class_offset, int32_t class_mask,
                             int32_t tree_id_offset, int32_t tree_id_type, const double scale[3], const double offset[3], double* out,
                             int32_t out_cols, int64_t first_row, int32_t path, tl_stream_t stream) {
  if (!records || !out || !scale || !offset || n < 0 || first_row < 0 || record_length < 20 || record_length > 65535) return TL_ERR_ARG;
  if (out_cols != 3 && out_cols != 4) return TL_ERR_ARG;
  if (path != kPathAuto && path != kPathPlain && path != kPathStaged) return TL_ERR_ARG;
  if (!aligned(records, 16) || !aligned(out, 8)) return TL_ERR_ARG;
  if (out_cols == 4) {
    const int w = type_width(tree_id_type);
    if (w == 0 || tree_id_offset < 12 || tree_id_offset + w > record_length) return TL_ERR_ARG;
    if (class_offset < 12 || class_offset >= record_length || class_mask < 1 || class_mask > 255) return TL_ERR_ARG;
  } else if (tree_id_type != 0) {
    return TL_ERR_ARG;
  }
  if (n > ((int64_t)1 << 40) || first_row > ((int64_t)1 << 40)) return TL_ERR_ARG;
  if (path == kPathStaged && record_length > kStagedMaxRec) return TL_ERR_UNSUPPORTED;
  if (n == 0) return TL_OK;
  DecodeParams P;
  P.rec_len = record_length; P.cls_off = class_offset; P.cls_mask = class_mask; P.tid_off = tree_id_offset; P.tid_type = tree_id_type;
  P.cols = out_cols;
  for (int a = 0; a < 3; ++a) { P.scale[a] = scale[a]; P.offset[a] = offset[a]; }
  double* o = out + first_row * out_cols;
  const bool staged = record_length <= kStagedMaxRec && (path == kPathStaged || (path == kPathAuto && out_cols == 4));
  if (staged) {
    const size_t lds = (((size_t)kBlock * record_length + 15) & ~(size_t)15) + 16;
    k_las_decode_staged<<<tl_grid(n, kBlock), kBlock, lds, tl_s(stream)>>>(records, n, P, o);
  } else {
    k_las_decode_plain<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(records, n, P, o);
  }
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int tl_las_encode(const void* coords, int dtype_f64, int64_t ld, int64_t n_src, const int64_t* labels, const int64_t* order,
                             int64_t n, const double scale[3], const double offset[3], const int64_t* seg_start, int64_t n_seg,
                             uint8_t* records, int32_t* err, int32_t* extremes_out, tl_stream_t stream) {
  if (!coords || !labels || !records || !err || !extremes_out || !scale || !offset) return TL_ERR_ARG;
  if (n < 0 || n_src < 0 || ld < 3 || (dtype_f64 != 0 && dtype_f64 != 1)) return TL_ERR_ARG;
  if (!order && n != n_src) return TL_ERR_ARG;
  if (seg_start ? n_seg < 1 : n_seg != 1) return TL_ERR_ARG;
  if (!finite3(scale) || !finite3(offset) || !(scale[0] > 0.0) || !(scale[1] > 0.0) || !(scale[2] > 0.0)) return TL_ERR_ARG;
  if (!aligned(coords, dtype_f64 ? 8 : 4) || !aligned(labels, 8) || !aligned(order, 8) || !aligned(seg_start, 8) || !aligned(records, 16) ||
      !aligned(err, 4) || !aligned(extremes_out, 4)) return TL_ERR_ARG;
  if (n > ((int64_t)1 << 40) || n_seg > ((int64_t)1 << 32)) return TL_ERR_ARG;
  hipStream_t s = tl_s(stream);
  if (hipMemsetAsync(err, 0, sizeof(int32_t), s) != hipSuccess) return TL_ERR_LAUNCH;
  k_las_ext_init<<<tl_grid(n_seg * 6, kBlock), kBlock, 0, s>>>(extremes_out, n_seg);
  TL_CHECK_LAUNCH();
  if (n == 0) return TL_OK;
  EncodeParams P;
  for (int a = 0; a < 3; ++a) { P.scale[a] = scale[a]; P.offset[a] = offset[a]; }
  const int64_t tiles = tl_cdiv(n, kBlock);
  const unsigned grid = (unsigned)(tiles < kEncodeBlocks ? tiles : kEncodeBlocks);
  if (dtype_f64)
    k_las_encode<double><<<grid, kBlock, 0, s>>>(static_cast<const double*>(coords), ld, n_src, labels, order, n, P, seg_start, n_seg, records, err,
                                                 extremes_out);
  else
    k_las_encode<float><<<grid, kBlock, 0, s>>>(static_cast<const float*>(coords), ld, n_src, labels, order, n, P, seg_start, n_seg, records, err,
                                                extremes_out);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
