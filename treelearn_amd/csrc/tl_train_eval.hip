// Validation metrics of a training run (reference tools/training/train.py:89-102 `pointwise_eval`, fed by `validate` :61-86).
// tl_pointwise_eval: one read of logits / offsets / labels / mask per row gives the confusion counts of the tree / non-tree decision
//   (softmax(logits)[0] >= 0.5 against semantic_labels == 0, fp32) and the sum of the fp32 offset errors |offset - label| over the tree rows,
//   ADDED to a 64-byte state that lives through a validation pass; nothing per point is kept.
// Two stages, no float atomics, so the state is bit-reproducible: every workgroup reduces its rows (registers -> wave shuffles -> LDS) to one
// partial in `ws`; a second launch sums the partials in index order and updates the state.
#include "tl_common.h"

namespace {
constexpr int kBlock = 1024;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxBlocks = 256;              // one 16-wave workgroup per CU: ~110 B per lane in flight x 16 waves keeps HBM busy, and the last stage
                                             // has at most 256 partials to sum one after another (1024 partials of 4 waves: 25 us against 16 us here)
constexpr int kFinishBlock = 256;
constexpr int kRowsPerThread = 4;            // a "quad": 4 rows = 32 B of f32 logits, 48 B of f32 offsets, 32 B of labels, 4 mask bytes
constexpr int kPartWords = 8;                // tp fp tn fn n_off (i64), sum_off (f64), 2 unused: 64 B per workgroup

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct Acc {
  uint32_t tp = 0, fp = 0, tn = 0, fn = 0, n_off = 0;
  double sum = 0.0;
};

template <int DT> __device__ __forceinline__ float widen(uint16_t h);
template <> __device__ __forceinline__ float widen<TL_BF16>(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
template <> __device__ __forceinline__ float widen<TL_F16>(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

// One row: l0, l1 logits, o[3] offsets, t[3] offset labels (all fp32 by now), label, mask byte.
__device__ __forceinline__ void row(Acc& a, float l0, float l1, const float* o, const float* t, int64_t label, uint32_t m) {
  if (!m) return;
  // torch softmax in fp32: exp(x - max) / sum; NaN logits compare false (predicted non-tree), as in the reference
  const float mx = fmaxf(l0, l1);
  const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
  const bool pred = e0 / (e0 + e1) >= 0.5f;
  const bool tree = label == 0;
  a.tp += pred && tree;
  a.fp += pred && !tree;
  a.tn += !pred && !tree;
  a.fn += !pred && tree;
  if (tree) {
    const float dx = o[0] - t[0], dy = o[1] - t[1], dz = o[2] - t[2];
    a.sum += (double)sqrtf(dx * dx + dy * dy + dz * dz);
    a.n_off += 1;
  }
}

template <int DT>
__device__ __forceinline__ void row_scalar(Acc& a, const void* logits, const void* offsets, const int64_t* __restrict__ sem,
                                           const float* __restrict__ lab, const uint8_t* __restrict__ mask, int64_t i) {
  float l0, l1, o[3];
  if (DT == TL_F32) {
    const float* L = static_cast<const float*>(logits); const float* O = static_cast<const float*>(offsets);
    l0 = L[2 * i]; l1 = L[2 * i + 1]; o[0] = O[3 * i]; o[1] = O[3 * i + 1]; o[2] = O[3 * i + 2];
  } else {
    constexpr int H = DT == TL_F32 ? TL_BF16 : DT;
    const uint16_t* L = static_cast<const uint16_t*>(logits); const uint16_t* O = static_cast<const uint16_t*>(offsets);
    l0 = widen<H>(L[2 * i]); l1 = widen<H>(L[2 * i + 1]);
    o[0] = widen<H>(O[3 * i]); o[1] = widen<H>(O[3 * i + 1]); o[2] = widen<H>(O[3 * i + 2]);
  }
  const float t[3] = {lab[3 * i], lab[3 * i + 1], lab[3 * i + 2]};
  row(a, l0, l1, o, t, sem[i], mask ? mask[i] : 1u);
}

// VEC: every array is 16-byte aligned (mask: 4-byte), each thread takes 4 consecutive rows per trip with 16-byte loads; rows past the last
// whole quad, and every row of the unaligned form, go through row_scalar.
template <int DT, bool VEC>
__global__ void __launch_bounds__(kBlock) k_pointwise_eval(const void* __restrict__ logits, const void* __restrict__ offsets,
                                                           const int64_t* __restrict__ sem, const float* __restrict__ lab,
                                                           const uint8_t* __restrict__ mask, int64_t n, uint64_t* __restrict__ ws) {
  Acc a;
  const int64_t tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  if (VEC) {
    const int64_t nquad = n / kRowsPerThread;
    for (int64_t q = tid; q < nquad; q += nthreads) {
      float l[8], o[12], t[12];
      int64_t s[4];
      if (DT == TL_F32) {
        const u32x4* L = static_cast<const u32x4*>(logits) + 2 * q;
        const u32x4* O = static_cast<const u32x4*>(offsets) + 3 * q;
#pragma unroll
        for (int k = 0; k < 2; ++k) { const u32x4 v = L[k]; for (int j = 0; j < 4; ++j) l[4 * k + j] = __uint_as_float(v[j]); }
#pragma unroll
        for (int k = 0; k < 3; ++k) { const u32x4 v = O[k]; for (int j = 0; j < 4; ++j) o[4 * k + j] = __uint_as_float(v[j]); }
      } else {
        constexpr int H = DT == TL_F32 ? TL_BF16 : DT;
        const u32x4 lv = static_cast<const u32x4*>(logits)[q];                                 // 8 halves
        const u32x2* O = reinterpret_cast<const u32x2*>(static_cast<const uint16_t*>(offsets) + 12 * q);   // 12 halves = 3 x 8 bytes
#pragma unroll
        for (int j = 0; j < 4; ++j) { l[2 * j] = widen<H>((uint16_t)(lv[j] & 0xFFFFu)); l[2 * j + 1] = widen<H>((uint16_t)(lv[j] >> 16)); }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const u32x2 v = O[k];
#pragma unroll
          for (int j = 0; j < 2; ++j) { o[4 * k + 2 * j] = widen<H>((uint16_t)(v[j] & 0xFFFFu)); o[4 * k + 2 * j + 1] = widen<H>((uint16_t)(v[j] >> 16)); }
        }
      }
      const u32x4* T = reinterpret_cast<const u32x4*>(lab) + 3 * q;
#pragma unroll
      for (int k = 0; k < 3; ++k) { const u32x4 v = T[k]; for (int j = 0; j < 4; ++j) t[4 * k + j] = __uint_as_float(v[j]); }
      const u32x4* S = reinterpret_cast<const u32x4*>(sem) + 2 * q;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const u32x4 v = S[k];
        s[2 * k] = (int64_t)(((uint64_t)v[1] << 32) | v[0]); s[2 * k + 1] = (int64_t)(((uint64_t)v[3] << 32) | v[2]);
      }
      const uint32_t m4 = mask ? reinterpret_cast<const uint32_t*>(mask)[q] : 0x01010101u;
#pragma unroll
      for (int r = 0; r < 4; ++r) row(a, l[2 * r], l[2 * r + 1], o + 3 * r, t + 3 * r, s[r], (m4 >> (8 * r)) & 0xFFu);
    }
    const int64_t tail = nquad * kRowsPerThread + tid;                 // the n % 4 rows after the last quad
    if (tail < n) row_scalar<DT>(a, logits, offsets, sem, lab, mask, tail);
  } else {
    for (int64_t i = tid; i < n; i += nthreads) row_scalar<DT>(a, logits, offsets, sem, lab, mask, i);
  }

  // registers -> wave (xor shuffles: every lane ends with the wave's total) -> LDS -> one partial per workgroup
  uint64_t c[5] = {a.tp, a.fp, a.tn, a.fn, a.n_off};
  double sum = a.sum;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) c[k] += (uint64_t)__shfl_xor((unsigned long long)c[k], off);
    sum += __shfl_xor(sum, off);
  }
  __shared__ uint64_t s_c[kWaves][5];
  __shared__ double s_sum[kWaves];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) s_c[wave][k] = c[k];
    s_sum[wave] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t* p = ws + (int64_t)blockIdx.x * kPartWords;
    double total = s_sum[0];
    for (int w = 1; w < kWaves; ++w) total += s_sum[w];                // wave order
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      uint64_t v = 0;
      for (int w = 0; w < kWaves; ++w) v += s_c[w][k];
      p[k] = v;
    }
    p[5] = __builtin_bit_cast(uint64_t, total);
    p[6] = 0; p[7] = 0;
  }
}

// Last stage, one workgroup: the partials go to LDS (one row per field, rows past nparts zero), then lanes 0..4 sum the counts and lane 5
// the float64 sums, each in index order over a fixed trip count (unrolled: the LDS reads run ahead of the add chain); state += totals.
__global__ void __launch_bounds__(kFinishBlock) k_pointwise_eval_finish(const uint64_t* __restrict__ ws, int nparts, uint64_t* __restrict__ state) {
  static_assert(kFinishBlock == kMaxBlocks, "one lane stages one partial");
  __shared__ uint64_t s_p[6][kMaxBlocks + 2];                          // + 2: the six rows start in different banks
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 6; ++k) s_p[k][t] = t < nparts ? ws[(int64_t)t * kPartWords + k] : 0;       // 0 is also +0.0
  __syncthreads();
  if (t < 5) {
    uint64_t v = 0;
#pragma unroll 8
    for (int b = 0; b < kMaxBlocks; ++b) v += s_p[t][b];
    state[t] = (uint64_t)((int64_t)state[t] + (int64_t)v);
  } else if (t == 5) {
    double v = 0.0;
#pragma unroll 8
    for (int b = 0; b < kMaxBlocks; ++b) v += __builtin_bit_cast(double, s_p[5][b]);
    state[5] = __builtin_bit_cast(uint64_t, __builtin_bit_cast(double, state[5]) + v);
  }
}

unsigned eval_grid(int64_t n) {
  int64_t g = tl_cdiv(tl_cdiv(n, kRowsPerThread), kBlock);
  if (g < 1) g = 1;
  if (g > kMaxBlocks) g = kMaxBlocks;
  return (unsigned)g;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <int DT>
void launch(bool vec, unsigned grid, hipStream_t s, const void* logits, const void* offsets, const int64_t* sem, const float* lab,
            const uint8_t* mask, int64_t n, uint64_t* ws) {
  if (vec) k_pointwise_eval<DT, true><<<grid, kBlock, 0, s>>>(logits, offsets, sem, lab, mask, n, ws);
  else k_pointwise_eval<DT, false><<<grid, kBlock, 0, s>>>(logits, offsets, sem, lab, mask, n, ws);
}
}  // namespace

extern "C" int64_t tl_pointwise_eval_ws_bytes(int64_t n) {
  return (int64_t)eval_grid(n < 0 ? 0 : n) * kPartWords * (int64_t)sizeof(uint64_t);
}

extern "C" int tl_pointwise_eval(const void* logits, const void* offsets, int dtype, const int64_t* semantic_labels, const float* offset_labels,
                                 const uint8_t* mask, int64_t n, void* state, void* ws, tl_stream_t stream) {
  if (!logits || !offsets || !semantic_labels || !offset_labels || !state || !ws || n < 0 || n >= ((int64_t)1 << 40)) return TL_ERR_ARG;
  if (dtype != TL_F32 && dtype != TL_BF16 && dtype != TL_F16) return TL_ERR_ARG;
  if (!aligned(state, 8) || !aligned(ws, 8) || !aligned(semantic_labels, 8) || !aligned(offset_labels, 4) ||
      !aligned(logits, dtype == TL_F32 ? 4 : 2) || !aligned(offsets, dtype == TL_F32 ? 4 : 2))
    return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  const bool vec = aligned(logits, 16) && aligned(offsets, dtype == TL_F32 ? 16 : 8) && aligned(semantic_labels, 16) && aligned(offset_labels, 16) &&
                   (!mask || aligned(mask, 4));
  const unsigned grid = eval_grid(n);
  hipStream_t s = tl_s(stream);
  uint64_t* w = static_cast<uint64_t*>(ws);
  if (dtype == TL_F32) launch<TL_F32>(vec, grid, s, logits, offsets, semantic_labels, offset_labels, mask, n, w);
  else if (dtype == TL_BF16) launch<TL_BF16>(vec, grid, s, logits, offsets, semantic_labels, offset_labels, mask, n, w);
  else launch<TL_F16>(vec, grid, s, logits, offsets, semantic_labels, offset_labels, mask, n, w);
  TL_CHECK_LAUNCH();
  k_pointwise_eval_finish<<<1, kFinishBlock, 0, s>>>(w, (int)grid, static_cast<uint64_t*>(state));
  TL_CHECK_LAUNCH();
  return TL_OK;
}
