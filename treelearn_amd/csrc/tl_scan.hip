// The shared passes of the stream compactions (tl_scan.h) and the stable row compaction built from them.
// Latency-bound integer work on a few KB of partials; the HBM traffic is in the callers' partials and scatter kernels.
#include "tl_scan.h"

namespace {

__global__ void __launch_bounds__(256) k_scan_parts(int32_t* __restrict__ part, int64_t nb, int groups, int32_t* __restrict__ totals32,
                                                    int64_t* __restrict__ totals64) {
  uint32_t carry = 0;
  for (int g = 0; g < groups; ++g) {
    const uint32_t start = carry;
    for (int64_t b0 = 0; b0 < nb; b0 += 256) {
      const int64_t i = b0 + threadIdx.x;
      const uint32_t v = i < nb ? (uint32_t)part[g * nb + i] : 0u;
      uint32_t tot; const uint32_t ex = tl_block_scan<4>(v, &tot);
      if (i < nb) part[g * nb + i] = (int32_t)(carry + ex);
      carry += tot;
    }
    if (threadIdx.x == 0) {
      if (totals32) totals32[g] = (int32_t)(carry - start);
      if (totals64) totals64[g] = (int64_t)(carry - start);
    }
  }
}

// ---------------------------------------------------------------- exclusive scan of int32[n] (3 passes)
__global__ void __launch_bounds__(256) k_i32_partials(const int32_t* __restrict__ f, int64_t n, int32_t* __restrict__ part) {
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int s = 0;
  for (int j = 0; j < kScanItems; ++j) if (base + j < n) s += f[base + j];
  int tot; tl_block_scan<4>(s, &tot);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// in and out may be the same array: a thread reads its own eight items before it writes them
__global__ void __launch_bounds__(256) k_i32_final(const int32_t* in, int64_t n, const int32_t* __restrict__ part, int32_t* out) {
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  int c[kScanItems]; int s = 0;
  for (int j = 0; j < kScanItems; ++j) { c[j] = (base + j < n) ? in[base + j] : 0; s += c[j]; }
  int tot; int ex = tl_block_scan<4>(s, &tot) + part[blockIdx.x];
  for (int j = 0; j < kScanItems; ++j) { if (base + j < n) out[base + j] = ex; ex += c[j]; }
}

// ---------------------------------------------------------------- stable row compaction
__global__ void __launch_bounds__(256) k_mask_partials(const uint8_t* __restrict__ m, int64_t n, int32_t* __restrict__ part) {
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t s = 0;
  for (int j = 0; j < kScanItems; ++j) if (base + j < n) s += m[base + j] != 0;
  uint32_t tot; tl_block_scan<4>(s, &tot);
  if (threadIdx.x == 0) part[blockIdx.x] = (int32_t)tot;
}
__global__ void __launch_bounds__(256) k_mask_scatter(const float* __restrict__ in, int C, const uint8_t* __restrict__ m, int64_t n,
                                                      const int32_t* __restrict__ part, float* __restrict__ out) {
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t s = 0; bool keep[kScanItems];
  for (int j = 0; j < kScanItems; ++j) { keep[j] = (base + j < n) && m[base + j] != 0; s += keep[j]; }
  uint32_t tot; uint32_t pos = tl_block_scan<4>(s, &tot) + (uint32_t)part[blockIdx.x];
  for (int j = 0; j < kScanItems; ++j) if (keep[j]) { for (int c = 0; c < C; ++c) out[(int64_t)pos * C + c] = in[(base + j) * C + c]; ++pos; }
}

}  // namespace

void tl_launch_scan_parts(int32_t* part, int64_t nb, int groups, int32_t* totals32, int64_t* totals64, hipStream_t s) {
  k_scan_parts<<<1, 256, 0, s>>>(part, nb, groups, totals32, totals64);
}

void tl_launch_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* total, int32_t* part, hipStream_t s) {
  const int64_t nb = tl_cdiv(n, kScanTile);
  k_i32_partials<<<(unsigned)nb, 256, 0, s>>>(in, n, part);
  tl_launch_scan_parts(part, nb, 1, total, nullptr, s);
  k_i32_final<<<(unsigned)nb, 256, 0, s>>>(in, n, part, out);
}

extern "C" {

int64_t tl_compact_ws_words(int64_t n) { return tl_scan_parts_words(n); }

int tl_compact_rows(const float* in, int C, const uint8_t* mask, int64_t n, float* out, int32_t* count, int32_t* ws, tl_stream_t stream) {
  if (!in || !mask || !out || !count || !ws || C <= 0 || n <= 0) return TL_ERR_ARG;
  const int64_t nb = tl_cdiv(n, kScanTile);
  hipStream_t s = tl_s(stream);
  k_mask_partials<<<(unsigned)nb, 256, 0, s>>>(mask, n, ws);
  tl_launch_scan_parts(ws, nb, 1, count, nullptr, s);
  k_mask_scatter<<<(unsigned)nb, 256, 0, s>>>(in, C, mask, n, ws, out);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

}  // extern "C"
