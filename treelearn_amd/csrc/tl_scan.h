// The one copy of what every stream compaction here is made of: the workgroup exclusive scan, the tile constants, the
// one-workgroup pass over the per-tile partials (tl_scan.hip) and the lock-free union-find of the two clusterings.
//
// A compaction is three launches: the stage's own partials kernel (one count per tile of kScanTile items -> part[]),
// tl_launch_scan_parts (part[] -> exclusive offsets + total), the stage's own scatter kernel (tl_block_scan again + part[tile]).
#pragma once
#include "tl_common.h"

constexpr int kScanItems = 8;                       // items per thread
constexpr int kScanTile = 256 * kScanItems;         // items per 256-thread workgroup

// words of int32 workspace for the partials of n items (+ 1 spare)
static inline int64_t tl_scan_parts_words(int64_t n) { return tl_cdiv(n, kScanTile) + 1; }

// Exclusive scan of v over a workgroup of kWaves waves (T = int or uint32_t); *total = the workgroup's sum, in every thread.
// Ends on a barrier, so a kernel may call it again at once.
template <int kWaves, typename T>
__device__ __forceinline__ T tl_block_scan(T v, T* total) {
  __shared__ T wsum[kWaves];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  T inc = v;
  for (int off = 1; off < 64; off <<= 1) { const T t = (T)__shfl_up((int)inc, off); if (lane >= off) inc += t; }
  if (lane == 63) wsum[wid] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  for (int w = 0; w < kWaves; ++w) { if (w < wid) base += wsum[w]; tot += wsum[w]; }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// Lock-free union-find on parent[] (parent[i] == i at the start): the larger root is hooked under the smaller, so a
// component's root is its smallest index.  tl_unite returns false when a and b were already one component.
__device__ __forceinline__ int tl_find_root(int* parent, int x) {
  while (true) {
    const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ bool tl_unite(int* parent, int a, int b) {
  while (true) {
    a = tl_find_root(parent, a); b = tl_find_root(parent, b);
    if (a == b) return false;
    if (a < b) { const int t = a; a = b; b = t; }
    if (atomicCAS(&parent[a], a, b) == a) return true;
  }
}

// tl_scan.hip.  Both only enqueue: the caller's TL_CHECK_LAUNCH reports a failed launch.
//
// part[groups][nb] tile counts -> exclusive offsets, in place, by one workgroup.  The carry runs on from group to group (group g's
// rows follow group g-1's); group g's own sum goes to totals32[g] and / or totals64[g], whichever is not NULL.
void tl_launch_scan_parts(int32_t* part, int64_t nb, int groups, int32_t* totals32, int64_t* totals64, hipStream_t s);
// out[i] = in[0] + .. + in[i-1] for i < n, *total = the whole sum.  out may be in (in place); total may be out + n (int[n + 1]).
// part: tl_scan_parts_words(n) words.
void tl_launch_scan_i32(const int32_t* in, int64_t n, int32_t* out, int32_t* total, int32_t* part, hipStream_t s);
