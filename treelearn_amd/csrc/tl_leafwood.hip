// Leaf-wood separation of the trees of a labelled cloud (the semantics are restated in numpy in
// tests/leafwood_restatement.py): a seed rule on the eigen-features of tl_eigen_features, then a vote among the rows of the same tree
// over the same radius neighbourhoods.  The connectivity filter behind the vote is the caller's, on tl_skel_voxel_keys / tl_skel_nodes.
//
// tl_leafwood_seed: one thread per row, four f32 features in, one byte out.
// tl_leafwood_seed_scales: the same rule at each of S scales (the rows of tl_eigen_features_scales), counted against scales_min (§26).
// tl_leafwood_vote: the work split of k_eigen_features (tl_features.hip): points sorted by a (radius)-sized cell key with z fastest, one
// wave per PIECE (up to 64 consecutive points of one (x, y) column of cells inside one aligned 64-block), one point per lane.  Lanes
// 0..17 find the ends of the 9 candidate ranges by binary search, once per piece; the ranges are staged through LDS in chunks of kChunk
// candidates of 28 bytes (xyz f64 and the i32 tag = tree << 1 | flag): the coalesced loads of the next chunk are in flight while every
// lane walks the current one with broadcast LDS reads.  Each lane counts the candidates of its own tree within the radius (a) and those
// of them that are flagged (w) and stores one byte (and the next round's tag).  Counts only: the result does not depend on the order of
// the candidates, so neither on the row order nor on the piece table.  No atomics, no scratch, no global read per candidate.
#include "tl_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kBits = 21;
constexpr int64_t kMask = (1ll << kBits) - 1;
constexpr int kChunk = 128;                         // candidates per LDS chunk: 3.5 KiB, two buffers
constexpr int kLoads = kChunk * 3 / 64;             // f64 loads per lane and chunk
constexpr int kTagLoads = kChunk / 64;              // i32 loads per lane and chunk

__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

__global__ void __launch_bounds__(kBlock) k_leafwood_seed(const float* __restrict__ feats, int64_t n, tl_leafwood_params a,
                                                          uint8_t* __restrict__ flag) {
  const double inf = __builtin_inf();
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    const float4 f = reinterpret_cast<const float4*>(feats)[j];
    const double lin = (double)f.x, pla = (double)f.y, ver = (double)f.z, nn = (double)f.w;
    const bool finite = fabs(lin) < inf && fabs(pla) < inf && fabs(ver) < inf;                    // (NaN fails)
    const bool limb = lin >= a.linearity_min, patch = pla >= a.planarity_min && ver >= a.verticality_min;
    flag[j] = (nn >= (double)a.min_neighbours && finite && (limb || patch)) ? 1 : 0;
  }
}

// The seed rule at S scales: feats f32 [n, S, 4]; the rule above per scale, the flag is 1 when at least scales_min hold.
__global__ void __launch_bounds__(kBlock) k_leafwood_seed_scales(const float* __restrict__ feats, int64_t n, int S, tl_leafwood_params a,
                                                                 int scales_min, uint8_t* __restrict__ flag) {
  const double inf = __builtin_inf();
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (int64_t)gridDim.x * kBlock) {
    int hold = 0;
    for (int k = 0; k < S; ++k) {
      const float4 f = reinterpret_cast<const float4*>(feats)[j * S + k];
      const double lin = (double)f.x, pla = (double)f.y, ver = (double)f.z, nn = (double)f.w;
      const bool finite = fabs(lin) < inf && fabs(pla) < inf && fabs(ver) < inf;                  // (NaN fails)
      const bool limb = lin >= a.linearity_min, patch = pla >= a.planarity_min && ver >= a.verticality_min;
      hold += (nn >= (double)a.min_neighbours && finite && (limb || patch)) ? 1 : 0;
    }
    flag[j] = hold >= scales_min ? 1 : 0;
  }
}

__global__ void __launch_bounds__(64) k_leafwood_vote(const double* __restrict__ xyz, const int64_t* __restrict__ keys, int64_t n, double r2,
                                                      int64_t nx, int64_t ny, const int64_t* __restrict__ piece_start, int64_t n_pieces,
                                                      const int32_t* __restrict__ tag, int percent, uint8_t* __restrict__ flag_out,
                                                      int32_t* __restrict__ tag_out) {
  __shared__ double buf[2][kChunk * 3];
  __shared__ int32_t tbuf[2][kChunk];
  __shared__ int64_t rng[18];                       // [r][lo, hi) of the 9 (dx, dy) columns, x-major
  const int lane = threadIdx.x;
  const int64_t w = blockIdx.x;
  if (w >= n_pieces) return;
  const int64_t start = piece_start[w];
  if (start < 0 || start >= n) return;              // (uniform: nothing in a table can send the wave out of the arrays)
  const int64_t key = keys[start], col = key >> kBits;
  const int64_t cx = key >> (2 * kBits), cy = (key >> kBits) & kMask;
  const int64_t blk_end = ((start >> 6) + 1) << 6 < n ? ((start >> 6) + 1) << 6 : n;     // a piece stays inside its aligned 64-block
  const int64_t i = start + lane;
  const bool valid = i < blk_end && (keys[i < blk_end ? i : start] >> kBits) == col;       // (a prefix of the lanes: the array is sorted)
  const int nvalid = __popcll(__ballot(valid));     // >= 1: lane 0 is valid
  if (lane < 18) {
    const int r = lane >> 1;
    const int64_t x = cx - 1 + r / 3, y = cy - 1 + r % 3;
    const int64_t zmin = key & kMask, zmax = keys[start + nvalid - 1] & kMask;
    const int64_t z0 = zmin > 0 ? zmin - 1 : 0, z1 = zmax < kMask ? zmax + 1 : kMask;
    int64_t v = 0;                                  // a column outside the plot: the empty range [0, 0)
    if (x >= 0 && x <= nx && y >= 0 && y <= ny) {
      const int64_t kb = (x << (2 * kBits)) | (y << kBits);
      v = lower_bound(keys, n, (lane & 1) ? (kb | z1) + 1 : (kb | z0));                    // in [0, n]
    }
    rng[lane] = v;
  }
  __syncthreads();
  const int64_t ip = valid ? i : start;
  const double px = xyz[ip * 3], py = xyz[ip * 3 + 1], pz = xyz[ip * 3 + 2];
  const int32_t ptree = tag[ip] >> 1;

  // the chunks of the 9 ranges, in order
  int r = -1; int64_t off = 0, hi = 0;
  auto next = [&](int64_t& c_off, int& c_cnt) -> bool {
    while (off >= hi) { if (++r >= 9) return false; off = rng[2 * r]; hi = rng[2 * r + 1]; }
    c_off = off; c_cnt = (int)((hi - off) < (int64_t)kChunk ? (hi - off) : (int64_t)kChunk); off += c_cnt;
    return true;
  };
  double reg[kLoads];
  int32_t treg[kTagLoads];
  auto fetch = [&](int64_t c_off, int c_cnt) {
    const double* __restrict__ src = xyz + c_off * 3;
    const int32_t* __restrict__ tsrc = tag + c_off;
#pragma unroll
    for (int k = 0; k < kLoads; ++k) { const int idx = k * 64 + lane; reg[k] = idx < c_cnt * 3 ? src[idx] : 0.0; }
#pragma unroll
    for (int k = 0; k < kTagLoads; ++k) { const int idx = k * 64 + lane; treg[k] = idx < c_cnt ? tsrc[idx] : -2; }
  };

  int32_t na = 0, nw = 0;
  int64_t c_off = 0; int c_cnt = 0, b = 0;
  bool have = next(c_off, c_cnt);
  if (have) fetch(c_off, c_cnt);
  while (have) {
    double* cur = buf[b];
    int32_t* tcur = tbuf[b];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) cur[k * 64 + lane] = reg[k];
#pragma unroll
    for (int k = 0; k < kTagLoads; ++k) tcur[k * 64 + lane] = treg[k];
    __syncthreads();
    const int m = c_cnt;
    have = next(c_off, c_cnt);
    if (have) fetch(c_off, c_cnt);                  // in flight while the lanes walk the current chunk
    for (int j = 0; j < m; ++j) {
      const int32_t t = tcur[j];
      bool in;
      {
#pragma clang fp contract(off)
        const double dx = cur[3 * j] - px, dy = cur[3 * j + 1] - py, dz = cur[3 * j + 2] - pz;
        in = dx * dx + dy * dy + dz * dz <= r2;
      }
      const int32_t hit = (in && (t >> 1) == ptree) ? 1 : 0;
      na += hit; nw += hit & t;
    }
    b ^= 1;
  }
  if (!valid) return;
  const int32_t f = 100 * (int64_t)nw >= (int64_t)percent * (int64_t)na ? 1 : 0;
  flag_out[i] = (uint8_t)f;
  if (tag_out) tag_out[i] = (ptree << 1) | f;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the constraints of the parameter table; NaN fails every one of them
bool params_ok(const tl_leafwood_params* p) {
  if (!p) return false;
  const double inf = __builtin_inf();
  if (!(p->radius > 0.0 && p->radius < inf) || !(p->voxel > 0.0 && p->voxel < inf)) return false;
  if (!(p->linearity_min >= 0.0 && p->linearity_min <= 1.0) || !(p->planarity_min >= 0.0 && p->planarity_min <= 1.0) ||
      !(p->verticality_min >= 0.0 && p->verticality_min <= 1.0))
    return false;
  if (p->min_neighbours < 3 || p->vote_iters < 0 || p->vote_iters > 8 || p->vote_percent < 1 || p->vote_percent > 100 || p->reach < 1 ||
      p->reach > 2 || p->min_component < 1 || p->filter < 0 || p->filter > 1)
    return false;
  return true;
}

}  // namespace

extern "C" {

int tl_leafwood_seed(const float* feats, int64_t n, const tl_leafwood_params* params, uint8_t* flag, tl_stream_t stream) {
  if (!feats || !flag || n < 0 || !aligned(feats, 16)) return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  k_leafwood_seed<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(feats, n, *params, flag);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_leafwood_seed_scales(const float* feats, int64_t n, int S, const tl_leafwood_params* params, int scales_min, uint8_t* flag,
                            tl_stream_t stream) {
  if (!feats || !flag || n < 0 || !aligned(feats, 16)) return TL_ERR_ARG;
  if (S < 1 || S > TL_FEAT_MAX_SCALES || scales_min < 1 || scales_min > S) return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (n == 0) return TL_OK;
  k_leafwood_seed_scales<<<tl_grid(n, kBlock), kBlock, 0, tl_s(stream)>>>(feats, n, S, *params, scales_min, flag);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

int tl_leafwood_vote(const double* xyz_sorted, const int64_t* sorted_keys, int64_t n, const int64_t* extent2, const int64_t* piece_start,
                     int64_t n_pieces, const int32_t* tag, const tl_leafwood_params* params, uint8_t* flag_out, int32_t* tag_out,
                     tl_stream_t stream) {
  if (!xyz_sorted || !sorted_keys || !extent2 || !piece_start || !tag || !flag_out || n < 0 || n_pieces < 0) return TL_ERR_ARG;
  if (!aligned(xyz_sorted, 8) || !aligned(sorted_keys, 8) || !aligned(extent2, 8) || !aligned(piece_start, 8) || !aligned(tag, 4) ||
      !aligned(tag_out, 4) || tag_out == tag)
    return TL_ERR_ARG;
  if (n_pieces > n || n_pieces > 0x7fffffffll) return TL_ERR_ARG;
  if (!params_ok(params)) return TL_ERR_ARG;
  if (extent2[0] < 0 || extent2[0] > kMask || extent2[1] < 0 || extent2[1] > kMask) return TL_ERR_ARG;
  if (n == 0 || n_pieces == 0) return TL_OK;
  k_leafwood_vote<<<(unsigned)n_pieces, 64, 0, tl_s(stream)>>>(xyz_sorted, sorted_keys, n, params->radius * params->radius, extent2[0],
                                                               extent2[1], piece_start, n_pieces, tag, (int)params->vote_percent, flag_out,
                                                               tag_out);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

}  // extern "C"
