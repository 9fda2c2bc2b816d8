// Training and validation batches prepared on the device: the per-item work of the reference's TreeDataset.__getitem__
// (tree_learn/dataset/dataset.py:34-140) and the concatenation of collate_fn (:167-226).
//
// tl_point_jitter: point jitter (dataset.py:92-95) from a counter-based generator -- NOT numpy's draws.
// tl_train_item : semantic labels, the augmentation matrix, offset labels (:111-140), the three masks, batch ids and centres of ONE crop or tile,
//   written at a row offset into batch-sized outputs.  Launches, all on the caller's stream, nothing read back:
//     memset      label table (int32 keys, 0 = empty: label 0 is the non-tree class and is never inserted) and the slot counter
//     k_insert    rows: label -> table entry (open addressing, linear probing, atomicCAS; a wave whose rows share one label probes once)
//     k_assign    table entries: occupied entry -> dense slot id, slot state initialised (only the slots in use are ever touched)
//     k_first     rows: slot id and the order-preserving u64 image of z (f64) stored per row; rows per slot; the slot's minimum m0
//     k_rank<1..3> rows: count of the rows equal to m(r-1), minimum m(r) above it -- only while the cumulative count is below 4
//     k_thresh    slots: low = the value of rank 3 (instances of more than 11 rows) or m0; threshold low + 0.5 in the coordinate type
//     k_sums      rows: the base rows (z <= threshold) are added to the slot's sums
//     k_pos       slots: position = f32(sum / count)
//     k_write     rows: every output
//   After k_first the row passes read 12 bytes per row (slot, z image), 23 MB for a 1.9 M-row item: they run out of the Infinity Cache.
//
// Determinism without an ordered merge: the base sums are EXACT.  Every addend is turned into a 128-bit fixed-point integer (60 fraction
// bits: resolution 2^-60, magnitudes below 2^32) and added with 64-bit integer atomics, the carry of the low word taken from the value the
// atomic returns.  Integer addition commutes, so the sums -- and every output bit -- do not depend on the order of arrival.  No
// floating-point atomic is used anywhere; minima and counts are integer atomics as well.
#include "tl_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kBlock = 256;
constexpr uint64_t kMax = ~0ull;

struct __attribute__((aligned(128))) Slot {
  uint64_t m[4];        // the four lowest distinct z images
  uint32_t c[3];        // rows equal to m[0..2]
  uint32_t rows;        // rows of the instance
  uint64_t sum[6];      // x, y, z sums: (low word, high word) each
  double thr;           // low + 0.5
  uint32_t nb;          // base rows
  float pos[3];
  uint64_t pad;
};
static_assert(sizeof(Slot) == 128, "one slot is one 128-byte line");

struct Mat { double v[9]; };

__host__ __device__ inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Layout {
  int64_t cap;          // table entries, a power of two >= 2 n
  int shift;            // 32 - log2(cap)
  int64_t keys, ids, counter, slot, zkey, slots, total;
};

Layout layout(int64_t n) {
  Layout L;
  int lg = 10;
  while (((int64_t)1 << lg) < 2 * n) ++lg;
  L.cap = (int64_t)1 << lg;
  L.shift = 32 - lg;
  int64_t o = 0;
  L.keys = o; o += align256(L.cap * 4);
  L.ids = o; o += align256(L.cap * 4);
  L.counter = o; o += 256;
  L.slot = o; o += align256(n * 4);
  L.zkey = o; o += align256(n * 8);
  L.slots = o; o += n * (int64_t)sizeof(Slot);
  L.total = o;
  return L;
}

// ---- order-preserving u64 image of a double (-0 folded into +0)
__device__ __forceinline__ uint64_t z_image(double z) {
  const uint64_t b = __builtin_bit_cast(uint64_t, z + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double z_value(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __builtin_bit_cast(double, b);
}

// ---- coordinates of a row in the item's coordinate type, as doubles (test mode: the widened float32)
template <bool TRAIN>
__device__ __forceinline__ void row_coords(const float* __restrict__ xyz, int64_t i, const Mat& m, double& x, double& y, double& z) {
  const double a = (double)xyz[3 * i], b = (double)xyz[3 * i + 1], c = (double)xyz[3 * i + 2];
  if (TRAIN) {
    x = a * m.v[0] + b * m.v[3] + c * m.v[6];
    y = a * m.v[1] + b * m.v[4] + c * m.v[7];
    z = a * m.v[2] + b * m.v[5] + c * m.v[8];
  } else {
    x = a; y = b; z = c;
  }
}
template <bool TRAIN>
__device__ __forceinline__ double row_z(const float* __restrict__ xyz, int64_t i, const Mat& m) {
  if (TRAIN) return (double)xyz[3 * i] * m.v[2] + (double)xyz[3 * i + 1] * m.v[5] + (double)xyz[3 * i + 2] * m.v[8];
  return (double)xyz[3 * i + 2];
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, off);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ void min_filtered(uint64_t* p, uint64_t key) {
  // the load is only a filter (a stale, larger value costs one more atomic); the atomic decides
  if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin((unsigned long long*)p, (unsigned long long)key);
}

// Called by EVERY lane of the wave.  Lanes with `want` lower slots[s].m[which] to their key; when they all name one slot, one lane does it.
__device__ __forceinline__ void slot_min(Slot* __restrict__ slots, int s, int which, uint64_t key, bool want) {
  const uint64_t act = __ballot(want);
  if (!act) return;
  const int lead = __ffsll((unsigned long long)act) - 1;
  const int s0 = __shfl(s, lead);
  if (__ballot(want && s != s0) == 0) {
    const uint64_t k = wave_min(want ? key : kMax);
    if ((int)(threadIdx.x & 63) == lead) min_filtered(&slots[s0].m[which], k);
  } else if (want) {
    min_filtered(&slots[s].m[which], key);
  }
}

__device__ __forceinline__ int probe(int32_t* __restrict__ keys, uint32_t mask, int shift, int32_t label) {
  uint32_t h = ((uint32_t)label * 2654435761u) >> shift;
  for (;;) {                                     // ends: the table has at least twice as many entries as there are rows
    const int32_t k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == label) return (int)h;
    if (k == 0) {
      const int32_t old = atomicCAS(&keys[h], 0, label);
      if (old == 0 || old == label) return (int)h;
    }
    h = (h + 1) & mask;
  }
}

// every row loop below is uniform per workgroup (base .. base + kBlock), so that whole waves reach the ballots and shuffles
#define TL_ROW_LOOP(i, active, n)                                                                         \
  for (int64_t base_ = (int64_t)blockIdx.x * kBlock; base_ < (n); base_ += (int64_t)gridDim.x * kBlock)   \
    if (const int64_t i = base_ + threadIdx.x; true)                                                      \
      if (const bool active = i < (n); true)

__global__ void __launch_bounds__(kBlock) k_insert(const int32_t* __restrict__ inst, int64_t n, int32_t* __restrict__ keys, uint32_t mask, int shift,
                                                   int32_t* __restrict__ entry) {
  TL_ROW_LOOP(i, active, n) {
    const int32_t label = active ? inst[i] : 0;
    const bool want = label != 0;
    const uint64_t act = __ballot(want);
    if (!act) { if (active) entry[i] = -1; continue; }
    const int lead = __ffsll((unsigned long long)act) - 1;
    const int32_t l0 = __shfl(label, lead);
    int e = -1;
    if (__ballot(want && label != l0) == 0) {
      if ((int)(threadIdx.x & 63) == lead) e = probe(keys, mask, shift, label);
      e = __shfl(e, lead);
      if (!want) e = -1;
    } else if (want) {
      e = probe(keys, mask, shift, label);
    }
    if (active) entry[i] = e;
  }
}

__global__ void __launch_bounds__(kBlock) k_assign(const int32_t* __restrict__ keys, int64_t cap, int32_t* __restrict__ ids, uint32_t* __restrict__ counter,
                                                   Slot* __restrict__ slots) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < cap; e += (int64_t)gridDim.x * kBlock) {
    if (keys[e] == 0) continue;
    const uint32_t id = atomicAdd(counter, 1u);          // at most one per distinct label: never more than n
    ids[e] = (int32_t)id;
    Slot s;
    for (int k = 0; k < 4; ++k) s.m[k] = kMax;
    for (int k = 0; k < 3; ++k) s.c[k] = 0;
    s.rows = 0;
    for (int k = 0; k < 6; ++k) s.sum[k] = 0;
    s.thr = 0.0; s.nb = 0; s.pos[0] = s.pos[1] = s.pos[2] = 0.f; s.pad = 0;
    slots[id] = s;
  }
}

template <bool TRAIN>
__global__ void __launch_bounds__(kBlock) k_first(const float* __restrict__ xyz, Mat m, int64_t n, const int32_t* __restrict__ ids,
                                                  int32_t* __restrict__ slot /* in: table entry, out: slot id */, uint64_t* __restrict__ zkey,
                                                  Slot* __restrict__ slots) {
  TL_ROW_LOOP(i, active, n) {
    int s = -1;
    uint64_t key = kMax;
    if (active) {
      const int e = slot[i];
      if (e >= 0) s = ids[e];
      key = z_image(row_z<TRAIN>(xyz, i, m));
      slot[i] = s;
      zkey[i] = key;
    }
    const bool want = s >= 0;
    const uint64_t act = __ballot(want);
    if (!act) continue;
    const int lead = __ffsll((unsigned long long)act) - 1;
    const int s0 = __shfl(s, lead);
    if (__ballot(want && s != s0) == 0) {
      if ((int)(threadIdx.x & 63) == lead) atomicAdd(&slots[s0].rows, (uint32_t)__popcll((unsigned long long)act));
    } else if (want) {
      atomicAdd(&slots[s].rows, 1u);
    }
    slot_min(slots, s, 0, key, want);
  }
}

template <int R>
__global__ void __launch_bounds__(kBlock) k_rank(const int32_t* __restrict__ slot, const uint64_t* __restrict__ zkey, int64_t n, Slot* __restrict__ slots) {
  TL_ROW_LOOP(i, active, n) {
    const int s = active ? slot[i] : -1;
    bool want = false;
    uint64_t key = kMax;
    if (s >= 0) {
      const Slot& S = slots[s];
      uint32_t cum = 0;
      for (int k = 0; k < R - 1; ++k) cum += S.c[k];
      if (S.rows > 11 && cum < 4) {
        key = zkey[i];
        const uint64_t prev = S.m[R - 1];
        if (key == prev) atomicAdd(&slots[s].c[R - 1], 1u);
        want = key > prev;
      }
    }
    slot_min(slots, s, R, key, want);
  }
}

template <bool TRAIN>
__global__ void __launch_bounds__(kBlock) k_thresh(Slot* __restrict__ slots, const uint32_t* __restrict__ counter) {
  const int64_t ns = *counter;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < ns; s += (int64_t)gridDim.x * kBlock) {
    Slot& S = slots[s];
    uint64_t low = S.m[0];
    if (S.rows > 11) {
      const uint32_t c0 = S.c[0], c1 = c0 + S.c[1], c2 = c1 + S.c[2];
      low = c0 >= 4 ? S.m[0] : c1 >= 4 ? S.m[1] : c2 >= 4 ? S.m[2] : S.m[3];
    }
    const double lowd = z_value(low);
    S.thr = TRAIN ? lowd + 0.5 : (double)((float)lowd + 0.5f);
  }
}

// x -> floor(x * 2^60) as a 128-bit two's-complement integer (hi, lo); |x| is clamped below 2^32
__device__ __forceinline__ void fixed128(double x, uint64_t& lo, uint64_t& hi) {
  x = fmin(fmax(x, -4294967295.0), 4294967295.0);
  const double a = trunc(x);                                 // x - trunc(x) is exact for every double (x - floor(x) is NOT: it rounds
  const int64_t ai = (int64_t)a;                             // for a negative x, up to 1.0 for a tiny one), keeps x's sign, |.| < 1
  const int64_t fi = (int64_t)floor((x - a) * 0x1p60);       // the scaling is exact; floor: -2^60 <= fi < 2^60
  const uint64_t alo = (uint64_t)ai << 60;
  lo = alo + (uint64_t)fi;                                   // (ai * 2^60) + sign-extended fi, as 128-bit two's complement
  hi = (uint64_t)(ai >> 4) + (uint64_t)(fi >> 63) + (uint64_t)(lo < alo);
}
__device__ __forceinline__ void add128(uint64_t* __restrict__ acc, double x) {
  uint64_t lo, hi;
  fixed128(x, lo, hi);
  const uint64_t old = (uint64_t)atomicAdd((unsigned long long*)&acc[0], (unsigned long long)lo);
  hi += (uint64_t)(old + lo < old);
  if (hi) atomicAdd((unsigned long long*)&acc[1], (unsigned long long)hi);
}
__device__ __forceinline__ double value128(const uint64_t* acc) {
  const uint64_t lo = acc[0];
  const int64_t hi = (int64_t)acc[1];
  return ((double)hi * 0x1p64 + (double)(lo >> 32) * 0x1p32 + (double)(lo & 0xFFFFFFFFull)) * 0x1p-60;
}

template <bool TRAIN>
__global__ void __launch_bounds__(kBlock) k_sums(const float* __restrict__ xyz, Mat m, const int32_t* __restrict__ slot, const uint64_t* __restrict__ zkey,
                                                 int64_t n, Slot* __restrict__ slots) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int s = slot[i];
    if (s < 0) continue;
    if (!(z_value(zkey[i]) <= slots[s].thr)) continue;
    double x, y, z;
    row_coords<TRAIN>(xyz, i, m, x, y, z);
    Slot& S = slots[s];
    add128(&S.sum[0], x); add128(&S.sum[2], y); add128(&S.sum[4], z);
    atomicAdd(&S.nb, 1u);
  }
}

__global__ void __launch_bounds__(kBlock) k_pos(Slot* __restrict__ slots, const uint32_t* __restrict__ counter) {
  const int64_t ns = *counter;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < ns; s += (int64_t)gridDim.x * kBlock) {
    Slot& S = slots[s];
    const double nb = (double)S.nb;                      // >= 1: the row of rank 3 (or the minimum) is a base row
    for (int k = 0; k < 3; ++k) S.pos[k] = (float)(value128(&S.sum[2 * k]) / nb);
  }
}

struct Out {
  float* coords; int64_t* sem; int64_t* inst; float* off; uint8_t* m_inner; uint8_t* m_off; uint8_t* m_sem; int64_t* bid; float* centers;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct RowOut {
  float c[3], o[3];
  int64_t sem, inst;
  uint8_t mi, mo, ms;
};

template <bool TRAIN>
__device__ __forceinline__ RowOut row_out(float a, float b, float c, int32_t label, int s, const Slot* __restrict__ slots, const Mat& m,
                                          double half_inner) {
  RowOut r;
  double x = (double)a, y = (double)b, z = (double)c;
  if (TRAIN) {
    x = (double)a * m.v[0] + (double)b * m.v[3] + (double)c * m.v[6];
    y = (double)a * m.v[1] + (double)b * m.v[4] + (double)c * m.v[7];
    z = (double)a * m.v[2] + (double)b * m.v[5] + (double)c * m.v[8];
  }
  float p[3] = {1.f, 1.f, 1.f};
  if (s >= 0) { p[0] = slots[s].pos[0]; p[1] = slots[s].pos[1]; p[2] = slots[s].pos[2]; }
  bool inner;
  if (TRAIN) {
    r.c[0] = (float)x; r.c[1] = (float)y; r.c[2] = (float)z;
    r.o[0] = (float)((double)p[0] - x); r.o[1] = (float)((double)p[1] - y); r.o[2] = (float)((double)p[2] - z);
    inner = fmax(fabs(x), fabs(y)) <= half_inner;
  } else {
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    r.c[0] = fx; r.c[1] = fy; r.c[2] = fz;
    r.o[0] = p[0] - fx; r.o[1] = p[1] - fy; r.o[2] = p[2] - fz;
    inner = fmaxf(fabsf(fx), fabsf(fy)) <= (float)half_inner;
  }
  const bool sem_ok = inner && label != -1;
  r.sem = label == 0 ? 1 : 0;
  r.inst = (int64_t)label;
  r.mi = inner; r.ms = sem_ok; r.mo = sem_ok && label != 0;
  return r;
}

// One lane per QUAD of output rows (output rows 4q .. 4q+3 of the batch arrays): a whole quad inside the item is stored with 16-byte
// stores (48 B of coords, offsets and centres, 32 B of each int64 array, 4 mask bytes each), the partial quads at the item's ends row by row.
// The inputs of a whole quad come in 16-byte loads as well when the item starts at a multiple of four batch rows (always, for a batch's first
// item and for a tile); at any other offset the output quads straddle the input quads and the rows are loaded one by one.
template <bool TRAIN, bool VEC>
__global__ void __launch_bounds__(kBlock) k_write(const float* __restrict__ xyz, const int32_t* __restrict__ inst, const int32_t* __restrict__ slot,
                                                  const Slot* __restrict__ slots, Mat m, double half_inner, float cx, float cy, float cz,
                                                  int64_t batch_id, int64_t row_offset, int64_t n, Out out) {
  const int64_t q0 = row_offset >> 2, q1 = (row_offset + n + 3) >> 2;
  // a whole output quad is a whole 16-byte-aligned input quad when the item starts at a multiple of four rows (slot: 256-byte aligned workspace)
  const bool in16 = (row_offset & 3) == 0 && ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(inst)) & 15) == 0;
  for (int64_t q = q0 + (int64_t)blockIdx.x * kBlock + threadIdx.x; q < q1; q += (int64_t)gridDim.x * kBlock) {
    const int64_t r0 = q * 4;
    const bool whole = VEC && r0 >= row_offset && r0 + 4 <= row_offset + n;
    if (whole) {
      RowOut r[4];
      const int64_t in0 = r0 - row_offset;
      if (in16) {                                            // the item's rows 4k .. 4k+3: 3 + 1 + 1 16-byte loads
        const u32x4* X = reinterpret_cast<const u32x4*>(xyz + 3 * in0);
        const u32x4 x0 = X[0], x1 = X[1], x2 = X[2];
        const u32x4 li = *reinterpret_cast<const u32x4*>(inst + in0), si = *reinterpret_cast<const u32x4*>(slot + in0);
        const uint32_t w[12] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y, x2.z, x2.w};
        const uint32_t l[4] = {li.x, li.y, li.z, li.w}, sl[4] = {si.x, si.y, si.z, si.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          r[j] = row_out<TRAIN>(__uint_as_float(w[3 * j]), __uint_as_float(w[3 * j + 1]), __uint_as_float(w[3 * j + 2]), (int32_t)l[j], (int)sl[j],
                                slots, m, half_inner);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          r[j] = row_out<TRAIN>(xyz[3 * (in0 + j)], xyz[3 * (in0 + j) + 1], xyz[3 * (in0 + j) + 2], inst[in0 + j], slot[in0 + j], slots, m, half_inner);
      }
      u32x4* C = reinterpret_cast<u32x4*>(out.coords + 3 * r0);
      u32x4* O = reinterpret_cast<u32x4*>(out.off + 3 * r0);
      u32x4* E = reinterpret_cast<u32x4*>(out.centers + 3 * r0);
      uint32_t c[12], o[12], e[12];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          c[3 * j + k] = __float_as_uint(r[j].c[k]); o[3 * j + k] = __float_as_uint(r[j].o[k]);
          e[3 * j + k] = __float_as_uint(k == 0 ? cx : k == 1 ? cy : cz);
        }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        C[k] = u32x4{c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]};
        O[k] = u32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
        E[k] = u32x4{e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3]};
      }
      u32x4* S = reinterpret_cast<u32x4*>(out.sem + r0);
      u32x4* I = reinterpret_cast<u32x4*>(out.inst + r0);
      u32x4* B = reinterpret_cast<u32x4*>(out.bid + r0);
      const uint32_t blo = (uint32_t)((uint64_t)batch_id & 0xFFFFFFFFull), bhi = (uint32_t)((uint64_t)batch_id >> 32);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const uint64_t i0 = (uint64_t)r[2 * k].inst, i1 = (uint64_t)r[2 * k + 1].inst;
        S[k] = u32x4{(uint32_t)r[2 * k].sem, 0u, (uint32_t)r[2 * k + 1].sem, 0u};
        I[k] = u32x4{(uint32_t)i0, (uint32_t)(i0 >> 32), (uint32_t)i1, (uint32_t)(i1 >> 32)};
        B[k] = u32x4{blo, bhi, blo, bhi};
      }
      uint32_t mi = 0, mo = 0, ms = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { mi |= (uint32_t)r[j].mi << (8 * j); mo |= (uint32_t)r[j].mo << (8 * j); ms |= (uint32_t)r[j].ms << (8 * j); }
      reinterpret_cast<uint32_t*>(out.m_inner)[q] = mi;
      reinterpret_cast<uint32_t*>(out.m_off)[q] = mo;
      reinterpret_cast<uint32_t*>(out.m_sem)[q] = ms;
    } else {
      for (int j = 0; j < 4; ++j) {
        const int64_t g = r0 + j;
        if (g < row_offset || g >= row_offset + n) continue;
        const int64_t i = g - row_offset;
        const RowOut r = row_out<TRAIN>(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], inst[i], slot[i], slots, m, half_inner);
        for (int k = 0; k < 3; ++k) { out.coords[3 * g + k] = r.c[k]; out.off[3 * g + k] = r.o[k]; }
        out.centers[3 * g] = cx; out.centers[3 * g + 1] = cy; out.centers[3 * g + 2] = cz;
        out.sem[g] = r.sem; out.inst[g] = r.inst; out.bid[g] = batch_id;
        out.m_inner[g] = r.mi; out.m_off[g] = r.mo; out.m_sem[g] = r.ms;
      }
    }
  }
}

// ---- jitter: splitmix64 of (key, row, component) -> two uniforms -> Box-Muller, all in f64
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__global__ void __launch_bounds__(kBlock) k_point_jitter(float* __restrict__ xyz, int64_t n3, uint64_t key) {
  for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n3; e += (int64_t)gridDim.x * kBlock) {
    const uint64_t row = (uint64_t)(e / 3), comp = (uint64_t)(e % 3);
    const uint64_t h1 = mix64(mix64(key) + (row * 4 + comp + 1) * 0x9E3779B97F4A7C15ull);
    const uint64_t h2 = mix64(h1 ^ 0xD6E8FEB86659FD93ull);
    const double u1 = ((double)(h1 >> 11) + 1.0) * 0x1p-53;            // (0, 1]
    const double u2 = (double)(h2 >> 11) * 0x1p-53;                    // [0, 1)
    const double g = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
    const double d = fmin(fmax(0.1 * g, -0.2), 0.2);
    xyz[e] = (float)((double)xyz[e] + d);
  }
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <bool TRAIN>
int run_item(const float* xyz, const int32_t* inst, int64_t n, const Mat& m, double half_inner, const float* c, int64_t batch_id, int64_t row_offset,
             const Out& out, char* ws, hipStream_t s) {
  const Layout L = layout(n);
  int32_t* keys = reinterpret_cast<int32_t*>(ws + L.keys);
  int32_t* ids = reinterpret_cast<int32_t*>(ws + L.ids);
  uint32_t* counter = reinterpret_cast<uint32_t*>(ws + L.counter);
  int32_t* slot = reinterpret_cast<int32_t*>(ws + L.slot);
  uint64_t* zkey = reinterpret_cast<uint64_t*>(ws + L.zkey);
  Slot* slots = reinterpret_cast<Slot*>(ws + L.slots);
  if (hipMemsetAsync(keys, 0, (size_t)(L.ids - L.keys), s) != hipSuccess) return TL_ERR_LAUNCH;
  if (hipMemsetAsync(counter, 0, 256, s) != hipSuccess) return TL_ERR_LAUNCH;
  const unsigned grows = tl_grid(n, kBlock), gslots = tl_grid(n < 65536 ? n : 65536, kBlock);
  k_insert<<<grows, kBlock, 0, s>>>(inst, n, keys, (uint32_t)(L.cap - 1), L.shift, slot);
  TL_CHECK_LAUNCH();
  k_assign<<<tl_grid(L.cap, kBlock), kBlock, 0, s>>>(keys, L.cap, ids, counter, slots);
  TL_CHECK_LAUNCH();
  k_first<TRAIN><<<grows, kBlock, 0, s>>>(xyz, m, n, ids, slot, zkey, slots);
  TL_CHECK_LAUNCH();
  k_rank<1><<<grows, kBlock, 0, s>>>(slot, zkey, n, slots);
  TL_CHECK_LAUNCH();
  k_rank<2><<<grows, kBlock, 0, s>>>(slot, zkey, n, slots);
  TL_CHECK_LAUNCH();
  k_rank<3><<<grows, kBlock, 0, s>>>(slot, zkey, n, slots);
  TL_CHECK_LAUNCH();
  k_thresh<TRAIN><<<gslots, kBlock, 0, s>>>(slots, counter);
  TL_CHECK_LAUNCH();
  k_sums<TRAIN><<<grows, kBlock, 0, s>>>(xyz, m, slot, zkey, n, slots);
  TL_CHECK_LAUNCH();
  k_pos<<<gslots, kBlock, 0, s>>>(slots, counter);
  TL_CHECK_LAUNCH();
  const bool vec = aligned(out.coords, 16) && aligned(out.off, 16) && aligned(out.centers, 16) && aligned(out.sem, 16) && aligned(out.inst, 16) &&
                   aligned(out.bid, 16) && aligned(out.m_inner, 4) && aligned(out.m_off, 4) && aligned(out.m_sem, 4);
  const float cx = c ? c[0] : 1.f, cy = c ? c[1] : 1.f, cz = c ? c[2] : 1.f;
  const unsigned gq = tl_grid(n / 4 + 2, kBlock);
  if (vec) k_write<TRAIN, true><<<gq, kBlock, 0, s>>>(xyz, inst, slot, slots, m, half_inner, cx, cy, cz, batch_id, row_offset, n, out);
  else k_write<TRAIN, false><<<gq, kBlock, 0, s>>>(xyz, inst, slot, slots, m, half_inner, cx, cy, cz, batch_id, row_offset, n, out);
  TL_CHECK_LAUNCH();
  return TL_OK;
}
}  // namespace

extern "C" int tl_point_jitter(float* xyz, int64_t n, uint64_t key, tl_stream_t stream) {
  if (!xyz || n <= 0 || n >= ((int64_t)1 << 40) || !aligned(xyz, 4)) return TL_ERR_ARG;
  k_point_jitter<<<tl_grid(3 * n, kBlock), kBlock, 0, tl_s(stream)>>>(xyz, 3 * n, key);
  TL_CHECK_LAUNCH();
  return TL_OK;
}

extern "C" int64_t tl_train_item_ws_bytes(int64_t n) {
  if (n <= 0 || n > ((int64_t)1 << 30)) return 0;
  return layout(n).total;
}

extern "C" int tl_train_item(const float* xyz, const int32_t* instance_label, int64_t n, const double* m, double half_inner, const float* center,
                             int64_t batch_id, int64_t row_offset, float* coords, int64_t* semantic_labels, int64_t* instance_labels,
                             float* offset_labels, uint8_t* masks_inner, uint8_t* masks_off, uint8_t* masks_sem, int64_t* batch_ids, float* centers,
                             void* ws, tl_stream_t stream) {
  if (!xyz || !instance_label || !coords || !semantic_labels || !instance_labels || !offset_labels || !masks_inner || !masks_off || !masks_sem ||
      !batch_ids || !centers || !ws)
    return TL_ERR_ARG;
  if (n <= 0 || n > ((int64_t)1 << 30) || row_offset < 0 || row_offset >= ((int64_t)1 << 40) || !(half_inner >= 0.0)) return TL_ERR_ARG;
  if (!aligned(xyz, 4) || !aligned(instance_label, 4) || !aligned(coords, 4) || !aligned(offset_labels, 4) || !aligned(centers, 4) ||
      !aligned(semantic_labels, 8) || !aligned(instance_labels, 8) || !aligned(batch_ids, 8) || !aligned(ws, 256))
    return TL_ERR_ARG;
  const Out out{coords, semantic_labels, instance_labels, offset_labels, masks_inner, masks_off, masks_sem, batch_ids, centers};
  Mat mat;
  for (int k = 0; k < 9; ++k) mat.v[k] = m ? m[k] : (k % 4 == 0 ? 1.0 : 0.0);
  hipStream_t s = tl_s(stream);
  char* w = static_cast<char*>(ws);
  return m ? run_item<true>(xyz, instance_label, n, mat, half_inner, center, batch_id, row_offset, out, w, s)
           : run_item<false>(xyz, instance_label, n, mat, half_inner, center, batch_id, row_offset, out, w, s);
}
