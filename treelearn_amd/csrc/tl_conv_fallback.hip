// The two fallback conv kernels of tl_conv_fwd's dispatch (tl_conv.hip): the fp32 tile kernel for shapes none of the resident-weight /
// streamed-weight families has an instantiation for, and the scalar kernel for everything else (any Cin / Cout).
//
// Output-stationary gather-GEMM: a workgroup owns 128 consecutive output rows (ascending voxel
// key => spatially adjacent), walks the kernel taps that have at least one present neighbour in the
// tile, gathers the neighbour rows (16-B loads, 128 B contiguous per row segment), applies the
// fused BatchNorm+ReLU prologue, stages them with the tap's weight slice in padded LDS and
// contracts on the matrix cores; every output row is written exactly once (no atomics =>
// bit-deterministic), with the residual add / BatchNorm+ReLU epilogue fused into the store.
//
//   fp32 : v_mfma_f32_32x32x2_f32 (exact fp32, bitwise an fmaf chain) -- the parity path.
//   bf16 : v_mfma_f32_32x32x16_bf16, fp32 accumulate                  -- the throughput path.
//
// LDS row pitch = 32 channels + 16 B pad: ds_read_b128 of 16 different rows at one column offset
// lands on 16 different 16-B slots (36*r mod 64 is a permutation of multiples of 4 for r mod 16),
// i.e. conflict-free for the b128 lane groups of MI355X_MICROARCH.md §LDS.
#include "tl_conv_internal.h"

namespace {

// ------------------------------------------------------------------ generic fallback (any Cin/Cout)
template <typename T>
__global__ void __launch_bounds__(256) k_conv_generic(ConvP p) {
  const T* in = (const T*)p.in; const T* w = (const T*)p.w; const T* res = (const T*)p.res;
  const int64_t total = p.n_out * p.Cout;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t o = t / p.Cout; const int j = (int)(t % p.Cout);
    float acc = 0.f;
    for (int k = 0; k < p.K; ++k) {
      const int64_t idx = p.table ? (int64_t)p.table[(int64_t)k * p.n_out + o] : o;
      if (idx < 0) continue;
      const T* x = in + idx * p.in_ld;
      const T* wr = w + ((int64_t)k * p.Cout + j) * p.Cin;
      for (int c = 0; c < p.Cin; ++c) {
        float v = ld_elem(x + c);
        if (p.in_scale) v = fmaf(v, p.in_scale[c], p.in_shift[c]);
        if (p.in_relu) v = fmaxf(v, 0.f);
        if (sizeof(T) == 2) v = __bfloat162float(__float2bfloat16(v));   // bf16 path feeds bf16 to the MFMA
        acc = fmaf(v, ld_elem(wr + c), acc);
      }
    }
    if (res) acc += ld_elem(res + o * p.res_ld + j);
    constexpr bool BF = sizeof(T) == 2;
    epi_store1<BF>(p.out, p.out_ld, p.out_scale, p.out_shift, p.out_relu, o, j, acc);
    if (p.out2) epi_store1<BF>(p.out2, p.out2_ld, p.out2_scale, p.out2_shift, p.out2_relu, o, j, acc);
    if (p.out3) epi_store1<BF>(p.out3, p.out3_ld, p.out3_scale, p.out3_shift, p.out3_relu, o, j, acc);
  }
}

// ------------------------------------------------------------------ fp32 MFMA kernel
constexpr int TM = TL_CONV_TILE_ROWS;   // output rows per workgroup
constexpr int KC = 32;           // input channels per step
constexpr int LDA = KC + 4;      // padded LDS pitch in floats (144 B)

template <int NB>                // NB = Cout / 32
__global__ void __launch_bounds__(256) k_conv_mfma_f32(ConvP p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* idx_s = reinterpret_cast<int*>(smem);                                   // [K][TM]
  unsigned* mask_s = reinterpret_cast<unsigned*>(idx_s + p.K * TM);             // [4] (16 B keeps alignment)
  float* As = reinterpret_cast<float*>(mask_s + 4);                             // [2][TM][LDA]
  float* Bs = As + 2 * TM * LDA;                                                // [2][NB*32][LDA]

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tile = xcd_tile(blockIdx.x, p.nblk);
  const int64_t r0 = (int64_t)tile * TM;
  const float* in = (const float*)p.in; const float* W = (const float*)p.w;

  if (tid == 0) mask_s[0] = 0;
  __syncthreads();
  unsigned local = 0;
  for (int e = tid; e < p.K * TM; e += 256) {
    const int k = e >> 7, r = e & (TM - 1);
    const int64_t row = r0 + r;
    int idx = -1;
    if (row < p.n_out) idx = p.table ? p.table[(int64_t)k * p.n_out + row] : (int)row;
    idx_s[e] = idx;
    if (idx >= 0) local |= 1u << k;
  }
  if (local) atomicOr(&mask_s[0], local);
  __syncthreads();
  unsigned mask = __builtin_amdgcn_readfirstlane(mask_s[0]);

  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.f;

  const int nchunk = p.Cin / KC;
  const int lrow = tid >> 3, c4 = (tid & 7) * 4;
  float4 ra[4];
  f32x4 rb[NB];                      // native vector type: HIP's float4 struct copies lower to memcpy and pin the array in scratch
  bool va[4];

  auto issue = [&](int k, int ch) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = idx_s[k * TM + lrow + 32 * i];
      va[i] = idx >= 0;
      ra[i] = va[i] ? *reinterpret_cast<const float4*>(in + (int64_t)idx * p.in_ld + ch * KC + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
      rb[i] = *reinterpret_cast<const f32x4*>(W + ((int64_t)k * p.Cout + lrow + 32 * i) * p.Cin + ch * KC + c4);
  };
  auto stage = [&](int buf, int ch) __attribute__((always_inline)) {
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.in_scale) {
      sc = *reinterpret_cast<const float4*>(p.in_scale + ch * KC + c4);
      sh = *reinterpret_cast<const float4*>(p.in_shift + ch * KC + c4);
    }
    float* a = As + buf * TM * LDA;
    float* b = Bs + buf * NB * 32 * LDA;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float4 v = ra[i];
      if (va[i]) {
        if (p.in_scale) { v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y); v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w); }
        if (p.in_relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      }
      *reinterpret_cast<float4*>(a + (lrow + 32 * i) * LDA + c4) = v;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) *reinterpret_cast<f32x4*>(b + (lrow + 32 * i) * LDA + c4) = rb[i];
  };

  if (mask) {
    int k = __builtin_ctz(mask), ch = 0;
    issue(k, ch);
    stage(0, ch);
    __syncthreads();
    int buf = 0;
    const int fi = lane & 31, fh = lane >> 5;
    while (true) {
      // next step
      int nk = k, nch = ch + 1;
      unsigned nmask = mask;
      if (nch == nchunk) { nch = 0; nmask = mask & (mask - 1); nk = nmask ? __builtin_ctz(nmask) : -1; }
      const bool more = nk >= 0;
      if (more) issue(nk, nch);

      const float* a = As + buf * TM * LDA + (wv * 32 + fi) * LDA + fh * 4;
      float4 af[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) af[j] = *reinterpret_cast<const float4*>(a + 8 * j);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float* b = Bs + buf * NB * 32 * LDA + (nb * 32 + fi) * LDA + fh * 4;
        float4 bf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bf[j] = *reinterpret_cast<const float4*>(b + 8 * j);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].x, bf[j].x, acc[nb], 0, 0, 0);
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].y, bf[j].y, acc[nb], 0, 0, 0);
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].z, bf[j].z, acc[nb], 0, 0, 0);
          acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].w, bf[j].w, acc[nb], 0, 0, 0);
        }
      }
      if (!more) break;
      stage(buf ^ 1, nch);
      __syncthreads();
      buf ^= 1; k = nk; ch = nch; mask = nmask;
    }
  }

  // epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const float* res = (const float*)p.res;
  const int col = lane & 31;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int j = nb * 32 + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = r0 + wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= p.n_out) continue;
      float v = acc[nb][r];
      if (res) v += res[row * p.res_ld + j];
      epi_store1<false>(p.out, p.out_ld, p.out_scale, p.out_shift, p.out_relu, row, j, v);
      if (p.out2) epi_store1<false>(p.out2, p.out2_ld, p.out2_scale, p.out2_shift, p.out2_relu, row, j, v);
      if (p.out3) epi_store1<false>(p.out3, p.out3_ld, p.out3_scale, p.out3_shift, p.out3_relu, row, j, v);
    }
  }
}

}  // namespace

// fp32, aligned rows, Cin % 32 == 0, Cout % 32 == 0, Cout <= 224 (checked by the caller)
int tl_launch_conv_mfma_f32(const ConvP& p, hipStream_t s) {
  switch (p.Cout / 32) {
#define TL_M(NB_) case NB_: return tl_launch_lds<k_conv_mfma_f32<NB_>>(p.nblk, 256, (size_t)p.K * TM * 4 + 16 + 2 * (size_t)TM * LDA * 4 + 2 * (size_t)NB_ * 32 * LDA * 4, s, p);
    TL_M(1) TL_M(2) TL_M(3) TL_M(4) TL_M(5) TL_M(6) TL_M(7)
#undef TL_M
  }
  return TL_ERR_UNSUPPORTED;
}

// TL_F32 / TL_BF16, anything
int tl_launch_conv_generic(const ConvP& p, int dtype, hipStream_t s) {
  const unsigned g = tl_grid(p.n_out * p.Cout, 256);
  return dtype == TL_F32 ? tl_launch<k_conv_generic<float>>(g, 256, 0, s, p) : tl_launch<k_conv_generic<__hip_bfloat16>>(g, 256, 0, s, p);
}
