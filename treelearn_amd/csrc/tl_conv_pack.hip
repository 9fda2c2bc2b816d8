// Weight packing for the conv kernels (reference layout [Cout][K][Cin] -> the kernel layouts) and the stand-alone BatchNorm affine + ReLU pass.
#include "tl_conv_internal.h"

namespace {

__global__ void k_pack_weight(const float* __restrict__ w, int Cout, int K, int Cin, void* __restrict__ o, int dtype) {
  const int64_t total = (int64_t)Cout * K * Cin;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(t % Cin); const int64_t r = t / Cin; const int j = (int)(r % Cout); const int k = (int)(r / Cout);
    const float v = w[((int64_t)j * K + k) * Cin + c];                 // reference layout [Cout][K][Cin]
    if (dtype == TL_F32) reinterpret_cast<float*>(o)[t] = v;
    else if (dtype == TL_F16) reinterpret_cast<_Float16*>(o)[t] = (_Float16)v;
    else reinterpret_cast<__hip_bfloat16*>(o)[t] = __float2bfloat16(v);
  }
}

// split-bf16 form of fp32 weights (tl_conv_internal.h: the bf16x3 contraction): [K][Cout][Cin / 32][64 x bf16] -- per 32-channel unit the hi
// parts of the four 8-channel pieces (J, fh) at 16-B slots 2 J + fh, the lo parts at slots 4 + 2 J + fh; piece (J, fh) = channels
// 16 J + 4 fh + {0..3}, 16 J + 8 + 4 fh + {0..3} of the unit
__global__ void k_pack_weight_x3(const float* __restrict__ w, int Cout, int K, int Cin, uint16_t* __restrict__ o) {
  // Cin >= 256: stored as TWO independent half-width convs (input channels [0, Cin / 2) then [Cin / 2, Cin)), each [K][Cout][Cin / 64][64]:
  // tl_conv_fwd runs such a conv as two launches of the kernel that has an instantiation for the half width
  const int un_all = Cin / 32, halves = Cin >= 256 ? 2 : 1, un = un_all / halves;
  const int64_t per_half = (int64_t)Cout * K * un * 64, total = per_half * halves;
  for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t0 < total; t0 += (int64_t)gridDim.x * blockDim.x) {
    const int hf = (int)(t0 / per_half); const int64_t t = t0 - hf * per_half;
    const int e = (int)(t & 63); const int64_t r = t >> 6; const int c = (int)(r % un); const int64_t r2 = r / un;
    const int n = (int)(r2 % Cout); const int k = (int)(r2 / Cout);
    const int half = e >> 5, piece = (e & 31) >> 3, q = e & 7, J = piece >> 1, fh = piece & 1;
    const int ch = 32 * (c + hf * un) + 16 * J + (q < 4 ? 4 * fh + q : 8 + 4 * fh + (q - 4));
    const float v = w[((int64_t)n * K + k) * Cin + ch];                // reference layout [Cout][K][Cin]
    const __hip_bfloat16 hi = __float2bfloat16(v);
    const __hip_bfloat16 lo = __float2bfloat16(v - __bfloat162float(hi));
    o[t0] = half ? __builtin_bit_cast(uint16_t, lo) : __builtin_bit_cast(uint16_t, hi);
    // second copy in MFMA-fragment order (Cout % 32 == 0, Cin < 256) behind the first: the 16-B piece j (0, 1 = hi of channel group J = j; 2, 3 =
    // lo of J = j - 2) of lane (n & 31, fh) for (tap, column block, unit) is one contiguous KB -- what the small-level kernel loads per
    // instruction (tl_conv_small.hip, FR): slot 2 J + fh / 4 + 2 J + fh of the record above
    if (halves == 1 && Cout % 32 == 0) {
      const int j = half ? 2 + J : J;
      const int lane = (n & 31) + 32 * fh, cbt = n >> 5, CBt = Cout >> 5;
      o[total + ((((((int64_t)k * CBt + cbt) * un + c) * 4 + j) * 64 + lane) * 8) + q] = half ? __builtin_bit_cast(uint16_t, lo) : __builtin_bit_cast(uint16_t, hi);
    }
  }
}

// weights of the input-gradient conv straight from the reference layout: o[k][ci][co] = w[co][flip ? K-1-k : k][ci]
__global__ void k_pack_weight_dgrad(const float* __restrict__ w, int Cout, int K, int Cin, int flip, void* __restrict__ o, int dtype) {
  const int64_t total = (int64_t)Cout * K * Cin;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(t % Cout); const int64_t r = t / Cout; const int ci = (int)(r % Cin); const int k = (int)(r / Cin);
    const float v = w[((int64_t)co * K + (flip ? K - 1 - k : k)) * Cin + ci];
    if (dtype == TL_F32) reinterpret_cast<float*>(o)[t] = v;
    else if (dtype == TL_F16) reinterpret_cast<_Float16*>(o)[t] = (_Float16)v;
    else reinterpret_cast<__hip_bfloat16*>(o)[t] = __float2bfloat16(v);
  }
}

// fragment order: vector v = ((((k*CB + cb)*CH + ch)*J + j)*64 + lane) holds 16 B = W[k][32cb + (lane&31)][32ch + (32j + 16(lane>>5))/EB ..]
__global__ void k_pack_weight_frag(const float* __restrict__ w, int Cout, int K, int Cin, void* __restrict__ o, int dtype) {
  const int EB = dtype == TL_F32 ? 4 : 2, J = 32 * EB / 32, EPV = 16 / EB;
  const int CB = Cout / 32, CH = Cin / 32;
  const int64_t nvec = (int64_t)K * CB * CH * J * 64;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(v & 63); int64_t r = v >> 6;
    const int j = (int)(r % J); r /= J; const int ch = (int)(r % CH); r /= CH; const int cb = (int)(r % CB); const int k = (int)(r / CB);
    const int col = cb * 32 + (lane & 31), c0 = ch * 32 + (32 * j + 16 * (lane >> 5)) / EB;
    for (int e = 0; e < EPV; ++e) {
      const float x = w[((int64_t)col * K + k) * Cin + c0 + e];
      if (dtype == TL_F32) reinterpret_cast<float*>(o)[v * EPV + e] = x;
      else if (dtype == TL_F16) reinterpret_cast<_Float16*>(o)[v * EPV + e] = (_Float16)x;
      else reinterpret_cast<__hip_bfloat16*>(o)[v * EPV + e] = __float2bfloat16(x);
    }
  }
}

// Every conv weight of a model in ONE launch (training: the optimizer changes all of them each step; per-layer packing was ~210 launches).
// Workgroup b serves 4096 consecutive output elements of ONE descriptor (blocks[b] = {descriptor, first element}); forms: 0 = [K][Cout][Cin],
// 1 = fragment order (k_pack_weight_frag), 2 / 3 = the input-gradient layout [K][Cin][Cout] without / with flipped taps.
__global__ void __launch_bounds__(256) k_pack_batch(const tl_pack_desc* __restrict__ descs, const int2* __restrict__ blocks, int dtype) {
  const int2 bd = blocks[blockIdx.x];
  const tl_pack_desc d = descs[bd.x];
  const int64_t total = (int64_t)d.Cout * d.K * d.Cin;
  const int EB = dtype == TL_F32 ? 4 : 2, EPV = 16 / EB;
  for (int i = 0; i < 16; ++i) {
    const int64_t t = (int64_t)bd.y * 4096 + i * 256 + threadIdx.x;
    if (t >= total) break;
    float v;
    if (d.form == 0) {
      const int c = (int)(t % d.Cin); const int64_t r = t / d.Cin; const int j = (int)(r % d.Cout); const int k = (int)(r / d.Cout);
      v = d.src[((int64_t)j * d.K + k) * d.Cin + c];
    } else if (d.form == 1) {
      const int J = 32 * EB / 32, CB = d.Cout / 32, CH = d.Cin / 32;
      const int64_t vec = t / EPV; const int e = (int)(t % EPV);
      const int lane = (int)(vec & 63); int64_t r = vec >> 6;
      const int j = (int)(r % J); r /= J; const int ch = (int)(r % CH); r /= CH; const int cb = (int)(r % CB); const int k = (int)(r / CB);
      const int col = cb * 32 + (lane & 31), c0 = ch * 32 + (32 * j + 16 * (lane >> 5)) / EB;
      v = d.src[((int64_t)col * d.K + k) * d.Cin + c0 + e];
    } else {
      const int co = (int)(t % d.Cout); const int64_t r = t / d.Cout; const int ci = (int)(r % d.Cin); const int k = (int)(r / d.Cin);
      v = d.src[((int64_t)co * d.K + (d.form == 3 ? d.K - 1 - k : k)) * d.Cin + ci];
    }
    if (dtype == TL_F32) reinterpret_cast<float*>(d.dst)[t] = v;
    else if (dtype == TL_F16) reinterpret_cast<_Float16*>(d.dst)[t] = (_Float16)v;
    else reinterpret_cast<__hip_bfloat16*>(d.dst)[t] = __float2bfloat16(v);
  }
}

template <typename T>
__global__ void k_affine_relu(const T* __restrict__ in, int64_t in_ld, T* __restrict__ out, int64_t out_ld, int64_t n, int C,
                              const float* __restrict__ scale, const float* __restrict__ shift, int relu) {
  const int64_t total = n * C;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / C; const int c = (int)(t % C);
    float v = ld_elem(in + r * in_ld + c);
    if (scale) v = fmaf(v, scale[c], shift[c]);
    if (relu) v = fmaxf(v, 0.f);
    st_elem(out + r * out_ld + c, v);
  }
}

// The same over 8-channel vectors (C % 8 == 0, 16-B aligned rows): one 16-B (bf16) / two 16-B (f32) loads and stores per thread and
// step; the grid stride is a multiple of the vectors per row, so a thread keeps ONE channel group and its scale / shift live in
// registers (the scalar kernel above re-reads them per element and moves 2 bytes per load: 1.7 TB/s on the training step's 67 passes).
// T16: 0 = fp32 rows, 1 = bf16, 2 = IEEE half (this unit is compiled once: the half conversions are spelled out here)
template <int T16>
__global__ void __launch_bounds__(256) k_affine_relu_v8(const void* __restrict__ in, int64_t in_ld, void* __restrict__ out, int64_t out_ld, int64_t n, int C,
                                                        const float* __restrict__ scale, const float* __restrict__ shift, int relu) {
  const int vpr = C >> 3;
  const int64_t total = n * vpr, stride = (int64_t)gridDim.x * 256;
  int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= total) return;
  const int c0 = (int)(v % vpr) * 8;
  float sc[8], sh[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) { sc[q] = scale ? scale[c0 + q] : 1.f; sh[q] = scale ? shift[c0 + q] : 0.f; }
  for (; v < total; v += stride) {
    const int64_t r = v / vpr;
    float x[8];
    typedef _Float16 hx2 __attribute__((ext_vector_type(2)));
    if constexpr (T16 == 1) {
      const u32x4 q4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>((const uint16_t*)in + r * in_ld + c0));
#pragma unroll
      for (int q = 0; q < 4; ++q) { x[2 * q] = bf16_lo(q4[q]); x[2 * q + 1] = bf16_hi(q4[q]); }
    } else if constexpr (T16 == 2) {
      // (a plain 16-B load: with __builtin_nontemporal_load hipcc 7.0 fetched ONE dword here and fed all eight v_fma_mix from it)
      const u32x4 q4 = *reinterpret_cast<const u32x4*>((const uint16_t*)in + r * in_ld + c0);
      const uint32_t w0 = q4[0], w1 = q4[1], w2 = q4[2], w3 = q4[3];
      const uint32_t ws[4] = {w0, w1, w2, w3};
#pragma unroll
      for (int q = 0; q < 4; ++q) { const hx2 h = __builtin_bit_cast(hx2, ws[q]); x[2 * q] = (float)h[0]; x[2 * q + 1] = (float)h[1]; }
    } else {
      const f32x4* s4 = reinterpret_cast<const f32x4*>((const float*)in + r * in_ld + c0);
      const f32x4 a = __builtin_nontemporal_load(s4), b = __builtin_nontemporal_load(s4 + 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) { x[q] = a[q]; x[q + 4] = b[q]; }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) { x[q] = fmaf(x[q], sc[q], sh[q]); if (relu) x[q] = fmaxf(x[q], 0.f); }
    if constexpr (T16 == 1) {
      u32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = pack_bf16x2(x[2 * q], x[2 * q + 1]);
      *reinterpret_cast<u32x4*>((uint16_t*)out + r * out_ld + c0) = o;
    } else if constexpr (T16 == 2) {
      u32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) { const hx2 h = {(_Float16)x[2 * q], (_Float16)x[2 * q + 1]}; o[q] = __builtin_bit_cast(uint32_t, h); }
      *reinterpret_cast<u32x4*>((uint16_t*)out + r * out_ld + c0) = o;
    } else {
      f32x4* d = reinterpret_cast<f32x4*>((float*)out + r * out_ld + c0);
      d[0] = f32x4{x[0], x[1], x[2], x[3]}; d[1] = f32x4{x[4], x[5], x[6], x[7]};
    }
  }
}

}  // namespace

extern "C" {

int tl_pack_weight(const float* w_ref, int Cout, int K, int Cin, void* w_packed, int dtype, tl_stream_t stream) {
  if (!w_ref || !w_packed || Cout <= 0 || K <= 0 || Cin <= 0 || (dtype != TL_F32 && dtype != TL_BF16 && dtype != TL_F16)) return TL_ERR_ARG;
  return tl_launch<k_pack_weight>(tl_grid((int64_t)Cout * K * Cin, 256), 256, 0, tl_s(stream), w_ref, Cout, K, Cin, w_packed, dtype);
}

int64_t tl_pack_weight_x3_bytes(int Cout, int K, int Cin) {
  if (Cout <= 0 || K <= 0 || Cin <= 0 || Cin % 32) return -1;
  const int64_t one = (int64_t)K * Cout * Cin * 4;
  return (Cin < 256 && Cout % 32 == 0) ? 2 * one : one;
}

int tl_pack_weight_x3(const float* w_ref, int Cout, int K, int Cin, void* w_x3, tl_stream_t stream) {
  if (!w_ref || !w_x3 || Cout <= 0 || K <= 0 || Cin <= 0 || Cin % 32) return TL_ERR_ARG;
  return tl_launch<k_pack_weight_x3>(tl_grid((int64_t)Cout * K * Cin * 2, 256), 256, 0, tl_s(stream), w_ref, Cout, K, Cin, reinterpret_cast<uint16_t*>(w_x3));
}

int tl_pack_weight_dgrad(const float* w_ref, int Cout, int K, int Cin, int flip, void* w_t, int dtype, tl_stream_t stream) {
  if (!w_ref || !w_t || Cout <= 0 || K <= 0 || Cin <= 0 || (dtype != TL_F32 && dtype != TL_BF16 && dtype != TL_F16)) return TL_ERR_ARG;
  return tl_launch<k_pack_weight_dgrad>(tl_grid((int64_t)Cout * K * Cin, 256), 256, 0, tl_s(stream), w_ref, Cout, K, Cin, flip, w_t, dtype);
}

int tl_pack_weights_batch(const tl_pack_desc* descs, const int32_t* blocks, int64_t n_blocks, int dtype, tl_stream_t stream) {
  if (!descs || !blocks || n_blocks <= 0 || n_blocks > 0x7FFFFFFF || (dtype != TL_F32 && dtype != TL_BF16 && dtype != TL_F16)) return TL_ERR_ARG;
  return tl_launch<k_pack_batch>((unsigned)n_blocks, 256, 0, tl_s(stream), descs, reinterpret_cast<const int2*>(blocks), dtype);
}

int tl_pack_weight_frag(const float* w_ref, int Cout, int K, int Cin, void* w_frag, int dtype, tl_stream_t stream) {
  if (!w_ref || !w_frag || Cout <= 0 || K <= 0 || Cin <= 0 || Cout % 32 || Cin % 32 || (dtype != TL_F32 && dtype != TL_BF16 && dtype != TL_F16)) return TL_ERR_ARG;
  return tl_launch<k_pack_weight_frag>(tl_grid((int64_t)Cout * K * Cin / 8, 256), 256, 0, tl_s(stream), w_ref, Cout, K, Cin, w_frag, dtype);
}

int tl_affine_relu(const void* in, int64_t in_ld, void* out, int64_t out_ld, int64_t n, int C, int dtype, const float* scale,
                   const float* shift, int relu, tl_stream_t stream) {
  if (!in || !out || n <= 0 || C <= 0 || (scale == nullptr) != (shift == nullptr)) return TL_ERR_ARG;
  if ((dtype == TL_F32 || dtype == TL_BF16 || dtype == TL_F16) && C % 8 == 0 && in_ld % 8 == 0 && out_ld % 8 == 0 && ((uintptr_t)in) % 16 == 0 && ((uintptr_t)out) % 16 == 0) {
    const int vpr = C / 8;
    int64_t gv = tl_cdiv(n * vpr, 256 * 4);                      // about four vectors per thread, at most 16 workgroups per CU
    if (gv > 256 * 16) gv = 256 * 16;
    gv = tl_cdiv(gv * 256, (int64_t)vpr * 256) * vpr;           // grid * 256 must be a multiple of the vectors per row
    if (dtype == TL_BF16) return tl_launch<k_affine_relu_v8<1>>((unsigned)gv, 256, 0, tl_s(stream), in, in_ld, out, out_ld, n, C, scale, shift, relu);
    else if (dtype == TL_F16) return tl_launch<k_affine_relu_v8<2>>((unsigned)gv, 256, 0, tl_s(stream), in, in_ld, out, out_ld, n, C, scale, shift, relu);
    else return tl_launch<k_affine_relu_v8<0>>((unsigned)gv, 256, 0, tl_s(stream), in, in_ld, out, out_ld, n, C, scale, shift, relu);
  }
  const unsigned g = tl_grid(n * C, 256);
  if (dtype == TL_F32) return tl_launch<k_affine_relu<float>>(g, 256, 0, tl_s(stream), (const float*)in, in_ld, (float*)out, out_ld, n, C, scale, shift, relu);
  else if (dtype == TL_BF16) return tl_launch<k_affine_relu<__hip_bfloat16>>(g, 256, 0, tl_s(stream), (const __hip_bfloat16*)in, in_ld, (__hip_bfloat16*)out, out_ld, n, C, scale, shift, relu);
  else if (dtype == TL_F16) return tl_launch<k_affine_relu<_Float16>>(g, 256, 0, tl_s(stream), (const _Float16*)in, in_ld, (_Float16*)out, out_ld, n, C, scale, shift, relu);
  else return TL_ERR_ARG;
}

}  // extern "C"
