// The 16x16 MFMA fragment vocabulary of the GEMM, attention and persistent kernels (gfx950 only).
//
// Both operands of a 16x16 tile use one lane -> element map: lane l (i = l & 15, g = l >> 4) owns row i and the 8 consecutive K
// elements 8g .. 8g + 7 of a 32-deep K step -- 16 contiguous bytes of a bf16 row, 32 of a float32 row, 8 of an fp8 row.
#pragma once
#include "common.h"

// a lane's fragment of an operand of element type T
template <typename T> struct Frag8;
template <> struct Frag8<bf16_t> { typedef bf16x8 type; };
template <> struct Frag8<float> { typedef f32x8 type; };
template <> struct Frag8<fp8_t> { typedef long type; };

// acc += A B^T over one 32-deep K step (float32: eight exact 16x16x4 steps)
__device__ __forceinline__ void mma(f32x4& acc, const bf16x8& a, const bf16x8& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x4& acc, const f32x8& a, const f32x8& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x4& acc, const long& a, const long& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, acc, 0, 0, 0);
}

// a fragment from LDS
__device__ __forceinline__ void lds_frag(bf16x8& f, const bf16_t* p) { f = *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ void lds_frag(f32x8& f, const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w;
  f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
}
__device__ __forceinline__ void lds_frag(long& f, const fp8_t* p) { f = *reinterpret_cast<const long*>(p); }

constexpr unsigned OOB = 0x80000000u;     // per-lane offset beyond every descriptor range: loads return 0 and move no bytes
constexpr int RSRC_FLAGS = 0x00020000;    // word 3 of a raw buffer descriptor: DATA_FORMAT = 32 bit, every other field 0 (plain byte offsets)

// a fragment through a buffer descriptor: address = base + voff + soff.  AUX: the cache-policy immediate (0 = cached, 2 = nt: bytes
// that are used once per launch)
template <int AUX>
__device__ __forceinline__ void buf_frag(bf16x8& f, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  f = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX));
}
template <int AUX>
__device__ __forceinline__ void buf_frag(f32x8& f, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  const u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX);
  const u32x4 hi = __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16u, soff, AUX);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f.v[j] = __uint_as_float(lo[j]);
    f.v[4 + j] = __uint_as_float(hi[j]);
  }
}
template <int AUX>
__device__ __forceinline__ void buf_frag(long& f, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  f = __builtin_bit_cast(long, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, AUX));
}

__device__ __forceinline__ void frag_zero(bf16x8& f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (bf16_t)0.f;
}
__device__ __forceinline__ void frag_zero(f32x8& f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f.v[j] = 0.f;
}
__device__ __forceinline__ void frag_zero(long& f) { f = 0; }
