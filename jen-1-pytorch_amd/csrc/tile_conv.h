// The arithmetic of the tile convolutions (gfx950 only) -- tile_gemm.hip, deep_kernel.hip's tile_unit, long_kernel.hip's long_unit -- between
// "the operands are here" and "store the result", and the normalisation finish of the other inference kernels.
//   norm_rstd        mean = s inv_count, var = max(q inv_count - mean^2, 0), returns 1 / sqrt(var + eps)
//   gn_affine        one entry of the prologue's table y = A x + S from a group's (sum, sumsq); film_affine: FiLM on top of the pair
//   fine_sum4        s, q += entries e[i0 .. i0 + cnt) in index order, four independent reads in flight
//   affine8, silu8, scale8, zero8   the steps of the staging prologue on a vector of 8 channels
//   subpixel_phase   GEMM row m = ph out_C + co of the sub-pixel form of ConvTranspose1d
//   sums4, rows4_sum the epilogue's (sum, sumsq) of a lane's 4 values; behind row16_sum, the wave's four rows in fixed order (uniform)
// Deliberate differences: tile_gemm applies SiLU also without GroupNorm and FiLM at table time, and pairs its statistics sums for atomics.
// The row map and the prologue's decision tree stay in each kernel: no stage_prologue8 (profiles/tile_conv_refactor.txt, section 3).
#pragma once
#include "common.h"

template <bool PRECISE>      // IEEE sqrt and division in the float32 parity mode, v_rsq otherwise
__device__ __forceinline__ float norm_rstd(float s, float q, float inv_count, float eps, float& mean) {
  mean = s * inv_count;
  float var = q * inv_count - mean * mean;
  var = var < 0.f ? 0.f : var;
  return PRECISE ? 1.0f / sqrtf(var + eps) : rsqrtf(var + eps);
}
// s, q: sums of the UNSCALED source; sc: the source's scale (src1_scale for the second source, else 1)
template <bool PRECISE>
__device__ __forceinline__ void gn_affine(float s, float q, float sc, float inv_count, float eps, float gamma, float beta, float& A, float& S) {
  s *= sc;
  q *= sc * sc;
  float mean;
  const float rstd = norm_rstd<PRECISE>(s, q, inv_count, eps, mean);
  A = rstd * gamma;
  S = beta - mean * A;
  A *= sc;
}
__device__ __forceinline__ void film_affine(float& A, float& S, float fs, float fh) {      // y <- y (1 + fs) + fh
  const float f1 = fs + 1.0f;
  A *= f1;
  S = S * f1 + fh;
}
__device__ __forceinline__ void fine_sum4(const float2* e, int i0, int cnt, float& s, float& q) {
  for (int i = 0; i < cnt; i += 4) {
    float2 e4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e4[j] = e[(i + j < cnt) ? i0 + i + j : i0];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s += (i + j < cnt) ? e4[j].x : 0.f;
      q += (i + j < cnt) ? e4[j].y : 0.f;
    }
  }
}

__device__ __forceinline__ void affine8(float (&x)[8], const float* A, const float* S) {
  const float4 a0 = *reinterpret_cast<const float4*>(A), a1 = *reinterpret_cast<const float4*>(A + 4);
  const float4 s0 = *reinterpret_cast<const float4*>(S), s1 = *reinterpret_cast<const float4*>(S + 4);
  x[0] = x[0] * a0.x + s0.x; x[1] = x[1] * a0.y + s0.y; x[2] = x[2] * a0.z + s0.z; x[3] = x[3] * a0.w + s0.w;
  x[4] = x[4] * a1.x + s1.x; x[5] = x[5] * a1.y + s1.y; x[6] = x[6] * a1.z + s1.z; x[7] = x[7] * a1.w + s1.w;
}
template <bool PRECISE>
__device__ __forceinline__ void silu8(float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = PRECISE ? silu_precise(x[j]) : silu_f(x[j]);
}
__device__ __forceinline__ void scale8(float (&x)[8], float s) {
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] *= s;
}
__device__ __forceinline__ void zero8(float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = 0.f;
}

__device__ __forceinline__ int subpixel_phase(int m, int out_C, int ps_f, int& co) {
  int ph = 0;
  for (int k = 1; k < ps_f; ++k) ph += (m >= k * out_C) ? 1 : 0;
  co = m - ph * out_C;
  return ph;
}

__device__ __forceinline__ void sums4(const float (&v)[4], float& gs, float& gq) {
  gs += (v[0] + v[1]) + (v[2] + v[3]);
  gq += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
}
__device__ __forceinline__ float rlane(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ float rows4_sum(float g) { return (rlane(g, 0) + rlane(g, 16)) + (rlane(g, 32) + rlane(g, 48)); }
