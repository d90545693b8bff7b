// Global conditioning (`features`, reference jen1/model/model.py:91-98, :204-223; jen1/conditioners.py:118-170), gfx950.
//   features_into_mapping   tf[r] += GELU(W_f feat[r % B] + b_f): the to_features branch summed into the time features, float32
//   film_select             rows [step B, step B + B) of the per-sample FiLM tables -> the B-row tables a sampler step reads
//   cond_embed              IntConditioner's embedding-row gather / NumberConditioner's clamp, normalise, Fourier features, Linear
#include "common.h"

namespace {

// one wavefront per output feature o: g[b] = GELU(w[o] . feat[b] + bias[o]) for every batch element, added to the rows r = b (mod B)
// of tf[rows][mf] (rows = B in the general forward, S * B in a sampler's table: row s B + b belongs to batch element b)
__global__ __launch_bounds__(256) void features_into_mapping_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, float* __restrict__ tf, int rows,
                                                                     int B, int F, int mf) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= mf) return;
  const float* wr = w + (size_t)o * F;
  const float bo = bias[o];
  for (int b = 0; b < B; ++b) {
    float s = 0.f;
    for (int i = lane; i < F; i += 64) s = fmaf(feat[(size_t)b * F + i], wr[i], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float g = gelu_erf(s + bo);
    for (long long r = b + (long long)lane * B; r < rows; r += 64ll * B) tf[(size_t)r * mf + o] += g;
  }
}

// blockIdx.y = which table; one float4 per thread.  The step counter is clamped into the table: a counter left behind the last step
// (the step kernel advances it) reads the last row block instead of memory behind the table.
__global__ __launch_bounds__(256) void film_select_kernel(const float4* __restrict__ film, const float4* __restrict__ film2,
                                                           float4* __restrict__ cur, float4* __restrict__ cur2,
                                                           const int32_t* __restrict__ step_idx, int n4, int n_steps) {
  int st = step_idx[0];
  st = st < 0 ? 0 : (st >= n_steps ? n_steps - 1 : st);
  const float4* src = (blockIdx.y ? film2 : film) + (size_t)st * n4;
  float4* dst = blockIdx.y ? cur2 : cur;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n4) dst[i] = src[i];
}

// IntConditioner: out[n] = table[clamp(x[n], lo, hi)] (the reference indexes with the clamped value itself, conditioners.py:131-134);
// the row index is also kept inside the table
__global__ __launch_bounds__(256) void cond_int_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                        float* __restrict__ out, int D, int rows, float lo, float hi) {
  const int n = blockIdx.x;
  float v = x[n];
  v = v < lo ? lo : (v > hi ? hi : v);
  int r = (int)v;
  r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
  for (int i = threadIdx.x; i < D; i += 256) out[(size_t)n * D + i] = table[(size_t)r * D + i];
}

// NumberConditioner: xn = (clamp(x, lo, hi) - lo) / (hi - lo); f = [xn, sin(2 pi xn w), cos(2 pi xn w)]; out = W f + bias
// (utils/module.py:58-79: the products in the reference's order x * w * 2 * pi)
__global__ __launch_bounds__(256) void cond_number_kernel(const float* __restrict__ x, const float* __restrict__ freq,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, int D, int half, float lo, float hi, float range) {
  extern __shared__ float feat[];   // [2 half + 1]
  const int n = blockIdx.x;
  float v = x[n];
  v = v < lo ? lo : (v > hi ? hi : v);
  const float xn = __fdiv_rn(__fsub_rn(v, lo), range);    // range = (float)(max_val - min_val), the difference formed in double by the caller
  const int nin = 2 * half + 1;
  for (int i = threadIdx.x; i < half; i += 256) {
    const float f = __fmul_rn(__fmul_rn(__fmul_rn(xn, freq[i]), 2.0f), 3.14159274101257324f);
    feat[1 + i] = sinf(f);
    feat[1 + half + i] = cosf(f);
  }
  if (threadIdx.x == 0) feat[0] = xn;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int o = wave; o < D; o += 4) {
    float s = 0.f;
    for (int i = lane; i < nin; i += 64) s = fmaf(feat[i], w[(size_t)o * nin + i], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[(size_t)n * D + o] = s + bias[o];
  }
}

}  // namespace

extern "C" int jen1_features_into_mapping(const float* feat, const float* w, const float* bias, float* tf, int rows, int B, int F, int mf,
                                          void* stream) {
  JEN1_CHECK(feat && w && bias && tf && B >= 1 && rows >= B && rows % B == 0 && F >= 1 && mf >= 1, "features_into_mapping: bad arguments");
  hipLaunchKernelGGL(features_into_mapping_kernel, dim3((mf + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), feat, w, bias, tf,
                     rows, B, F, mf);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_film_select(const float* film, const float* film2, float* film_cur, float* film2_cur, const int32_t* step_idx, int B,
                                int film_ld, int n_steps, void* stream) {
  JEN1_CHECK(film && film_cur && step_idx && B >= 1 && film_ld >= 4 && n_steps >= 1 && (film2 == nullptr) == (film2_cur == nullptr),
             "film_select: bad arguments");
  JEN1_CHECK(film_ld % 4 == 0 && (((uintptr_t)film | (uintptr_t)film2 | (uintptr_t)film_cur | (uintptr_t)film2_cur) & 15) == 0,
             "film_select: film_ld=%d must be a multiple of 4 and the tables 16-byte aligned", film_ld);
  JEN1_CHECK((int64_t)B * film_ld / 4 < ((int64_t)1 << 31) / 256 * 256, "film_select: %d rows of %d floats are too many", B, film_ld);
  const int n4 = B * (film_ld / 4);
  hipLaunchKernelGGL(film_select_kernel, dim3((n4 + 255) / 256, film2 ? 2 : 1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(film), reinterpret_cast<const float4*>(film2), reinterpret_cast<float4*>(film_cur),
                     reinterpret_cast<float4*>(film2_cur), step_idx, n4, n_steps);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_cond_embed(const float* x, int kind, const float* table, const float* freq, const float* bias, float* out, int n, int D,
                               int rows_or_half, float min_val, float max_val, float range, void* stream) {
  JEN1_CHECK(x && table && out && n >= 1 && D >= 1 && rows_or_half >= 1 && (kind == 0 || kind == 1), "cond_embed: bad arguments");
  JEN1_CHECK(max_val >= min_val, "cond_embed: max_val < min_val");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (kind == 0) {
    hipLaunchKernelGGL(cond_int_kernel, dim3(n), dim3(256), 0, s, x, table, out, D, rows_or_half, min_val, max_val);
  } else {
    JEN1_CHECK(freq && bias && max_val > min_val && range > 0.f && rows_or_half <= 4096,
               "cond_embed: the number form needs freq, bias, max_val > min_val, range > 0 and half <= 4096");
    hipLaunchKernelGGL(cond_number_kernel, dim3(n), dim3(256), sizeof(float) * (2 * rows_or_half + 1), s, x, freq, table, bias, out, D,
                       rows_or_half, min_val, max_val, range);
  }
  JEN1_HIP(hipGetLastError());
  return 0;
}
