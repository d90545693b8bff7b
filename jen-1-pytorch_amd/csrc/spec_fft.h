// The tile FFT shared by the kernels that transform frames in LDS (spectral.hip: jen1_stft, jen1_mel, jen1_spectral_distance,
// jen1_music_features; vocoder.hip: jen1_istft): the framing record of a launch, the in-place transform, and where its results lie.
//
//   * One workgroup of SPEC_THREADS threads transforms P buffers of n_fft complex floats together (P = 4 at n_fft >= 2048, 8 at 1024,
//     16 below: 128 KiB at 4096, 64 KiB or less otherwise).
//   * The FFT is decimation in frequency, radix 4 with one radix-2 stage at the end when log2 n_fft is odd, IN PLACE.  The result is in
//     digit-reversed order and stays there: whatever follows reads bin k at spec_rev(k), so no reordering pass and no second buffer.
//   * Twiddles come from the host's table (float64 cos / sin rounded once to float32), read through the cache; no fast-math sincos.
//
// LDS banks (64 dwords wide; a ds_read_b64 is served in two groups of 32 lanes, a float2 per lane and bank pair): a radix-4 butterfly
// with quarter span q reads float2 [base + s q], base = 4 (u - u % q) + u % q over consecutive lanes u.  q >= 32: consecutive float2,
// conflict-free.  q = 16: 2-way.  q = 4 and q = 1: 4-way.  The radix-2 tail: 2-way.  No stage is worse than 4-way, so the butterflies
// are not padded.  The pass BEHIND the transform is: lanes that differ in the frame read the same digit-reversed position of different
// buffers, and buffers n_fft float2 apart would all fall on one bank pair (up to 16-way).  Every buffer is therefore one float2 longer
// than n_fft (pitch n_fft + 1): buffer p is shifted by p bank pairs and the frames of a lane group are conflict-free.
#pragma once
#include "common.h"

namespace {

constexpr int SPEC_THREADS = 1024;         // 16 waves: with one workgroup per CU at n_fft = 4096 (128 KiB of LDS) still 4 waves per SIMD
constexpr int SPEC_WAVES = SPEC_THREADS / 64;

inline bool spec_nfft_ok(int N) { return N == 256 || N == 512 || N == 1024 || N == 2048 || N == 4096; }
inline int spec_pairs(int N) { return N >= 2048 ? 4 : N == 1024 ? 8 : 16; }
inline size_t spec_lds_bytes(int N) { return (size_t)spec_pairs(N) * (size_t)(N + 1) * sizeof(float2); }
constexpr int SPEC_LDS_MAX = 4 * (4096 + 1) * 8;

struct SpecFrame {                 // the framing of one launch
  const float* window;
  const float2* tw;
  long long n, frames;
  int N, logN, hop, win, left, pad, P, logP;
};

// where bin k of an N-point transform lies after the in-place stages (radix 4 from the top, radix 2 last)
__device__ __forceinline__ int spec_rev(int k, int N) {
  int p = 0, L = N;
  while (L >= 4) {
    L >>= 2;
    p += (k & 3) * L;
    k >>= 2;
  }
  if (L == 2) p += k & 1;
  return p;
}

__device__ __forceinline__ float2 spec_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// P transforms of N points, in place, buffer p at buf + p * pitch.  The caller has synchronised behind its stores; every stage ends
// with a barrier.  `tws`: the stride of the twiddle table (2: the table of 2 N points serves a transform of N).
__device__ __forceinline__ void spec_fft(float2* buf, const float2* __restrict__ tw, int N, int logN, int P, int pitch, int tws = 1) {
  const int quarter = N >> 2, logQ4 = logN - 2;
  int L = N;
  for (; L >= 4; L >>= 2) {
    const int q = L >> 2, tstep = N / L;
    for (int u = threadIdx.x; u < P * quarter; u += SPEC_THREADS) {
      const int p = u >> logQ4, r = u & (quarter - 1);
      const int j = r & (q - 1);
      float2* z = buf + p * pitch + ((r - j) << 2) + j;
      const float2 a0 = z[0], a1 = z[q], a2 = z[2 * q], a3 = z[3 * q];
      const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
      const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y);
      const float2 t3 = make_float2(a1.y - a3.y, a3.x - a1.x);                       // -i (a1 - a3)
      const int m = j * tstep * tws;
      z[0] = make_float2(t0.x + t2.x, t0.y + t2.y);
      z[q] = spec_cmul(make_float2(t1.x + t3.x, t1.y + t3.y), tw[m]);
      z[2 * q] = spec_cmul(make_float2(t0.x - t2.x, t0.y - t2.y), tw[2 * m]);
      z[3 * q] = spec_cmul(make_float2(t1.x - t3.x, t1.y - t3.y), tw[3 * m]);
    }
    __syncthreads();
  }
  if (L == 2) {
    const int half = N >> 1;
    for (int u = threadIdx.x; u < P * half; u += SPEC_THREADS) {
      const int p = u >> (logN - 1), r = u & (half - 1);
      float2* z = buf + p * pitch + 2 * r;
      const float2 a = z[0], b = z[1];
      z[0] = make_float2(a.x + b.x, a.y + b.y);
      z[1] = make_float2(a.x - b.x, a.y - b.y);
    }
    __syncthreads();
  }
}

}  // namespace
