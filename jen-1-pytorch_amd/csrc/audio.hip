// Sample-rate and channel conversion of waveforms (include/jen1_hip.h: jen1_resample): the step in front of the Encodec encoder
// (generation.py:95 ``convert_audio``) and behind its decoder (``generate(output_sr=...)``).
//
// Polyphase windowed-sinc filter with o input samples and n output samples per frame (o / n = sr / target_sr in lowest terms):
//   y[j n + p] = sum_t taps[p][t] * xp[j o + first[p] + t],   xp[i] = x[i - w], zero outside [0, L)
// ``taps`` holds only the W taps of a phase that are not zero (the dense row has 2 w + o), so an output costs W multiply-adds.
//
// One workgroup owns one (row, tile of F frames).  It stages the tile's input window -- F o + 2 w samples, channel mix applied -- in LDS
// once, zeros where the window leaves [0, L), then every thread forms outputs m, m + 256, ... of the tile: consecutive lanes store
// consecutive floats.  The taps are read through L2 (the table is a few KB and shared by every workgroup).  Sums run in float32 in
// ascending tap order, one thread per output: the same bits on every run.
#include "common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE_OUTPUTS = 2048;     // F <= RS_TILE_OUTPUTS / n
constexpr int RS_TILE_INPUTS = 4096;      // F <= RS_TILE_INPUTS / o: bounds the LDS window when o >> n
constexpr int RS_MAX_LDS = 64 * 1024;

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at any float address

inline int rs_tile_frames(int o, int n) {
  int f = RS_TILE_OUTPUTS / n, g = RS_TILE_INPUTS / o;
  f = f < g ? f : g;
  return f < 1 ? 1 : f;
}

// CL = channels held in LDS: 2 only for stereo -> stereo; WT = W at compile time (0: the run-time value)
template <int CL, int WT>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ taps,
                                                              const int32_t* __restrict__ first, int c_in, int c_out, long long L,
                                                              long long L_out, int o, int n, int w, int W_rt, int F, int tiles, int win4) {
  extern __shared__ __attribute__((aligned(16))) float xs[];        // [CL][win4]
  const int W = WT ? WT : W_rt;
  const int tid = threadIdx.x;
  const long long row = blockIdx.x / tiles, j0 = (long long)(blockIdx.x % tiles) * F;
  const long long s0 = j0 * o - w;                                  // x index of window slot 0
  const float* xr = x + row * c_in * L;
  const bool mix = c_in == 2 && CL == 1;
  // ---- stage: four window slots per thread and pass; one 16-byte load per channel where all four lie inside [0, L)
  for (int q = tid * 4; q < win4; q += RS_THREADS * 4) {
    const long long i = s0 + q;
#pragma unroll
    for (int c = 0; c < CL; ++c) {
      const float* a = xr + (long long)c * L;
      float4 v;
      if (i >= 0 && i + 3 < L) {
        const f32x4u u = *reinterpret_cast<const f32x4u*>(a + i);
        v = make_float4(u[0], u[1], u[2], u[3]);
        if (mix) {
          const f32x4u r = *reinterpret_cast<const f32x4u*>(a + L + i);
          v = make_float4((v.x + r[0]) * 0.5f, (v.y + r[1]) * 0.5f, (v.z + r[2]) * 0.5f, (v.w + r[3]) * 0.5f);
        }
      } else {
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long long ik = i + k;
          const bool in = ik >= 0 && ik < L;
          e[k] = in ? a[ik] : 0.f;
          if (mix) e[k] = in ? (e[k] + a[L + ik]) * 0.5f : 0.f;
        }
        v = make_float4(e[0], e[1], e[2], e[3]);
      }
      *reinterpret_cast<float4*>(xs + c * win4 + q) = v;
    }
  }
  __syncthreads();
  // ---- outputs m = j0 n + ml, ml = tid, tid + 256, ...: (frame, phase) advance without a division per output
  const int K = 2 * w + o;
  const long long m0 = j0 * n;
  long long left = L_out - m0;
  const int count = (int)(left < (long long)F * n ? left : (long long)F * n);
  const int dj = RS_THREADS / n, dp = RS_THREADS % n;
  int jl = tid / n, p = tid % n;
  float* yr = y + row * c_out * L_out + m0;
  for (int ml = tid; ml < count; ml += RS_THREADS) {
    int f = first[p];
    f = f < 0 ? 0 : (f > K - W ? K - W : f);                        // a row of the table never leaves the window
    const float* h = taps + (long long)p * W;
    const float* s = xs + jl * o + f;
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int t = 0; t < W; ++t) {
      const float ht = h[t];
      acc0 = fmaf(ht, s[t], acc0);
      if (CL == 2) acc1 = fmaf(ht, s[win4 + t], acc1);
    }
    yr[ml] = acc0;
    if (CL == 2) yr[L_out + ml] = acc1;
    else if (c_out == 2) yr[L_out + ml] = acc0;                     // mono -> stereo: computed once, stored twice
    p += dp;
    jl += dj;
    if (p >= n) {
      p -= n;
      ++jl;
    }
  }
}

template <int CL>
void rs_launch(int WT, dim3 grid, size_t lds, hipStream_t st, const float* x, float* y, const float* taps, const int32_t* first, int c_in, int c_out,
               long long L, long long L_out, int o, int n, int w, int W, int F, int tiles, int win4) {
#define RS_GO(WC) \
  hipLaunchKernelGGL((resample_kernel<CL, WC>), grid, dim3(RS_THREADS), lds, st, x, y, taps, first, c_in, c_out, L, L_out, o, n, w, W, F, tiles, win4)
  switch (WT) {                       // the supports of the common rate pairs (13: every up-conversion, 14: 48 k -> 44.1 k, 25: 2 -> 1)
    case 13: RS_GO(13); break;
    case 14: RS_GO(14); break;
    case 25: RS_GO(25); break;
    default: RS_GO(0); break;
  }
#undef RS_GO
}

}  // namespace

extern "C" int jen1_resample(const float* x, float* y, const float* taps, const int32_t* first, int rows, int c_in, int c_out, int64_t L,
                             int64_t L_out, int o, int n, int w, int W, void* stream) {
  JEN1_CHECK(x != nullptr && y != nullptr && taps != nullptr && first != nullptr, "jen1_resample: null pointer");
  JEN1_CHECK(c_in == 1 || c_in == 2, "jen1_resample: c_in = %d, must be 1 or 2", c_in);
  JEN1_CHECK(c_out == 1 || c_out == 2, "jen1_resample: c_out = %d, must be 1 or 2", c_out);
  JEN1_CHECK(rows >= 0 && L >= 0 && o >= 1 && n >= 1 && w >= 0, "jen1_resample: bad shape (rows %d, L %lld, o %d, n %d, w %d)", rows, (long long)L, o, n, w);
  JEN1_CHECK(W >= 1 && W <= 2 * (long long)w + o, "jen1_resample: W = %d, must be in [1, 2 w + o = %lld]", W, 2 * (long long)w + o);
  JEN1_CHECK(L < (1ll << 40), "jen1_resample: L = %lld is too long", (long long)L);
  const long long want = ((long long)n * L + o - 1) / o;
  JEN1_CHECK(L_out == want, "jen1_resample: L_out = %lld, must be ceil(n L / o) = %lld", (long long)L_out, want);
  if (rows == 0 || L_out == 0) return 0;
  const int F = rs_tile_frames(o, n);
  const long long frames = (L_out + n - 1) / n, tiles = (frames + F - 1) / F;
  JEN1_CHECK(tiles * rows < (1ll << 31), "jen1_resample: %lld tiles x %d rows exceed the grid", tiles, rows);
  const int cl = (c_in == 2 && c_out == 2) ? 2 : 1;
  const long long win = (long long)F * o + 2ll * w, win4 = (win + 3) / 4 * 4;
  const long long lds = cl * win4 * (long long)sizeof(float);
  JEN1_CHECK(lds <= RS_MAX_LDS, "jen1_resample: the window of one frame (o = %d, w = %d) needs %lld bytes of LDS, more than %d", o, w, lds, RS_MAX_LDS);
  const dim3 grid((unsigned)(tiles * rows));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (cl == 2) rs_launch<2>(W, grid, (size_t)lds, st, x, y, taps, first, c_in, c_out, L, L_out, o, n, w, W, F, (int)tiles, (int)win4);
  else rs_launch<1>(W, grid, (size_t)lds, st, x, y, taps, first, c_in, c_out, L, L_out, o, n, w, W, F, (int)tiles, (int)win4);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_resample_tile_frames(int o, int n) { return (o >= 1 && n >= 1) ? rs_tile_frames(o, n) : 0; }
