// Spectral metrics of waveforms (include/jen1_spectral.h: jen1_stft, jen1_mel, jen1_spectral_distance): a framed, windowed real FFT in
// the layout of torch.stft, a banded filterbank on it, and the distance sums of the multi-resolution STFT loss.  Not in the reference.
//
// One workgroup of 1024 threads owns a tile of consecutive frames of one row and transforms them together in LDS with the tile FFT of
// spec_fft.h (in place, digit-reversed results, buffers of pitch n_fft + 1):
//   * Two real frames share one complex FFT of n_fft points: frame 2p is the real part and frame 2p + 1 the imaginary part of buffer p
//     (jen1_stft, jen1_mel), or the frame of x is the real and the same frame of y the imaginary part (jen1_spectral_distance).  They
//     come apart behind the transform as  A[k] = (Z[k] + conj Z[N - k]) / 2,  B[k] = (Z[k] - conj Z[N - k]) / 2i,  which needs no
//     twiddle.  A lone last frame is a pair whose imaginary part is zero.
//   * Frames are read with the reflect padding of center = 1 done on the index; the window (centred in the frame when shorter) is
//     applied on the way into LDS, and samples under the zero part of the window are not read at all.
//   * Everything that leaves LDS is indexed (bin or band, frame) with the frame fastest, so a wave stores runs of consecutive frames
//     of the [.., frames] output.
//
// The distance sums are float64: every thread adds its (bin, frame) terms in a fixed order, the workgroup reduces them in a fixed order (a halving tree
// across each wave, then the waves in turn) and writes three partials at its own slot; a second launch adds a row's partials the same way.  No
// atomics: the same bits on every run, and a row's sums do not depend on the other rows of the call.
#include <math.h>

#include "common.h"
#include "jen1_analysis.h"
#include "jen1_spectral.h"
#include "spec_fft.h"

namespace {

constexpr int SPEC_MAX_BANDS = 65536;

struct SpecBands {                 // a banded matrix in device memory
  const int32_t* lo;
  const int32_t* hi;
  const int32_t* off;
  const float* w;
  long long n_weights;
  int n_bands;
};

// sample i of frame `frame` of one row, windowed; 0 under the zero part of the window and for a frame past the last one
__device__ __forceinline__ float spec_sample(const float* __restrict__ row, const SpecFrame& f, long long frame, int i) {
  const int wi = i - f.left;
  if (wi < 0 || wi >= f.win || frame >= f.frames) return 0.f;
  long long s = frame * f.hop + i - f.pad;
  if (s < 0) s = -s;                                    // reflect (n > pad: one mirror is enough on either side)
  if (s >= f.n) s = 2 * (f.n - 1) - s;
  s = s < 0 ? 0 : (s >= f.n ? f.n - 1 : s);              // never outside the row, whatever the arguments
  return f.window[wi] * row[s];
}

// the two real transforms packed in buffer z at bin k: A from the real parts, B from the imaginary parts
__device__ __forceinline__ void spec_untangle(const float2* z, int k, int N, float2& A, float2& B) {
  const float2 z1 = z[spec_rev(k, N)], z2 = z[spec_rev((N - k) & (N - 1), N)];
  A = make_float2(0.5f * (z1.x + z2.x), 0.5f * (z1.y - z2.y));
  B = make_float2(0.5f * (z1.y + z2.y), 0.5f * (z2.x - z1.x));
}

__device__ __forceinline__ float spec_value(float2 X, int kind) {
  const float p = X.x * X.x + X.y * X.y;
  return kind == JEN1_SPEC_POWER ? p : sqrtf(p);
}

// frames [f0, f0 + 2 P) of one row into the P buffers: frame 2p real, frame 2p + 1 imaginary
__device__ __forceinline__ void spec_load_pairs(float2* buf, const float* __restrict__ xr, const SpecFrame& f, long long f0, int pitch) {
  float* bf = reinterpret_cast<float*>(buf);
  for (int e = threadIdx.x; e < 2 * f.P * f.N; e += SPEC_THREADS) {
    const int j = e >> f.logN, i = e & (f.N - 1);
    bf[((j >> 1) * pitch + i) * 2 + (j & 1)] = spec_sample(xr, f, f0 + j, i);
  }
  __syncthreads();
}

// (value of frame 2p, value of frame 2p + 1) -- or (value of x, value of y) -- of bin k, written over Z at spec_rev(k).  A thread
// reads Z at spec_rev(k) and spec_rev(N - k) and writes the first; N - k > N / 2 is nobody's k, so no thread reads what another writes.
__device__ __forceinline__ void spec_values_in_place(float2* buf, const SpecFrame& f, int kind, int pitch) {
  const int bins = f.N / 2 + 1;
  for (int e = threadIdx.x; e < bins * f.P; e += SPEC_THREADS) {
    const int p = e & (f.P - 1), k = e >> f.logP;
    float2* z = buf + p * pitch;
    float2 A, B;
    spec_untangle(z, k, f.N, A, B);
    z[spec_rev(k, f.N)] = make_float2(spec_value(A, kind), spec_value(B, kind));
  }
  __syncthreads();
}

// the clipped bin range of band b and the index of its first weight; false for an empty or ill-formed band
__device__ __forceinline__ bool spec_band(const SpecBands& B, int b, int bins, int& lo, int& hi, long long& w0) {
  const int lo0 = B.lo[b], hi0 = B.hi[b];
  const long long off = B.off[b];
  if (hi0 <= lo0 || off < 0 || off + ((long long)hi0 - lo0) > B.n_weights) return false;
  lo = lo0 < 0 ? 0 : lo0;
  hi = hi0 > bins ? bins : hi0;
  w0 = off - lo0;
  return hi > lo;
}

// fixed-order sum of three doubles over the workgroup: a halving tree across the lanes of every wave, then the waves in ascending
// order; thread 0 gets the result
__device__ __forceinline__ void spec_reduce3(double (&s)[3], double (*red)[SPEC_WAVES]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += __shfl_down(s[c], o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][threadIdx.x >> 6] = s[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double a = 0.0;
      for (int w = 0; w < SPEC_WAVES; ++w) a += red[c][w];
      s[c] = a;
    }
  }
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_stft_kernel(const float* __restrict__ x, long long row_stride, float* __restrict__ out,
                                                                 SpecFrame f, int kind, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  const long long row = blockIdx.x / tiles, f0 = (long long)(blockIdx.x % tiles) * (2 * f.P);
  const int pitch = f.N + 1, TF = 2 * f.P, bins = f.N / 2 + 1;
  spec_load_pairs(buf, x + row * row_stride, f, f0, pitch);
  spec_fft(buf, f.tw, f.N, f.logN, f.P, pitch);
  for (int e = threadIdx.x; e < bins * TF; e += SPEC_THREADS) {
    const int j = e & (TF - 1), k = e >> (f.logP + 1);
    const long long fr = f0 + j;
    if (fr >= f.frames) continue;
    float2 A, B;
    spec_untangle(buf + (j >> 1) * pitch, k, f.N, A, B);
    const float2 X = (j & 1) ? B : A;
    const long long o = (row * bins + k) * f.frames + fr;
    if (kind == JEN1_SPEC_COMPLEX)
      reinterpret_cast<float2*>(out)[o] = X;
    else
      out[o] = spec_value(X, kind);
  }
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_mel_kernel(const float* __restrict__ x, long long row_stride, float* __restrict__ out,
                                                                SpecFrame f, SpecBands B, int kind, int log_mode, float floor, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  const long long row = blockIdx.x / tiles, f0 = (long long)(blockIdx.x % tiles) * (2 * f.P);
  const int pitch = f.N + 1, TF = 2 * f.P, bins = f.N / 2 + 1;
  spec_load_pairs(buf, x + row * row_stride, f, f0, pitch);
  spec_fft(buf, f.tw, f.N, f.logN, f.P, pitch);
  spec_values_in_place(buf, f, kind, pitch);
  const float* bf = reinterpret_cast<const float*>(buf);
  for (int e = threadIdx.x; e < B.n_bands * TF; e += SPEC_THREADS) {
    const int j = e & (TF - 1), b = e >> (f.logP + 1);
    const long long fr = f0 + j;
    if (fr >= f.frames) continue;
    float acc = 0.f;
    int lo, hi;
    long long w0;
    if (spec_band(B, b, bins, lo, hi, w0)) {
      const float* zf = bf + (size_t)(j >> 1) * pitch * 2 + (j & 1);
      for (int k = lo; k < hi; ++k) acc = fmaf(B.w[w0 + k], zf[2 * spec_rev(k, f.N)], acc);
    }
    // the logarithms in float64, rounded once: a silent frame gives the float32 nearest to log(floor)
    if (log_mode == JEN1_SPEC_LOG_E) acc = (float)log((double)fmaxf(acc, floor));
    if (log_mode == JEN1_SPEC_LOG_DB) acc = (float)(10.0 * log10((double)fmaxf(acc, floor)));
    out[(row * B.n_bands + b) * f.frames + fr] = acc;
  }
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_distance_kernel(const float* __restrict__ x, long long x_stride, const float* __restrict__ y,
                                                                     long long y_stride, double* __restrict__ part, SpecFrame f, SpecBands B,
                                                                     int kind, float floor, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  __shared__ double red[3][SPEC_WAVES];
  const long long row = blockIdx.x / tiles, f0 = (long long)(blockIdx.x % tiles) * f.P;
  const int pitch = f.N + 1, bins = f.N / 2 + 1;
  const float* xr = x + row * x_stride;
  const float* yr = y + row * y_stride;
  for (int e = threadIdx.x; e < f.P * f.N; e += SPEC_THREADS) {
    const int p = e >> f.logN, i = e & (f.N - 1);
    buf[p * pitch + i] = make_float2(spec_sample(xr, f, f0 + p, i), spec_sample(yr, f, f0 + p, i));
  }
  __syncthreads();
  spec_fft(buf, f.tw, f.N, f.logN, f.P, pitch);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  if (B.n_bands == 0) {
    for (int e = threadIdx.x; e < bins * f.P; e += SPEC_THREADS) {
      const int p = e & (f.P - 1), k = e >> f.logP;
      if (f0 + p >= f.frames) continue;
      float2 X, Y;
      spec_untangle(buf + p * pitch, k, f.N, X, Y);
      const float mx = sqrtf(X.x * X.x + X.y * X.y), my = sqrtf(Y.x * Y.x + Y.y * Y.y);
      const double d = (double)mx - (double)my;
      s0 = fma(d, d, s0);
      s1 += (double)Y.x * (double)Y.x + (double)Y.y * (double)Y.y;
      s2 += (double)fabsf(logf(fmaxf(mx, floor) / fmaxf(my, floor)));      // one rounding in the quotient, then a log near its argument
    }
  } else {
    spec_values_in_place(buf, f, kind, pitch);
    for (int e = threadIdx.x; e < B.n_bands * f.P; e += SPEC_THREADS) {
      const int p = e & (f.P - 1), b = e >> f.logP;
      if (f0 + p >= f.frames) continue;
      float ax = 0.f, ay = 0.f;
      int lo, hi;
      long long w0;
      if (spec_band(B, b, bins, lo, hi, w0)) {
        const float2* z = buf + p * pitch;
        for (int k = lo; k < hi; ++k) {
          const float w = B.w[w0 + k];
          const float2 v = z[spec_rev(k, f.N)];
          ax = fmaf(w, v.x, ax);
          ay = fmaf(w, v.y, ay);
        }
      }
      const double d = (double)ax - (double)ay;
      s0 = fma(d, d, s0);
      s1 = fma((double)ay, (double)ay, s1);
      s2 += (double)fabsf(logf(fmaxf(ax, floor) / fmaxf(ay, floor)));
    }
  }
  double s[3] = {s0, s1, s2};
  spec_reduce3(s, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) part[(long long)blockIdx.x * 3 + c] = s[c];
  }
}

// out[row][c] = the row's partials [tiles][3] added in one fixed order
__global__ __launch_bounds__(SPEC_THREADS) void spec_distance_sum_kernel(const double* __restrict__ part, double* __restrict__ out, int tiles) {
  __shared__ double red[3][SPEC_WAVES];
  const double* pr = part + (long long)blockIdx.x * tiles * 3;
  const int t = threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = t; i < tiles; i += SPEC_THREADS) {
    s[0] += pr[i * 3LL + 0];
    s[1] += pr[i * 3LL + 1];
    s[2] += pr[i * 3LL + 2];
  }
  spec_reduce3(s, red);
  if (t == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(long long)blockIdx.x * 3 + c] = s[c];
  }
}

// ---- jen1_music_features (include/jen1_analysis.h).  A frame's values must not depend on its neighbours (the same bits whichever tile it
// falls in), so frames are not packed in pairs here: a real frame of N samples is N / 2 complex points z[m] = x[2m] + i x[2m+1] -- the
// frame as it lies in memory -- one transform of N / 2 points (the table of N at stride 2), and
//   X[k] = E[k] + W_N^k O[k],  X[N/2 - k] = conj(E[k] - W_N^k O[k]),  E, O = what spec_untangle gives at k of the N / 2 points.
// 2 P buffers of N / 2 + 1 float2 (the same bytes as the P buffers above, the same shift of one bank pair per buffer); a tile is 2 P
// consecutive frames, the first of which is only there for the flux of the second: tiles overlap by one frame.
constexpr int FEAT_LDS_MAX = 160 * 1024;
inline int feat_tile(int N) { return 2 * spec_pairs(N); }
inline size_t feat_buf_bytes(int N) { return (size_t)feat_tile(N) * (size_t)(N / 2 + 1) * sizeof(float2); }
inline size_t feat_part_bytes(int N) { return (size_t)SPEC_WAVES * 12 * feat_tile(N) * sizeof(double); }        // per wave [12][tile] chroma sums
inline size_t feat_lds_bytes(int N, int n_bands) { return feat_buf_bytes(N) + feat_part_bytes(N) + (size_t)feat_tile(N) * n_bands * sizeof(float); }
inline int feat_max_bands(int N) {
  const long long v = ((long long)FEAT_LDS_MAX - (long long)feat_buf_bytes(N) - (long long)feat_part_bytes(N)) / ((long long)feat_tile(N) * 4);
  return (int)(v > SPEC_MAX_BANDS ? SPEC_MAX_BANDS : v);
}

// spec_rev(k, 1 << logN) without the loop: the base-4 digits of the low bits in reverse order (a bit reversal, then the two bits of
// every digit swapped back), and with an odd logN the top bit of k last
__device__ __forceinline__ int feat_rev(int k, int logN) {
  const int m2 = logN & ~1;
  unsigned r = __builtin_bitreverse32((unsigned)k & ((1u << m2) - 1u)) >> (32 - m2);
  r = ((r & 0xAAAAAAAAu) >> 1) | ((r & 0x55555555u) << 1);
  return (logN & 1) ? (int)((r << 1) | ((unsigned)k >> m2)) : (int)r;
}

// where (|X[k]|^2, |X[k]|) of bin k in [0, N2] lies in a buffer of N2 = N / 2 points: bin N2 in the padding slot behind them
__device__ __forceinline__ int feat_pos(int k, int N2, int logN2) { return k == N2 ? N2 : feat_rev(k, logN2); }

__global__ __launch_bounds__(SPEC_THREADS) void spec_features_kernel(const float* __restrict__ x, long long row_stride, float* __restrict__ onset,
                                                                     float* __restrict__ chroma, const float* __restrict__ chroma_w, SpecFrame f,
                                                                     SpecBands B, float gamma, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  const int N2 = f.N >> 1, pitch = N2 + 1, TF = 2 * f.P, logTF = f.logP + 1, bins = N2 + 1;
  const int logN2 = f.logN - 1;
  double* part = reinterpret_cast<double*>(buf + (size_t)TF * pitch);                   // [waves][12][TF] partial chroma sums
  float* mel = reinterpret_cast<float*>(part + SPEC_WAVES * 12 * TF);                    // [n_bands][TF]
  const long long row = blockIdx.x / tiles, g0 = (long long)(blockIdx.x % tiles) * (TF - 1) - 1;      // frame of slot 0 (-1 in the first tile)
  const float* xr = x + row * row_stride;
  float* bf = reinterpret_cast<float*>(buf);
  for (int e = threadIdx.x; e < TF * f.N; e += SPEC_THREADS) {
    const int j = e >> f.logN, i = e & (f.N - 1);
    const long long g = g0 + j;
    bf[(size_t)j * pitch * 2 + i] = g < 0 ? 0.f : spec_sample(xr, f, g, i);
  }
  __syncthreads();
  spec_fft(buf, f.tw, N2, f.logN - 1, TF, pitch, 2);
  // bins k and N2 - k of slot j from the points k and N2 - k, written over them: a thread reads and writes only its own two slots
  for (int e = threadIdx.x; e < (N2 / 2 + 1) * TF; e += SPEC_THREADS) {
    const int j = e & (TF - 1), k = e >> logTF;
    float2* z = buf + j * pitch;
    float2 E, O;
    spec_untangle(z, k, N2, E, O);
    const float2 T = spec_cmul(O, f.tw[k]);
    const float pa = (E.x + T.x) * (E.x + T.x) + (E.y + T.y) * (E.y + T.y);
    const float pb = (E.x - T.x) * (E.x - T.x) + (E.y - T.y) * (E.y - T.y);
    z[spec_rev(k, N2)] = make_float2(pa, sqrtf(pa));
    if (k == 0)
      z[N2] = make_float2(pb, sqrtf(pb));
    else if (2 * k != N2)
      z[spec_rev(N2 - k, N2)] = make_float2(pb, sqrtf(pb));
  }
  __syncthreads();
  // Y[b][j] = log1p(gamma * sum_k w[b][k] |X[k]|): float64 sums, the logarithm in float64 rounded once
  for (int e = threadIdx.x; e < B.n_bands * TF; e += SPEC_THREADS) {
    const int j = e & (TF - 1), b = e >> logTF;
    double acc = 0.0;
    int lo, hi;
    long long w0;
    if (spec_band(B, b, bins, lo, hi, w0)) {
      const float2* z = buf + j * pitch;
      for (int k = lo; k < hi; ++k) acc = fma((double)B.w[w0 + k], (double)z[feat_pos(k, N2, logN2)].y, acc);
    }
    mel[e] = (float)log1p((double)gamma * acc);
  }
  // chroma: lane (frame j, group g) owns a run of consecutive bins and all twelve classes of it (runs, because neighbouring bins lie
  // n_fft / 8 apart after the digit reversal -- one bank pair -- while the starts of runs do not); a wave adds its groups frame by
  // frame in a halving tree, the waves follow in ascending order
  {
    const int j = threadIdx.x & (TF - 1), g = threadIdx.x >> logTF, G = SPEC_THREADS >> logTF, run = (bins + G - 1) / G;
    const float2* z = buf + j * pitch;
    const int k1 = min(bins, (g + 1) * run);
    double acc[12];
#pragma unroll
    for (int p = 0; p < 12; ++p) acc[p] = 0.0;
    for (int k = g * run; k < k1; ++k) {
      const double v = (double)z[feat_pos(k, N2, logN2)].x;
#pragma unroll
      for (int p = 0; p < 12; ++p) acc[p] = fma((double)chroma_w[(size_t)p * bins + k], v, acc[p]);
    }
#pragma unroll
    for (int p = 0; p < 12; ++p) {
      double v = acc[p];
      for (int o = 32; o >= TF; o >>= 1) v += __shfl_down(v, o);
      if ((threadIdx.x & 63) < TF) part[((threadIdx.x >> 6) * 12 + p) * TF + j] = v;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 12 * TF; e += SPEC_THREADS) {
    const int j = e & (TF - 1), p = e >> logTF;
    const long long g = g0 + j;
    if (j == 0 || g >= f.frames) continue;
    double acc = 0.0;
    for (int w = 0; w < SPEC_WAVES; ++w) acc += part[(w * 12 + p) * TF + j];
    chroma[(row * 12 + p) * f.frames + g] = (float)acc;
  }
  // the flux of slot j >= 1 against slot j - 1, the bands in ascending order
  if (threadIdx.x >= SPEC_THREADS - TF) {
    const int j = threadIdx.x - (SPEC_THREADS - TF);
    const long long g = g0 + j;
    if (j >= 1 && g < f.frames) {
      double acc = 0.0;
      if (g >= 1)
        for (int b = 0; b < B.n_bands; ++b) acc += (double)fmaxf(0.f, mel[b * TF + j] - mel[b * TF + j - 1]);
      onset[row * f.frames + g] = (float)(acc / (double)B.n_bands);
    }
  }
}

inline long long spec_frames(long long n, int N, int hop, int center) {
  if (!spec_nfft_ok(N) || hop < 1 || hop > N || (center != 0 && center != 1) || n < 1 || n >= (1ll << 40)) return -1;
  if (center) return n > N / 2 ? 1 + n / hop : -1;
  return n >= N ? 1 + (n - N) / hop : -1;
}

// the checks every entry point shares, and the framing they agree on
int spec_plan(const char* who, const void* x, const void* window, const void* twiddle, int rows, long long n, long long stride, int N, int hop,
              int win, int center, int frames_per_group, SpecFrame* f, long long* tiles) {
  JEN1_CHECK(spec_nfft_ok(N), "%s: n_fft = %d, must be 256, 512, 1024, 2048 or 4096", who, N);
  JEN1_CHECK(hop >= 1 && hop <= N, "%s: hop = %d, must be in [1, n_fft = %d]", who, hop, N);
  JEN1_CHECK(win >= 1 && win <= N, "%s: win_length = %d, must be in [1, n_fft = %d]", who, win, N);
  JEN1_CHECK(center == 0 || center == 1, "%s: center = %d, must be 0 or 1", who, center);
  JEN1_CHECK(rows >= 0 && n >= 1 && n < (1ll << 40), "%s: bad shape (rows %d, n %lld)", who, rows, n);
  JEN1_CHECK(stride >= n, "%s: row stride %lld is shorter than a row of n = %lld", who, stride, n);
  JEN1_CHECK(!center || n > N / 2, "%s: center = 1 needs n > n_fft / 2 for the reflect padding (n %lld, n_fft %d)", who, n, N);
  JEN1_CHECK(center || n >= N, "%s: center = 0 needs n >= n_fft (n %lld, n_fft %d)", who, n, N);
  JEN1_CHECK(x != nullptr && window != nullptr && twiddle != nullptr, "%s: null pointer", who);
  f->window = static_cast<const float*>(window);
  f->tw = static_cast<const float2*>(twiddle);
  f->n = n;
  f->frames = spec_frames(n, N, hop, center);
  f->N = N;
  f->logN = 0;
  while ((1 << f->logN) < N) ++f->logN;
  f->hop = hop;
  f->win = win;
  f->left = (N - win) / 2;
  f->pad = center ? N / 2 : 0;
  f->P = spec_pairs(N);
  f->logP = 0;
  while ((1 << f->logP) < f->P) ++f->logP;
  const long long per = (long long)frames_per_group * f->P;
  *tiles = (f->frames + per - 1) / per;
  JEN1_CHECK(*tiles * (rows > 0 ? rows : 1) < (1ll << 31), "%s: %lld tiles x %d rows exceed the grid", who, *tiles, rows);
  JEN1_CHECK((long long)rows * (N / 2 + 1) < (1ll << 40) / f->frames * (1ll << 20), "%s: the output is too large", who);
  return 0;
}

int spec_bands(const char* who, const int32_t* lo, const int32_t* hi, const int32_t* off, const float* w, int n_bands, long long n_weights,
               SpecBands* B) {
  JEN1_CHECK(n_bands >= 1 && n_bands <= SPEC_MAX_BANDS, "%s: n_bands = %d, must be in [1, %d]", who, n_bands, SPEC_MAX_BANDS);
  JEN1_CHECK(n_weights >= 1 && n_weights < (1ll << 31), "%s: n_weights = %lld is out of range", who, n_weights);
  JEN1_CHECK(lo != nullptr && hi != nullptr && off != nullptr && w != nullptr, "%s: null pointer (bands)", who);
  B->lo = lo;
  B->hi = hi;
  B->off = off;
  B->w = w;
  B->n_weights = n_weights;
  B->n_bands = n_bands;
  return 0;
}

}  // namespace

extern "C" int64_t jen1_stft_frames(int64_t n, int n_fft, int hop, int center) { return spec_frames(n, n_fft, hop, center); }

extern "C" int jen1_stft_tile_frames(int n_fft) { return spec_nfft_ok(n_fft) ? 2 * spec_pairs(n_fft) : 0; }

extern "C" int jen1_spectral_distance_tile_frames(int n_fft) { return spec_nfft_ok(n_fft) ? spec_pairs(n_fft) : 0; }

extern "C" int jen1_stft(const float* x, int64_t row_stride, float* out, const float* window, const float* twiddle, int rows, int64_t n, int n_fft,
                         int hop, int win_length, int center, int kind, void* stream) {
  SpecFrame f;
  long long tiles = 0;
  if (int rc = spec_plan("jen1_stft", x, window, twiddle, rows, n, row_stride, n_fft, hop, win_length, center, 2, &f, &tiles)) return rc;
  JEN1_CHECK(kind >= JEN1_SPEC_COMPLEX && kind <= JEN1_SPEC_POWER, "jen1_stft: kind = %d is not a JEN1_SPEC_* value", kind);
  JEN1_CHECK(out != nullptr, "jen1_stft: null pointer");
  JEN1_CHECK(kind != JEN1_SPEC_COMPLEX || (reinterpret_cast<uintptr_t>(out) & 7u) == 0, "jen1_stft: a complex output must be 8-byte aligned");
  if (rows == 0) return 0;
  JEN1_MAX_LDS_ONCE(spec_stft_kernel, SPEC_LDS_MAX);
  hipLaunchKernelGGL(spec_stft_kernel, dim3((unsigned)(tiles * rows)), dim3(SPEC_THREADS), spec_lds_bytes(n_fft), reinterpret_cast<hipStream_t>(stream),
                     x, (long long)row_stride, out, f, kind, (int)tiles);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_mel(const float* x, int64_t row_stride, float* out, const float* window, const float* twiddle, const int32_t* band_lo,
                        const int32_t* band_hi, const int32_t* band_off, const float* band_w, int n_bands, int64_t n_weights, int rows, int64_t n,
                        int n_fft, int hop, int win_length, int center, int kind, int log_mode, float floor, void* stream) {
  SpecFrame f;
  SpecBands B;
  long long tiles = 0;
  if (int rc = spec_plan("jen1_mel", x, window, twiddle, rows, n, row_stride, n_fft, hop, win_length, center, 2, &f, &tiles)) return rc;
  if (int rc = spec_bands("jen1_mel", band_lo, band_hi, band_off, band_w, n_bands, n_weights, &B)) return rc;
  JEN1_CHECK(kind == JEN1_SPEC_MAGNITUDE || kind == JEN1_SPEC_POWER, "jen1_mel: kind = %d, must be JEN1_SPEC_MAGNITUDE or JEN1_SPEC_POWER", kind);
  JEN1_CHECK(log_mode >= JEN1_SPEC_LOG_NONE && log_mode <= JEN1_SPEC_LOG_DB, "jen1_mel: log_mode = %d is not a JEN1_SPEC_LOG_* value", log_mode);
  JEN1_CHECK(log_mode == JEN1_SPEC_LOG_NONE || (floor > 0.f && isfinite(floor)), "jen1_mel: floor = %g, must be positive for a log mode", (double)floor);
  JEN1_CHECK(out != nullptr, "jen1_mel: null pointer");
  if (rows == 0) return 0;
  JEN1_MAX_LDS_ONCE(spec_mel_kernel, SPEC_LDS_MAX);
  hipLaunchKernelGGL(spec_mel_kernel, dim3((unsigned)(tiles * rows)), dim3(SPEC_THREADS), spec_lds_bytes(n_fft), reinterpret_cast<hipStream_t>(stream),
                     x, (long long)row_stride, out, f, B, kind, log_mode, floor, (int)tiles);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t jen1_spectral_distance_workspace_bytes(int rows, int64_t n, int n_fft, int hop, int center) {
  const long long frames = spec_frames(n, n_fft, hop, center);
  if (frames < 1 || rows < 0) return 0;
  const long long P = spec_pairs(n_fft), tiles = (frames + P - 1) / P;
  return (int64_t)((rows > 0 ? rows : 1) * tiles * 3 * (long long)sizeof(double));
}

extern "C" int jen1_spectral_distance(const float* x, int64_t x_stride, const float* y, int64_t y_stride, double* out, const float* window,
                                      const float* twiddle, const int32_t* band_lo, const int32_t* band_hi, const int32_t* band_off,
                                      const float* band_w, int n_bands, int64_t n_weights, int rows, int64_t n, int n_fft, int hop, int win_length,
                                      int center, int kind, float floor, void* workspace, int64_t workspace_bytes, void* stream) {
  SpecFrame f;
  SpecBands B = {nullptr, nullptr, nullptr, nullptr, 0, 0};
  long long tiles = 0;
  if (int rc = spec_plan("jen1_spectral_distance", x, window, twiddle, rows, n, x_stride, n_fft, hop, win_length, center, 1, &f, &tiles)) return rc;
  JEN1_CHECK(y != nullptr && out != nullptr && workspace != nullptr, "jen1_spectral_distance: null pointer");
  JEN1_CHECK(y_stride >= n, "jen1_spectral_distance: row stride %lld of y is shorter than a row of n = %lld", (long long)y_stride, (long long)n);
  JEN1_CHECK(n_bands >= 0, "jen1_spectral_distance: n_bands = %d is negative", n_bands);
  if (n_bands > 0) {
    if (int rc = spec_bands("jen1_spectral_distance", band_lo, band_hi, band_off, band_w, n_bands, n_weights, &B)) return rc;
    JEN1_CHECK(kind == JEN1_SPEC_MAGNITUDE || kind == JEN1_SPEC_POWER,
               "jen1_spectral_distance: kind = %d, must be JEN1_SPEC_MAGNITUDE or JEN1_SPEC_POWER with bands", kind);
  }
  JEN1_CHECK(floor > 0.f && isfinite(floor), "jen1_spectral_distance: floor = %g, must be positive", (double)floor);
  const long long need = (long long)(rows > 0 ? rows : 1) * tiles * 3 * (long long)sizeof(double);
  JEN1_CHECK(workspace_bytes >= need, "jen1_spectral_distance: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, need);
  JEN1_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "jen1_spectral_distance: workspace is not 8-byte aligned");
  if (rows == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  JEN1_MAX_LDS_ONCE(spec_distance_kernel, SPEC_LDS_MAX);
  hipLaunchKernelGGL(spec_distance_kernel, dim3((unsigned)(tiles * rows)), dim3(SPEC_THREADS), spec_lds_bytes(n_fft), s, x, (long long)x_stride, y,
                     (long long)y_stride, static_cast<double*>(workspace), f, B, kind, floor, (int)tiles);
  hipLaunchKernelGGL(spec_distance_sum_kernel, dim3((unsigned)rows), dim3(SPEC_THREADS), 0, s, static_cast<const double*>(workspace), out, (int)tiles);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_music_features_tile_frames(int n_fft) { return spec_nfft_ok(n_fft) ? feat_tile(n_fft) - 1 : 0; }

extern "C" int jen1_music_features_max_bands(int n_fft) { return spec_nfft_ok(n_fft) ? feat_max_bands(n_fft) : 0; }

extern "C" int jen1_music_features(const float* x, int64_t row_stride, float* onset, float* chroma, const float* window, const float* twiddle,
                                   const int32_t* band_lo, const int32_t* band_hi, const int32_t* band_off, const float* band_w, int n_bands,
                                   int64_t n_weights, const float* chroma_w, float gamma, int rows, int64_t n, int n_fft, int hop, int win_length,
                                   int center, void* stream) {
  SpecFrame f;
  SpecBands B;
  long long tiles = 0;
  if (int rc = spec_plan("jen1_music_features", x, window, twiddle, rows, n, row_stride, n_fft, hop, win_length, center, 2, &f, &tiles)) return rc;
  if (int rc = spec_bands("jen1_music_features", band_lo, band_hi, band_off, band_w, n_bands, n_weights, &B)) return rc;
  JEN1_CHECK(n_bands <= feat_max_bands(n_fft), "jen1_music_features: n_bands = %d, at most %d fit in LDS at n_fft = %d", n_bands, feat_max_bands(n_fft),
             n_fft);
  JEN1_CHECK(gamma > 0.f && isfinite(gamma), "jen1_music_features: gamma = %g, must be positive", (double)gamma);
  JEN1_CHECK(onset != nullptr && chroma != nullptr && chroma_w != nullptr, "jen1_music_features: null pointer");
  const long long per = feat_tile(n_fft) - 1;
  tiles = (f.frames + per - 1) / per;
  JEN1_CHECK(tiles * (rows > 0 ? rows : 1) < (1ll << 31), "jen1_music_features: %lld tiles x %d rows exceed the grid", tiles, rows);
  if (rows == 0) return 0;
  JEN1_MAX_LDS_ONCE(spec_features_kernel, FEAT_LDS_MAX);
  hipLaunchKernelGGL(spec_features_kernel, dim3((unsigned)(tiles * rows)), dim3(SPEC_THREADS), feat_lds_bytes(n_fft, n_bands),
                     reinterpret_cast<hipStream_t>(stream), x, (long long)row_stride, onset, chroma, chroma_w, f, B, gamma, (int)tiles);
  JEN1_HIP(hipGetLastError());
  return 0;
}
