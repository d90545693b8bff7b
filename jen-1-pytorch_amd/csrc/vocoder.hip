// The way back from a spectrogram and the map between two of them (include/jen1_vocoder.h: jen1_istft, jen1_phase_vocoder).  Not in the
// reference.
//
// jen1_istft is the gather form of the overlap-add, like jen1_codec_overlap_add: no atomics.  One workgroup of 1024 threads owns a run
// of R consecutive output samples of one row and inverse-transforms the frames whose windows touch the run, 2 P of them per pass with
// the tile FFT of spec_fft.h (frames a neighbouring run needs too are transformed again there: (R + n_fft) / R of the arithmetic):
//   * Two Hermitian spectra share one complex transform, Z = A + i B with Z[N - k] = conj A[k] + i conj B[k]: the real part of the
//     inverse is frame 2p and the imaginary part frame 2p + 1.  The imaginary parts of bins 0 and N / 2 are dropped, as irfft does.
//   * The inverse comes from the forward transform by conjugation, N ifft(Z) = conj fft(conj Z): conj Z goes into LDS, and sample i of
//     the pair is (z.x, -z.y) / N of z at spec_rev(i) -- the results stay in digit-reversed order, there is no reordering pass.
//   * Every output sample belongs to one thread, which adds w[i] x_t[i] of the frames t that reach it in ascending t, pass after pass,
//     into an LDS accumulator, and at the end divides by sum_t w^2 gathered over the same frames (float64).  A sample no frame reaches
//     has an empty sum and is written as an exact zero.
//   * LDS banks.  Consecutive samples of a frame lie n_fft / 4 float2 apart after the digit reversal -- one bank pair -- so the lanes of
//     a wave do not take consecutive samples while they read the transform: lane l takes sample l n_fft / 64 + c of an aligned block of
//     n_fft samples.  The top six bits of the sample index then differ from lane to lane, and those are the low six bits of its
//     position: no two lanes of a 32-lane group on one bank pair within a frame (read as a float2; 2-way if the compiler reads the one
//     float it needs, whose banks count modulo 32).  The accumulator is indexed s + s / 64 so that this stride (4 .. 64 floats) does
//     not fall on one bank either (at most 2-way); the final pass reads it with consecutive lanes on consecutive samples and stores
//     whole lines.
//   * LDS budget, against the 160 KiB of a CU (as FEAT_LDS_MAX in spectral.hip): the P buffers of pitch n_fft + 1 (128 KiB at 4096,
//     64 KiB otherwise) and the accumulator of R + R / 64 + 1 floats.  R is the largest power of two up to 8192 that fits: 8192 (32.5 KiB)
//     below n_fft = 4096 and 4096 there (8192 would miss the budget by 548 bytes).
//
// jen1_phase_vocoder: the phase of output frame j is phi_0 plus the sum of all phase advances in front of it, the only sequential part.
// One wave owns a (row, bin) and walks its output frames 64 at a time, a lane per frame: the lane forms its frame's magnitude and
// phase advance from the two input frames around tau_j = j rate in float64 (atan2, not fast-math), turns the advance into a 64-bit
// fixed-point fraction of a turn, and the wave adds the fractions with an inclusive scan of shuffles; the sum of a step is carried into
// the next.  Integer addition modulo 2^64 IS addition of turns modulo 1, exact and associative: the phase has the same bits on every run
// and in every scan order, and it does not grow with the frame count (a float32 sum of radians has lost the phase after a hundred
// frames at 800 rad per frame).  Both the input ([.., frames] with the frame fastest) and the output are touched in runs.
#include <math.h>

#include "common.h"
#include "jen1_vocoder.h"
#include "spec_fft.h"

namespace {

constexpr int VOC_LDS_MAX = 160 * 1024;
constexpr int VOC_RUN_MAX = 8192;
constexpr int PV_THREADS = 256;           // four waves, a (row, bin) each
constexpr int PV_STEP = 64;               // output frames per step of the scan: a wave

__host__ __device__ inline size_t voc_acc_floats(int R) { return (size_t)R + (size_t)(R >> 6) + 1; }
inline size_t voc_lds_bytes(int N, int R) { return spec_lds_bytes(N) + voc_acc_floats(R) * sizeof(float); }
inline int voc_run(int N) {
  int R = VOC_RUN_MAX;
  while (R > N && voc_lds_bytes(N, R) > (size_t)VOC_LDS_MAX) R >>= 1;
  return R;
}

struct IstftArgs {
  const float2* spec;
  float* out;
  const float* window;
  const float2* tw;
  long long out_stride, frames, length;
  int N, logN, hop, win, left, pad, P, logP, R, runs;
};

__host__ __device__ __forceinline__ long long voc_floordiv(long long a, long long b) {        // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

__device__ __forceinline__ int voc_acc_index(int s) { return s + (s >> 6); }

__global__ __launch_bounds__(SPEC_THREADS) void voc_istft_kernel(IstftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float2 buf[];
  const int N = a.N, pitch = N + 1, TF = 2 * a.P, bins = N / 2 + 1, half = N >> 1;
  float* acc = reinterpret_cast<float*>(buf + (size_t)a.P * pitch);
  const long long row = blockIdx.x / a.runs, s0 = (long long)(blockIdx.x % a.runs) * a.R;
  const long long u0 = s0 + a.pad;                                     // the run in the coordinates of the frames
  const long long rest = a.length - s0;
  const int R = rest < a.R ? (int)rest : a.R;
  const long long reach = (long long)a.left + a.win;                    // frame t holds the window on [t hop + left, t hop + reach)
  long long t_lo = voc_floordiv(u0 - reach, a.hop) + 1, t_hi = voc_floordiv(u0 + R - 1 - a.left, a.hop);
  if (t_lo < 0) t_lo = 0;
  if (t_hi > a.frames - 1) t_hi = a.frames - 1;
  const float2* sp = a.spec + row * bins * a.frames;
  const float inv = 1.0f / (float)N;
  for (int e = threadIdx.x; e < (int)voc_acc_floats(a.R); e += SPEC_THREADS) acc[e] = 0.f;
  for (long long f0 = t_lo; f0 <= t_hi; f0 += TF) {
    // conj Z of the pairs (f0 + 2p, f0 + 2p + 1) into buffer p; a frame past the last one is zero
    for (int e = threadIdx.x; e < bins * a.P; e += SPEC_THREADS) {
      const int p = e & (a.P - 1), k = e >> a.logP;
      const long long t = f0 + 2 * p;
      const float2* sk = sp + (long long)k * a.frames;
      float2 A = make_float2(0.f, 0.f), B = A;
      if (t < a.frames) A = sk[t];
      if (t + 1 < a.frames) B = sk[t + 1];
      float2* z = buf + p * pitch;
      if (k == 0 || k == half) {
        z[k] = make_float2(A.x, -B.x);
      } else {
        z[k] = make_float2(A.x - B.y, -(A.y + B.x));
        z[N - k] = make_float2(A.x + B.y, A.y - B.x);
      }
    }
    __syncthreads();
    spec_fft(buf, a.tw, N, a.logN, a.P, pitch);
    const long long f1 = (f0 + TF - 1 < t_hi) ? f0 + TF - 1 : t_hi;
    for (int e = threadIdx.x; e < a.R; e += SPEC_THREADS) {
      const int w = e & (N - 1);
      const int s = (e - w) + (w & 63) * (N >> 6) + (w >> 6);
      if (s >= R) continue;
      const long long u = u0 + s;
      long long ta = voc_floordiv(u - reach, a.hop) + 1, tb = voc_floordiv(u - a.left, a.hop);
      if (ta < f0) ta = f0;
      if (tb > f1) tb = f1;
      if (tb < ta) continue;
      float v = acc[voc_acc_index(s)];
      for (long long t = ta; t <= tb; ++t) {
        const int i = (int)(u - t * a.hop), j = (int)(t - f0);           // i in [left, left + win), j in [0, 2 P)
        const float2 z = buf[(j >> 1) * pitch + spec_rev(i, N)];
        v = fmaf(a.window[i - a.left], ((j & 1) ? -z.y : z.x) * inv, v);
      }
      acc[voc_acc_index(s)] = v;
    }
    __syncthreads();
  }
  __syncthreads();
  float* orow = a.out + row * a.out_stride + s0;
  for (int s = threadIdx.x; s < R; s += SPEC_THREADS) {
    const long long u = u0 + s;
    long long ta = voc_floordiv(u - reach, a.hop) + 1, tb = voc_floordiv(u - a.left, a.hop);
    if (ta < 0) ta = 0;
    if (tb > a.frames - 1) tb = a.frames - 1;
    double env = 0.0;
    for (long long t = ta; t <= tb; ++t) {
      const double w = (double)a.window[(int)(u - t * a.hop) - a.left];
      env = fma(w, w, env);
    }
    orow[s] = env > 0.0 ? (float)((double)acc[voc_acc_index(s)] / env) : 0.f;
  }
}

// ---- phase vocoder
__device__ __forceinline__ double pv_turns(float2 X) {                   // arg X in turns; arg 0 = 0
  return (X.x == 0.f && X.y == 0.f) ? 0.0 : atan2((double)X.y, (double)X.x) * 0.15915494309189533577;
}

// a number of turns modulo 1 as a 64-bit fixed-point fraction (2^-62 of a turn is below what a double in [-1/2, 1/2] resolves)
__device__ __forceinline__ unsigned long long pv_fix(double turns) {
  turns -= rint(turns);
  return ((unsigned long long)llrint(turns * 4611686018427387904.0)) << 2;
}

__global__ __launch_bounds__(PV_THREADS) void voc_phase_kernel(const float2* __restrict__ spec, float2* __restrict__ out, long long pairs, long long T,
                                                               long long J, int bins, int N, int hop, double rate) {
  const long long wave = (long long)blockIdx.x * (PV_THREADS / 64) + (threadIdx.x >> 6);
  if (wave >= pairs) return;                                            // a whole wave
  const int lane = threadIdx.x & 63, k = (int)(wave % bins);
  const float2* sp = spec + wave * T;
  float2* op = out + wave * J;
  const double af = (double)(((long long)hop * k) % N) / (double)N;     // the expected advance in turns, modulo 1: exact
  unsigned long long carry = pv_fix(pv_turns(sp[0]));
  for (long long j0 = 0; j0 < J; j0 += PV_STEP) {
    const long long j = j0 + lane;
    unsigned long long d = 0ull;
    double mag = 0.0;
    if (j < J) {
      const double tau = (double)j * rate;
      long long i = (long long)floor(tau);
      if (i > T - 1) i = T - 1;                                         // j rate < T holds for every j < J; never outside the row anyway
      const double alpha = tau - (double)i;
      const float2 X0 = sp[i], X1 = i + 1 < T ? sp[i + 1] : make_float2(0.f, 0.f);
      const double m0 = sqrt((double)X0.x * (double)X0.x + (double)X0.y * (double)X0.y);
      const double m1 = sqrt((double)X1.x * (double)X1.x + (double)X1.y * (double)X1.y);
      mag = alpha * m1 + (1.0 - alpha) * m0;
      double dd = pv_turns(X1) - pv_turns(X0) - af;
      dd -= rint(dd);
      d = pv_fix(dd + af);
    }
    unsigned long long s = d;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long v = __shfl_up(s, o);
      if (lane >= o) s += v;
    }
    const unsigned long long phase = carry + (s - d);                   // phi_0 + the advances in front of frame j
    carry += __shfl(s, 63);
    if (j < J) {
      double sn, cs;
      sincospi(2.0 * ((double)(long long)phase * 5.42101086242752217e-20), &sn, &cs);      // 2^-64: turns in [-1/2, 1/2)
      op[j] = make_float2((float)(mag * cs), (float)(mag * sn));
    }
  }
}

long long voc_frames(long long T, double rate) {
  if (T < 1 || !(rate > 0.0) || !isfinite(rate)) return -1;
  const double q = ceil((double)T / rate);
  if (!(q < 2147483648.0)) return -1;
  long long J = (long long)q;
  if (J < 1) J = 1;
  while (J > 1 && (double)(J - 1) * rate >= (double)T) --J;
  while ((double)J * rate < (double)T) ++J;
  return J < (1ll << 31) ? J : -1;
}

// sum_t w^2 at position u of the frames' coordinates, float64
double voc_envelope(const float* w, int win, int left, int hop, long long frames, long long u) {
  long long ta = voc_floordiv(u - left - win, hop) + 1, tb = voc_floordiv(u - left, hop);
  if (ta < 0) ta = 0;
  if (tb > frames - 1) tb = frames - 1;
  double env = 0.0;
  for (long long t = ta; t <= tb; ++t) {
    const double v = (double)w[u - t * hop - left];
    env += v * v;
  }
  return env;
}

// the least envelope over [lo, hi): both ends sample by sample; between them every frame that could reach a sample exists, the
// envelope has period hop, and one period stands for all
double voc_envelope_min(const float* w, int N, int win, int left, int hop, long long frames, long long lo, long long hi) {
  double least = INFINITY;
  const long long in0 = N, in1 = (frames - 1) * hop;                     // [in0, in1): the periodic part
  for (long long u = lo; u < hi; ++u) {
    if (u >= in0 + hop && u < in1) {
      u = in1 - 1;
      continue;
    }
    const double e = voc_envelope(w, win, left, hop, frames, u);
    if (e < least) least = e;
  }
  return least;
}

}  // namespace

extern "C" int jen1_istft_tile_samples(int n_fft) { return spec_nfft_ok(n_fft) ? voc_run(n_fft) : 0; }

extern "C" int jen1_istft_tile_frames(int n_fft) { return spec_nfft_ok(n_fft) ? 2 * spec_pairs(n_fft) : 0; }

extern "C" int jen1_istft(const float* spec, float* out, int64_t out_stride, const float* window, const float* window_host, const float* twiddle,
                          int rows, int64_t frames, int64_t length, int n_fft, int hop, int win_length, int center, void* stream) {
  const int N = n_fft;
  JEN1_CHECK(spec_nfft_ok(N), "jen1_istft: n_fft = %d, must be 256, 512, 1024, 2048 or 4096", N);
  JEN1_CHECK(hop >= 1 && hop <= N, "jen1_istft: hop = %d, must be in [1, n_fft = %d]", hop, N);
  JEN1_CHECK(win_length >= 1 && win_length <= N, "jen1_istft: win_length = %d, must be in [1, n_fft = %d]", win_length, N);
  JEN1_CHECK(center == 0 || center == 1, "jen1_istft: center = %d, must be 0 or 1", center);
  JEN1_CHECK(rows >= 0 && frames >= 1 && frames < (1ll << 31), "jen1_istft: bad shape (rows %d, frames %lld)", rows, (long long)frames);
  JEN1_CHECK(length >= 1 && length < (1ll << 40), "jen1_istft: length = %lld is too short or too long, must be in [1, 2^40)", (long long)length);
  JEN1_CHECK(out_stride >= length, "jen1_istft: row stride %lld is shorter than a row of length = %lld", (long long)out_stride, (long long)length);
  JEN1_CHECK(spec != nullptr && out != nullptr && window != nullptr && window_host != nullptr && twiddle != nullptr, "jen1_istft: null pointer");
  JEN1_CHECK((reinterpret_cast<uintptr_t>(spec) & 7u) == 0, "jen1_istft: a complex input must be 8-byte aligned");
  JEN1_CHECK((long long)rows * (N / 2 + 1) < (1ll << 40) / frames * (1ll << 20), "jen1_istft: the input is too large");
  IstftArgs a;
  a.spec = reinterpret_cast<const float2*>(spec);
  a.out = out;
  a.window = window;
  a.tw = reinterpret_cast<const float2*>(twiddle);
  a.out_stride = out_stride;
  a.frames = frames;
  a.length = length;
  a.N = N;
  a.logN = 0;
  while ((1 << a.logN) < N) ++a.logN;
  a.hop = hop;
  a.win = win_length;
  a.left = (N - win_length) / 2;
  a.pad = center ? N / 2 : 0;
  a.P = spec_pairs(N);
  a.logP = 0;
  while ((1 << a.logP) < a.P) ++a.logP;
  a.R = voc_run(N);
  // NOLA over the samples the frames reach: [pad, pad + length) cut at n_fft + hop (frames - 1)
  const long long held = (long long)N + (long long)hop * (frames - 1);
  const long long lo = a.pad, hi = a.pad + length < held ? a.pad + length : held;
  JEN1_CHECK(hi > lo, "jen1_istft: center = 1 trims n_fft / 2 = %d samples and the %lld frames hold only %lld", a.pad, (long long)frames, held);
  const double least = voc_envelope_min(window_host, N, a.win, a.left, hop, frames, lo, hi);
  JEN1_CHECK(least > 1e-11,
             "jen1_istft: the window does not overlap-add to a non-zero envelope (NOLA): the least sum of w^2 over the %lld samples the frames "
             "reach is %g (win_length %d, hop %d)", hi - lo, least, win_length, hop);
  const long long runs = (length + a.R - 1) / a.R;
  JEN1_CHECK(runs * (rows > 0 ? rows : 1) < (1ll << 31), "jen1_istft: %lld runs x %d rows exceed the grid", runs, rows);
  a.runs = (int)runs;
  if (rows == 0) return 0;
  JEN1_MAX_LDS_ONCE(voc_istft_kernel, VOC_LDS_MAX);
  hipLaunchKernelGGL(voc_istft_kernel, dim3((unsigned)(runs * rows)), dim3(SPEC_THREADS), voc_lds_bytes(N, a.R), reinterpret_cast<hipStream_t>(stream), a);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t jen1_vocoder_frames(int64_t frames, double rate) { return voc_frames(frames, rate); }

extern "C" int jen1_phase_vocoder_tile_frames(void) { return PV_STEP; }

extern "C" int jen1_phase_vocoder(const float* spec, float* out, int rows, int64_t frames, int n_fft, int hop, double rate, void* stream) {
  JEN1_CHECK(spec_nfft_ok(n_fft), "jen1_phase_vocoder: n_fft = %d, must be 256, 512, 1024, 2048 or 4096", n_fft);
  JEN1_CHECK(hop >= 1 && hop <= n_fft, "jen1_phase_vocoder: hop = %d, must be in [1, n_fft = %d]", hop, n_fft);
  JEN1_CHECK(rate > 0.0 && isfinite(rate), "jen1_phase_vocoder: rate = %g, must be positive and finite", rate);
  JEN1_CHECK(rows >= 0 && frames >= 1 && frames < (1ll << 31), "jen1_phase_vocoder: bad shape (rows %d, frames %lld)", rows, (long long)frames);
  const long long J = voc_frames(frames, rate);
  JEN1_CHECK(J >= 1, "jen1_phase_vocoder: rate = %g gives too many frames from %lld", rate, (long long)frames);
  JEN1_CHECK(spec != nullptr && out != nullptr, "jen1_phase_vocoder: null pointer");
  JEN1_CHECK(((reinterpret_cast<uintptr_t>(spec) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0, "jen1_phase_vocoder: complex tensors must be 8-byte aligned");
  const long long pairs = (long long)rows * (n_fft / 2 + 1);
  JEN1_CHECK(pairs < (1ll << 40) / (frames > J ? frames : J), "jen1_phase_vocoder: the tensors are too large");
  const long long blocks = (pairs + PV_THREADS / 64 - 1) / (PV_THREADS / 64);
  JEN1_CHECK(blocks < (1ll << 31), "jen1_phase_vocoder: %lld workgroups exceed the grid", blocks);
  if (rows == 0) return 0;
  hipLaunchKernelGGL(voc_phase_kernel, dim3((unsigned)blocks), dim3(PV_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float2*>(spec), reinterpret_cast<float2*>(out), pairs, (long long)frames, J, n_fft / 2 + 1, n_fft, hop, rate);
  JEN1_HIP(hipGetLastError());
  return 0;
}
