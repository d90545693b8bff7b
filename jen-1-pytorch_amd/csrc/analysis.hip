// Tempo and key estimators (include/jen1_analysis.h: jen1_tempo, jen1_key) on the onset envelope and the chromagram that
// jen1_music_features (csrc/spectral.hip) forms.  Not in the reference.
//
// Every sum over time is float64 in one fixed order: a lane adds its frames (64 apart) in ascending order, the
// lanes of a wave are added by a halving tree, and where a sum spans the workgroup the waves follow in ascending order.  No atomics, no
// host synchronisation, and nothing a row computes depends on the other rows of the call.  Frames behind frames[r] are never read.
//   jen1_tempo  eight workgroups per row share the lags: each forms the mean, then a wave the autocorrelation at one lag at a time
//               (the row is read through the cache: at 300 s it is 110 KiB and every lag walks it once), into the workspace; a
//               second launch forms the weighted values and picks: a few hundred float64 operations and one thread's scan
//   jen1_key    wave p adds class p; 24 lanes form the 24 correlations, one lane picks the key
#include <math.h>

#include "common.h"
#include "jen1_analysis.h"

namespace {

constexpr int AN_THREADS = 1024;
constexpr int AN_WAVES = AN_THREADS / 64;
constexpr int AN_MAX_LAGS = 2048;        // a float64 array of it in LDS

__device__ __forceinline__ double an_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;                                   // lane 0 has the sum
}

// ceil(60 fps / bpm_max), floor(60 fps / bpm_min): the same expressions on host and device
__host__ __device__ inline long long an_lag_min(double fps, double bpm_max) { return (long long)ceil(60.0 * fps / bpm_max); }
__host__ __device__ inline long long an_lag_max(double fps, double bpm_min) { return (long long)floor(60.0 * fps / bpm_min); }

constexpr int AN_SPLIT = 8;          // workgroups that share the lags of one row

// r[row][i] at lag lag0 + i for i < lags, r[row][lags] at lag 0.  Workgroup `part` of a row forms the lags part * 16 + wave, then
// AN_SPLIT * 16 further on; every one of them forms the mean itself, in the same order, so a lag's bits do not depend on the split.
__global__ __launch_bounds__(AN_THREADS) void an_acf_kernel(const float* __restrict__ onset, long long frame_stride, const int32_t* __restrict__ frames,
                                                            double* __restrict__ r, double* __restrict__ acf, int lag0, int lags) {
  __shared__ double red[AN_WAVES];
  const int row = blockIdx.x / AN_SPLIT, part = blockIdx.x % AN_SPLIT, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* u = onset + (long long)row * frame_stride;
  long long F = frames ? (long long)frames[row] : frame_stride;
  F = F < 0 ? 0 : (F > frame_stride ? frame_stride : F);
  double sum = 0.0;
  for (long long t = threadIdx.x; t < F; t += AN_THREADS) sum += (double)u[t];
  sum = an_wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  double mean = 0.0;
  for (int w = 0; w < AN_WAVES; ++w) mean += red[w];
  mean = F > 0 ? mean / (double)F : 0.0;
  for (int i = part * AN_WAVES + wave; i <= lags; i += AN_SPLIT * AN_WAVES) {
    const long long l = i == lags ? 0 : lag0 + i;
    double acc = 0.0;
    for (long long t = lane; t + l < F; t += 64) acc = fma((double)u[t] - mean, (double)u[t + l] - mean, acc);
    acc = an_wave_sum(acc);
    if (lane == 0) {
      r[(long long)row * (lags + 1) + i] = acc;
      if (acf != nullptr && i < lags) acf[(long long)row * lags + i] = acc;
    }
  }
}

// the weighted values, the arg max and the parabola of one row
__global__ __launch_bounds__(256) void an_tempo_kernel(const double* __restrict__ r_all, long long frame_stride, const int32_t* __restrict__ frames,
                                                       float* __restrict__ tempo, float* __restrict__ strength, double fps, int lag0, int lag_hi,
                                                       int lags, double prior_bpm, double prior_octaves) {
  __shared__ double s[AN_MAX_LAGS];
  const int row = blockIdx.x;
  const double* r = r_all + (long long)row * (lags + 1);
  long long F = frames ? (long long)frames[row] : frame_stride;
  F = F < 0 ? 0 : (F > frame_stride ? frame_stride : F);
  const double lp = log2(prior_bpm);
  for (int i = threadIdx.x; i < lags; i += 256) {
    const double z = (log2(60.0 * fps / (double)(lag0 + i)) - lp) / prior_octaves;
    s[i] = r[i] * exp(-0.5 * z * z);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // candidates: index 1 (lag lag0 + 1) ... the lag min(lag_hi, F - 2); both neighbours of every candidate are in the list
    const long long last = (long long)lag_hi < F - 2 ? (long long)lag_hi : F - 2;
    const double r0 = r[lags];
    float bpm = 0.f, st = 0.f;
    if (last >= lag0 + 1 && r0 > 0.0) {
      int best = 1;
      for (int i = 2; lag0 + i <= last; ++i)
        if (s[i] > s[best]) best = i;
      const double a = s[best - 1], b = s[best], c = s[best + 1], d = a - 2.0 * b + c;
      double l = (double)(lag0 + best);
      if (d < 0.0) l += 0.5 * (a - c) / d;
      bpm = (float)(60.0 * fps / l);
      st = (float)(r[best] / r0);
    }
    tempo[row] = bpm;
    strength[row] = st;
  }
}

__constant__ double AN_KK[2][12] = {{6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88},
                                    {6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17}};

__global__ __launch_bounds__(AN_THREADS) void an_key_kernel(const float* __restrict__ chroma, long long frame_stride, const int32_t* __restrict__ frames,
                                                            int32_t* __restrict__ key, float* __restrict__ strength, double* __restrict__ profile,
                                                            float* __restrict__ corr) {
  __shared__ double prof[12];
  __shared__ double cr[24];
  const int row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long long F = frames ? (long long)frames[row] : frame_stride;
  F = F < 0 ? 0 : (F > frame_stride ? frame_stride : F);
  if (wave < 12) {
    const float* c = chroma + ((long long)row * 12 + wave) * frame_stride;
    double acc = 0.0;
    for (long long t = lane; t < F; t += 64) acc += (double)c[t];
    acc = an_wave_sum(acc);
    if (lane == 0) {
      prof[wave] = acc;
      profile[(long long)row * 12 + wave] = acc;
    }
  }
  __syncthreads();
  if (threadIdx.x < 24) {
    const int j = threadIdx.x, tonic = j % 12, mode = j / 12;
    double mx = 0.0, mk = 0.0, lo = prof[0], hi = prof[0];
    for (int i = 0; i < 12; ++i) {
      mx += prof[i];
      mk += AN_KK[mode][i];
      lo = fmin(lo, prof[i]);
      hi = fmax(hi, prof[i]);
    }
    const bool varies = hi > lo;      // all twelve equal: no variance, whatever the mean rounds to
    mx /= 12.0;
    mk /= 12.0;
    double sxy = 0.0, sxx = 0.0, syy = 0.0;
    for (int i = 0; i < 12; ++i) {
      const double dx = prof[i] - mx, dy = AN_KK[mode][(i - tonic + 12) % 12] - mk;
      sxy = fma(dx, dy, sxy);
      sxx = fma(dx, dx, sxx);
      syy = fma(dy, dy, syy);
    }
    const double v = varies && sxx > 0.0 ? sxy / sqrt(sxx * syy) : 0.0;
    cr[j] = varies && sxx > 0.0 ? v : -2.0;         // -2: no variance
    corr[(long long)row * 24 + j] = (float)v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = -1;
    float st = 0.f;
    if (cr[0] >= -1.5) {
      best = 0;
      for (int j = 1; j < 24; ++j)
        if (cr[j] > cr[best]) best = j;
      st = (float)cr[best];
    }
    key[row] = best;
    strength[row] = st;
  }
}

}  // namespace

extern "C" int jen1_tempo_lags(double fps, double bpm_min, double bpm_max) {
  if (!(fps > 0.0) || !(bpm_min > 0.0) || !(bpm_max > bpm_min) || !isfinite(fps) || !isfinite(bpm_max)) return 0;
  if (!(60.0 * fps / bpm_min < 1e9)) return 0;
  const long long lo = an_lag_min(fps, bpm_max), hi = an_lag_max(fps, bpm_min);
  if (lo < 2 || hi < lo || hi - lo + 3 > AN_MAX_LAGS) return 0;
  return (int)(hi - lo + 3);
}

extern "C" int64_t jen1_tempo_workspace_bytes(int rows, double fps, double bpm_min, double bpm_max) {
  const int lags = jen1_tempo_lags(fps, bpm_min, bpm_max);
  if (lags < 1 || rows < 0) return 0;
  return (int64_t)(rows > 0 ? rows : 1) * (lags + 1) * (int64_t)sizeof(double);
}

extern "C" int jen1_tempo(const float* onset, int64_t frame_stride, const int32_t* frames, float* tempo, float* strength, double* acf, int rows,
                          double fps, double bpm_min, double bpm_max, double prior_bpm, double prior_octaves, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  JEN1_CHECK(rows >= 0 && frame_stride >= 1 && frame_stride < (1ll << 40), "jen1_tempo: bad shape (rows %d, frame_stride %lld)", rows,
             (long long)frame_stride);
  JEN1_CHECK(fps > 0.0 && isfinite(fps), "jen1_tempo: fps = %g, must be positive", fps);
  JEN1_CHECK(bpm_min > 0.0 && bpm_max > bpm_min && isfinite(bpm_max), "jen1_tempo: bpm range [%g, %g] must be positive and not empty", bpm_min, bpm_max);
  JEN1_CHECK(prior_bpm > 0.0 && isfinite(prior_bpm) && prior_octaves > 0.0 && isfinite(prior_octaves),
             "jen1_tempo: prior_bpm = %g and prior_octaves = %g must be positive", prior_bpm, prior_octaves);
  const int lags = jen1_tempo_lags(fps, bpm_min, bpm_max);
  JEN1_CHECK(lags > 0, "jen1_tempo: the lags of [%g, %g] bpm at %g frames per second must start at 2 or more and be at most %d", bpm_min, bpm_max, fps,
             AN_MAX_LAGS - 2);
  JEN1_CHECK(onset != nullptr && tempo != nullptr && strength != nullptr, "jen1_tempo: null pointer");
  JEN1_CHECK(acf == nullptr || (reinterpret_cast<uintptr_t>(acf) & 7u) == 0, "jen1_tempo: acf is not 8-byte aligned");
  JEN1_CHECK(rows < (1 << 27), "jen1_tempo: %d rows exceed the grid", rows);
  const long long need = jen1_tempo_workspace_bytes(rows, fps, bpm_min, bpm_max);
  JEN1_CHECK(workspace != nullptr && workspace_bytes >= need, "jen1_tempo: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, need);
  JEN1_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "jen1_tempo: workspace is not 8-byte aligned");
  if (rows == 0) return 0;
  const int lag0 = (int)an_lag_min(fps, bpm_max) - 1, lag_hi = (int)an_lag_max(fps, bpm_min);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(an_acf_kernel, dim3((unsigned)rows * AN_SPLIT), dim3(AN_THREADS), 0, st, onset, (long long)frame_stride, frames,
                     static_cast<double*>(workspace), acf, lag0, lags);
  hipLaunchKernelGGL(an_tempo_kernel, dim3((unsigned)rows), dim3(256), 0, st, static_cast<const double*>(workspace), (long long)frame_stride, frames,
                     tempo, strength, fps, lag0, lag_hi, lags, prior_bpm, prior_octaves);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_key(const float* chroma, int64_t frame_stride, const int32_t* frames, int32_t* key, float* strength, double* profile,
                        float* corr, int rows, void* stream) {
  JEN1_CHECK(rows >= 0 && frame_stride >= 1 && frame_stride < (1ll << 36), "jen1_key: bad shape (rows %d, frame_stride %lld)", rows,
             (long long)frame_stride);
  JEN1_CHECK(chroma != nullptr && key != nullptr && strength != nullptr && profile != nullptr && corr != nullptr, "jen1_key: null pointer");
  JEN1_CHECK((reinterpret_cast<uintptr_t>(profile) & 7u) == 0, "jen1_key: profile is not 8-byte aligned");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(an_key_kernel, dim3((unsigned)rows), dim3(AN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), chroma, (long long)frame_stride,
                     frames, key, strength, profile, corr);
  JEN1_HIP(hipGetLastError());
  return 0;
}
