// True-peak meter and look-ahead true-peak limiter (include/jen1_limiter.h: jen1_true_peak, jen1_limit_true_peak): ITU-R BS.1770-4
// Annex 2 read as a 4x (2x, 1x) polyphase interpolator whose phase 0 is the signal itself, and an offline limiter on the envelope the
// meter leaves: hold, release, attack window, one gain for every channel of a row.  Not in the reference.
//
//   tp_tile       one workgroup per tile of TP_TILE samples of a row: every channel's tile + 8 samples of halo on each side in LDS, the
//                 F - 1 filtered phases as 16 float64 FMAs each, env = max over channels and phases, the tile's peak -> part
//   tp_rows       one workgroup per row: peak = max of the row's partial peaks (a max has no order: no atomics are needed for the bits)
//   lim_hold      q = 1 - min(1, c / env) for a tile of the hold's domain (b = i + A in [0, L + A)) with A samples of its left
//                 neighbour; the running maximum over A + 1 samples by doubling (W_2k[m] = max(W_k[m], W_k[m + k])); Q -> workspace; the
//                 tile's composite of the release scan -> comp
//   lim_carry     one workgroup per row: the state in front of every tile.  The release step s -> max(Q, rho s) composes as
//                 (a, C) o (a', C') = (a a', max(C, a C')), and a = rho^n depends on the length alone, so a tile is one number.  256
//                 threads own a run of tiles each: run totals from zero, a serial pass over the 256 totals, every run again from its
//                 true start (kw_carry of loudness.hip, with a scalar state)
//   lim_release   a tile again from its true start: d over Q in the workspace, in place
//   lim_apply     d of a tile and A samples of its right neighbour in LDS, s = 1 - sum_j w[j] d[n - j], y = float(s (double)x)
// Inside a tile the scan has the same three steps: a thread owns LIM_CHUNK consecutive samples (LDS index e + e / 8: conflict-free
// reads at a lane stride of 9 doubles), thread 0 passes over the 256 chunk totals with rho^LIM_CHUNK.
// Separate launches at ordinary kernel boundaries; no workgroup waits on another.  Everything is float64 until the one rounding at
// the store of y.
#include <math.h>

#include "common.h"
#include "jen1_limiter.h"

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_TILE = 2048;             // samples per workgroup
constexpr int TP_TAPS = 16;               // taps per phase
constexpr int TP_HALO = TP_TAPS / 2;
constexpr int LIM_CHUNK = TP_TILE / TP_THREADS;
constexpr int LIM_MAX_A = 512;            // look-ahead cap: the tile + halo of lim_hold / lim_apply is (2048 + 512) doubles = 20 KiB of LDS
constexpr int LIM_STAGE = TP_TILE + LIM_MAX_A;
constexpr int LIM_PER = LIM_STAGE / TP_THREADS;
static_assert(LIM_CHUNK == 8 && LIM_STAGE % TP_THREADS == 0, "lim_pad and the doubling loop assume these");

struct TpTaps {
  double h[3][TP_TAPS];
};

__device__ __forceinline__ int lim_pad(int e) { return e + (e >> 3); }
constexpr int LIM_PADDED = TP_TILE + TP_TILE / 8;

// max over the workgroup, fixed tree; every thread gets it
__device__ __forceinline__ double tp_block_max(double (&sh)[TP_THREADS], double v) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  __syncthreads();
  for (int w = TP_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] = fmax(sh[t], sh[t + w]);
    __syncthreads();
  }
  return sh[0];
}

template <int F>
__global__ __launch_bounds__(TP_THREADS) void tp_tile_kernel(const float* __restrict__ x, double* __restrict__ env, long long env_stride,
                                                             double* __restrict__ part, TpTaps taps, int C, long long L, int tiles) {
  __shared__ float xs[2][TP_TILE + 2 * TP_HALO];
  __shared__ double sh[TP_THREADS];
  const long long row = blockIdx.x / tiles, t0 = (long long)(blockIdx.x % tiles) * TP_TILE;
  for (int c = 0; c < C; ++c) {
    const float* line = x + (row * C + c) * L;
    for (int m = threadIdx.x; m < TP_TILE + 2 * TP_HALO; m += TP_THREADS) {
      const long long s = t0 - TP_HALO + m;
      xs[c][m] = (s >= 0 && s < L) ? line[s] : 0.f;
    }
  }
  __syncthreads();
  double top = 0.0;
  for (int r = threadIdx.x; r < TP_TILE; r += TP_THREADS) {
    if (t0 + r >= L) break;
    double e = 0.0;
    for (int c = 0; c < C; ++c) {
      const float* w = xs[c] + r;                              // w[m] = x[t0 + r - 8 + m]: x[n + 8 - k] = w[16 - k]
      e = fmax(e, fabs((double)w[TP_HALO]));
      if (F > 1) {
        double v[TP_TAPS];
#pragma unroll
        for (int k = 0; k < TP_TAPS; ++k) v[k] = (double)w[TP_TAPS - k];
#pragma unroll
        for (int p = 0; p < F - 1; ++p) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < TP_TAPS; ++k) acc = fma(taps.h[p][k], v[k], acc);
          e = fmax(e, fabs(acc));
        }
      }
    }
    if (env != nullptr) env[row * env_stride + t0 + r] = e;
    top = fmax(top, e);
  }
  top = tp_block_max(sh, top);
  if (threadIdx.x == 0) part[row * tiles + blockIdx.x % tiles] = top;
}

__global__ __launch_bounds__(TP_THREADS) void tp_rows_kernel(const double* __restrict__ part, double* __restrict__ peak, int tiles) {
  __shared__ double sh[TP_THREADS];
  const double* p = part + (long long)blockIdx.x * tiles;
  double top = 0.0;
  for (int j = threadIdx.x; j < tiles; j += TP_THREADS) top = fmax(top, p[j]);
  top = tp_block_max(sh, top);
  if (threadIdx.x == 0) peak[blockIdx.x] = top;
}

// the chunk of thread t of the padded tile P from state s: the state behind it; WRITE stores d over Q
template <bool WRITE>
__device__ __forceinline__ double lim_chunk_scan(double* P, double s, double rho) {
  const int e0 = threadIdx.x * LIM_CHUNK;
#pragma unroll
  for (int j = 0; j < LIM_CHUNK; ++j) {
    s = fmax(P[lim_pad(e0 + j)], rho * s);
    if (WRITE) P[lim_pad(e0 + j)] = s;
  }
  return s;
}

__global__ __launch_bounds__(TP_THREADS) void lim_hold_kernel(const double* __restrict__ env, long long env_stride, double* __restrict__ Qb,
                                                              double* __restrict__ comp, long long L, long long M, int A, double c,
                                                              double rho, double rho_chunk, int tiles) {
  __shared__ double S[LIM_STAGE];
  __shared__ double P[LIM_PADDED];
  __shared__ double tc[TP_THREADS];
  const long long row = blockIdx.x / tiles, b0 = (long long)(blockIdx.x % tiles) * TP_TILE;
  const int n = TP_TILE + A;                                   // S[m] = q[b0 - A + m], zero outside the row
  const double* er = env + row * env_stride;
  for (int m = threadIdx.x; m < n; m += TP_THREADS) {
    const long long k = b0 - A + m;
    S[m] = (k >= 0 && k < L) ? 1.0 - fmin(1.0, c / er[k]) : 0.0;
  }
  __syncthreads();
  int p = 1;
  for (; 2 * p <= A + 1; p *= 2) {                             // S = W_p: W_p[m] = max S[m .. m + p - 1] wherever that lies inside n
    double v[LIM_PER];
#pragma unroll
    for (int i = 0; i < LIM_PER; ++i) {
      const int m = threadIdx.x + i * TP_THREADS;
      v[i] = 0.0;
      if (m < n) v[i] = m + p < n ? fmax(S[m], S[m + p]) : S[m];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LIM_PER; ++i) {
      const int m = threadIdx.x + i * TP_THREADS;
      if (m < n) S[m] = v[i];
    }
    __syncthreads();
  }
  const int off = A + 1 - p;                                   // two windows of p cover A + 1 samples; r + off + p - 1 = r + A < n
  for (int r = threadIdx.x; r < TP_TILE; r += TP_THREADS) {
    const bool in = b0 + r < M;
    const double q = in ? fmax(S[r], S[r + off]) : 0.0;
    P[lim_pad(r)] = q;
    if (in) Qb[row * M + b0 + r] = q;
  }
  __syncthreads();
  tc[threadIdx.x] = lim_chunk_scan<false>(P, 0.0, rho);
  __syncthreads();
  if (threadIdx.x == 0) {
    double cur = 0.0;
#pragma unroll 8
    for (int j = 0; j < TP_THREADS; ++j) cur = fmax(tc[j], rho_chunk * cur);
    comp[row * tiles + blockIdx.x % tiles] = cur;
  }
}

__global__ __launch_bounds__(TP_THREADS) void lim_carry_kernel(const double* __restrict__ comp, double* __restrict__ start, int tiles, int R,
                                                               double rho_tile, double rho_run) {
  __shared__ double tot[TP_THREADS], from[TP_THREADS];
  const double* cr = comp + (long long)blockIdx.x * tiles;
  double* sr = start + (long long)blockIdx.x * tiles;
  const int t = threadIdx.x;
  const long long lo64 = (long long)t * R;
  const int lo = (int)(lo64 < tiles ? lo64 : tiles);
  const int run = lo + R < tiles ? R : tiles - lo;
  double s = 0.0;
  for (int k = 0; k < run; ++k) s = fmax(cr[lo + k], rho_tile * s);
  tot[t] = s;
  __syncthreads();
  if (t == 0) {                                                // (a short last run has no successor: its total is never used)
    double cur = 0.0;
#pragma unroll 8
    for (int j = 0; j < TP_THREADS; ++j) {
      from[j] = cur;
      cur = fmax(tot[j], rho_run * cur);
    }
  }
  __syncthreads();
  s = from[t];
  for (int k = 0; k < run; ++k) {
    sr[lo + k] = s;
    s = fmax(cr[lo + k], rho_tile * s);
  }
}

__global__ __launch_bounds__(TP_THREADS) void lim_release_kernel(double* __restrict__ Qb, const double* __restrict__ start, long long M, double rho,
                                                                 double rho_chunk, int tiles) {
  __shared__ double P[LIM_PADDED];
  __shared__ double tc[TP_THREADS], from[TP_THREADS];
  const long long row = blockIdx.x / tiles, b0 = (long long)(blockIdx.x % tiles) * TP_TILE;
  double* qr = Qb + row * M;
  for (int r = threadIdx.x; r < TP_TILE; r += TP_THREADS) P[lim_pad(r)] = b0 + r < M ? qr[b0 + r] : 0.0;
  __syncthreads();
  tc[threadIdx.x] = lim_chunk_scan<false>(P, 0.0, rho);
  __syncthreads();
  if (threadIdx.x == 0) {
    double cur = start[row * tiles + blockIdx.x % tiles];
#pragma unroll 8
    for (int j = 0; j < TP_THREADS; ++j) {
      from[j] = cur;
      cur = fmax(tc[j], rho_chunk * cur);
    }
  }
  __syncthreads();
  lim_chunk_scan<true>(P, from[threadIdx.x], rho);
  __syncthreads();
  for (int r = threadIdx.x; r < TP_TILE; r += TP_THREADS)
    if (b0 + r < M) qr[b0 + r] = P[lim_pad(r)];
}

// x and y may be the same buffer: a thread reads a sample and writes the same sample
__global__ __launch_bounds__(TP_THREADS) void lim_apply_kernel(const float* x, float* y, long long y_stride, double* __restrict__ red,
                                                               long long red_stride, const double* __restrict__ d, const double* __restrict__ window,
                                                               int C, long long L, long long M, int A, int tiles) {
  __shared__ double D[LIM_STAGE];
  __shared__ double W[LIM_MAX_A + 1];
  const long long row = blockIdx.x / tiles, n0 = (long long)(blockIdx.x % tiles) * TP_TILE;
  const double* dr = d + row * M;                              // d of sample i at dr[i + A]: D[m] = d[n0 - A + m]
  for (int m = threadIdx.x; m < TP_TILE + A; m += TP_THREADS) D[m] = n0 + m < M ? dr[n0 + m] : 0.0;
  for (int j = threadIdx.x; j <= A; j += TP_THREADS) W[j] = window[j];
  __syncthreads();
  for (int r = threadIdx.x; r < TP_TILE; r += TP_THREADS) {
    const long long n = n0 + r;
    if (n >= L) break;
    double acc = 0.0;
    for (int j = 0; j <= A; ++j) acc = fma(W[j], D[r + A - j], acc);
    const double s = 1.0 - acc;
    for (int c = 0; c < C; ++c) y[row * y_stride + c * L + n] = (float)(s * (double)x[(row * C + c) * L + n]);
    if (red != nullptr) red[row * red_stride + n] = acc;
  }
}

inline bool tp_shape_ok(int rows, int C, long long L) { return rows >= 0 && (C == 1 || C == 2) && L >= 1 && L < (1ll << 40); }
inline long long tp_tiles(long long n) { return (n + TP_TILE - 1) / TP_TILE; }

}  // namespace

extern "C" int jen1_true_peak_tile(void) { return TP_TILE; }

extern "C" int jen1_limiter_chunk(void) { return LIM_CHUNK; }

extern "C" int jen1_limiter_max_lookahead(void) { return LIM_MAX_A; }

extern "C" int64_t jen1_true_peak_workspace_bytes(int rows, int C, int64_t L) {
  if (!tp_shape_ok(rows, C, L)) return 0;
  return (long long)rows * tp_tiles(L) * (long long)sizeof(double);
}

extern "C" int jen1_true_peak(const float* x, double* env, int64_t env_stride, double* peak, const double* taps, int F, int rows, int C,
                              int64_t L, void* workspace, int64_t workspace_bytes, void* stream) {
  JEN1_CHECK(C == 1 || C == 2, "jen1_true_peak: C = %d, must be 1 or 2", C);
  JEN1_CHECK(F == 1 || F == 2 || F == 4, "jen1_true_peak: F = %d, must be 1, 2 or 4", F);
  JEN1_CHECK(rows >= 0 && L >= 1 && L < (1ll << 40), "jen1_true_peak: bad shape (rows %d, L %lld)", rows, (long long)L);
  JEN1_CHECK(x != nullptr && peak != nullptr && workspace != nullptr && (taps != nullptr || F == 1), "jen1_true_peak: null pointer");
  JEN1_CHECK(env == nullptr || env_stride >= L, "jen1_true_peak: env_stride = %lld is shorter than a row of %lld", (long long)env_stride, (long long)L);
  JEN1_CHECK(((reinterpret_cast<uintptr_t>(env) | reinterpret_cast<uintptr_t>(peak) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0,
             "jen1_true_peak: env, peak and workspace must be 8-byte aligned");
  TpTaps h;
  memset(&h, 0, sizeof(h));
  for (int i = 0; i < (F - 1) * TP_TAPS; ++i) {
    JEN1_CHECK(isfinite(taps[i]), "jen1_true_peak: taps[%d] is not finite", i);
    h.h[i / TP_TAPS][i % TP_TAPS] = taps[i];
  }
  const long long tiles = tp_tiles(L), need = (long long)rows * tiles * (long long)sizeof(double);
  JEN1_CHECK(workspace_bytes >= need, "jen1_true_peak: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, need);
  JEN1_CHECK(tiles * rows < (1ll << 31), "jen1_true_peak: %lld tiles x %d rows exceed the grid", tiles, rows);
  if (rows == 0) return 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  const dim3 grid((unsigned)(tiles * rows)), block(TP_THREADS);
  if (F == 1)
    hipLaunchKernelGGL((tp_tile_kernel<1>), grid, block, 0, s, x, env, (long long)env_stride, part, h, C, (long long)L, (int)tiles);
  else if (F == 2)
    hipLaunchKernelGGL((tp_tile_kernel<2>), grid, block, 0, s, x, env, (long long)env_stride, part, h, C, (long long)L, (int)tiles);
  else
    hipLaunchKernelGGL((tp_tile_kernel<4>), grid, block, 0, s, x, env, (long long)env_stride, part, h, C, (long long)L, (int)tiles);
  hipLaunchKernelGGL(tp_rows_kernel, dim3((unsigned)rows), block, 0, s, part, peak, (int)tiles);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int64_t jen1_limiter_workspace_bytes(int rows, int64_t L, int A) {
  if (!tp_shape_ok(rows, 1, L) || A < 0 || A > LIM_MAX_A) return 0;
  const long long M = L + A;
  return (long long)rows * (M + 2 * tp_tiles(M)) * (long long)sizeof(double);
}

extern "C" int jen1_limit_true_peak(const float* x, float* y, int64_t y_stride, double* red, int64_t red_stride, const double* env,
                                    int64_t env_stride, const double* window, int rows, int C, int64_t L, int A, double ceiling, double rho,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  JEN1_CHECK(C == 1 || C == 2, "jen1_limit_true_peak: C = %d, must be 1 or 2", C);
  JEN1_CHECK(rows >= 0 && L >= 1 && L < (1ll << 40), "jen1_limit_true_peak: bad shape (rows %d, L %lld)", rows, (long long)L);
  JEN1_CHECK(A >= 0 && A <= LIM_MAX_A, "jen1_limit_true_peak: lookahead A = %d samples, must be in [0, %d]", A, LIM_MAX_A);
  JEN1_CHECK(isfinite(ceiling) && ceiling > 0.0, "jen1_limit_true_peak: ceiling = %g, must be positive and finite", ceiling);
  JEN1_CHECK(rho >= 0.0 && rho < 1.0, "jen1_limit_true_peak: rho = %g, must be in [0, 1)", rho);
  JEN1_CHECK(x != nullptr && y != nullptr && env != nullptr && window != nullptr && workspace != nullptr, "jen1_limit_true_peak: null pointer");
  JEN1_CHECK(y_stride >= (long long)C * L, "jen1_limit_true_peak: y_stride = %lld is shorter than a row of %lld", (long long)y_stride, (long long)C * L);
  JEN1_CHECK(static_cast<const void*>(x) != static_cast<const void*>(y) || y_stride == (long long)C * L,
             "jen1_limit_true_peak: in place (y == x) needs y_stride = C L");
  JEN1_CHECK(env_stride >= L, "jen1_limit_true_peak: env_stride = %lld is shorter than a row of %lld", (long long)env_stride, (long long)L);
  JEN1_CHECK(red == nullptr || red_stride >= L, "jen1_limit_true_peak: red_stride = %lld is shorter than a row of %lld", (long long)red_stride, (long long)L);
  JEN1_CHECK(((reinterpret_cast<uintptr_t>(env) | reinterpret_cast<uintptr_t>(red) | reinterpret_cast<uintptr_t>(window) |
               reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0,
             "jen1_limit_true_peak: env, red, window and workspace must be 8-byte aligned");
  const long long M = L + A, tiles = tp_tiles(M), tiles_out = tp_tiles(L);
  const long long need = (long long)rows * (M + 2 * tiles) * (long long)sizeof(double);
  JEN1_CHECK(workspace_bytes >= need, "jen1_limit_true_peak: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, need);
  JEN1_CHECK(tiles * rows < (1ll << 31), "jen1_limit_true_peak: %lld tiles x %d rows exceed the grid", tiles, rows);
  if (rows == 0) return 0;
  double* Qb = static_cast<double*>(workspace);
  double* comp = Qb + (long long)rows * M;
  double* start = comp + (long long)rows * tiles;
  const int R = (int)((tiles + TP_THREADS - 1) / TP_THREADS);
  const double rho_chunk = pow(rho, (double)LIM_CHUNK), rho_tile = pow(rho, (double)TP_TILE), rho_run = pow(rho, (double)TP_TILE * R);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 block(TP_THREADS);
  hipLaunchKernelGGL(lim_hold_kernel, dim3((unsigned)(tiles * rows)), block, 0, s, env, (long long)env_stride, Qb, comp, (long long)L, M, A, ceiling,
                     rho, rho_chunk, (int)tiles);
  hipLaunchKernelGGL(lim_carry_kernel, dim3((unsigned)rows), block, 0, s, comp, start, (int)tiles, R, rho_tile, rho_run);
  hipLaunchKernelGGL(lim_release_kernel, dim3((unsigned)(tiles * rows)), block, 0, s, Qb, start, M, rho, rho_chunk, (int)tiles);
  hipLaunchKernelGGL(lim_apply_kernel, dim3((unsigned)(tiles_out * rows)), block, 0, s, x, y, (long long)y_stride, red, (long long)red_stride, Qb,
                     window, C, (long long)L, M, A, (int)tiles_out);
  JEN1_HIP(hipGetLastError());
  return 0;
}
