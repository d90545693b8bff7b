// Programme loudness of waveforms (include/jen1_hip.h: jen1_kweight_energy, jen1_loudness_gate, jen1_gain_apply): ITU-R BS.1770-4
// integrated loudness with every channel weight 1.0, and the gain + limiter that bring a waveform to a target.  Not in the reference.
//
// K-weighting is two biquads in series (high shelf, then high-pass), a recurrence over every sample of a channel.  A channel is cut
// into chunks of N samples, N a divisor of the hop (kw_chunk), and the chunk-to-chunk dependency is carried as STATE, exactly:
// with the cascade in transposed direct form II its four state words obey  s[i + 1] = A s[i] + B x[i],  so the state behind a chunk
// that started from s is  A^N s + f,  f = the state behind the same chunk started from zero.
//   kw_state    one thread per chunk: f, and the chunk's sum of x^2 and max |x| on the way
//   kw_carry    one workgroup per (row, channel): s[c + 1] = A^N s[c] + f[c] over the chunks in order; f is replaced by the START state
//               of every chunk.  256 threads own a run of K chunks each: run totals from zero, a serial pass over the 256 totals with
//               A^(N K), then every run again from its true start.  The row's statistics are reduced in the same order.  The states
//               are stored transposed (kw_slot) so that this kernel, two workgroups on a stereo piece, reads and writes whole lines.
//   kw_energy   one thread per chunk: the filter again from the chunk's start state, sum of y^2 of the chunk
//   kw_hops     one thread per hop: the hop's chunks summed in ascending order; the two channels' statistics joined
// Separate launches at ordinary kernel boundaries; no workgroup waits on another.  Recurrence state and every sum are float64 (a float32
// recurrence through the 38 Hz high-pass, poles at radius 0.995, loses 2e-6 of a hop's energy).  Every sum has one fixed order and
// there are no float atomics: the same bits on every run.
//
// kw_state and kw_energy stage a tile of T consecutive chunks in LDS with coalesced dword loads (consecutive lanes, consecutive
// floats: whole cache lines whatever the alignment of a channel, which starts at an arbitrary float), chunk q at q (N | 1) so that the
// per-thread reads of the recurrence (lane stride N | 1 dwords, odd) are free of bank conflicts.
#include <math.h>

#include "common.h"

namespace {

constexpr int KW_THREADS = 128;           // chunks per tile at most: one thread per chunk
constexpr int KW_LDS_FLOATS = 15872;      // 62 KiB: two workgroups per CU
constexpr int KW_CHUNK_MAX = 128;         // the rule prefers the largest divisor of the hop up to here ...
constexpr int KW_CHUNK_MIN = 16;          // ... and goes ABOVE it where that divisor would be shorter than this
constexpr int KW_CARRY_THREADS = 256;
constexpr int KW_CARRY_BATCH = 8;
constexpr int GATE_THREADS = 256;
constexpr int GAIN_THREADS = 256;
constexpr int GAIN_TILE = 256 * 4 * 8;    // floats per workgroup of the gain kernel

struct KwCoef {                            // shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2
  double c[10];
};
struct KwMat {                             // row-major 4 x 4
  double m[16];
};

inline int kw_chunk(int hop) {
  if (hop < 1) return 0;
  int best = 1;
  for (int d = 1; d <= KW_CHUNK_MAX && d <= hop; ++d)
    if (hop % d == 0) best = d;
  if (best >= KW_CHUNK_MIN || best == hop) return best;
  for (int d = KW_CHUNK_MAX + 1; d <= hop; ++d)         // an awkward hop (2 x prime, ...): the smallest divisor above the window
    if (hop % d == 0) return d;
  return hop;
}
inline int kw_pitch(int N) { return N | 1; }
inline int kw_tile_chunks(int N) {
  const int t = KW_LDS_FLOATS / kw_pitch(N);
  return t > KW_THREADS ? KW_THREADS : t;
}

// one sample through the cascade; s = {shelf s1, shelf s2, high-pass s1, high-pass s2}
__device__ __forceinline__ double kw_step(const KwCoef& k, double (&s)[4], double x) {
  const double y1 = fma(k.c[0], x, s[0]);
  s[0] = fma(k.c[1], x, fma(-k.c[3], y1, s[1]));
  s[1] = fma(k.c[2], x, -k.c[4] * y1);
  const double y2 = fma(k.c[5], y1, s[2]);
  s[2] = fma(k.c[6], y1, fma(-k.c[8], y2, s[3]));
  s[3] = fma(k.c[7], y1, -k.c[9] * y2);
  return y2;
}

__device__ __forceinline__ void kw_matvec(const KwMat& M, const double (&s)[4], const double (&f)[4], double (&o)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = fma(M.m[4 * i + 0], s[0], fma(M.m[4 * i + 1], s[1], fma(M.m[4 * i + 2], s[2], fma(M.m[4 * i + 3], s[3], f[i]))));
}

// the tile's samples [t0, t0 + count) of one channel into LDS, chunk q at q * pitch
__device__ __forceinline__ void kw_stage(float* xs, const float* __restrict__ line, long long t0, int count, int N, int pitch) {
  const int dq = KW_THREADS / N, dr = KW_THREADS % N;
  int q = threadIdx.x / N, r = threadIdx.x % N;
  for (int i = threadIdx.x; i < count; i += KW_THREADS) {
    xs[q * pitch + r] = line[t0 + i];
    q += dq;
    r += dr;
    if (r >= N) {
      r -= N;
      ++q;
    }
  }
  __syncthreads();
}

// Where the state of chunk c = t K + k of a line lives: component i at st[i * slots + k * KW_CARRY_THREADS + t] (slots = K *
// KW_CARRY_THREADS), so that in the carry kernel, where thread t walks chunks t K .. t K + K - 1, consecutive lanes read consecutive
// doubles at every step.  The strided side of the transpose falls to the two chunk kernels, which have a workgroup on every CU and
// touch the state once per N samples.  sx and mx use the same slot.
__device__ __forceinline__ long long kw_slot(long long c, long long K) { return (c % K) * KW_CARRY_THREADS + c / K; }

// ENERGY = false: zero-state end state -> st, sum x^2 -> sx, max |x| -> mx.  ENERGY = true: from the start state in st, sum y^2 -> ce.
template <bool ENERGY>
__global__ __launch_bounds__(KW_THREADS) void kw_chunk_kernel(const float* __restrict__ x, double* __restrict__ st, double* __restrict__ sx,
                                                              double* __restrict__ mx, double* __restrict__ ce, KwCoef k, long long L,
                                                              int N, int pitch, int T, long long nch, int tiles, long long K) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const long long line = blockIdx.x / tiles;                  // row * C + channel
  const long long c0 = (long long)(blockIdx.x % tiles) * T;   // first chunk of the tile
  const long long t0 = c0 * N;
  const long long left = L - t0;
  const int count = (int)(left < (long long)T * N ? left : (long long)T * N);
  kw_stage(xs, x + line * L, t0, count, N, pitch);
  const int q = threadIdx.x;
  if (q >= T || c0 + q >= nch) return;
  int n = count - q * N;                                       // samples of this chunk (the last one of a channel may be short)
  n = n > N ? N : n;
  const float* xq = xs + q * pitch;
  const long long slots = K * KW_CARRY_THREADS, slot = kw_slot(c0 + q, K);
  double* sq = st + line * slots * 4 + slot;
  double s[4];
  if (ENERGY) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = sq[i * slots];
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
      const double y = kw_step(k, s, (double)xq[i]);
      acc = fma(y, y, acc);
    }
    ce[line * nch + c0 + q] = acc;
  } else {
    s[0] = s[1] = s[2] = s[3] = 0.0;
    double acc = 0.0;
    float top = 0.f;
    for (int i = 0; i < n; ++i) {
      const float v = xq[i];
      kw_step(k, s, (double)v);
      acc = fma((double)v, (double)v, acc);
      top = fmaxf(top, fabsf(v));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sq[i * slots] = s[i];
    sx[line * slots + slot] = acc;
    mx[line * slots + slot] = (double)top;
  }
}

__global__ __launch_bounds__(KW_CARRY_THREADS) void kw_carry_kernel(double* __restrict__ st, const double* __restrict__ sx,
                                                                    const double* __restrict__ mx, double* __restrict__ part, KwMat AN,
                                                                    KwMat ANK, long long nch, long long K) {
  __shared__ double tot[KW_CARRY_THREADS][4], from[KW_CARRY_THREADS][4];
  __shared__ double tsx[KW_CARRY_THREADS], tmx[KW_CARRY_THREADS];
  const long long line = blockIdx.x, slots = K * KW_CARRY_THREADS;
  const int t = threadIdx.x;
  double* f = st + line * slots * 4 + t;                        // chunk t K + k, component i: f[i * slots + k * KW_CARRY_THREADS]
  const double* qx = sx + line * slots + t;
  const double* qm = mx + line * slots + t;
  const long long lo = t * K < nch ? t * K : nch;
  const int run = (int)(lo + K < nch ? K : nch - lo);           // chunks of this thread's run (K < 2^31: the grid check of the launcher)
  double s[4] = {0.0, 0.0, 0.0, 0.0}, o[4];
  double acc = 0.0, top = 0.0;
  // both passes read KW_CARRY_BATCH chunks ahead of the dependent chain, so that the loads of a batch are in flight together
  for (int k0 = 0; k0 < run; k0 += KW_CARRY_BATCH) {            // the run from zero state
    double fc[KW_CARRY_BATCH][4], bx[KW_CARRY_BATCH], bm[KW_CARRY_BATCH];
#pragma unroll
    for (int j = 0; j < KW_CARRY_BATCH; ++j) {
      const long long kj = (long long)(k0 + j < run ? k0 + j : run - 1) * KW_CARRY_THREADS;
#pragma unroll
      for (int i = 0; i < 4; ++i) fc[j][i] = f[i * slots + kj];
      bx[j] = qx[kj];
      bm[j] = qm[kj];
    }
#pragma unroll
    for (int j = 0; j < KW_CARRY_BATCH; ++j) {
      if (k0 + j < run) {
        kw_matvec(AN, s, fc[j], o);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = o[i];
        acc += bx[j];
        top = fmax(top, bm[j]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) tot[t][i] = s[i];
  tsx[t] = acc;
  tmx[t] = top;
  __syncthreads();
  if (t == 0) {                                                // the start state of every run; the statistics in run order
    double cur[4] = {0.0, 0.0, 0.0, 0.0};
    double a = 0.0, m = 0.0;
#pragma unroll 8
    for (int j = 0; j < KW_CARRY_THREADS; ++j) {
      const double v[4] = {tot[j][0], tot[j][1], tot[j][2], tot[j][3]};
#pragma unroll
      for (int i = 0; i < 4; ++i) from[j][i] = cur[i];
      kw_matvec(ANK, cur, v, o);                               // (a short last run has no successor: its total is never used)
#pragma unroll
      for (int i = 0; i < 4; ++i) cur[i] = o[i];
      a += tsx[j];
      m = fmax(m, tmx[j]);
    }
    part[line * 2 + 0] = a;
    part[line * 2 + 1] = m;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = from[t][i];
  for (int k0 = 0; k0 < run; k0 += KW_CARRY_BATCH) {            // again from the true start: f becomes the START state of every chunk
    double fc[KW_CARRY_BATCH][4];
#pragma unroll
    for (int j = 0; j < KW_CARRY_BATCH; ++j) {
      const long long kj = (long long)(k0 + j < run ? k0 + j : run - 1) * KW_CARRY_THREADS;
#pragma unroll
      for (int i = 0; i < 4; ++i) fc[j][i] = f[i * slots + kj];
    }
#pragma unroll
    for (int j = 0; j < KW_CARRY_BATCH; ++j) {
      if (k0 + j < run) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i * slots + (long long)(k0 + j) * KW_CARRY_THREADS] = s[i];
        kw_matvec(AN, s, fc[j], o);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = o[i];
      }
    }
  }
}

__global__ __launch_bounds__(256) void kw_hops_kernel(const double* __restrict__ ce, const double* __restrict__ part, double* __restrict__ e,
                                                      double* __restrict__ stats, int rows, int C, long long H, long long nch, int P) {
  const long long total = (long long)rows * C * H;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g < total) {
    const long long line = g / H, h = g % H;
    const double* p = ce + line * nch + h * P;
    double acc = 0.0;
    for (int i = 0; i < P; ++i) acc += p[i];
    e[g] = acc;
  }
  if (g < rows) {
    double a = 0.0, m = 0.0;
    for (int c = 0; c < C; ++c) {
      a += part[(g * C + c) * 2 + 0];
      m = fmax(m, part[(g * C + c) * 2 + 1]);
    }
    stats[g * 2 + 0] = a;
    stats[g * 2 + 1] = m;
  }
}

// fixed-order sum of (v, n) over the workgroup: strided partials, then a halving tree in LDS; every thread gets the result
__device__ __forceinline__ void gate_reduce(double (&sh)[GATE_THREADS], double (&shn)[GATE_THREADS], double& v, double& n) {
  const int t = threadIdx.x;
  __syncthreads();
  sh[t] = v;
  shn[t] = n;
  __syncthreads();
  for (int w = GATE_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) {
      sh[t] += sh[t + w];
      shn[t] += shn[t + w];
    }
    __syncthreads();
  }
  v = sh[0];
  n = shn[0];
}

__device__ __forceinline__ double gate_block(const double* __restrict__ er, int C, long long H, long long j, double inv) {
  double s = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* p = er + c * H + j;
    s += (p[0] + p[1] + p[2] + p[3]) * inv;
  }
  return s;
}

__global__ __launch_bounds__(GATE_THREADS) void loudness_gate_kernel(const double* __restrict__ e, double* __restrict__ lufs, int C, long long H,
                                                                     int hop) {
  __shared__ double sh[GATE_THREADS], shn[GATE_THREADS];
  const long long J = H >= 4 ? H - 3 : 0;
  const double* er = e + (long long)blockIdx.x * C * H;
  const double inv = 1.0 / (4.0 * (double)hop);
  double v = 0.0, n = 0.0;
  for (long long j = threadIdx.x; j < J; j += GATE_THREADS) {          // absolute gate
    const double s = gate_block(er, C, H, j, inv);
    if (-0.691 + 10.0 * log10(s) > -70.0) {
      v += s;
      n += 1.0;
    }
  }
  gate_reduce(sh, shn, v, n);
  double out = -INFINITY;
  if (n > 0.0) {                                                       // (uniform over the workgroup)
    const double gamma = -0.691 + 10.0 * log10(v / n) - 10.0;
    v = 0.0;
    n = 0.0;
    for (long long j = threadIdx.x; j < J; j += GATE_THREADS) {        // relative gate, inside the absolute one
      const double s = gate_block(er, C, H, j, inv);
      const double l = -0.691 + 10.0 * log10(s);
      if (l > -70.0 && l > gamma) {
        v += s;
        n += 1.0;
      }
    }
    gate_reduce(sh, shn, v, n);
    if (n > 0.0) out = -0.691 + 10.0 * log10(v / n);
  }
  if (threadIdx.x == 0) lufs[blockIdx.x] = out;
}

__device__ __forceinline__ float gain_limit(float v, int limit) {
  if (limit == JEN1_LIMIT_CLIP) return fminf(fmaxf(v, -1.0f), 1.0f);
  if (limit == JEN1_LIMIT_TANH) return tanhf(v);
  return v;
}

__global__ __launch_bounds__(GAIN_THREADS) void gain_apply_kernel(const float* x, float* y, float* __restrict__ gain,
                                                                  const double* __restrict__ lufs, const double* __restrict__ stats,
                                                                  const double* __restrict__ target, long long n_row, double count,
                                                                  int strategy, int limit, double headroom_db, double energy_floor, int tiles) {
  const long long row = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  // every workgroup of a row forms the row's gain from the same words with the same operations: the same float
  double g = 1.0;
  if (strategy == JEN1_GAIN_LOUDNESS) {
    const double l = lufs[row], rms = sqrt(stats[row * 2] / count);
    if (l > -INFINITY && l < INFINITY && rms >= energy_floor) g = pow(10.0, (target[row] - l) / 20.0);
  } else if (strategy == JEN1_GAIN_PEAK) {
    const double peak = stats[row * 2 + 1];
    if (peak > 0.0) g = pow(10.0, -headroom_db / 20.0) / peak;
  } else if (strategy == JEN1_GAIN_RMS) {
    const double rms = sqrt(stats[row * 2] / count);
    if (rms > 0.0) g = pow(10.0, -headroom_db / 20.0) / rms;
  }
  const float gf = (float)g;
  if (tile == 0 && threadIdx.x == 0) gain[row] = gf;
  const long long a0 = tile * GAIN_TILE;
  const long long a1 = a0 + GAIN_TILE < n_row ? a0 + GAIN_TILE : n_row;
  const float* xr = x + row * n_row;
  float* yr = y + row * n_row;
  // a row starts at an arbitrary float: scalar up to the first 16-byte boundary of x, float4 behind it when y shares the alignment
  const bool same = ((reinterpret_cast<uintptr_t>(xr + a0) ^ reinterpret_cast<uintptr_t>(yr + a0)) & 15u) == 0;
  if (same) {
    long long head = (long long)((16u - (reinterpret_cast<uintptr_t>(xr + a0) & 15u)) & 15u) / 4;
    head = head < a1 - a0 ? head : a1 - a0;
    if (threadIdx.x < head) yr[a0 + threadIdx.x] = gain_limit(gf * xr[a0 + threadIdx.x], limit);
    const long long b0 = a0 + head, n4 = (a1 - b0) / 4;
    for (long long i = threadIdx.x; i < n4; i += GAIN_THREADS) {
      const float4 v = *reinterpret_cast<const float4*>(xr + b0 + i * 4);
      *reinterpret_cast<float4*>(yr + b0 + i * 4) =
          make_float4(gain_limit(gf * v.x, limit), gain_limit(gf * v.y, limit), gain_limit(gf * v.z, limit), gain_limit(gf * v.w, limit));
    }
    const long long t0 = b0 + n4 * 4;
    if (t0 + threadIdx.x < a1) yr[t0 + threadIdx.x] = gain_limit(gf * xr[t0 + threadIdx.x], limit);
  } else {
    for (long long i = a0 + threadIdx.x; i < a1; i += GAIN_THREADS) yr[i] = gain_limit(gf * xr[i], limit);
  }
}

// the cascade's state matrix A (s[i + 1] = A s[i] + B x[i]) and its power, on the host in float64
void kw_state_matrix(const double* k, double* A) {
  const double a1 = k[3], a2 = k[4], c0 = k[5], c1 = k[6], c2 = k[7], d1 = k[8], d2 = k[9];
  const double m[16] = {-a1, 1.0, 0.0, 0.0,
                        -a2, 0.0, 0.0, 0.0,
                        c1 - d1 * c0, 0.0, -d1, 1.0,
                        c2 - d2 * c0, 0.0, -d2, 0.0};
  memcpy(A, m, sizeof(m));
}
void kw_matmul(const double* a, const double* b, double* o) {
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double acc = 0.0;
      for (int t = 0; t < 4; ++t) acc += a[4 * i + t] * b[4 * t + j];
      r[4 * i + j] = acc;
    }
  memcpy(o, r, sizeof(r));
}
void kw_matpow(const double* A, long long p, double* o) {
  double base[16], acc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  memcpy(base, A, sizeof(base));
  while (p > 0) {
    if (p & 1) kw_matmul(acc, base, acc);
    kw_matmul(base, base, base);
    p >>= 1;
  }
  memcpy(o, acc, sizeof(acc));
}

struct KwPlan {
  int N, pitch, T, P;
  long long nch, tiles, lines, K;
};
inline KwPlan kw_plan(int rows, int C, long long L, int hop) {
  KwPlan p;
  p.N = kw_chunk(hop);
  p.pitch = kw_pitch(p.N);
  p.T = kw_tile_chunks(p.N);
  p.P = hop / p.N;
  p.nch = (L + p.N - 1) / p.N;
  p.tiles = p.T > 0 ? (p.nch + p.T - 1) / p.T : 0;
  p.lines = (long long)rows * C;
  p.K = (p.nch + KW_CARRY_THREADS - 1) / KW_CARRY_THREADS;
  return p;
}
// doubles: states [lines][4][slots], sum x^2 [lines][slots], max |x| [lines][slots] (slots = 256 K >= nch, kw_slot), chunk energies
// [lines][nch], per-line statistics [lines][2]
inline long long kw_workspace_doubles(const KwPlan& p) { return p.lines * (p.K * KW_CARRY_THREADS * 6 + p.nch + 2); }

}  // namespace

extern "C" int jen1_kweight_chunk(int hop) { return kw_chunk(hop); }

extern "C" int jen1_kweight_tile_chunks(int hop) { return hop >= 1 ? kw_tile_chunks(kw_chunk(hop)) : 0; }

extern "C" int64_t jen1_kweight_energy_workspace_bytes(int rows, int C, int64_t L, int hop) {
  if (rows < 0 || (C != 1 && C != 2) || L < 1 || L >= (1ll << 40) || hop < 1) return 0;
  return kw_workspace_doubles(kw_plan(rows, C, L, hop)) * (long long)sizeof(double);
}

extern "C" int jen1_kweight_energy(const float* x, double* e, double* stats, const double* coef, int rows, int C, int64_t L, int hop,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  JEN1_CHECK(C == 1 || C == 2, "jen1_kweight_energy: C = %d, must be 1 or 2", C);
  JEN1_CHECK(hop >= 1, "jen1_kweight_energy: hop = %d, must be positive", hop);
  JEN1_CHECK(rows >= 0 && L >= 1 && L < (1ll << 40), "jen1_kweight_energy: bad shape (rows %d, L %lld)", rows, (long long)L);
  const long long H = L / hop;
  JEN1_CHECK(x != nullptr && stats != nullptr && coef != nullptr && workspace != nullptr && (e != nullptr || H == 0),
             "jen1_kweight_energy: null pointer");
  for (int i = 0; i < 10; ++i) JEN1_CHECK(isfinite(coef[i]), "jen1_kweight_energy: coef[%d] is not finite", i);
  const KwPlan p = kw_plan(rows, C, L, hop);
  JEN1_CHECK(p.T >= 1, "jen1_kweight_energy: hop = %d has no divisor whose chunk (%d samples) fits the staging tile", hop, p.N);
  const long long need = kw_workspace_doubles(p) * (long long)sizeof(double);
  JEN1_CHECK(workspace_bytes >= need, "jen1_kweight_energy: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, need);
  JEN1_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "jen1_kweight_energy: workspace is not 8-byte aligned");
  JEN1_CHECK(p.tiles * p.lines < (1ll << 31) && p.lines * H < (1ll << 38), "jen1_kweight_energy: %lld tiles x %lld lines exceed the grid", p.tiles, p.lines);
  if (rows == 0) return 0;
  KwCoef k;
  memcpy(k.c, coef, sizeof(k.c));
  KwMat AN, ANK;
  double A[16];
  kw_state_matrix(coef, A);
  kw_matpow(A, p.N, AN.m);
  kw_matpow(AN.m, p.K, ANK.m);
  double* st = static_cast<double*>(workspace);
  const long long slots = p.K * KW_CARRY_THREADS;
  double* sx = st + p.lines * slots * 4;
  double* mx = sx + p.lines * slots;
  double* ce = mx + p.lines * slots;
  double* part = ce + p.lines * p.nch;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(p.tiles * p.lines));
  const size_t lds = (size_t)p.T * p.pitch * sizeof(float);
  hipLaunchKernelGGL((kw_chunk_kernel<false>), grid, dim3(KW_THREADS), lds, s, x, st, sx, mx, ce, k, (long long)L, p.N, p.pitch, p.T, p.nch, (int)p.tiles, p.K);
  hipLaunchKernelGGL(kw_carry_kernel, dim3((unsigned)p.lines), dim3(KW_CARRY_THREADS), 0, s, st, sx, mx, part, AN, ANK, p.nch, p.K);
  hipLaunchKernelGGL((kw_chunk_kernel<true>), grid, dim3(KW_THREADS), lds, s, x, st, sx, mx, ce, k, (long long)L, p.N, p.pitch, p.T, p.nch, (int)p.tiles, p.K);
  long long work = p.lines * H;
  work = work > rows ? work : rows;
  hipLaunchKernelGGL(kw_hops_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, ce, part, e, stats, rows, C, H, p.nch, p.P);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_loudness_gate(const double* e, double* lufs, int rows, int C, int64_t H, int hop, void* stream) {
  JEN1_CHECK(C == 1 || C == 2, "jen1_loudness_gate: C = %d, must be 1 or 2", C);
  JEN1_CHECK(hop >= 1, "jen1_loudness_gate: hop = %d, must be positive", hop);
  JEN1_CHECK(rows >= 0 && H >= 0 && H < (1ll << 36), "jen1_loudness_gate: bad shape (rows %d, H %lld)", rows, (long long)H);
  JEN1_CHECK(lufs != nullptr && (e != nullptr || H == 0), "jen1_loudness_gate: null pointer");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(loudness_gate_kernel, dim3((unsigned)rows), dim3(GATE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), e, lufs, C, (long long)H, hop);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_gain_apply(const float* x, float* y, float* gain, const double* lufs, const double* stats, const double* target, int rows,
                               int C, int64_t L, int strategy, int limit, double headroom_db, double energy_floor, void* stream) {
  JEN1_CHECK(C == 1 || C == 2, "jen1_gain_apply: C = %d, must be 1 or 2", C);
  JEN1_CHECK(strategy >= JEN1_GAIN_LOUDNESS && strategy <= JEN1_GAIN_CLIP, "jen1_gain_apply: strategy = %d is not a JEN1_GAIN_* value", strategy);
  JEN1_CHECK(limit >= JEN1_LIMIT_NONE && limit <= JEN1_LIMIT_TANH, "jen1_gain_apply: limit = %d is not a JEN1_LIMIT_* value", limit);
  JEN1_CHECK(rows >= 0 && L >= 1 && L < (1ll << 40), "jen1_gain_apply: bad shape (rows %d, L %lld)", rows, (long long)L);
  JEN1_CHECK(x != nullptr && y != nullptr && gain != nullptr, "jen1_gain_apply: null pointer");
  JEN1_CHECK(strategy != JEN1_GAIN_LOUDNESS || (lufs != nullptr && target != nullptr), "jen1_gain_apply: null pointer (lufs / target of the loudness strategy)");
  JEN1_CHECK(strategy == JEN1_GAIN_CLIP || stats != nullptr, "jen1_gain_apply: null pointer (stats)");
  JEN1_CHECK(isfinite(headroom_db) && energy_floor >= 0.0, "jen1_gain_apply: headroom_db / energy_floor out of range");
  if (rows == 0) return 0;
  const long long n_row = (long long)C * L, tiles = (n_row + GAIN_TILE - 1) / GAIN_TILE;
  JEN1_CHECK(tiles * rows < (1ll << 31), "jen1_gain_apply: %lld tiles x %d rows exceed the grid", tiles, rows);
  hipLaunchKernelGGL(gain_apply_kernel, dim3((unsigned)(tiles * rows)), dim3(GAIN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), x, y, gain,
                     lufs, stats, target, n_row, (double)n_row, strategy, limit, headroom_db, energy_floor, (int)tiles);
  JEN1_HIP(hipGetLastError());
  return 0;
}
