// Whitening of the codec latents (include/jen1_hip.h: jen1_latent_moments, jen1_latent_affine; jen1_amd/normalizer.py).  The reference
// has only an empty stub (jen1/normalizer.py); the statistics and the map are the JEN-1 paper's: zero mean per channel, identity covariance.
//
//   moments   z [B][C][T] float32 -> n, S1[c] = sum z_c, S2[c][d] = sum z_c z_d, ADDED to a float64 state [1 + C + C C].
//     latent_moments_kernel   one workgroup per run of MOM_RUN frames of one row: the run's [C][frames] block staged in LDS (frames
//       beyond the row's length are staged as zeros and add nothing), Z Z^T of the run on v_mfma_f64_16x16x4_f64 -- a product of two
//       float32 values is exact in float64, so the only rounding is in the sums.  Only the 16 x 16 tiles on or above the diagonal
//       are formed (36 of 64 at C = 128, 9 per wave); the result goes to the workgroup's own float64 partial.
//     latent_moments_reduce   one thread per word of the state: the partials in ascending order, then state += sum.  Element (c, d)
//       with c > d reads the partial of (d, c): S2 is symmetric bit for bit by construction.
//     No atomics, no workgroup waits on another, every sum has one fixed order: the same bits on every run.
//
//   affine    y[b, :, t] = A (z[b, :, t] - pre) + post on v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain).  A workgroup
//     stages A once (64 KiB at C = 128) and runs tiles of AFF_TILE frames through it: the tile's C channels minus pre into LDS, a
//     barrier, the products, then the stores -- every channel of a frame is read before any is written and a tile belongs to one
//     workgroup, so y may alias z.  With A = I and no pre / post every output is fma(1, z, 0) behind exact zeros: the input.
#include "common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int LN_THREADS = 256;                 // 4 waves
constexpr int LN_WAVES = LN_THREADS / JEN1_WAVE;
constexpr int LN_CMAX = 128;
constexpr int MOM_RUN = 128;                    // frames per workgroup
constexpr int MOM_PITCH = MOM_RUN + 4;          // lane (i, g) of an operand read hits bank 4 i + g: all 64 distinct
constexpr int MOM_WAVE_TILES = 9;               // 36 upper-triangle tiles of C = 128 over 4 waves
constexpr int LEN_PACK = 256;                   // lengths that ride in one launch's arguments
constexpr int AFF_TILE = 64;                    // frames per tile: 16 per wave
constexpr int AFF_ZPITCH = AFF_TILE + 16;       // operand read of lane (i, g): bank 16 g + i
constexpr int AFF_MAX_GRID = 256;               // one workgroup per CU holds A

struct LenPack {
  int v[LEN_PACK];
};

inline bool ln_channels_ok(int C) { return C >= 16 && C <= LN_CMAX && C % 16 == 0; }
inline long long mom_runs(int T) { return ((long long)T + MOM_RUN - 1) / MOM_RUN; }
inline long long mom_words(int C) { return 1ll + C + (long long)C * C; }
inline long long mom_partial_bytes(int B, int C, int T) { return (long long)B * mom_runs(T) * mom_words(C) * (long long)sizeof(double); }

// the host's lengths reach the device in the launch arguments: no copy, no synchronisation
__global__ __launch_bounds__(LEN_PACK) void latent_lengths_kernel(int* __restrict__ dst, LenPack p, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = p.v[threadIdx.x];
}

__global__ __launch_bounds__(LN_THREADS) void latent_moments_kernel(const float* __restrict__ z, const int* __restrict__ lengths,
                                                                    double* __restrict__ part, int C, int T, int runs) {
  extern __shared__ __attribute__((aligned(16))) float zs[];          // [C][MOM_PITCH]
  const int b = blockIdx.x / runs, t0 = (blockIdx.x % runs) * MOM_RUN;
  const int len = lengths != nullptr ? lengths[b] : T;                // 0 <= len <= T (the launcher's check)
  int nv = len - t0;                                                  // valid frames of this run
  nv = nv < 0 ? 0 : (nv > MOM_RUN ? MOM_RUN : nv);
  const float* zb = z + (long long)b * C * T + t0;
  for (int i = threadIdx.x; i < C * MOM_RUN; i += LN_THREADS) {
    const int c = i / MOM_RUN, f = i % MOM_RUN;
    zs[c * MOM_PITCH + f] = f < nv ? zb[(long long)c * T + f] : 0.f;
  }
  __syncthreads();
  double* out = part + (long long)blockIdx.x * (1 + C + C * C);
  const int lane = threadIdx.x % JEN1_WAVE, w = threadIdx.x / JEN1_WAVE, i = lane & 15, g = lane >> 4;
  const int nt = C / 16, ntri = nt * (nt + 1) / 2;
  // tile s of this wave is upper-triangle tile w + 4 s, counted row by row: (ti, tj), ti <= tj
  int ra[MOM_WAVE_TILES], rb[MOM_WAVE_TILES];
  f64x4 acc[MOM_WAVE_TILES];
#pragma unroll
  for (int s = 0; s < MOM_WAVE_TILES; ++s) {
    int ti = 0, r = w + LN_WAVES * s;
    if (r < ntri) {
      while (r >= nt - ti) {
        r -= nt - ti;
        ++ti;
      }
      ra[s] = ti * 16;
      rb[s] = (ti + r) * 16;
    } else {
      ra[s] = rb[s] = -1;
    }
    acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  const int kend = (nv + 3) & ~3;                                     // (frames nv .. kend - 1 are staged zeros)
  for (int k = 0; k < kend; k += 4) {
#pragma unroll
    for (int s = 0; s < MOM_WAVE_TILES; ++s) {
      if (ra[s] >= 0) {                                               // (uniform over the wave)
        // A[i][k] = z[ti 16 + i][k], B[k][j] = z[tj 16 + j][k]: lane (i, g) holds row i, frame k + g of both
        const double a = (double)zs[(ra[s] + i) * MOM_PITCH + k + g];
        const double bb = (double)zs[(rb[s] + i) * MOM_PITCH + k + g];
        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bb, acc[s], 0, 0, 0);
      }
    }
  }
  // the f64 form's own C/D map: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
  for (int s = 0; s < MOM_WAVE_TILES; ++s) {
    if (ra[s] >= 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[1 + C + (ra[s] + g + 4 * r) * C + rb[s] + i] = acc[s][r];
    }
  }
  if ((int)threadIdx.x < C) {                                         // S1: the row's frames in one fixed order, rotated by the channel
    const int c = threadIdx.x;                                        // so that the lanes of a wave read distinct banks
    double s1 = 0.0;
    for (int j = 0; j < MOM_RUN; ++j) {
      const int f = (j + c) % MOM_RUN;
      s1 += (double)zs[c * MOM_PITCH + f];                            // (zeros beyond nv)
    }
    out[1 + c] = s1;
  }
  if (threadIdx.x == 0) out[0] = (double)nv;
}

__global__ __launch_bounds__(LN_THREADS) void latent_moments_reduce(const double* __restrict__ part, double* __restrict__ state, int C,
                                                                    int parts) {
  const int words = 1 + C + C * C;
  const int e = blockIdx.x * LN_THREADS + threadIdx.x;
  if (e >= words) return;
  int src = e;
  if (e >= 1 + C) {
    const int c = (e - 1 - C) / C, d = (e - 1 - C) % C;
    src = 1 + C + (c <= d ? c * C + d : d * C + c);
  }
  double sum = 0.0;
  for (int p = 0; p < parts; ++p) sum += part[(long long)p * words + src];
  state[e] += sum;
}

__global__ __launch_bounds__(LN_THREADS) void latent_affine_kernel(const float* z, float* y, const float* __restrict__ A,
                                                                   const float* __restrict__ pre, const float* __restrict__ post, int C,
                                                                   int T, int tiles_t, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int pa = C + 4;                                               // operand read of lane (i, g): bank 4 i + g
  float* As = sm;                                                     // [C][pa]
  float* zs = sm + C * pa;                                            // [C][AFF_ZPITCH]
  for (int e = threadIdx.x; e < C * C; e += LN_THREADS) As[(e / C) * pa + e % C] = A[e];
  const int lane = threadIdx.x % JEN1_WAVE, w = threadIdx.x / JEN1_WAVE, i = lane & 15, g = lane >> 4;
  const int nt = C / 16;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tiles_t, t0 = (tile % tiles_t) * AFF_TILE;
    const int nf = T - t0 < AFF_TILE ? T - t0 : AFF_TILE;
    const long long base = (long long)b * C * T + t0;
    __syncthreads();                                                  // the previous tile's operand reads are done
    for (int e = threadIdx.x; e < C * AFF_TILE; e += LN_THREADS) {
      const int c = e / AFF_TILE, f = e % AFF_TILE;
      float v = f < nf ? z[base + (long long)c * T + f] : 0.f;
      if (pre != nullptr) v -= pre[c];
      zs[c * AFF_ZPITCH + f] = v;
    }
    __syncthreads();                                                  // every channel of the tile's frames has been read
    f32x4 acc[LN_CMAX / 16];
#pragma unroll
    for (int m = 0; m < LN_CMAX / 16; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < C; k += 4) {
      const float bv = zs[(k + g) * AFF_ZPITCH + w * 16 + i];         // B[k][j]: channel k + g of frame 16 w + j
#pragma unroll
      for (int m = 0; m < LN_CMAX / 16; ++m)
        if (m < nt) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[(m * 16 + i) * pa + k + g], bv, acc[m], 0, 0, 0);
    }
    const int f = w * 16 + i;                                         // C/D: column = lane & 15, row = 4 (lane >> 4) + reg
    if (f < nf) {
#pragma unroll
      for (int m = 0; m < LN_CMAX / 16; ++m) {
        if (m < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = m * 16 + g * 4 + r;
            y[base + (long long)c * T + f] = post != nullptr ? acc[m][r] + post[c] : acc[m][r];
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int64_t jen1_latent_moments_workspace(int B, int C, int T) {
  if (B < 1 || T < 1 || !ln_channels_ok(C)) return 0;
  return mom_partial_bytes(B, C, T) + (((long long)B * (long long)sizeof(int) + 7) & ~7ll);
}

extern "C" int jen1_latent_moments(const float* z, const int32_t* lengths, double* state, void* workspace, int64_t workspace_bytes, int B,
                                   int C, int T, void* stream) {
  JEN1_CHECK(ln_channels_ok(C), "jen1_latent_moments: C = %d, must be a multiple of 16 in 16..%d", C, LN_CMAX);
  JEN1_CHECK(B >= 1 && T >= 1, "jen1_latent_moments: bad shape (B %d, T %d)", B, T);
  JEN1_CHECK(z != nullptr && state != nullptr && workspace != nullptr, "jen1_latent_moments: null pointer");
  if (lengths != nullptr)
    for (int b = 0; b < B; ++b)
      JEN1_CHECK(lengths[b] >= 0 && lengths[b] <= T, "jen1_latent_moments: lengths[%d] = %d is outside 0..T = %d", b, lengths[b], T);
  const long long need = jen1_latent_moments_workspace(B, C, T);
  JEN1_CHECK(workspace_bytes >= need, "jen1_latent_moments: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, need);
  JEN1_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "jen1_latent_moments: workspace is not 8-byte aligned");
  const long long runs = mom_runs(T), parts = (long long)B * runs;
  JEN1_CHECK(parts < (1ll << 31), "jen1_latent_moments: %lld runs exceed the grid", parts);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  int* dlen = nullptr;
  if (lengths != nullptr) {
    dlen = reinterpret_cast<int*>(static_cast<char*>(workspace) + mom_partial_bytes(B, C, T));
    for (int b0 = 0; b0 < B; b0 += LEN_PACK) {
      LenPack p;
      const int n = B - b0 < LEN_PACK ? B - b0 : LEN_PACK;
      memset(p.v, 0, sizeof(p.v));
      memcpy(p.v, lengths + b0, (size_t)n * sizeof(int));
      hipLaunchKernelGGL(latent_lengths_kernel, dim3(1), dim3(LEN_PACK), 0, s, dlen + b0, p, n);
    }
  }
  const size_t lds = (size_t)C * MOM_PITCH * sizeof(float);
  JEN1_MAX_LDS_ONCE(latent_moments_kernel, (int)(LN_CMAX * MOM_PITCH * sizeof(float)));
  hipLaunchKernelGGL(latent_moments_kernel, dim3((unsigned)parts), dim3(LN_THREADS), lds, s, z, dlen, part, C, T, (int)runs);
  const int words = (int)mom_words(C);
  hipLaunchKernelGGL(latent_moments_reduce, dim3((unsigned)((words + LN_THREADS - 1) / LN_THREADS)), dim3(LN_THREADS), 0, s, part, state, C,
                     (int)parts);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_latent_affine(const float* z, float* y, const float* A, const float* pre, const float* post, int B, int C, int T,
                                  void* stream) {
  JEN1_CHECK(ln_channels_ok(C), "jen1_latent_affine: C = %d, must be a multiple of 16 in 16..%d", C, LN_CMAX);
  JEN1_CHECK(B >= 1 && T >= 1, "jen1_latent_affine: bad shape (B %d, T %d)", B, T);
  JEN1_CHECK(z != nullptr && y != nullptr && A != nullptr, "jen1_latent_affine: null pointer");
  const long long tiles_t = ((long long)T + AFF_TILE - 1) / AFF_TILE, ntiles = tiles_t * B;
  JEN1_CHECK(ntiles < (1ll << 31), "jen1_latent_affine: %lld tiles exceed the grid", ntiles);
  const size_t lds = ((size_t)C * (C + 4) + (size_t)C * AFF_ZPITCH) * sizeof(float);
  JEN1_MAX_LDS_ONCE(latent_affine_kernel, (int)((LN_CMAX * (LN_CMAX + 4) + LN_CMAX * AFF_ZPITCH) * sizeof(float)));
  const unsigned grid = (unsigned)(ntiles < AFF_MAX_GRID ? ntiles : AFF_MAX_GRID);
  hipLaunchKernelGGL(latent_affine_kernel, dim3(grid), dim3(LN_THREADS), lds, reinterpret_cast<hipStream_t>(stream), z, y, A, pre, post, C, T,
                     (int)tiles_t, (int)ntiles);
  JEN1_HIP(hipGetLastError());
  return 0;
}
