// The VGGish embedder of the Frechet Audio Distance (include/jen1_fad.h; jen1_amd/fad.py).  Not in the reference.  Float32 NHWC
// activations [N][H][W][C], H = frames, W = mel bands; float32 accumulation everywhere.
//
//   vggish_conv1_kernel   Cin = 1, K = 9: the vector ALU.  A workgroup takes 4 pooled rows of one example: the 10 x 66 patch of the
//     linear mel (jen1_mel's [rows][64][frames]) goes through log(v + 0.01) into LDS, zeros outside the example; every thread then forms
//     one pooled output at a time -- the four 3 x 3 sums of its 2 x 2 window (taps in ascending order), bias, ReLU, max -- with the
//     channel on the fastest thread index, so NHWC stores are contiguous.
//
//   conv3x3_kernel   implicit GEMM over K = 9 Cin on v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain).  A workgroup (4 waves)
//     owns an 8 x 8 block of positions of ONE example (even-aligned: whole pooling windows) and 64 output channels.  Per chunk of 16
//     input channels it stages the 10 x 10 halo block [pixel][16 + 4] (pixels outside the tensor: zeros by a predicate, never loaded)
//     and the chunk's packed weights [tap][c4][n tile][64 lanes]; the nine taps are nine LDS offsets.  M = positions, N = channels:
//       position p = 4 q + 2 dy + dx of M tile t is pixel (2 t + dy, 2 q + dx)   -- an M tile is two rows of the block
//     so the four accumulator registers of a lane (rows 4 (lane / 16) + r of the C/D map) are exactly one 2 x 2 pooling window and the
//     pool is a max over registers; the column of the map is the channel, so 16 lanes store 64 contiguous bytes.  A wave holds 2 x 2
//     tiles: four independent accumulators (the 16x16x4 form needs two to reach its issue rate), two A and two B reads per four
//     instructions.  The next chunk's global loads are issued before the current chunk's products and land in registers.
//     LDS pitches: a pixel is 20 floats and a pixel row 224 = 32 (mod 64), so lane (i, g) of an A read hits bank 20 col + 32 dy + g
//     (mod 64) with col = 0..7: 20 col = 4 (5 col mod 16) are eight distinct multiples of 4 whose slots 5 col mod 16 never differ by 8,
//     so the second row's + 32 falls on the other eight: all 64 lanes on distinct banks.  The B read is 64 consecutive floats.
//     K order: chunk, tap, channel -- fixed; no atomics, no split over K.  A chunk's 144 products are summed from zero and the chunk
//     sums are added in ascending order: chains of 144 fmas and Cin / 16 adds instead of one chain of 9 Cin (the rounding error of a
//     float32 chain grows with its length; K reaches 4608 here).
#include "common.h"
#include "jen1_fad.h"

namespace {

constexpr int CV_THREADS = 256;
constexpr int CV_TB = 8;                            // block side in positions
constexpr int CV_HALO = CV_TB + 2;
constexpr int CV_KC = JEN1_CONV3X3_KC;
constexpr int CV_BN = JEN1_CONV3X3_BN;
constexpr int CV_P = CV_KC + 4;                     // floats per staged pixel
constexpr int CV_ROWP = 224;                        // floats per staged pixel row: >= 10 * 20, and 32 (mod 64)
constexpr int CV_XS = CV_HALO * CV_ROWP;
constexpr int CV_WS = 9 * (CV_KC / 4) * (CV_BN / 16) * 64;      // floats of one (channel group, chunk) block of the packed weights
constexpr int CV_XV = CV_HALO * CV_HALO * (CV_KC / 4);          // float4 loads of the input block
constexpr int CV_XR = (CV_XV + CV_THREADS - 1) / CV_THREADS;
constexpr int CV_WR = CV_WS / 4 / CV_THREADS;
static_assert(CV_ROWP >= CV_HALO * CV_P && CV_ROWP % 64 == 32 && CV_P % 8 == 4, "the bank argument above");
static_assert(CV_WS % (4 * CV_THREADS) == 0, "whole float4 rounds");

constexpr int C1_THREADS = 256;
constexpr int C1_ROWS = 4;                          // pooled rows per workgroup
constexpr int C1_FR = 2 * C1_ROWS + 2;              // staged frames
constexpr int C1_BP = JEN1_VGGISH_BANDS + 2;        // staged bands
constexpr int C1_STRIPS = JEN1_VGGISH_FRAMES / 2 / C1_ROWS;
constexpr int C1_CMAX = 512;

inline bool channels_ok(int c) { return c >= 16 && c <= 512 && c % 16 == 0; }

__global__ __launch_bounds__(CV_THREADS) void conv3x3_kernel(const float* __restrict__ x, const float* __restrict__ packed,
                                                             const float* __restrict__ bias, float* __restrict__ y, int H, int W, int cin,
                                                             int cout, int pool, int bx, int nsb) {
  __shared__ __attribute__((aligned(16))) float xs[CV_XS];
  __shared__ __attribute__((aligned(16))) float ws[CV_WS];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / nsb, sb = blockIdx.x % nsb, grp = blockIdx.y;
  const int Y0 = (sb / bx) * CV_TB, X0 = (sb % bx) * CV_TB;
  const int Q = cin / CV_KC;
  const float* xn = x + (long long)n * H * W * cin;
  const float* wg = packed + (long long)grp * Q * CV_WS;

  // this thread's share of a chunk: CV_XR float4 of the halo block (zeros outside the tensor), CV_WR float4 of the weights
  int xdst[CV_XR];
  long long xsrc[CV_XR];                             // -1: not loaded
#pragma unroll
  for (int r = 0; r < CV_XR; ++r) {
    const int e = tid + r * CV_THREADS;
    xdst[r] = -1;
    xsrc[r] = -1;
    if (e < CV_XV) {
      const int pix = e / (CV_KC / 4), v = e % (CV_KC / 4);
      const int py = pix / CV_HALO, px = pix % CV_HALO;
      const int gy = Y0 - 1 + py, gx = X0 - 1 + px;
      xdst[r] = py * CV_ROWP + px * CV_P + 4 * v;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) xsrc[r] = ((long long)gy * W + gx) * cin + 4 * v;
    }
  }
  float4 xr[CV_XR], wr[CV_WR];
  auto fetch = [&](int q) {
#pragma unroll
    for (int r = 0; r < CV_XR; ++r)
      xr[r] = xsrc[r] >= 0 ? *reinterpret_cast<const float4*>(xn + xsrc[r] + q * CV_KC) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* wq = reinterpret_cast<const float4*>(wg + (long long)q * CV_WS);
#pragma unroll
    for (int r = 0; r < CV_WR; ++r) wr[r] = wq[tid + r * CV_THREADS];
  };

  const int lane = tid % JEN1_WAVE, wv = tid / JEN1_WAVE, i = lane & 15, g4 = lane >> 4;
  const int mt0 = (wv & 1) * 2, nt0 = (wv >> 1) * 2;
  const int left = (cout - grp * CV_BN) / 16;        // valid channel tiles of this group (>= 1)
  bool m_ok[2], n_ok[2];
  int aoff[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    m_ok[m] = Y0 + 2 * (mt0 + m) < H;                // (uniform over the wave) an M tile below the tensor is not multiplied
    n_ok[m] = nt0 + m < left;
    aoff[m] = (2 * (mt0 + m) + ((i >> 1) & 1)) * CV_ROWP + (2 * (i >> 2) + (i & 1)) * CV_P + g4;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) acc[m][nn] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  for (int q = 0; q < Q; ++q) {
    __syncthreads();                                 // the previous chunk's operand reads are done
#pragma unroll
    for (int r = 0; r < CV_XR; ++r)
      if (xdst[r] >= 0) *reinterpret_cast<float4*>(xs + xdst[r]) = xr[r];
#pragma unroll
    for (int r = 0; r < CV_WR; ++r) reinterpret_cast<float4*>(ws)[tid + r * CV_THREADS] = wr[r];
    __syncthreads();
    if (q + 1 < Q) fetch(q + 1);
    f32x4 part[2][2];                                // the chunk's own sums: chains of 36 instructions, then one add into the total
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) part[m][nn] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = (tap / 3) * CV_ROWP + (tap % 3) * CV_P;
#pragma unroll
      for (int c4 = 0; c4 < CV_KC / 4; ++c4) {
        float a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) a[m] = xs[aoff[m] + toff + 4 * c4];
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) b[nn] = ws[((tap * (CV_KC / 4) + c4) * (CV_BN / 16) + nt0 + nn) * 64 + lane];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int nn = 0; nn < 2; ++nn)
            if (m_ok[m] && n_ok[nn]) part[m][nn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[nn], part[m][nn], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nn = 0; nn < 2; ++nn) acc[m][nn] += part[m][nn];
  }

  // C/D: column = lane & 15 = channel, row = 4 (lane >> 4) + reg = position: window lane >> 4 of the M tile, reg = 2 dy + dx
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  float* yn = y + (long long)n * Ho * Wo * cout;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int nn = 0; nn < 2; ++nn) {
      if (!(m_ok[m] && n_ok[nn])) continue;
      const int c = grp * CV_BN + (nt0 + nn) * 16 + i;
      const float bv = bias[c];
      const int y0 = Y0 + 2 * (mt0 + m), x0 = X0 + 2 * g4;
      if (pool) {
        if (y0 < H && x0 < W) {                      // H and W are even: the whole window is inside
          float v = 0.f;                             // max(relu(.)) = max(0, .)
#pragma unroll
          for (int r = 0; r < 4; ++r) v = fmaxf(v, acc[m][nn][r] + bv);
          yn[((long long)(y0 >> 1) * Wo + (x0 >> 1)) * cout + c] = v;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int yy = y0 + (r >> 1), xx = x0 + (r & 1);
          if (yy < H && xx < W) yn[((long long)yy * W + xx) * cout + c] = fmaxf(acc[m][nn][r] + bv, 0.f);
        }
      }
    }
  }
}

// example n of a run of rows with `epr` examples each: (row n / epr, first frame 96 (n % epr)); element (frame f, band m) of a row lies at
// m * frames + f of linear mel (logmel == 0: jen1_mel's layout) or at f * 64 + m of finished log-mel (logmel == 1: examples)
__device__ __forceinline__ const float* example_src(const float* src, long long frames, int epr, int n, int logmel, long long& sf, long long& sb) {
  const int row = n / epr, e = n % epr;
  sf = logmel ? JEN1_VGGISH_BANDS : 1;
  sb = logmel ? 1 : frames;
  return src + (long long)row * JEN1_VGGISH_BANDS * frames + (long long)e * JEN1_VGGISH_FRAMES * sf;
}

__global__ __launch_bounds__(C1_THREADS) void vggish_conv1_kernel(const float* __restrict__ mel, long long frames, int epr, int skip, int logmel,
                                                                  const float* __restrict__ w, const float* __restrict__ bias,
                                                                  float* __restrict__ y, int cout) {
  __shared__ float ps[C1_FR * C1_BP];                 // [frame][band + 1], log(mel + 0.01), zeros outside the example
  __shared__ float wsm[10 * C1_CMAX];                 // [9 taps + bias][cout]
  const int n = blockIdx.x / C1_STRIPS, s = blockIdx.x % C1_STRIPS;
  long long sf, sb;
  const float* src = example_src(mel, frames, epr, n + skip, logmel, sf, sb);
  const int f0 = 2 * C1_ROWS * s - 1;                 // first staged frame of the example
  for (int k = threadIdx.x; k < C1_FR * C1_BP; k += C1_THREADS) {
    const int fr = k % C1_FR, bp = k / C1_FR;         // frames are contiguous in mel
    const int f = f0 + fr, band = bp - 1;
    float v = 0.f;
    if (f >= 0 && f < JEN1_VGGISH_FRAMES && band >= 0 && band < JEN1_VGGISH_BANDS) {
      v = src[band * sb + f * sf];
      if (!logmel) v = logf(v + 0.01f);
    }
    ps[fr * C1_BP + bp] = v;
  }
  for (int k = threadIdx.x; k < 10 * cout; k += C1_THREADS) wsm[k] = k < 9 * cout ? w[k] : bias[k - 9 * cout];
  __syncthreads();
  constexpr int WO = JEN1_VGGISH_BANDS / 2, HO = JEN1_VGGISH_FRAMES / 2;
  float* yn = y + ((long long)n * HO + C1_ROWS * s) * WO * cout;
  for (int k = threadIdx.x; k < C1_ROWS * WO * cout; k += C1_THREADS) {
    const int c = k % cout, pos = k / cout, px = pos % WO, py = pos / WO;
    float p[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) p[a][b] = ps[(2 * py + a) * C1_BP + 2 * px + b];
    float wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = wsm[t * cout + c];
    const float bv = wsm[9 * cout + c];
    float best = 0.f;                                 // max(relu(.)) = max(0, .)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) sum = fmaf(wt[t], p[dy + t / 3][dx + t % 3], sum);
        best = fmaxf(best, sum + bv);
      }
    yn[k] = best;
  }
}

// examples [n][96][64] = log(mel + 0.01) of the frames of each example: one workgroup per example, reads along frames, writes along bands
__global__ __launch_bounds__(C1_THREADS) void vggish_examples_kernel(const float* __restrict__ mel, long long frames, int epr,
                                                                     float* __restrict__ out) {
  __shared__ float t[JEN1_VGGISH_BANDS * (JEN1_VGGISH_FRAMES + 1)];
  long long sf, sb;
  const float* src = example_src(mel, frames, epr, blockIdx.x, 0, sf, sb);
  for (int k = threadIdx.x; k < JEN1_VGGISH_BANDS * JEN1_VGGISH_FRAMES; k += C1_THREADS) {
    const int f = k % JEN1_VGGISH_FRAMES, m = k / JEN1_VGGISH_FRAMES;
    t[m * (JEN1_VGGISH_FRAMES + 1) + f] = logf(src[m * sb + f] + 0.01f);
  }
  __syncthreads();
  float* o = out + (long long)blockIdx.x * JEN1_VGGISH_FRAMES * JEN1_VGGISH_BANDS;
  for (int k = threadIdx.x; k < JEN1_VGGISH_BANDS * JEN1_VGGISH_FRAMES; k += C1_THREADS)
    o[k] = t[(k % JEN1_VGGISH_BANDS) * (JEN1_VGGISH_FRAMES + 1) + k / JEN1_VGGISH_BANDS];
}

__global__ __launch_bounds__(256) void vggish_relu_kernel(float* __restrict__ x, long long n) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < n) x[k] = fmaxf(x[k], 0.f);
}

}  // namespace

extern "C" int64_t jen1_conv3x3_packed_floats(int cin, int cout) {
  if (!channels_ok(cin) || !channels_ok(cout)) return 0;
  return (int64_t)((cout + CV_BN - 1) / CV_BN) * (cin / CV_KC) * CV_WS;
}

extern "C" int jen1_conv3x3(const float* x, const float* packed, const float* bias, float* y, int N, int H, int W, int cin, int cout, int pool,
                            void* stream) {
  JEN1_CHECK(channels_ok(cin) && channels_ok(cout), "jen1_conv3x3: cin = %d, cout = %d, must be multiples of 16 in 16..512", cin, cout);
  JEN1_CHECK(N >= 1 && H >= 1 && W >= 1, "jen1_conv3x3: bad shape (N %d, H %d, W %d)", N, H, W);
  JEN1_CHECK(pool == 0 || pool == 1, "jen1_conv3x3: pool = %d, must be 0 or 1", pool);
  JEN1_CHECK(!pool || (H % 2 == 0 && W % 2 == 0), "jen1_conv3x3: the 2x2 pool needs even H and W, not %d x %d", H, W);
  JEN1_CHECK(x != nullptr && packed != nullptr && bias != nullptr && y != nullptr, "jen1_conv3x3: null pointer");
  JEN1_CHECK(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(packed)) & 15u) == 0,
             "jen1_conv3x3: x and packed must be 16-byte aligned");
  const long long in_elems = (long long)N * H * W * cin, out_elems = (long long)N * (pool ? H / 2 : H) * (pool ? W / 2 : W) * cout;
  JEN1_CHECK(x + in_elems <= y || y + out_elems <= x, "jen1_conv3x3: x and y overlap");
  const int bx = (W + CV_TB - 1) / CV_TB, by = (H + CV_TB - 1) / CV_TB;
  const long long nsb = (long long)bx * by, blocks = nsb * N;
  JEN1_CHECK(blocks < (1ll << 31), "jen1_conv3x3: %lld position blocks exceed the grid", blocks);
  hipLaunchKernelGGL(conv3x3_kernel, dim3((unsigned)blocks, (unsigned)((cout + CV_BN - 1) / CV_BN)), dim3(CV_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), x, packed, bias, y, H, W, cin, cout, pool, bx, (int)nsb);
  JEN1_HIP(hipGetLastError());
  return 0;
}

namespace {
// the examples [first, first + n) of the rows, run by run of rows with one count: fn(first row of the run, its count, examples of the run to
// skip, examples to take, examples already taken)
template <typename F> void for_each_run(const int32_t* counts, int rows, long long first, long long n, F fn) {
  long long seen = 0, done = 0;
  for (int r0 = 0; r0 < rows && done < n;) {
    int r1 = r0 + 1;
    while (r1 < rows && counts[r1] == counts[r0]) ++r1;
    const long long in_run = (long long)(r1 - r0) * counts[r0];
    const long long lo = first + done > seen ? first + done - seen : 0;
    if (lo < in_run) {
      const long long take = in_run - lo < n - done ? in_run - lo : n - done;
      fn(r0, counts[r0], lo, take, done);
      done += take;
    }
    seen += in_run;
    r0 = r1;
  }
}

int check_counts(const char* who, const int32_t* counts, int rows, int64_t frames, long long& total) {
  JEN1_CHECK(rows >= 1 && frames >= 1, "%s: bad shape (rows %d, frames %lld)", who, rows, (long long)frames);
  JEN1_CHECK(counts != nullptr, "%s: counts is NULL", who);
  total = 0;
  for (int r = 0; r < rows; ++r) {
    JEN1_CHECK(counts[r] >= 0 && (long long)counts[r] * JEN1_VGGISH_FRAMES <= frames, "%s: counts[%d] = %d examples do not fit %lld frames", who, r,
               counts[r], (long long)frames);
    total += counts[r];
  }
  JEN1_CHECK(total < (1ll << 31) / C1_STRIPS, "%s: %lld examples exceed the grid", who, total);
  return 0;
}
}  // namespace

extern "C" int jen1_vggish_conv1(const float* src, const int32_t* counts, int rows, int64_t frames, int logmel, int64_t first, int64_t n,
                                 const float* w, const float* bias, float* y, int cout, void* stream) {
  JEN1_CHECK(channels_ok(cout), "jen1_vggish_conv1: cout = %d, must be a multiple of 16 in 16..512", cout);
  JEN1_CHECK(src != nullptr && w != nullptr && bias != nullptr && y != nullptr, "jen1_vggish_conv1: null pointer");
  JEN1_CHECK(logmel == 0 || logmel == 1, "jen1_vggish_conv1: logmel = %d, must be 0 or 1", logmel);
  long long total = 0;
  if (check_counts("jen1_vggish_conv1", counts, rows, frames, total)) return 1;
  JEN1_CHECK(first >= 0 && n >= 1 && first + n <= total, "jen1_vggish_conv1: examples [%lld, %lld) of %lld", (long long)first,
             (long long)(first + n), total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long long per_example = (long long)(JEN1_VGGISH_FRAMES / 2) * (JEN1_VGGISH_BANDS / 2) * cout;
  for_each_run(counts, rows, first, n, [&](int r0, int epr, long long skip, long long take, long long done) {
    hipLaunchKernelGGL(vggish_conv1_kernel, dim3((unsigned)(take * C1_STRIPS)), dim3(C1_THREADS), 0, s,
                       src + (long long)r0 * JEN1_VGGISH_BANDS * frames, (long long)frames, epr, (int)skip, logmel, w, bias, y + done * per_example,
                       cout);
  });
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_vggish_examples(const float* mel, const int32_t* counts, int rows, int64_t frames, float* out, void* stream) {
  JEN1_CHECK(mel != nullptr && out != nullptr, "jen1_vggish_examples: null pointer");
  long long total = 0;
  if (check_counts("jen1_vggish_examples", counts, rows, frames, total)) return 1;
  JEN1_CHECK(total >= 1, "jen1_vggish_examples: no example in any row");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for_each_run(counts, rows, 0, total, [&](int r0, int epr, long long skip, long long take, long long done) {
    (void)skip;
    hipLaunchKernelGGL(vggish_examples_kernel, dim3((unsigned)take), dim3(C1_THREADS), 0, s, mel + (long long)r0 * JEN1_VGGISH_BANDS * frames,
                       (long long)frames, epr, out + done * JEN1_VGGISH_FRAMES * JEN1_VGGISH_BANDS);
  });
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_vggish_relu(float* x, int64_t n, void* stream) {
  JEN1_CHECK(x != nullptr && n >= 1, "jen1_vggish_relu: null pointer or n = %lld", (long long)n);
  const long long blocks = ((long long)n + 255) / 256;
  JEN1_CHECK(blocks < (1ll << 31), "jen1_vggish_relu: %lld elements exceed the grid", (long long)n);
  hipLaunchKernelGGL(vggish_relu_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, (long long)n);
  JEN1_HIP(hipGetLastError());
  return 0;
}
