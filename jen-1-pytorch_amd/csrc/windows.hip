// Long-form sampling on overlapping windows (include/jen1_hip.h: jen1_window_merge, jen1_window_gather; jen1_amd/windows.py).
//
// The latents of a piece live on a canvas [n][C][L]; the sampler denoises W windows of T frames per piece as ordinary batch rows
// [n W][C][T] (row s W + j = window j of piece s, starting at canvas frame offsets[j]).  After every sampler update the windows are
// averaged where they overlap and set back to the average, so all of them are crops of one canvas again:
//
//   k(p)  = min(p + 1, T - p, ramp)                       integer cross-fade weight of window position p
//   acc   = fmaf((float)k_j, x_j, acc)  from acc = 0,     over the windows j covering canvas frame l, ascending j, p = l - offsets[j]
//   m     = acc / (float)(sum k_j)                        written to every covering row element (and to canvas[s][c][l])
//
// A frame covered by one window is not recomputed (k x / k is not always x): its row element keeps its bits.
//
// One thread owns a canvas element and is the only one to read or write the row elements
// lying on it -- row element (j, p) lies on canvas frame offsets[j] + p and on no other.  So the launch works in place without a
// second buffer, has no race, and every sum runs in one fixed order: the same bits on every run.
//
// Why this is a launch of its own and not part of pack_input_kernel (csrc/elementwise.hip), which reads the same latents next: a block
// there owns rows of ONE window, and the merged value of its frames needs the neighbouring windows' elements, which the neighbours'
// blocks overwrite with their own merged values in the same launch -- a read of either the old or the new value, whichever block ran
// first.  Here the ownership follows the canvas, not the window.
//
// Both kernels only move bytes (4 B read + 4 B written per covered row element, ~no arithmetic).  The gather, which also copies the
// whole per-step noise table (hundreds of MB), moves four frames per lane: one 16-byte store (T a multiple of four) and one 16-byte
// load where the canvas address allows -- a canvas row starts at a multiple of L floats, which need not be one of four (L = 6750).
// The merge moves ONE frame per lane.  A form with four frames per lane (16-byte accesses wherever a window's offset is a multiple of
// four) was built and measured at the long-form shape (n = 1, W = 8, C = 128, T = 1500, L = 6750: 10.75 MB moved): 11.3 us against
// 8.1 us for this one.  At that size the launch is bound by the latency of its dependent loads, not by bandwidth, and four times
// the threads hide it better; larger n has not been measured.
#include "common.h"

namespace {

constexpr int WM_THREADS = 256;
constexpr int WM_MAX_BLOCKS = 8192;          // beyond it a block strides over the work
constexpr int WM_MAX_WINDOWS = 8192;         // offsets staged in LDS by the merge: 32 KiB

__host__ __device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ int win_k(int p, int T, int ramp) {
  const int a = p + 1 < T - p ? p + 1 : T - p;
  return a < ramp ? a : ramp;
}

// first j with offs[j] > v (offs ascending, in LDS): the windows covering frame l are ub(l - T) .. ub(l) - 1
__device__ __forceinline__ int ub(const int* offs, int W, int v) {
  int lo = 0, hi = W;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] > v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// one canvas element; ``row0`` = rows + ((s W) C + c) T: the element's channel in window 0 of its piece, windows C T floats apart.
// Every access is guarded by 0 <= p < T, so a table that is not ascending costs coverage, never an access outside a row
__device__ __forceinline__ void merge_one(float* __restrict__ row0, const int* offs, float* __restrict__ cv, int l, int W, long long win_stride,
                                          int T, int ramp) {
  const int jlo = ub(offs, W, l - T), jhi = ub(offs, W, l) - 1;
  float acc = 0.f, first = 0.f;
  int ksum = 0, cnt = 0;
  for (int j = jlo; j <= jhi; ++j) {
    const int p = l - offs[j];
    if ((unsigned)p >= (unsigned)T) continue;
    const float x = row0[j * win_stride + p];
    const int k = win_k(p, T, ramp);
    acc = fmaf((float)k, x, acc);
    ksum += k;
    if (cnt == 0) first = x;
    ++cnt;
  }
  if (cnt == 0) return;                                            // (a gap in the offsets: the host refuses such a plan)
  const float m = cnt == 1 ? first : acc / (float)ksum;
  if (cv != nullptr) cv[l] = m;
  if (cnt == 1) return;
  for (int j = jlo; j <= jhi; ++j) {
    const int p = l - offs[j];
    if ((unsigned)p < (unsigned)T) row0[j * win_stride + p] = m;
  }
}

// one work item = one canvas element.  The offsets are staged in LDS once per block (W ints of dynamic LDS): read from global memory
// inside the loops they are one dependent scalar load per window and loop
__global__ __launch_bounds__(WM_THREADS) void window_merge_kernel(float* __restrict__ rows, const int32_t* __restrict__ offsets,
                                                                   float* __restrict__ canvas, long long items, int W, int C, int T, int L,
                                                                   int ramp) {
  extern __shared__ int offs[];
  for (int j = threadIdx.x; j < W; j += WM_THREADS) offs[j] = offsets[j];
  __syncthreads();
  const long long win_stride = (long long)C * T;
  for (long long it = (long long)blockIdx.x * WM_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * WM_THREADS) {
    const long long sc = it / L;                                   // s C + c
    const int l = (int)(it - sc * L), c = (int)(sc % C);
    const long long s = sc / C;
    merge_one(rows + (s * W * C + c) * (long long)T, offs, canvas == nullptr ? nullptr : canvas + sc * (long long)L, l, W, win_stride, T, ramp);
  }
}

// rows[z][s W + j][c][t] = canvas[z][s][c][off_j + t]; one work item = one row element (VEC, T % 4 == 0 and ``rows`` 16-byte aligned:
// four consecutive frames of a row, one 16-byte store, and one 16-byte load where the canvas address allows).  An offset outside
// [0, L - T] is clamped into it: the launch never reads outside the canvas whatever the table holds
template <bool VEC>
__global__ __launch_bounds__(WM_THREADS) void window_gather_kernel(const float* __restrict__ canvas, float* __restrict__ rows,
                                                                    const int32_t* __restrict__ offsets, long long items, int n, int W, int C,
                                                                    int T, int L) {
  const int per = VEC ? T / 4 : T;
  for (long long it = (long long)blockIdx.x * WM_THREADS + threadIdx.x; it < items; it += (long long)gridDim.x * WM_THREADS) {
    const long long rc = it / per;                                 // ((z n + s) W + j) C + c
    const int g = (int)(it - rc * per), c = (int)(rc % C);
    const long long r = rc / C;                                    // (z n + s) W + j
    const int j = (int)(r % W);
    const long long zs = r / W;                                    // z n + s
    int off = offsets[j];
    off = off < 0 ? 0 : (off > L - T ? L - T : off);
    const float* src = canvas + (zs * C + c) * (long long)L + off;
    float* dst = rows + rc * (long long)T;
    if (!VEC) {
      dst[g] = src[g];
    } else if (aligned16(src + 4 * g)) {
      *reinterpret_cast<float4*>(dst + 4 * g) = *reinterpret_cast<const float4*>(src + 4 * g);
    } else {
      const float a = src[4 * g], b = src[4 * g + 1], d = src[4 * g + 2], e = src[4 * g + 3];
      *reinterpret_cast<float4*>(dst + 4 * g) = make_float4(a, b, d, e);
    }
  }
}

inline unsigned wm_blocks(long long items) {
  const long long b = (items + WM_THREADS - 1) / WM_THREADS;
  return (unsigned)(b < WM_MAX_BLOCKS ? b : WM_MAX_BLOCKS);
}

// the shape checks both entry points share; ``lead`` = 1 for the merge
int window_shape_check(const char* who, long long lead, int n, int W, int C, int T, int L) {
  JEN1_CHECK(lead >= 1 && n >= 0 && C >= 1, "%s: bad shape (lead %lld, n %d, C %d)", who, lead, n, C);
  JEN1_CHECK(W >= 1, "%s: W = %d, must be at least 1", who, W);
  JEN1_CHECK(T >= 1 && T <= L, "%s: T = %d, must be in [1, L = %d]", who, T, L);
  JEN1_CHECK(L < (1 << 30), "%s: L = %d is too long", who, L);
  // element indices are 64-bit; the products below are formed in 64 bits and bounded so that they cannot wrap
  JEN1_CHECK((long long)n * W < (1ll << 31) && lead * n * W * (long long)C < (1ll << 40) && lead * n * W * (long long)C * T < (1ll << 46) &&
                 lead * n * (long long)C * L < (1ll << 46),
             "%s: lead %lld x n %d x W %d x C %d x T %d (canvas L %d) exceeds the index range", who, lead, n, W, C, T, L);
  return 0;
}

}  // namespace

extern "C" int jen1_window_merge(float* rows, const int32_t* offsets, int n, int W, int C, int T, int L, int ramp, float* canvas, void* stream) {
  JEN1_CHECK(rows != nullptr && offsets != nullptr, "jen1_window_merge: null pointer");
  if (int rc = window_shape_check("jen1_window_merge", 1, n, W, C, T, L)) return rc;
  JEN1_CHECK(ramp >= 1 && ramp <= T, "jen1_window_merge: ramp = %d, must be in [1, T = %d]", ramp, T);
  JEN1_CHECK((long long)W * ramp <= (1ll << 24), "jen1_window_merge: W x ramp = %lld: a sum of weights must stay exact in float32 (<= 2^24)",
             (long long)W * ramp);
  JEN1_CHECK(W <= WM_MAX_WINDOWS, "jen1_window_merge: W = %d windows, the kernel keeps at most %d offsets in LDS", W, WM_MAX_WINDOWS);
  if (n == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long long items = (long long)n * C * L;
  hipLaunchKernelGGL(window_merge_kernel, dim3(wm_blocks(items)), dim3(WM_THREADS), (size_t)W * sizeof(int), st, rows, offsets, canvas, items, W, C, T,
                     L, ramp);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_window_gather(const float* canvas, float* rows, const int32_t* offsets, int lead, int n, int W, int C, int T, int L, void* stream) {
  JEN1_CHECK(canvas != nullptr && rows != nullptr && offsets != nullptr, "jen1_window_gather: null pointer");
  if (int rc = window_shape_check("jen1_window_gather", lead, n, W, C, T, L)) return rc;
  if (n == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool vec = T % 4 == 0 && aligned16(rows);
  const long long items = (long long)lead * n * W * C * (vec ? T / 4 : T);
  if (vec) hipLaunchKernelGGL((window_gather_kernel<true>), dim3(wm_blocks(items)), dim3(WM_THREADS), 0, st, canvas, rows, offsets, items, n, W, C, T, L);
  else hipLaunchKernelGGL((window_gather_kernel<false>), dim3(wm_blocks(items)), dim3(WM_THREADS), 0, st, canvas, rows, offsets, items, n, W, C, T, L);
  JEN1_HIP(hipGetLastError());
  return 0;
}
