// The T5 / flan-T5 encoder stack behind Jen1's text conditioner (include/jen1_t5.h; reference jen1/conditioners.py:32-111 runs
// transformers.T5EncoderModel on stock operators): what lies between the stack's linears, which are jen1_train_gemm products.
//
//   jen1_t5_embed      row gather of the token table into the float32 residual stream
//   jen1_t5_rmsnorm    h += add (float32, in place), then T5LayerNorm of the row in the compute dtype: one workgroup per row
//   jen1_t5_attention  scores + relative-position bias + key mask + softmax + P V on the matrix cores, one launch per block
//   jen1_t5_gate       gelu_new(wi_0 x) * wi_1 x (flan-t5) or relu(wi x) (t5)
//
// jen1_t5_attention: a workgroup of four waves owns 64 query rows of one (sample, head); each wave owns 16 of them.  K goes into LDS as it
// lies in memory ([key][d], the B operand of Q K^T reads along d), V transposed ([d][key], the B operand of P V reads along the keys),
// both zero-filled up to a multiple of 32 keys.  A wave keeps its 16 x N scores in accumulator registers (one 16 x 16 tile per 16 keys),
// adds the bias from a [2 N - 1] LDS row, reduces max and sum over the 16 lanes that share a query row, and hands P to the second
// product through a 16 x N LDS tile of its own (the accumulator layout has the key on the lane, the A operand wants it along K).
// Operand fragments are 16 bytes per lane: 8 bf16 = one 16x16x32 step, or 4 floats = four 16x16x4 steps whose K order is the same
// permutation on both operands.
#include "mfma_frag.h"
#include "jen1_t5.h"

namespace {

constexpr int T5_NT = 256;
constexpr int TA_ROWS = 64;                    // query rows per workgroup (16 per wave)
constexpr int TA_BIAS_BYTES = 2 * JEN1_T5_MAX_TOKENS * 4;
constexpr int TA_MAX_LDS = 160 * 1024;

template <typename T> struct TaFrag;
template <> struct TaFrag<bf16_t> { typedef bf16x8 type; };
template <> struct TaFrag<float> { typedef f32x4 type; };

using ::mma;      // the bf16 step (mfma_frag.h); this kernel's float32 fragments hold 4 elements, not 8
__device__ __forceinline__ void mma(f32x4& acc, const f32x4& a, const f32x4& b) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
}

__device__ __forceinline__ float xor16_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  v = fmaxf(v, __shfl_xor(v, 4));
  return fmaxf(v, __shfl_xor(v, 8));
}
__device__ __forceinline__ float xor16_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v + __shfl_xor(v, 8);
}

__host__ __device__ inline int ta_keys_padded(int N) { return (N + 31) & ~31; }
template <typename T>
size_t ta_lds_bytes(int N, int d) {
  const int EV = 16 / (int)sizeof(T), Np = ta_keys_padded(N);
  return TA_BIAS_BYTES + ((size_t)Np * (d + EV) + (size_t)d * (Np + EV) + (size_t)TA_ROWS * (Np + EV)) * sizeof(T);
}

template <typename T>
__global__ __launch_bounds__(T5_NT) void t5_attn_kernel(const T* __restrict__ qkv, long long ld, T* __restrict__ o, long long ldo,
                                                        const float* __restrict__ bias_tab, const int* __restrict__ key_mask, int H, int N,
                                                        int d, int qtiles) {
  typedef typename TaFrag<T>::type Frag;
  constexpr int EV = 16 / (int)sizeof(T);      // elements of one lane's fragment
  constexpr int KC = 4 * EV;                   // K indices one fragment step covers over the four lane groups
  constexpr int QC = 64 / KC;                  // fragment steps along d at d = 64
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const int qt = blockIdx.x % qtiles, z = blockIdx.x / qtiles, b = z / H, h = z - b * H;
  const int Np = ta_keys_padded(N), NT = Np >> 4;
  const int KP = d + EV, VP = Np + EV, PP = Np + EV;
  float* bs = reinterpret_cast<float*>(lds_raw);                     // [2 N - 1]
  T* Ks = reinterpret_cast<T*>(lds_raw + TA_BIAS_BYTES);             // [Np][KP]
  T* Vt = Ks + Np * KP;                                              // [d][VP]
  T* Ps = Vt + d * VP + wave * 16 * PP;                              // [16][PP] of this wave
  const int inner = H * d;
  const T* qb = qkv + (long long)b * N * ld + h * d;
  const T* kb = qb + inner;
  const T* vb = kb + inner;
  Frag zero;
#pragma unroll
  for (int u = 0; u < EV; ++u) zero[u] = (T)0.f;

  for (int e = tid; e < 2 * N - 1; e += T5_NT) bs[e] = bias_tab[(long long)h * (2 * N - 1) + e];
  const int vpr = d / EV;
  for (int e = tid; e < Np * vpr; e += T5_NT) {
    const int j = e / vpr, c = (e - j * vpr) * EV;
    Frag kw = zero, vw = zero;
    if (j < N) {
      kw = *reinterpret_cast<const Frag*>(kb + (long long)j * ld + c);
      vw = *reinterpret_cast<const Frag*>(vb + (long long)j * ld + c);
    }
    *reinterpret_cast<Frag*>(Ks + j * KP + c) = kw;
#pragma unroll
    for (int u = 0; u < EV; ++u) Vt[(c + u) * VP + j] = vw[u];
  }
  // this lane's part of the A operand of Q K^T: query row row0 + c16, K indices q KC + g EV ..
  const int row0 = qt * TA_ROWS + wave * 16;
  Frag qf[QC];
#pragma unroll
  for (int q = 0; q < QC; ++q) {
    const int k = q * KC + g * EV;
    qf[q] = zero;
    if (row0 + c16 < N && k < d) qf[q] = *reinterpret_cast<const Frag*>(qb + (long long)(row0 + c16) * ld + k);
  }
  __syncthreads();

  // scores: tile t holds keys 16 t .. 16 t + 15; acc[t][r] is (query row0 + 4 g + r, key 16 t + c16)
  f32x4 acc[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t < NT) {
#pragma unroll
      for (int q = 0; q < QC; ++q) {
        if (q * KC < d) {
          const int k = q * KC + g * EV;
          Frag kf = zero;
          if (k < d) kf = *reinterpret_cast<const Frag*>(Ks + (t * 16 + c16) * KP + k);
          mma(acc[t], qf[q], kf);
        }
      }
    }
  }
  unsigned keep = 0u;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int j = t * 16 + c16;
    if (t < NT && j < N && key_mask[(long long)b * N + j] != 0) keep |= 1u << t;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = row0 + g * 4 + r;
    const bool row_ok = i < N;
    float m = -3.0e38f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if ((keep >> t) & 1u) {
        const float s = acc[t][r] + (row_ok ? bs[t * 16 + c16 - i + N - 1] : 0.f);
        acc[t][r] = s;
        m = fmaxf(m, s);
      }
    }
    m = xor16_max(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float p = ((keep >> t) & 1u) ? expf(acc[t][r] - m) : 0.f;
      acc[t][r] = p;
      sum += p;
    }
    sum = xor16_sum(sum);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t)
      if (t < NT) Ps[(g * 4 + r) * PP + t * 16 + c16] = (T)(acc[t][r] * inv);
  }
  __syncthreads();

  // O = P V: 16 channels per tile, K runs over the padded keys
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    if (ct * 16 < d) {
      f32x4 oa = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k = g * EV; k < Np; k += KC)
        mma(oa, *reinterpret_cast<const Frag*>(Ps + c16 * PP + k), *reinterpret_cast<const Frag*>(Vt + (ct * 16 + c16) * VP + k));
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = row0 + g * 4 + r;
        if (i < N) o[((long long)b * N + i) * ldo + h * d + ct * 16 + c16] = (T)oa[r];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(T5_NT) void t5_rmsnorm_kernel(float* __restrict__ h, const float* __restrict__ add, const float* __restrict__ weight,
                                                           T* __restrict__ y, int C, float eps) {
  __shared__ float part[T5_NT / 64];
  const long long base = (long long)blockIdx.x * C;
  float ss = 0.f;
  for (int c = threadIdx.x; c < C; c += T5_NT) {
    float v = h[base + c];
    if (add != nullptr) {
      v += add[base + c];
      h[base + c] = v;                    // (read back below by the thread that wrote it)
    }
    ss += v * v;
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < T5_NT / 64; ++w) tot += part[w];
  const float rs = 1.0f / sqrtf(tot / (float)C + eps);
  for (int c = threadIdx.x; c < C; c += T5_NT) y[base + c] = (T)(h[base + c] * rs * weight[c]);
}

__global__ __launch_bounds__(T5_NT) void t5_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ table,
                                                         float* __restrict__ out, int* __restrict__ err_flag, int vocab, int C) {
  const long long id = ids[blockIdx.x];
  const bool ok = id >= 0 && id < (long long)vocab;
  if (!ok && threadIdx.x == 0) atomicOr(err_flag, 1);
  const float* src = table + (ok ? id : 0) * (long long)C;
  float* dst = out + (long long)blockIdx.x * C;
  for (int c = threadIdx.x; c < C; c += T5_NT) dst[c] = ok ? src[c] : 0.f;
}

__device__ __forceinline__ float gelu_new_f(float a) {
  return 0.5f * a * (1.0f + tanhf(0.79788456080286535588f * (a + 0.044715f * a * a * a)));
}

template <typename T>
__global__ __launch_bounds__(T5_NT) void t5_gate_kernel(const T* __restrict__ x, T* __restrict__ y, long long total, int F, int act) {
  for (long long e = (long long)blockIdx.x * T5_NT + threadIdx.x; e < total; e += (long long)gridDim.x * T5_NT) {
    const long long r = e / F;
    const int f = (int)(e - r * F);
    if (act == JEN1_T5_ACT_GELU_NEW) {
      const float a = (float)x[r * 2 * F + f], bgate = (float)x[r * 2 * F + F + f];
      y[e] = (T)(gelu_new_f(a) * bgate);
    } else {
      y[e] = (T)fmaxf((float)x[e], 0.f);
    }
  }
}

int check_dtype(const char* who, int dtype) {
  JEN1_CHECK(dtype == JEN1_F32 || dtype == JEN1_BF16, "%s: dtype must be JEN1_F32 or JEN1_BF16", who);
  return 0;
}

}  // namespace

extern "C" int jen1_t5_embed(const int64_t* ids, const float* table, float* out, int32_t* err_flag, int rows, int vocab, int C, void* stream) {
  JEN1_CHECK(ids && table && out && err_flag, "jen1_t5_embed: NULL argument");
  JEN1_CHECK(rows >= 1 && vocab >= 1 && C >= 1, "jen1_t5_embed: rows, vocab, C must be >= 1");
  hipLaunchKernelGGL(t5_embed_kernel, dim3(rows), dim3(T5_NT), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(ids),
                     table, out, reinterpret_cast<int*>(err_flag), vocab, C);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_t5_rmsnorm(float* h, const float* add, const float* weight, void* y, int rows, int C, float eps, int dtype, void* stream) {
  if (check_dtype("jen1_t5_rmsnorm", dtype)) return 1;
  JEN1_CHECK(h && weight && y, "jen1_t5_rmsnorm: NULL argument");
  JEN1_CHECK(rows >= 1 && C >= 1, "jen1_t5_rmsnorm: rows and C must be >= 1");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == JEN1_F32) hipLaunchKernelGGL(t5_rmsnorm_kernel<float>, dim3(rows), dim3(T5_NT), 0, s, h, add, weight, reinterpret_cast<float*>(y), C, eps);
  else hipLaunchKernelGGL(t5_rmsnorm_kernel<bf16_t>, dim3(rows), dim3(T5_NT), 0, s, h, add, weight, reinterpret_cast<bf16_t*>(y), C, eps);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_t5_attention(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* bias_tab, const int32_t* key_mask, int B, int heads,
                                 int N, int d, int dtype, void* stream) {
  if (check_dtype("jen1_t5_attention", dtype)) return 1;
  JEN1_CHECK(qkv && o && bias_tab && key_mask, "jen1_t5_attention: NULL argument");
  JEN1_CHECK(B >= 1 && heads >= 1 && N >= 1, "jen1_t5_attention: B, heads, N must be >= 1");
  JEN1_CHECK(N <= JEN1_T5_MAX_TOKENS, "jen1_t5_attention: N = %d, at most %d tokens", N, JEN1_T5_MAX_TOKENS);
  JEN1_CHECK(d == 16 || d == 32 || d == 64, "jen1_t5_attention: d = %d, must be 16, 32 or 64", d);
  JEN1_CHECK(ld >= 3ll * heads * d && ldo >= (long long)heads * d, "jen1_t5_attention: ld / ldo are shorter than the heads they hold");
  JEN1_CHECK(ld % 8 == 0 && ldo % 8 == 0 && ((uintptr_t)qkv & 15) == 0 && ((uintptr_t)o & 15) == 0,
             "jen1_t5_attention: qkv / o must lie on 16-byte boundaries with ld, ldo multiples of 8");
  const int qtiles = (N + TA_ROWS - 1) / TA_ROWS;
  const long long wgs = (long long)B * heads * qtiles;
  JEN1_CHECK(wgs < (1ll << 31), "jen1_t5_attention: too many (sample, head) pairs");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == JEN1_F32) {
    const size_t lds = ta_lds_bytes<float>(N, d);
    JEN1_CHECK(lds <= (size_t)TA_MAX_LDS, "jen1_t5_attention: N = %d, d = %d need %zu bytes of LDS", N, d, lds);
    JEN1_MAX_LDS_ONCE(t5_attn_kernel<float>, TA_MAX_LDS);
    hipLaunchKernelGGL(t5_attn_kernel<float>, dim3((unsigned)wgs), dim3(T5_NT), lds, s, reinterpret_cast<const float*>(qkv), (long long)ld,
                       reinterpret_cast<float*>(o), (long long)ldo, bias_tab, reinterpret_cast<const int*>(key_mask), heads, N, d, qtiles);
  } else {
    const size_t lds = ta_lds_bytes<bf16_t>(N, d);
    JEN1_CHECK(lds <= (size_t)TA_MAX_LDS, "jen1_t5_attention: N = %d, d = %d need %zu bytes of LDS", N, d, lds);
    JEN1_MAX_LDS_ONCE(t5_attn_kernel<bf16_t>, TA_MAX_LDS);
    hipLaunchKernelGGL(t5_attn_kernel<bf16_t>, dim3((unsigned)wgs), dim3(T5_NT), lds, s, reinterpret_cast<const bf16_t*>(qkv), (long long)ld,
                       reinterpret_cast<bf16_t*>(o), (long long)ldo, bias_tab, reinterpret_cast<const int*>(key_mask), heads, N, d, qtiles);
  }
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_t5_gate(const void* x, void* y, int rows, int F, int act, int dtype, void* stream) {
  if (check_dtype("jen1_t5_gate", dtype)) return 1;
  JEN1_CHECK(x && y, "jen1_t5_gate: NULL argument");
  JEN1_CHECK(rows >= 1 && F >= 1, "jen1_t5_gate: rows and F must be >= 1");
  JEN1_CHECK(act == JEN1_T5_ACT_GELU_NEW || act == JEN1_T5_ACT_RELU, "jen1_t5_gate: act must be JEN1_T5_ACT_GELU_NEW or JEN1_T5_ACT_RELU");
  const long long total = (long long)rows * F;
  long long blocks = (total + T5_NT - 1) / T5_NT;
  if (blocks > 8192) blocks = 8192;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == JEN1_F32)
    hipLaunchKernelGGL(t5_gate_kernel<float>, dim3((unsigned)blocks), dim3(T5_NT), 0, s, reinterpret_cast<const float*>(x), reinterpret_cast<float*>(y), total, F, act);
  else
    hipLaunchKernelGGL(t5_gate_kernel<bf16_t>, dim3((unsigned)blocks), dim3(T5_NT), 0, s, reinterpret_cast<const bf16_t*>(x), reinterpret_cast<bf16_t*>(y), total, F, act);
  JEN1_HIP(hipGetLastError());
  return 0;
}
