// Encodec pieces either side of the sampler (include/jen1_train.h): the residual-vector-quantizer decode that turns
// codes into the latents the denoiser works on (generation.py:145-150) and the LSTM of the SEANet decoder that turns
// sampled latents back into audio (generation.py:130).  The convolutions / transposed convolutions / GroupNorm / ELU
// of the decoder run on jen1_train_gemm and the train_ops kernels (jen1_amd/encodec.py).
#include "common.h"
#include "jen1_train.h"

namespace {

// out[b][d][t] = sum_q tables[q][codes[q][b][t]][d] : one block per (b, 64 frames); rows of the codebooks are
// read 128 floats at a time (coalesced), the transposed store goes through LDS.
__global__ __launch_bounds__(256) void rvq_decode_kernel(const long long* __restrict__ codes, const float* __restrict__ tables,
                                                         float* __restrict__ out, int n_q, int B, int T, int bins, int D) {
  __shared__ float tile[64][129];
  const int b = blockIdx.y, t0 = blockIdx.x * 64;
  for (int d0 = 0; d0 < D; d0 += 128) {
    for (int e = threadIdx.x; e < 64 * 128; e += 256) {
      const int tl = e / 128, d = d0 + e % 128, t = t0 + tl;
      float acc = 0.f;
      if (t < T && d < D) {
        for (int q = 0; q < n_q; ++q) {
          long long idx = codes[((long long)q * B + b) * T + t];
          idx = idx < 0 ? 0 : (idx >= bins ? bins - 1 : idx);
          acc += tables[((long long)q * bins + idx) * D + d];
        }
      }
      tile[tl][e % 128] = acc;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 128; e += 256) {
      const int dl = e / 64, tl = e % 64, d = d0 + dl, t = t0 + tl;
      if (t < T && d < D) out[((long long)b * D + d) * T + t] = tile[tl][dl];
    }
    __syncthreads();
  }
}

// ---- jen1_rvq_encode: the whole residual search of ResidualVectorQuantization.encode, and its decode, in one launch ----
// A workgroup of 4 waves owns RVQE_FT = 32 frames for all n_q codebooks (the residual makes the codebooks sequential).  Every wave keeps
// the residual of those 32 frames in registers as the B operand of v_mfma_f32_32x32x2_f32 (frame on the lane, 64 of the 128 k per lane
// half), the codebook streams through two LDS buffers in chunks of 128 entries (the next chunk and its |e|^2 travel from L2 through
// registers into the other buffer while this one is searched) and wave w searches entries 32 w .. 32 w + 31 of the chunk: its 16 LDS
// fragments first, then 64 MFMAs on one accumulator (issue interval = dependent latency for this shape).  The score 2 r.e - |e|^2 of an
// entry is lane-local (entries are the rows of the result), so the running (best score, best index) per frame lives in two registers;
// the lane halves and the 4 waves are combined once per codebook, and the 32 chosen rows are fetched once per workgroup into LDS for
// the subtract.  The dot product is an f32 fmaf chain in a fixed order of k that depends on nothing but k, so a frame's codes do not
// depend on the launch shape or on its place in the tile.
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int RVQE_FT = 32, RVQE_CH = 128, RVQE_LD = 132, RVQE_WAVES = 4, RVQE_THREADS = 64 * RVQE_WAVES, RVQE_MAXQ = 32, RVQE_D = 128;
// LDS, in floats: two codebook buffers | the waves' (score, index) candidates | the tile's codes | |e|^2 of the two buffers' entries | the chosen rows
constexpr int RVQE_OFF_RED = 2 * RVQE_CH * RVQE_LD, RVQE_OFF_CODE = RVQE_OFF_RED + 2 * RVQE_WAVES * RVQE_FT,
              RVQE_OFF_ESQ = RVQE_OFF_CODE + RVQE_MAXQ * RVQE_FT, RVQE_OFF_ROW = RVQE_OFF_ESQ + 2 * RVQE_CH,
              RVQE_LDS_BYTES = (RVQE_OFF_ROW + RVQE_FT * RVQE_LD) * 4;
static_assert(RVQE_LDS_BYTES <= 160 * 1024 && RVQE_OFF_ESQ % 4 == 0 && RVQE_OFF_ROW % 4 == 0 && RVQE_THREADS >= RVQE_CH && RVQE_THREADS == 8 * RVQE_FT,
              "rvq_encode_kernel: LDS carve");

// on exact ties the LOWEST index wins (torch.argmax on the GEMM's scores returns the first maximum)
__device__ __forceinline__ bool rvqe_better(float s, int i, float bs, int bi) { return s > bs || (s == bs && i < bi); }

__device__ __forceinline__ void rvqe_fetch(const float* __restrict__ tables, const float* __restrict__ e_sq, int q, int c0, int bins, float4 (&pf)[16],
                                           float& sq) {
  const int r = c0 + (int)threadIdx.x;
  sq = (int)threadIdx.x < RVQE_CH && r < bins ? e_sq[(long long)q * bins + r] : 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = (int)threadIdx.x + RVQE_THREADS * u, row = c0 + (e >> 5), c4 = e & 31;
    pf[u] = row < bins ? *reinterpret_cast<const float4*>(tables + ((long long)q * bins + row) * RVQE_D + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ void rvqe_stage(float* __restrict__ buf, float* __restrict__ esq, const float4 (&pf)[16], float sq) {
  if ((int)threadIdx.x < RVQE_CH) esq[threadIdx.x] = sq;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = (int)threadIdx.x + RVQE_THREADS * u;
    *reinterpret_cast<float4*>(buf + (e >> 5) * RVQE_LD + (e & 31) * 4) = pf[u];
  }
}

__global__ __launch_bounds__(RVQE_THREADS) void rvq_encode_kernel(const float* __restrict__ emb, const float* __restrict__ tables,
                                                                  const float* __restrict__ e_sq, long long* __restrict__ codes,
                                                                  float* __restrict__ latents, int n_q, long long F, int T, int bins, int B_out,
                                                                  long long codes_T, long long codes_t0, long long lat_T, long long lat_t0) {
  extern __shared__ __attribute__((aligned(16))) float rvqe_lds[];
  float* red_s = rvqe_lds + RVQE_OFF_RED;                              // [RVQE_WAVES][RVQE_FT]
  int* red_i = reinterpret_cast<int*>(red_s + RVQE_WAVES * RVQE_FT);   // [RVQE_WAVES][RVQE_FT]
  int* code_s = reinterpret_cast<int*>(rvqe_lds + RVQE_OFF_CODE);      // [RVQE_MAXQ][RVQE_FT]
  float* esq_s = rvqe_lds + RVQE_OFF_ESQ;                              // [2][RVQE_CH]
  float* row_s = rvqe_lds + RVQE_OFF_ROW;                              // [RVQE_FT][RVQE_LD]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
  const long long f0 = (long long)blockIdx.x * RVQE_FT, f = f0 + j;
  const bool valid = f < F;
  const long long row = valid ? f / T : 0;
  const int t = valid ? (int)(f - row * T) : 0;

  // residual: register 4 s + m holds k = 8 s + 4 h + m (the k the lane's float4 of an entry holds at step s)
  float res[64];
#pragma unroll
  for (int s = 0; s < 16; ++s)
#pragma unroll
    for (int m = 0; m < 4; ++m) res[4 * s + m] = valid ? emb[(row * RVQE_D + 8 * s + 4 * h + m) * T + t] : 0.f;

  const int nch = (bins + RVQE_CH - 1) / RVQE_CH;
  float4 pf[16];
  float pf_sq;
  rvqe_fetch(tables, e_sq, 0, 0, bins, pf, pf_sq);
  rvqe_stage(rvqe_lds, esq_s, pf, pf_sq);
  int cur = 0;
  __syncthreads();
  for (int q = 0; q < n_q; ++q) {
    float best = -INFINITY;
    int bidx = 0;
    for (int c = 0; c < nch; ++c) {
      const int c0 = c * RVQE_CH;
      const float* chunk = rvqe_lds + cur * (RVQE_CH * RVQE_LD);
      const bool more = c + 1 < nch || q + 1 < n_q;                   // block-uniform
      if (c + 1 < nch) rvqe_fetch(tables, e_sq, q, c0 + RVQE_CH, bins, pf, pf_sq);
      else if (q + 1 < n_q) rvqe_fetch(tables, e_sq, q + 1, 0, bins, pf, pf_sq);
      const int ebase = c0 + 32 * w;                                  // wave-uniform
      if (ebase < bins) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const float* arow = chunk + (32 * w + j) * RVQE_LD + 4 * h;
        // all 16 fragments of the wave's entries first: a read issued between the dependent MFMAs would only overlap with the last of them
        float4 a[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) a[s] = *reinterpret_cast<const float4*>(arow + 8 * s);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].x, res[4 * s + 0], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].y, res[4 * s + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].z, res[4 * s + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].w, res[4 * s + 3], acc, 0, 0, 0);
        }
        // register 4 g + x is entry ebase + 8 g + 4 h + x: ascending with the register, so '>' keeps the lowest index of a tie
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 sq = *reinterpret_cast<const float4*>(esq_s + cur * RVQE_CH + 32 * w + 8 * g + 4 * h);
          const float sc[4] = {2.f * acc[4 * g + 0] - sq.x, 2.f * acc[4 * g + 1] - sq.y, 2.f * acc[4 * g + 2] - sq.z, 2.f * acc[4 * g + 3] - sq.w};
#pragma unroll
          for (int x = 0; x < 4; ++x)
            if (sc[x] > best) { best = sc[x]; bidx = ebase + 8 * g + 4 * h + x; }
        }
      }
      // the other buffer was last read before the previous barrier
      if (more) rvqe_stage(rvqe_lds + (cur ^ 1) * (RVQE_CH * RVQE_LD), esq_s + (cur ^ 1) * RVQE_CH, pf, pf_sq);
      cur ^= 1;
      __syncthreads();
    }
    {
      const float os = __shfl_xor(best, 32);
      const int oi = __shfl_xor(bidx, 32);
      if (rvqe_better(os, oi, best, bidx)) { best = os; bidx = oi; }
    }
    if (h == 0) { red_s[w * RVQE_FT + j] = best; red_i[w * RVQE_FT + j] = bidx; }
    __syncthreads();          // the next write of red_* is behind the barrier of the next codebook's first chunk
    best = red_s[j];
    bidx = red_i[j];
#pragma unroll
    for (int v = 1; v < RVQE_WAVES; ++v) {
      const float os = red_s[v * RVQE_FT + j];
      const int oi = red_i[v * RVQE_FT + j];
      if (rvqe_better(os, oi, best, bidx)) { best = os; bidx = oi; }
    }
    if (w == 0 && h == 0) {
      code_s[q * RVQE_FT + j] = bidx;
      if (codes && valid) {
        const long long r_b = row % B_out, r_j = row / B_out;
        codes[((long long)q * B_out + r_b) * codes_T + codes_t0 + r_j * T + t] = bidx;
      }
    }
    // the 32 chosen rows through LDS (8 threads per row, 64 bytes each), then r = r - e_idx: a plain float32 subtract
    {
      const int fr = tid >> 3, part = (tid & 7) * 16;
      const int idx_fr = __shfl(bidx, fr);                       // lane j of every wave holds frame j's index
      const float* src = tables + ((long long)q * bins + idx_fr) * RVQE_D + part;
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(src + 4 * u);
#pragma unroll
      for (int u = 0; u < 4; ++u) *reinterpret_cast<float4*>(row_s + fr * RVQE_LD + part + 4 * u) = v[u];
    }
    __syncthreads();          // the next write of row_s is behind the barriers of the next codebook's chunks
    const float* erow = row_s + j * RVQE_LD + 4 * h;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const float4 ev = *reinterpret_cast<const float4*>(erow + 8 * s);
      res[4 * s + 0] -= ev.x;
      res[4 * s + 1] -= ev.y;
      res[4 * s + 2] -= ev.z;
      res[4 * s + 3] -= ev.w;
    }
  }
  if (!latents) return;
  __syncthreads();
  // the sum rvq_decode_kernel forms, in its order: 0 + e_idx0 + e_idx1 + ...
  for (int e = tid; e < RVQE_FT * RVQE_D; e += RVQE_THREADS) {
    const int tl = e & 31, d = e >> 5;
    const long long fe = f0 + tl;
    if (fe >= F) continue;
    float acc = 0.f;
    for (int q = 0; q < n_q; ++q) acc += tables[((long long)q * bins + code_s[q * RVQE_FT + tl]) * RVQE_D + d];
    const long long r = fe / T, r_b = r % B_out, r_j = r / B_out;
    latents[(r_b * RVQE_D + d) * lat_T + lat_t0 + r_j * T + (fe - r * T)] = acc;
  }
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// One workgroup per sequence; 1024 threads own the 4H gate rows (RPT = 4H / 1024 each).  Per step every thread adds
// W_hh^T[k][row] * h[k] over k: the [H][4H] layout makes the weight reads coalesced, and the k loop is unrolled by 8
// with all loads issued before the FMAs, so the step is bound by streaming the matrix from L2 (it is re-read every
// step: 2 MB in bf16), not by one load latency per k.  Then H threads update (c, h).  Sequential in T by nature; the
// sequences of a batch run in parallel on different CUs.
template <typename T, int RPT>
__global__ __launch_bounds__(1024) void lstm_layer_kernel(const float* __restrict__ gin, const void* whh_t_, const void* skip_, void* y_,
                                                          int Tn, int H, int ld_y) {
  extern __shared__ float smem[];
  float* h = smem;              // [H]
  float* gates = smem + H;      // [4H]
  const T* whh_t = reinterpret_cast<const T*>(whh_t_);
  const T* skip = reinterpret_cast<const T*>(skip_);
  T* y = reinterpret_cast<T*>(y_);
  const int b = blockIdx.x, tid = threadIdx.x, G = 4 * H;      // G == RPT * 1024 (checked by the launcher)
  float c = 0.f;                 // cell state of hidden unit `tid` (threads < H)
  for (int j = tid; j < H; j += 1024) h[j] = 0.f;
  __syncthreads();
  constexpr int KU = 8;
  for (int t = 0; t < Tn; ++t) {
    const float* g_in = gin + ((long long)b * Tn + t) * G;
    float acc[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) acc[r] = g_in[tid + r * 1024];
    for (int k0 = 0; k0 < H; k0 += KU) {          // H % 8 == 0 (checked by the launcher)
      T w[KU][RPT];
#pragma unroll
      for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int r = 0; r < RPT; ++r) w[u][r] = whh_t[(long long)(k0 + u) * G + tid + r * 1024];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const float hk = h[k0 + u];
#pragma unroll
        for (int r = 0; r < RPT; ++r) acc[r] += (float)w[u][r] * hk;
      }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) gates[tid + r * 1024] = acc[r];
    __syncthreads();
    for (int j = tid; j < H; j += 1024) {     // H <= 1024: each unit belongs to one thread for the whole sequence
      const float ig = sigmoid_f(gates[j]), fg = sigmoid_f(gates[H + j]), gg = tanhf(gates[2 * H + j]), og = sigmoid_f(gates[3 * H + j]);
      c = fg * c + ig * gg;
      const float hn = og * tanhf(c);
      h[j] = hn;
      const long long o = ((long long)b * Tn + t) * ld_y + j;
      y[o] = (T)(hn + (skip != nullptr ? (float)skip[o] : 0.f));
    }
    __syncthreads();
  }
}

// ---- LSTM layer spread over NW workgroups (the fast path) -----------------------------------------------------------
// Workgroup w owns UPW = 32 hidden units = 128 gate rows; its slice of W_hh (128 x H) lives in registers for the whole
// sequence: thread (row r, k slice s) holds W_hh[row r][s * KS .. s * KS + KS).  Up to LB = 8 sequences advance together.
// Per step: h_t of all sequences is in LDS; every thread forms its partial dot products for the LB sequences (LDS
// broadcast reads), the k slices are summed through LDS, 32 x LB threads apply the gates, publish h_{t+1} of their
// units with write-through stores, and one grid barrier (relaxed agent-scope atomics, tools/microbench/gridbar.hip:
// ~1 us at 16 workgroups) separates the steps.  The spin is bounded (2^26 polls, seconds): a workgroup that never
// becomes resident turns into an error flag that the host side checks (jen1_amd/encodec.py), never into a hang.
constexpr int LSTM_UPW = 32, LSTM_LB = 8, LSTM_NS = 8;

template <typename T, int KS>    // KS = H / LSTM_NS k values per thread
__global__ __launch_bounds__(1024) void lstm_multi_kernel(const float* __restrict__ gin, const void* whh_, const void* skip_, void* y_,
                                                          float* hbuf, unsigned* ctr, int B, int Tn, int H, int ld_y) {
  __shared__ float h_s[LSTM_LB][1024];                 // h_t of the sequences of this group (H <= 1024)
  __shared__ float red[LSTM_NS][128][LSTM_LB + 1];
  __shared__ float gates[LSTM_LB][128];
  const T* whh = reinterpret_cast<const T*>(whh_);
  const T* skip = reinterpret_cast<const T*>(skip_);
  T* y = reinterpret_cast<T*>(y_);
  const int tid = threadIdx.x, NW = gridDim.x, w = blockIdx.x, grp = blockIdx.y;
  const int b0 = grp * LSTM_LB, nb = min(LSTM_LB, B - b0);
  const int rl = tid & 127, sl = tid >> 7;            // gate row within the workgroup, k slice
  const int gate = rl >> 5, u = rl & 31;
  const int grow = gate * H + w * LSTM_UPW + u;        // row of W_hh / entry of the 4H gate vector
  float wreg[KS];
#pragma unroll
  for (int j = 0; j < KS; ++j) wreg[j] = (float)whh[(long long)grow * H + sl * KS + j];
  float* hb = hbuf + (long long)grp * 2 * LSTM_LB * H;   // [2][LB][H] ping-pong of the published hidden state
  unsigned* my_ctr = ctr + grp * 32;
  unsigned epoch = 0;
  float c = 0.f;                                         // cell state of (unit u2, sequence b2) for threads < 32 * LB
  const int u2 = tid & 31, b2 = tid >> 5;
  for (int i = tid; i < LSTM_LB * 1024; i += 1024) (&h_s[0][0])[i] = 0.f;
  __syncthreads();
  for (int t = 0; t < Tn; ++t) {
    // partial dot products of this thread's k slice for every sequence
    // the input projection of this step is fetched first: its latency hides behind the dot products
    const float g_in = (sl < nb) ? gin[((long long)(b0 + sl) * Tn + t) * (4 * H) + grow] : 0.f;
    float part[LSTM_LB];
#pragma unroll
    for (int b = 0; b < LSTM_LB; ++b) part[b] = 0.f;
#pragma unroll
    for (int b = 0; b < LSTM_LB; ++b) {
      if (b < nb) {                                  // uniform: absent sequences cost nothing
#pragma unroll
        for (int j = 0; j < KS; j += 4) {
          const float4 hv = *reinterpret_cast<const float4*>(&h_s[b][sl * KS + j]);
          part[b] += wreg[j] * hv.x + wreg[j + 1] * hv.y + wreg[j + 2] * hv.z + wreg[j + 3] * hv.w;
        }
      }
    }
#pragma unroll
    for (int b = 0; b < LSTM_LB; ++b) red[sl][rl][b] = part[b];
    __syncthreads();
    {   // thread (rl, b = sl) sums the k slices and adds the input projection
      const int b = sl;
      float g = 0.f;
#pragma unroll
      for (int s2 = 0; s2 < LSTM_NS; ++s2) g += red[s2][rl][b];
      gates[b][rl] = g + g_in;
    }
    __syncthreads();
    float* hnext = hb + (long long)((t + 1) & 1) * LSTM_LB * H;
    if (tid < 32 * LSTM_LB && b2 < nb) {
      const float ig = sigmoid_f(gates[b2][u2]), fg = sigmoid_f(gates[b2][32 + u2]), gg = tanhf(gates[b2][64 + u2]), og = sigmoid_f(gates[b2][96 + u2]);
      c = fg * c + ig * gg;
      const float hn = og * tanhf(c);
      const int j = w * LSTM_UPW + u2;
      __hip_atomic_store(hnext + b2 * H + j, hn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const long long o = ((long long)(b0 + b2) * Tn + t) * ld_y + j;
      y[o] = (T)(hn + (skip != nullptr ? (float)skip[o] : 0.f));
    }
    // grid barrier over the NW workgroups of this group
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      ++epoch;
      __hip_atomic_fetch_add(my_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned target = epoch * NW;
      int spins = 0;
      while (__hip_atomic_load(my_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 26)) { __hip_atomic_store(my_ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
      }
    }
    __syncthreads();
    if (t + 1 < Tn) {
      for (int i = tid; i < nb * H; i += 1024) {
        const int b = i / H, j = i - b * H;
        h_s[b][j] = __hip_atomic_load(hnext + b * H + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
    }
  }
}

// ---- the same layer with the recurrent product on the matrix cores (bf16 weights) -----------------------------------
// Workgroup w owns the same 128 gate rows; wave v holds the MFMA A fragments of row tile v % 8 for the K half v / 8
// (8 fragments = 32 VGPRs, resident for the whole sequence).  Up to 16 sequences are the 16 MFMA columns.  h_t stays
// float32 in the exchange buffer and is split into a bf16 high and low part when it is staged into LDS (two MFMAs per
// fragment), so the recurrence sees h at ~16 mantissa bits while the weights are the bf16 ones of the bf16 mode.
constexpr int LSTM_MB = 16;
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(1024) void lstm_multi_mfma_kernel(const float* __restrict__ gin, const bf16_t* __restrict__ whh,
                                                               const bf16_t* __restrict__ skip, bf16_t* __restrict__ y, float* hbuf,
                                                               unsigned* ctr, int B, int Tn, int H, int ld_y) {
  // H == 512 (checked by the launcher): K halves of 256 = 8 MFMA steps of 32
  __shared__ __attribute__((aligned(16))) bf16_t h_hi[LSTM_MB][512 + 8];
  __shared__ __attribute__((aligned(16))) bf16_t h_lo[LSTM_MB][512 + 8];
  __shared__ float part[8][64][4];
  __shared__ float gates[LSTM_MB][128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = gridDim.x, w = blockIdx.x, grp = blockIdx.y;
  const int b0 = grp * LSTM_MB, nb = min(LSTM_MB, B - b0);
  const int rt = wave & 7, kh = wave >> 3;
  // gate rows of tile rt: rl = rt * 16 + i  ->  gate rl / 32, unit rl % 32
  const int rl_a = rt * 16 + (lane & 15);
  const int grow_a = (rl_a >> 5) * H + w * LSTM_UPW + (rl_a & 31);
  bf16x8 wf[8];
#pragma unroll
  for (int s2 = 0; s2 < 8; ++s2)
    wf[s2] = *reinterpret_cast<const bf16x8*>(whh + (long long)grow_a * H + kh * 256 + s2 * 32 + (lane >> 4) * 8);
  float* hb = hbuf + (long long)grp * 2 * LSTM_MB * H;
  unsigned* my_ctr = ctr + grp * 32;
  unsigned epoch = 0;
  float c = 0.f;
  const int u2 = tid & 31, b2 = tid >> 5;           // unit / sequence of the update threads (tid < 32 * 16 = 512)
  for (int i = tid; i < LSTM_MB * (512 + 8); i += 1024) { (&h_hi[0][0])[i] = (bf16_t)0.f; (&h_lo[0][0])[i] = (bf16_t)0.f; }
  __syncthreads();
  for (int t = 0; t < Tn; ++t) {
    // input projection of the 4 gate rows x 1 sequence this lane will own after the reduction (waves 0..7)
    const int col = lane & 15;
    const int rl0 = rt * 16 + (lane >> 4) * 4;
    const int grow0 = (rl0 >> 5) * H + w * LSTM_UPW + (rl0 & 31);
    float4 g_in = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kh == 0 && col < nb) g_in = *reinterpret_cast<const float4*>(gin + ((long long)(b0 + col) * Tn + t) * (4 * H) + grow0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) {
      const int k = kh * 256 + s2 * 32 + (lane >> 4) * 8;
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&h_hi[col][k]);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&h_lo[col][k]);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s2], bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s2], bl, acc, 0, 0, 0);
    }
    if (kh == 1) *reinterpret_cast<float4*>(&part[rt][lane][0]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    if (kh == 0) {
      const float4 o = *reinterpret_cast<const float4*>(&part[rt][lane][0]);
      if (col < nb) {
        gates[col][rl0 + 0] = acc[0] + o.x + g_in.x;
        gates[col][rl0 + 1] = acc[1] + o.y + g_in.y;
        gates[col][rl0 + 2] = acc[2] + o.z + g_in.z;
        gates[col][rl0 + 3] = acc[3] + o.w + g_in.w;
      }
    }
    __syncthreads();
    float* hnext = hb + (long long)((t + 1) & 1) * LSTM_MB * H;
    if (tid < 32 * LSTM_MB && b2 < nb) {
      const float ig = sigmoid_f(gates[b2][u2]), fg = sigmoid_f(gates[b2][32 + u2]), gg = tanhf(gates[b2][64 + u2]), og = sigmoid_f(gates[b2][96 + u2]);
      c = fg * c + ig * gg;
      const float hn = og * tanhf(c);
      const int j = w * LSTM_UPW + u2;
      __hip_atomic_store(hnext + b2 * H + j, hn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const long long o = ((long long)(b0 + b2) * Tn + t) * ld_y + j;
      y[o] = (bf16_t)(hn + (skip != nullptr ? (float)skip[o] : 0.f));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      ++epoch;
      __hip_atomic_fetch_add(my_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned target = epoch * NW;
      int spins = 0;
      while (__hip_atomic_load(my_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 26)) { __hip_atomic_store(my_ctr + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
      }
    }
    __syncthreads();
    if (t + 1 < Tn) {
      // restage h_{t+1}: 16-byte sc1 loads (nb * 512 floats = nb * 128 vectors), split into bf16 high + low
      const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(hnext, 0, LSTM_MB * 512 * 4, 0x00020000);
      for (int i = tid; i < nb * 128; i += 1024) {
        const int b = i >> 7, j = (i & 127) * 4;
        const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rh, (unsigned)(b * 512 + j) * 4u, 0, 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float hv = __uint_as_float(q[e]);
          const bf16_t hi = (bf16_t)hv;
          h_hi[b][j + e] = hi;
          h_lo[b][j + e] = (bf16_t)(hv - (float)hi);
        }
      }
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// EncodecModel.encode / .decode around the SEANet halves: segment scales, segment cut, pad1d and the linear overlap-add
// ---------------------------------------------------------------------------------------------------------------------

// scale[b][s] = 1e-8 + sqrt(mean_n (mean_c x)^2) over segment s: one workgroup per (s, b); every thread sums its strided share in
// double, then a tree over LDS in a fixed order (the result does not depend on scheduling)
__global__ __launch_bounds__(256) void codec_segment_scales_kernel(const float* __restrict__ audio, float* __restrict__ scale, int C,
                                                                   long long N, int Lseg, int stride, int S) {
  __shared__ double part[256];
  const int s = blockIdx.x, b = blockIdx.y;
  const long long n0 = (long long)s * stride;
  const long long rest = N - n0;
  const int len = rest < Lseg ? (int)rest : Lseg;
  const float* x = audio + (long long)b * C * N + n0;
  double acc = 0.0;
  for (int i = threadIdx.x; i < len; i += 256) {
    float m = 0.f;
    for (int c = 0; c < C; ++c) m += x[(long long)c * N + i];
    const double md = (double)m / (double)C;
    acc += md * md;
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) scale[(long long)b * S + s] = (float)(1e-8 + sqrt(part[0] / (double)len));
}

// rows[(j B + b)][i][0..7] = audio[b][c][(s0 + j) stride + i] / scale[b][s0 + j] (a true float32 division; scale == NULL: the plain
// cut), columns C..7 zero: the channel-last rows the encoder's first convolution reads
template <typename T>
__global__ __launch_bounds__(256) void codec_segment_cut_kernel(const float* __restrict__ audio, const float* __restrict__ scale,
                                                                T* __restrict__ rows, int B, int C, long long N, int Lsel, int stride, int S,
                                                                int s0) {
  const int i = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
  if (i >= Lsel) return;
  const int j = row / B, b = row - j * B, s = s0 + j;
  const float* x = audio + (long long)b * C * N + (long long)s * stride + i;
  const float sc = scale ? scale[(long long)b * S + s] : 1.0f;
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    v[c] = 0.f;
    if (c < C) {
      const float a = x[(long long)c * N];
      v[c] = scale ? a / sc : a;
    }
  }
  store8(rows + ((long long)row * Lsel + i) * 8, v);
}

// pad1d(mode="reflect") of encodec modules/conv.py on channel-last rows, 16 bytes per thread: y[r][j] = z[reflect(j - left)] with
// z = x zero-extended on the right to Lz = L + extra (extra = max(left, right) - L + 1 when L <= max(left, right), else 0); the
// `extra` entries the package drops from the end are never produced
__global__ __launch_bounds__(256) void codec_pad1d_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, long long total, int L, int units,
                                                          int left, int right) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int Lp = L + left + right;
  const int u = (int)(e % units);
  const long long rj = e / units;
  const int j = (int)(rj % Lp);
  const long long r = rj / Lp;
  const int max_pad = left > right ? left : right;
  const int Lz = L <= max_pad ? max_pad + 1 : L;
  int q = j - left;
  if (q < 0) q = -q;
  if (q >= Lz) q = 2 * (Lz - 1) - q;
  y[e] = q < L ? x[(r * L + q) * units + u] : make_uint4(0u, 0u, 0u, 0u);
}

// EncodecModel._linear_overlap_add in gather form: one thread per (b, n) walks the segments that cover n in ascending order (no
// atomics: bit-identical from run to run), reads the decoder's final rows (8 wide) and writes channel-first float32.  No contraction
// of the multiply-adds: the sums are the ones a float32 restatement of the formula makes.
template <typename T>
__global__ __launch_bounds__(256) void codec_overlap_add_kernel(const jen1_ola_seg* __restrict__ segs, int S, const float* __restrict__ scale,
                                                                float* __restrict__ out, int C, int N_out, int stride, int L0) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (n >= N_out) return;
  int s_hi = n / stride;
  if (s_hi > S - 1) s_hi = S - 1;
  const int s_lo = n < L0 ? 0 : (n - L0) / stride + 1;          // the first s with n - s stride < L0
  float num[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) num[c] = 0.f;
  float den = 0.f;
  const float span = (float)(L0 + 1);
  for (int s = s_lo; s <= s_hi; ++s) {
    const jen1_ola_seg e = segs[s];
    const int i = n - s * stride;
    if (i >= e.len) continue;
    const float t = (float)(i + 1) / span;
    const float w = 0.5f - fabsf(t - 0.5f);
    float v[8];
    load8(reinterpret_cast<const T*>(e.rows) + ((long long)(e.row0 + b) * e.len + i) * 8, v);
    if (scale) {
      const float sc = scale[(long long)b * S + s];
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = v[c] * sc;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) num[c] = num[c] + w * v[c];
    den = den + w;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < C) out[((long long)b * C + c) * N_out + n] = den > 0.f ? num[c] / den : 0.f;
}

}  // namespace

extern "C" int jen1_rvq_decode(const int64_t* codes, const float* tables, float* out, int n_q, int B, int T, int bins, int D, void* stream) {
  JEN1_CHECK(codes && tables && out, "jen1_rvq_decode: NULL argument");
  JEN1_CHECK(n_q >= 1 && B >= 1 && T >= 1 && bins >= 1 && D >= 1 && B <= 65535, "jen1_rvq_decode: bad shape");
  hipLaunchKernelGGL(rvq_decode_kernel, dim3((T + 63) / 64, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(codes), tables, out, n_q, B, T, bins, D);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_rvq_encode(const float* emb, const float* tables, const float* e_sq, int64_t* codes, float* latents, int n_q, int rows, int T,
                               int bins, int D, int B_out, int64_t codes_T, int64_t codes_t0, int64_t lat_T, int64_t lat_t0, void* stream) {
  JEN1_CHECK(emb && tables && e_sq, "jen1_rvq_encode: NULL argument");
  JEN1_CHECK(codes || latents, "jen1_rvq_encode: codes and latents are both NULL");
  JEN1_CHECK(D == RVQE_D, "jen1_rvq_encode: D must be %d, not %d", RVQE_D, D);
  JEN1_CHECK(bins % 64 == 0 && bins >= 64 && bins <= 2048, "jen1_rvq_encode: bins=%d must be a multiple of 64 in [64, 2048]", bins);
  JEN1_CHECK(n_q >= 1 && n_q <= RVQE_MAXQ && rows >= 1 && T >= 1 && B_out >= 1, "jen1_rvq_encode: bad shape n_q=%d rows=%d T=%d B_out=%d", n_q, rows, T,
             B_out);
  JEN1_CHECK(rows % B_out == 0, "jen1_rvq_encode: rows=%d is no multiple of B_out=%d", rows, B_out);
  const int64_t span = (int64_t)(rows / B_out) * T;
  JEN1_CHECK(!codes || (codes_t0 >= 0 && codes_t0 + span <= codes_T), "jen1_rvq_encode: codes slot %lld + %lld exceeds codes_T=%lld", (long long)codes_t0,
             (long long)span, (long long)codes_T);
  JEN1_CHECK(!latents || (lat_t0 >= 0 && lat_t0 + span <= lat_T), "jen1_rvq_encode: latents slot %lld + %lld exceeds lat_T=%lld", (long long)lat_t0,
             (long long)span, (long long)lat_T);
  const int64_t F = (int64_t)rows * T, tiles = (F + RVQE_FT - 1) / RVQE_FT;
  JEN1_CHECK(tiles <= 0x7fffffffLL, "jen1_rvq_encode: too many frames");
  JEN1_MAX_LDS_ONCE(rvq_encode_kernel, RVQE_LDS_BYTES);
  hipLaunchKernelGGL(rvq_encode_kernel, dim3((unsigned)tiles), dim3(RVQE_THREADS), RVQE_LDS_BYTES, reinterpret_cast<hipStream_t>(stream), emb, tables,
                     e_sq, reinterpret_cast<long long*>(codes), latents, n_q, (long long)F, T, bins, B_out, (long long)codes_T, (long long)codes_t0,
                     (long long)lat_T, (long long)lat_t0);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_lstm_layer_multi(const float* gin, const void* whh, const void* skip, void* y, float* hbuf, uint32_t* counters,
                                     int B, int T, int H, int ld_y, int dtype, void* stream) {
  JEN1_CHECK(dtype == JEN1_F32 || dtype == JEN1_BF16, "jen1_lstm_layer_multi: dtype must be JEN1_F32 or JEN1_BF16");
  JEN1_CHECK(gin && whh && y && hbuf && counters, "jen1_lstm_layer_multi: NULL argument");
  JEN1_CHECK(B >= 1 && T >= 1 && ld_y >= H, "jen1_lstm_layer_multi: bad shape B=%d T=%d H=%d ld_y=%d", B, T, H, ld_y);
  JEN1_CHECK(H == 256 || H == 512 || H == 1024, "jen1_lstm_layer_multi: H must be 256, 512 or 1024");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == JEN1_BF16 && H == 512 && B > 1) {
    // matrix-core variant: 16 sequences per group (hbuf / counters are sized for 8 per group by the caller: half as many groups)
    const int groups16 = (B + LSTM_MB - 1) / LSTM_MB;
    JEN1_CHECK(groups16 * (H / LSTM_UPW) <= 256, "jen1_lstm_layer_multi: too many workgroups to be co-resident");
    hipLaunchKernelGGL(lstm_multi_mfma_kernel, dim3(H / LSTM_UPW, groups16), dim3(1024), 0, s, gin, reinterpret_cast<const bf16_t*>(whh),
                       reinterpret_cast<const bf16_t*>(skip), reinterpret_cast<bf16_t*>(y), hbuf, counters, B, T, H, ld_y);
    JEN1_HIP(hipGetLastError());
    return 0;
  }
  const int groups = (B + LSTM_LB - 1) / LSTM_LB, nw = H / LSTM_UPW;
  JEN1_CHECK(groups * nw <= 256, "jen1_lstm_layer_multi: %d workgroups must be co-resident (at most 256)", groups * nw);
  const dim3 grid(nw, groups);
#define JEN1_LSTMM(TT, KS) hipLaunchKernelGGL((lstm_multi_kernel<TT, KS>), grid, dim3(1024), 0, s, gin, whh, skip, y, hbuf, counters, B, T, H, ld_y)
  if (dtype == JEN1_F32) { if (H == 256) JEN1_LSTMM(float, 32); else if (H == 512) JEN1_LSTMM(float, 64); else JEN1_LSTMM(float, 128); }
  else { if (H == 256) JEN1_LSTMM(bf16_t, 32); else if (H == 512) JEN1_LSTMM(bf16_t, 64); else JEN1_LSTMM(bf16_t, 128); }
#undef JEN1_LSTMM
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_lstm_layer(const float* gin, const void* whh_t, const void* skip, void* y, int B, int T, int H, int ld_y, int dtype,
                               void* stream) {
  JEN1_CHECK(dtype == JEN1_F32 || dtype == JEN1_BF16, "jen1_lstm_layer: dtype must be JEN1_F32 or JEN1_BF16");
  JEN1_CHECK(gin && whh_t && y, "jen1_lstm_layer: NULL argument");
  JEN1_CHECK(B >= 1 && T >= 1 && ld_y >= H, "jen1_lstm_layer: bad shape B=%d T=%d H=%d ld_y=%d", B, T, H, ld_y);
  JEN1_CHECK(H == 256 || H == 512 || H == 1024, "jen1_lstm_layer: H must be 256, 512 or 1024 (4H a multiple of the 1024 threads)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t lds = sizeof(float) * 5 * H;
#define JEN1_LSTM(TT, RPT) hipLaunchKernelGGL((lstm_layer_kernel<TT, RPT>), dim3(B), dim3(1024), lds, s, gin, whh_t, skip, y, T, H, ld_y)
  const int rpt = 4 * H / 1024;
  if (dtype == JEN1_F32) { if (rpt == 1) JEN1_LSTM(float, 1); else if (rpt == 2) JEN1_LSTM(float, 2); else JEN1_LSTM(float, 4); }
  else { if (rpt == 1) JEN1_LSTM(bf16_t, 1); else if (rpt == 2) JEN1_LSTM(bf16_t, 2); else JEN1_LSTM(bf16_t, 4); }
#undef JEN1_LSTM
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_codec_segment_scales(const float* audio, float* scale, int B, int C, int64_t N, int L, int stride, int S, void* stream) {
  JEN1_CHECK(audio && scale, "jen1_codec_segment_scales: NULL argument");
  JEN1_CHECK(B >= 1 && B <= 65535 && C >= 1 && N >= 1 && L >= 1 && stride >= 1 && S >= 1, "jen1_codec_segment_scales: bad shape");
  JEN1_CHECK((int64_t)(S - 1) * stride < N, "jen1_codec_segment_scales: segment %d starts past the %lld samples", S - 1, (long long)N);
  hipLaunchKernelGGL(codec_segment_scales_kernel, dim3(S, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), audio, scale, C,
                     (long long)N, L, stride, S);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_codec_segment_cut(const float* audio, const float* scale, void* rows, int B, int C, int64_t N, int L, int stride, int S,
                                      int s0, int n_sel, int dtype, void* stream) {
  JEN1_CHECK(dtype == JEN1_F32 || dtype == JEN1_BF16, "jen1_codec_segment_cut: dtype must be JEN1_F32 or JEN1_BF16");
  JEN1_CHECK(audio && rows, "jen1_codec_segment_cut: NULL argument");
  JEN1_CHECK(B >= 1 && C >= 1 && C <= 8 && N >= 1 && L >= 1 && stride >= 1 && S >= 1, "jen1_codec_segment_cut: bad shape");
  JEN1_CHECK(s0 >= 0 && n_sel >= 1 && s0 + n_sel <= S && (int64_t)n_sel * B <= 65535, "jen1_codec_segment_cut: bad segment range %d + %d of %d",
             s0, n_sel, S);
  JEN1_CHECK((int64_t)(s0 + n_sel - 1) * stride + L <= N, "jen1_codec_segment_cut: segment %d of length %d ends past the %lld samples",
             s0 + n_sel - 1, L, (long long)N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((L + 255) / 256, n_sel * B);
  if (dtype == JEN1_F32)
    hipLaunchKernelGGL(codec_segment_cut_kernel<float>, grid, dim3(256), 0, s, audio, scale, reinterpret_cast<float*>(rows), B, C, (long long)N, L,
                       stride, S, s0);
  else
    hipLaunchKernelGGL(codec_segment_cut_kernel<bf16_t>, grid, dim3(256), 0, s, audio, scale, reinterpret_cast<bf16_t*>(rows), B, C, (long long)N,
                       L, stride, S, s0);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_codec_pad1d(const void* x, void* y, int rows, int L, int ld, int left, int right, int dtype, void* stream) {
  JEN1_CHECK(dtype == JEN1_F32 || dtype == JEN1_BF16, "jen1_codec_pad1d: dtype must be JEN1_F32 or JEN1_BF16");
  JEN1_CHECK(x && y, "jen1_codec_pad1d: NULL argument");
  JEN1_CHECK(rows >= 1 && L >= 1 && ld >= 8 && ld % 8 == 0 && left >= 0 && right >= 0, "jen1_codec_pad1d: bad shape rows=%d L=%d ld=%d (%d, %d)",
             rows, L, ld, left, right);
  const int units = ld * (dtype == JEN1_F32 ? 4 : 2) / 16;
  const long long total = (long long)rows * (L + left + right) * units;
  JEN1_CHECK(total <= 0x7fffffffLL * 256, "jen1_codec_pad1d: too many elements");
  hipLaunchKernelGGL(codec_pad1d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(y), total, L, units, left, right);
  JEN1_HIP(hipGetLastError());
  return 0;
}

extern "C" int jen1_codec_overlap_add(const jen1_ola_seg* segs, int S, const float* scale, float* out, int B, int C, int ld, int N_out,
                                      int stride, int L0, int L_last, int dtype, void* stream) {
  JEN1_CHECK(dtype == JEN1_F32 || dtype == JEN1_BF16, "jen1_codec_overlap_add: dtype must be JEN1_F32 or JEN1_BF16");
  JEN1_CHECK(segs && out, "jen1_codec_overlap_add: NULL argument");
  JEN1_CHECK(S >= 1 && B >= 1 && B <= 65535 && C >= 1 && C <= 8 && ld == 8, "jen1_codec_overlap_add: bad shape S=%d B=%d C=%d ld=%d (ld must be 8)",
             S, B, C, ld);
  JEN1_CHECK(stride >= 1 && L0 >= 1 && L_last >= 1 && L_last <= L0 && (S == 1 || stride <= L0),
             "jen1_codec_overlap_add: bad frames stride=%d L0=%d L_last=%d", stride, L0, L_last);
  JEN1_CHECK(N_out >= 1 && (int64_t)N_out <= (int64_t)stride * (S - 1) + L_last, "jen1_codec_overlap_add: N_out=%d is more than the frames cover",
             N_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((N_out + 255) / 256, B);
  if (dtype == JEN1_F32)
    hipLaunchKernelGGL(codec_overlap_add_kernel<float>, grid, dim3(256), 0, s, segs, S, scale, out, C, N_out, stride, L0);
  else
    hipLaunchKernelGGL(codec_overlap_add_kernel<bf16_t>, grid, dim3(256), 0, s, segs, S, scale, out, C, N_out, stride, L0);
  JEN1_HIP(hipGetLastError());
  return 0;
}
