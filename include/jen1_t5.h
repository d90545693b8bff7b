/*
 * libjen1_hip.so -- the text side of the conditioning: the encoder stack of T5 / flan-T5 (transformers.T5EncoderModel, eval mode) that
 * turns token ids into the cross-attention context of the denoiser (reference jen1/conditioners.py:32-111).  The linears of the stack are
 * jen1_train_gemm products (include/jen1_train.h); the four kernels here are what lies between them.  jen1_amd/t5.py is the host side.
 *
 * dtype (JEN1_F32 / JEN1_BF16, include/jen1_hip.h) is the COMPUTE dtype: what the linears read and write.  The residual stream is
 * float32 in either mode.  Every function returns 0, or non-zero with jen1_last_error() set; `stream` is a hipStream_t.
 */
#ifndef JEN1_T5_H
#define JEN1_T5_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JEN1_T5_MAX_TOKENS 128      /* longest sequence jen1_t5_attention takes (the reference tokenises to max_length = 128) */
#define JEN1_T5_ACT_GELU_NEW 0      /* gated: gelu_new(a) * b, the flan-t5 family */
#define JEN1_T5_ACT_RELU 1          /* not gated: relu(a), the t5 family */

/* out[r][0 .. C) = table[ids[r]][0 .. C), float32.  An id outside [0, vocab) is never used as an index: its row is written as zeros and
 * *err_flag (int32 in device memory, zeroed by the caller) becomes 1. */
int jen1_t5_embed(const int64_t* ids, const float* table, float* out, int32_t* err_flag, int rows, int vocab, int C, void* stream);

/* T5LayerNorm with the residual add in front of it:
 *   if add != NULL: h[r][c] += add[r][c]   (h and add float32, rows C apart; h is updated in place)
 *   y[r][c] = (dtype) (h[r][c] * rsqrt(mean_c h[r][c]^2 + eps) * weight[c])     (no mean subtraction, no bias; the mean in float32)
 * y: rows C apart, of `dtype`.  Any rows >= 1 and C >= 1. */
int jen1_t5_rmsnorm(float* h, const float* add, const float* weight, void* y, int rows, int C, float eps, int dtype, void* stream);

/* Self-attention of one T5 block on the matrix cores, one workgroup per (sample, head, 64 query rows):
 *   S[i][j] = q_i . k_j + bias_tab[h][j - i + N - 1]      (no 1 / sqrt(d) scale)
 *   P = softmax_j over the keys with key_mask[b][j] != 0 (float32);   o_i = sum_j P[i][j] v_j
 * qkv: [B][N][ld] of `dtype`, the output of the stacked q | k | v projection: q of head h in columns [h d, (h + 1) d), k at + heads * d,
 * v at + 2 * heads * d.  o: [B][N][ldo] of `dtype`, head h in columns [h d, (h + 1) d).  bias_tab: float32 [heads][2 N - 1].
 * key_mask: int32 [B][N], any pattern; a sample without a single kept key gives zero rows (the host side refuses such a mask).
 * N <= JEN1_T5_MAX_TOKENS, d in {16, 32, 64}; qkv / o on 16-byte boundaries, ld and ldo multiples of 8. */
int jen1_t5_attention(const void* qkv, int64_t ld, void* o, int64_t ldo, const float* bias_tab, const int32_t* key_mask, int B, int heads,
                      int N, int d, int dtype, void* stream);

/* The feed-forward activation between wi and wo:
 *   JEN1_T5_ACT_GELU_NEW: x [rows][2 F] holds wi_0 x | wi_1 x;  y[r][f] = gelu_new(x[r][f]) * x[r][F + f]
 *   JEN1_T5_ACT_RELU:     x [rows][F];                           y[r][f] = max(x[r][f], 0)
 * gelu_new(a) = 0.5 a (1 + tanh(sqrt(2 / pi) (a + 0.044715 a^3))).  x and y of `dtype`, y [rows][F]. */
int jen1_t5_gate(const void* x, void* y, int rows, int F, int act, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
