/*
 * libjen1_hip.so -- the second half of ITU-R BS.1770-4 (Annex 2): a true-peak meter that reads a waveform between its samples, and
 * the look-ahead limiter that holds a waveform under a true-peak ceiling.  Not in the reference.  csrc/limiter.hip holds the
 * kernels, jen1_amd/audio.py (true_peak, limit_true_peak, normalize_audio(limit="truepeak")) the host side.
 *
 * Common arguments
 *   x           float32 [rows][C][L], packed; C is 1 or 2
 *   env         float64, row r at env + r * env_stride (env_stride >= L, in doubles): the linked envelope
 *                 env[r][n] = max over the channels and the F phases of |o[n F + p]|,
 *                 o[n F + p] = sum_{k < 16} taps[p - 1][k] x[n + 8 - k]   (p = 1 .. F - 1, zeros outside the row),   o[n F] = x[n]
 *               in float64, the sum as 16 FMAs in ascending k
 * Every function validates its arguments on the host before anything is launched and returns 0, or non-zero with jen1_last_error()
 * set; `stream` is a hipStream_t.  No kernel uses float atomics and every sum has one order: the same bits on every run, wherever in
 * the batch a row sits.
 */
#ifndef JEN1_LIMITER_H
#define JEN1_LIMITER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* consecutive samples of one row that one workgroup of the meter, of the scan and of the gain kernel owns */
int jen1_true_peak_tile(void);

/* samples one thread of the release scan owns (a chunk): a workgroup's tile is 256 chunks, and the scan carries its state from
 * chunk to chunk inside a tile and from tile to tile between the launches */
int jen1_limiter_chunk(void);

/* the longest look-ahead in samples (what the gain kernel's tile keeps of its neighbour in LDS) */
int jen1_limiter_max_lookahead(void);

/* bytes of scratch jen1_true_peak needs (one partial peak per tile); 0 for a bad shape */
int64_t jen1_true_peak_workspace_bytes(int rows, int C, int64_t L);

/* env (may be NULL: the peak alone) and peak [rows] float64 = max_n env[r][n], linear (0 for silence).
 *   taps   float64 [F - 1][16] in HOST memory (read before the launch; NULL is allowed for F = 1);  F is 1, 2 or 4 */
int jen1_true_peak(const float* x, double* env, int64_t env_stride, double* peak, const double* taps, int F, int rows, int C, int64_t L,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* bytes of scratch jen1_limit_true_peak needs (the held reduction over L + A samples, one composite and one start state per tile);
 * 0 for a bad shape or a look-ahead outside [0, jen1_limiter_max_lookahead()] */
int64_t jen1_limiter_workspace_bytes(int rows, int64_t L, int A);

/* y[r][c][n] = float32(s[r][n] * (double)x[r][c][n]), one gain for every channel of a row, and optionally red[r][n] = 1 - s[r][n]:
 *   q[n] = 1 - min(1, ceiling / env[n])
 *   Q[i] = max q[k], k = max(i, 0) .. min(i + A, L - 1),  i = -A .. L - 1          (hold: the row is preceded by A samples of silence)
 *   d[i] = max(Q[i], rho d[i - 1]),  d[-A - 1] = 0                                   (release)
 *   s[n] = 1 - sum_{j = 0 .. A} window[j] d[n - j]                                   (attack: FMAs in ascending j)
 * all in float64.  A row with env <= ceiling everywhere has d = 0 and s = 1: it comes back bit for bit.
 *   y        row r at y + r * y_stride (y_stride >= C L, in floats); y == x with y_stride == C L is allowed
 *   red      float64, row r at red + r * red_stride (red_stride >= L); may be NULL
 *   env      as jen1_true_peak wrote it
 *   window   float64 [A + 1] in device memory, 8-byte aligned: non-negative weights that sum to 1
 *   ceiling  linear, positive and finite;  rho in [0, 1);  A in [0, jen1_limiter_max_lookahead()] */
int jen1_limit_true_peak(const float* x, float* y, int64_t y_stride, double* red, int64_t red_stride, const double* env, int64_t env_stride,
                         const double* window, int rows, int C, int64_t L, int A, double ceiling, double rho, void* workspace,
                         int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
