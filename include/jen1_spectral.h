/*
 * libjen1_hip.so -- spectral metrics of waveforms: a framed, windowed real FFT (the layout and framing of torch.stft), a banded
 * filterbank on its power or magnitude (log-mel), and the two-signal distance sums of the multi-resolution STFT loss.  Not in the
 * reference.  csrc/spectral.hip holds the kernels, jen1_amd/spectral.py the host side.
 *
 * Common arguments
 *   x           float32 [rows][n], row r at x + r * row_stride (row_stride >= n, in floats)
 *   window      float32 [win_length] in device memory; win_length <= n_fft, centred in the frame with (n_fft - win_length) / 2 zeros
 *               on its left (the difference may be odd)
 *   twiddle     float32 [n_fft][2] in device memory: (cos, -sin)(2 pi m / n_fft), formed in float64 and rounded once
 *   n_fft       256, 512, 1024, 2048 or 4096;  hop in [1, n_fft];  center 0 or 1
 *   center = 1  reflect padding of n_fft / 2 on either side by index mirroring (needs n > n_fft / 2); frames = 1 + n / hop
 *   center = 0  needs n >= n_fft; frames = 1 + (n - n_fft) / hop
 * Every function validates its arguments on the host before anything is launched and returns 0, or non-zero with jen1_last_error()
 * set; `stream` is a hipStream_t.  The sums of jen1_spectral_distance have one fixed order and use no atomics: the same bits on every
 * run, wherever in the batch a row sits.
 */
#ifndef JEN1_SPECTRAL_H
#define JEN1_SPECTRAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JEN1_SPEC_COMPLEX 0         /* interleaved (re, im) float32 pairs */
#define JEN1_SPEC_MAGNITUDE 1       /* |X| */
#define JEN1_SPEC_POWER 2           /* |X|^2 */

#define JEN1_SPEC_LOG_NONE 0
#define JEN1_SPEC_LOG_E 1           /* log(max(v, floor)) */
#define JEN1_SPEC_LOG_DB 2          /* 10 log10(max(v, floor)) */

/* frames of the framing above; -1 for arguments the transforms refuse */
int64_t jen1_stft_frames(int64_t n, int n_fft, int hop, int center);

/* consecutive frames of one row that one workgroup of jen1_stft / jen1_mel transforms (two per complex FFT); 0 for a bad n_fft */
int jen1_stft_tile_frames(int n_fft);

/* out [rows][n_fft / 2 + 1][frames] (frames fastest) of `kind`: float32, two per element for JEN1_SPEC_COMPLEX */
int jen1_stft(const float* x, int64_t row_stride, float* out, const float* window, const float* twiddle, int rows, int64_t n, int n_fft,
              int hop, int win_length, int center, int kind, void* stream);

/* The same framing with a banded matrix applied to the spectrum while it is in LDS:
 *   v[b] = sum_{k in [band_lo[b], band_hi[b])} band_w[band_off[b] + k - band_lo[b]] * S[k],   S = |X|^2 (JEN1_SPEC_POWER) or |X|
 * band_lo / band_hi / band_off: int32 [n_bands], band_w: float32 [n_weights], all in device memory.  A band that leaves [0, n_fft/2 + 1]
 * is clipped to it and a band whose weights would leave [0, n_weights) counts as empty: no index is formed from them unchecked.
 * out [rows][n_bands][frames] float32, through log_mode with `floor` (> 0 when a log is asked for). */
int jen1_mel(const float* x, int64_t row_stride, float* out, const float* window, const float* twiddle, const int32_t* band_lo,
             const int32_t* band_hi, const int32_t* band_off, const float* band_w, int n_bands, int64_t n_weights, int rows, int64_t n,
             int n_fft, int hop, int win_length, int center, int kind, int log_mode, float floor, void* stream);

/* frames of a row per workgroup of jen1_spectral_distance (one per complex FFT: x real, y imaginary); 0 for a bad n_fft */
int jen1_spectral_distance_tile_frames(int n_fft);

/* bytes of the per-workgroup partial sums; 0 for arguments the call refuses */
int64_t jen1_spectral_distance_workspace_bytes(int rows, int64_t n, int n_fft, int hop, int center);

/* x (test) and y (reference), same shape.  out [rows][3] float64:
 *   out[r][0] = sum (|X| - |Y|)^2     out[r][1] = sum |Y|^2     out[r][2] = sum |log max(|X|, floor) - log max(|Y|, floor)|
 * over all bins and frames of row r.  With n_bands > 0 the sums run over the banded values of jen1_mel (of `kind`) instead of the
 * bins' magnitudes; with n_bands == 0 the band pointers are ignored.  floor > 0.  workspace: 8-byte aligned device memory. */
int jen1_spectral_distance(const float* x, int64_t x_stride, const float* y, int64_t y_stride, double* out, const float* window,
                           const float* twiddle, const int32_t* band_lo, const int32_t* band_hi, const int32_t* band_off,
                           const float* band_w, int n_bands, int64_t n_weights, int rows, int64_t n, int n_fft, int hop, int win_length,
                           int center, int kind, float floor, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
