/*
 * libjen1_hip.so -- the way back from a spectrogram and the map between two of them: an inverse STFT with a deterministic
 * overlap-add (the semantics of torch.istft on the layout jen1_stft writes) and the phase vocoder that changes a spectrogram's frame
 * rate.  Not in the reference.  csrc/vocoder.hip holds the kernels, jen1_amd/spectral.py (istft, phase_vocoder) and
 * jen1_amd/effects.py (time_stretch, pitch_shift) the host side.
 *
 * Common arguments
 *   spec        float32 [rows][n_fft / 2 + 1][frames][2]: interleaved (re, im), frames fastest, 8-byte aligned, rows packed
 *   n_fft       256, 512, 1024, 2048 or 4096;  hop in [1, n_fft]
 * Every function validates its arguments on the host before anything is launched and returns 0, or non-zero with jen1_last_error()
 * set; `stream` is a hipStream_t.  Neither kernel uses atomics: the same bits on every run, wherever in the batch a row sits.
 */
#ifndef JEN1_VOCODER_H
#define JEN1_VOCODER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* consecutive output samples of one row that one workgroup of jen1_istft owns; 0 for a bad n_fft */
int jen1_istft_tile_samples(int n_fft);

/* frames one workgroup of jen1_istft inverse-transforms per pass (two per complex FFT); 0 for a bad n_fft */
int jen1_istft_tile_frames(int n_fft);

/* out [rows][length] float32, row r at out + r * out_stride (out_stride >= length, in floats):
 *   y[s] = sum_t w[u - t hop] irfft(X_t)[u - t hop] / sum_t w^2[u - t hop],   u = s + (center ? n_fft / 2 : 0),
 * over the frames t in [0, frames) that reach u, in ascending t; w is the window centred in the frame ((n_fft - win_length) / 2 zeros
 * on its left); the imaginary parts of the DC and Nyquist bins are ignored.  Samples at or past u = n_fft + hop (frames - 1) are exact
 * zeros, so `length` may exceed what the frames hold.
 *   window       float32 [win_length] in device memory
 *   window_host  the same values in HOST memory: NOLA is checked with them in float64 before the launch, and the call is refused
 *                when the least sum_t w^2 over the samples the frames reach is at most 1e-11 (the threshold of torch.istft)
 *   twiddle      float32 [n_fft][2] in device memory: (cos, -sin)(2 pi m / n_fft), the table of jen1_stft */
int jen1_istft(const float* spec, float* out, int64_t out_stride, const float* window, const float* window_host, const float* twiddle,
               int rows, int64_t frames, int64_t length, int n_fft, int hop, int win_length, int center, void* stream);

/* frames of the vocoder's output for `frames` input frames: how many j >= 0 have j * rate < frames (len(numpy.arange(0, frames,
 * rate))); -1 for frames < 1, a rate that is not positive and finite, or a count of 2^31 or more */
int64_t jen1_vocoder_frames(int64_t frames, double rate);

/* output frames one step of the phase scan covers (a wave's lanes): the scan carries its sum across steps of this length */
int jen1_phase_vocoder_tile_frames(void);

/* spec [rows][bins][frames] -> out [rows][bins][J] complex, J = jen1_vocoder_frames(frames, rate), with X_frames = 0:
 *   tau_j = j rate,  i = floor tau_j,  alpha = tau_j - i
 *   |Y_j| = alpha |X_{i+1}| + (1 - alpha) |X_i|
 *   dphi_j = wrap(arg X_{i+1} - arg X_i - a_k) + a_k,   a_k = 2 pi hop k / n_fft,  wrap to (-pi, pi] by the nearest whole turn
 *   phi_0 = arg X_0,  phi_j = phi_0 + sum_{m < j} dphi_m,   Y_j = |Y_j| exp(i phi_j),   arg 0 = 0
 * Angles and magnitudes are formed in float64; the phase sum is exact: turns modulo 1 in 64-bit fixed point, with
 * a_k / 2 pi mod 1 = ((hop k) mod n_fft) / n_fft.  One rounding to float32, at the store.  bins = n_fft / 2 + 1. */
int jen1_phase_vocoder(const float* spec, float* out, int rows, int64_t frames, int n_fft, int hop, double rate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
