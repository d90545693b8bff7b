/*
 * libjen1_hip.so -- tempo and key of waveforms: the onset-strength envelope (log-compressed mel flux) and the 12-class chromagram in one
 * pass over the waveform, and two fixed-order float64 estimators on them.  Not in the reference.  csrc/spectral.hip holds
 * jen1_music_features (next to the tile FFT it uses), csrc/analysis.hip the estimators, jen1_amd/analysis.py the host side.
 *
 * x, row_stride, window, twiddle, rows, n, n_fft, hop, win_length, center and the band_* arguments are those of include/jen1_spectral.h.
 * Every function validates its arguments on the host before anything is launched and returns 0, or non-zero with jen1_last_error()
 * set; `stream` is a hipStream_t.  Every sum has one fixed order and nothing uses atomics: the same bits on every run, wherever in the
 * batch a row sits and whichever tile a frame falls in.
 */
#ifndef JEN1_ANALYSIS_H
#define JEN1_ANALYSIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* frames of one row whose results one workgroup of jen1_music_features writes (it transforms one more, the frame in front of them,
 * for the flux of its first); 0 for a bad n_fft */
int jen1_music_features_tile_frames(int n_fft);

/* the largest n_bands whose mel columns fit in LDS next to the transform buffers at this n_fft; 0 for a bad n_fft */
int jen1_music_features_max_bands(int n_fft);

/* With |X[k,t]| the magnitude spectrum of frame t (the framing of jen1_stft) and melW the banded matrix:
 *   Y[b,t]      = log1p(gamma * sum_k melW[b,k] |X[k,t]|)
 *   onset[t]    = (1 / n_bands) sum_b max(0, Y[b,t] - Y[b,t-1])  for t >= 1,  onset[0] = 0          float32 [rows][frames]
 *   chroma[p,t] = sum_k chroma_w[p][k] |X[k,t]|^2                                                   float32 [rows][12][frames]
 * chroma_w: float32 [12][n_fft / 2 + 1], dense, in device memory.  gamma > 0.  Neither spectrum nor mel values are written anywhere. */
int jen1_music_features(const float* x, int64_t row_stride, float* onset, float* chroma, const float* window, const float* twiddle,
                        const int32_t* band_lo, const int32_t* band_hi, const int32_t* band_off, const float* band_w, int n_bands,
                        int64_t n_weights, const float* chroma_w, float gamma, int rows, int64_t n, int n_fft, int hop, int win_length,
                        int center, void* stream);

/* the lags jen1_tempo forms for these arguments: ceil(60 fps / bpm_max) - 1 ... floor(60 fps / bpm_min) + 1; 0 for arguments it refuses */
int jen1_tempo_lags(double fps, double bpm_min, double bpm_max);

/* bytes of jen1_tempo's workspace (the autocorrelation of every row, float64); 0 for arguments it refuses */
int64_t jen1_tempo_workspace_bytes(int rows, double fps, double bpm_min, double bpm_max);

/* onset float32 [rows][frame_stride]; frames int32 [rows] in device memory (valid frames of a row, clipped to [0, frame_stride]; NULL:
 * frame_stride for every row).  Per row with F = frames[r]:
 *   u = onset - mean(onset[0:F]);   r[l] = sum_{t < F - l} u[t] u[t + l]  (float64)
 *   candidates l in [ceil(60 fps / bpm_max), min(floor(60 fps / bpm_min), F - 2)]
 *   s[l] = r[l] exp(-0.5 ((log2(60 fps / l) - log2(prior_bpm)) / prior_octaves)^2);   L = argmax s, the lowest lag on a tie
 *   a, b, c = s[L-1], s[L], s[L+1];  d = a - 2 b + c;  l* = L + 0.5 (a - c) / d if d < 0, else L
 *   tempo = 60 fps / l*,  strength = r[L] / r[0];   no candidate or r[0] == 0: tempo = strength = 0
 * tempo, strength: float32 [rows].  acf: NULL or float64 [rows][jen1_tempo_lags(...)], r[l] from l = ceil(60 fps / bpm_max) - 1 on.
 * workspace: 8-byte aligned device memory.  Two launches: the autocorrelation (several workgroups per row), then the choice. */
int jen1_tempo(const float* onset, int64_t frame_stride, const int32_t* frames, float* tempo, float* strength, double* acf, int rows,
               double fps, double bpm_min, double bpm_max, double prior_bpm, double prior_octaves, void* workspace, int64_t workspace_bytes,
               void* stream);

/* chroma float32 [rows][12][frame_stride]; frames as above.  profile float64 [rows][12]: the sums over the valid frames; corr float32
 * [rows][24]: the Pearson correlation of the profile with the Krumhansl-Kessler profile of key j (tonic j % 12, 0 = C; minor for
 * j >= 12); key int32 [rows] = argmax corr, the lowest index on a tie; strength float32 [rows] = corr[key].  A profile without variance:
 * key = -1, strength = 0, corr = 0. */
int jen1_key(const float* chroma, int64_t frame_stride, const int32_t* frames, int32_t* key, float* strength, double* profile, float* corr,
             int rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif
