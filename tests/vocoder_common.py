"""Oracle of the inverse STFT and the phase vocoder (csrc/vocoder.hip, jen1_amd/spectral.py, jen1_amd/effects.py), restated without the
package: ``torch.istft`` on the CPU in float64, and the textbook phase vocoder (``torchaudio.functional.phase_vocoder``'s formulas) in
numpy float64.  The float32 variants serve only to size tolerances: a kernel is allowed spectral_common.TOL_FACTOR times what float32
alone costs on the same input."""
import numpy as np
import torch

import spectral_common as SC

RATES = (0.5, 0.8, 1.0, 1.25, 2.0, 2.0 ** (1.0 / 12.0))

# (n_fft, hop, win_length, n): the shapes of the inverse transform
ISTFT_SHAPES = [
    (256, 64, 256, 129),           # 3 frames: a lone last frame in the only pass
    (256, 64, 256, 1000),          # 16 frames, n % hop != 0
    (256, 100, 200, 1000),         # hop does not divide n_fft, the window is shorter than the frame
    (2048, 512, 2048, 24000),      # more than two output runs and more than two frame passes
    (4096, 1024, 4096, 24000),     # largest transform: the tightest LDS budget
]


def window_of(win_length, lifted=False):
    """float32 values, as float64: the periodic Hann window, or (``lifted``) 0.1 + 0.9 Hann, which has no zero at its ends -- what
    center=False needs, where the first sample is under the first frame's first window value alone"""
    w = SC.window64(win_length)
    return (0.1 + 0.9 * w).float().double() if lifted else w


def istft_cpu(spec, n_fft, hop, win_length, center=True, length=None, dtype=torch.float64, lifted=False):
    """``torch.istft`` of complex [rows, bins, frames] on the CPU in ``dtype``: real [rows, length]"""
    cdt = torch.complex128 if dtype == torch.float64 else torch.complex64
    w = window_of(win_length, lifted).to(dtype)
    return torch.istft(torch.from_numpy(np.ascontiguousarray(spec)).to(cdt), n_fft, hop_length=hop, win_length=win_length, window=w, center=center,
                       length=length).numpy()


def vocoder_frames(T, rate):
    return len(np.arange(0, T, rate))


def phase_vocoder64(spec, rate, hop, n_fft, float32_magnitudes=False):
    """the textbook phase vocoder on complex [rows, bins, T] in float64: complex128 [rows, bins, J].

        tau_j = j rate, i = floor tau_j, alpha = tau_j - i, two zero frames appended
        |Y_j| = alpha |X_{i+1}| + (1 - alpha) |X_i|
        dphi_j = wrap(arg X_{i+1} - arg X_i - a_k) + a_k,  a_k = 2 pi hop k / n_fft;   phi_j = arg X_0 + sum_{m < j} dphi_m;  arg 0 = 0

    The phase is summed in TURNS reduced to [0, 1) term by term, so the float64 sum stays below J and keeps 1e-12 of a turn over thousands
    of frames (a sum of radians that reaches 1e6 would not).  ``float32_magnitudes``: the magnitudes and the result rounded to float32,
    everything else unchanged -- the part of the error float32 storage alone accounts for."""
    X = np.asarray(spec).astype(np.complex128)
    rows, bins, T = X.shape
    assert bins == n_fft // 2 + 1
    tau = np.arange(0, T, rate)
    i = np.floor(tau).astype(np.int64)
    alpha = tau - i
    Xp = np.concatenate([X, np.zeros((rows, bins, 2), np.complex128)], axis=2)
    mag = np.abs(Xp)
    if float32_magnitudes:
        mag = mag.astype(np.float32).astype(np.float64)
    turns = np.where(Xp == 0, 0.0, np.angle(Xp)) / (2.0 * np.pi)
    a = ((hop * np.arange(bins)) % n_fft) / float(n_fft)                     # a_k / 2 pi modulo 1, exact
    d = turns[:, :, i + 1] - turns[:, :, i] - a[None, :, None]
    d = d - np.round(d) + a[None, :, None]
    d = d - np.floor(d)
    phi = turns[:, :, :1] + np.concatenate([np.zeros((rows, bins, 1)), np.cumsum(d[:, :, :-1], axis=2)], axis=2)
    phi = 2.0 * np.pi * (phi - np.floor(phi))
    Y = (alpha * mag[:, :, i + 1] + (1.0 - alpha) * mag[:, :, i]) * (np.cos(phi) + 1j * np.sin(phi))
    return Y.astype(np.complex64).astype(np.complex128) if float32_magnitudes else Y


def peak_hz(x, sr):
    """the frequency of the largest bin of a Hann-windowed spectrum of x, refined by a parabola through the log magnitudes around it"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    S = np.abs(np.fft.rfft(x * np.hanning(n)))
    k = int(np.argmax(S[1:-1])) + 1
    a, b, c = np.log(S[k - 1] + 1e-300), np.log(S[k] + 1e-300), np.log(S[k + 1] + 1e-300)
    return (k + 0.5 * (a - c) / (a - 2.0 * b + c)) * sr / n
