"""Oracle of the spectral metrics (jen1_amd/spectral.py, csrc/spectral.hip), restated without the package: ``torch.stft`` on the CPU in
float64, the mel filterbank formula in numpy float64, and the two distance definitions in float64.  The same chain in float32 on the CPU
serves only to size tolerances: a kernel is allowed 8x the error that float32 ``torch.stft`` itself makes on the same input."""
import math

import numpy as np
import torch

SR = 48000
TOL_FACTOR = 8.0

# (n_fft, hop, win_length, n, rows, center): the smallest shapes at which the kernel can still go wrong
SHAPES = [
    (256, 64, 256, 129, 1, True),         # shortest legal reflect pad; every frame touches a mirror
    (256, 64, 256, 1000, 3, True),        # odd frame count (lone last frame), n % hop != 0, rows not a power of two
    (512, 128, 512, 4096, 2, True),       # hop divides n: the last frame starts exactly at the end
    (1024, 100, 480, 5000, 2, True),      # window shorter than the frame
    (1024, 100, 481, 5000, 1, True),      # odd (n_fft - win_length)
    (2048, 240, 1200, 24000, 4, True),    # frame count spans more than two frame tiles
    (4096, 480, 2400, 24000, 2, True),    # largest transform
    (512, 512, 512, 4096, 1, False),      # center=False, hop = n_fft (no overlap)
    (512, 1, 512, 600, 1, True),          # hop 1
]
KINDS = ("noise", "tone", "chirp", "quiet", "zeros", "impulse")


def signal(kind: str, n: int, seed: int = 0) -> np.ndarray:
    """float32 [n]: one of the six test signals at 48 kHz, seeded"""
    rng = np.random.default_rng([seed, KINDS.index(kind), n])
    t = np.arange(n, dtype=np.float64)
    bed = 1e-3 * rng.standard_normal(n)
    if kind == "noise":
        x = 0.3 * rng.standard_normal(n)
    elif kind == "tone":
        x = 0.8 * np.sin(2 * np.pi * 997.0 * t / SR) + bed
    elif kind == "chirp":
        x = 0.5 * np.sin(2 * np.pi * (100.0 * t + 0.5 * (12000.0 - 100.0) / max(n, 1) * t * t) / SR) + bed
    elif kind == "quiet":
        x = 1e-4 * rng.standard_normal(n)
    elif kind == "zeros":
        x = np.zeros(n)
    elif kind == "impulse":
        x = np.zeros(n)
        x[min(3, n - 1)] = 1.0                 # inside the reflect region of every n_fft: it shows up mirrored in the first frames
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def signals(n: int, rows: int, kinds=KINDS, seed: int = 0) -> np.ndarray:
    """float32 [rows, n]: the kinds cycled over the rows"""
    return np.stack([signal(kinds[r % len(kinds)], n, seed + r // len(kinds)) for r in range(rows)])


def window64(win_length: int) -> torch.Tensor:
    """the periodic Hann window the kernel gets: float64 values rounded to float32, as float64"""
    return torch.hann_window(win_length, periodic=True, dtype=torch.float64).float().double()


def stft_cpu(x: np.ndarray, n_fft: int, hop: int, win_length: int, center: bool, dtype=torch.float64) -> np.ndarray:
    """``torch.stft`` of x [rows, n] on the CPU in ``dtype``: complex [rows, n_fft / 2 + 1, frames]"""
    w = window64(win_length).to(dtype)
    return torch.stft(torch.from_numpy(np.ascontiguousarray(x)).to(dtype), n_fft, hop_length=hop, win_length=win_length, window=w, center=center,
                      pad_mode="reflect", return_complex=True).numpy()


def frames_of(n: int, n_fft: int, hop: int, center: bool) -> int:
    return 1 + n // hop if center else 1 + (n - n_fft) // hop


def row_error(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """per row: max |got - want| / max |want| (0 for an all-zero row whose result is all zero too)"""
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    top = np.abs(w).max(axis=1)
    err = np.abs(g.astype(w.dtype) - w).max(axis=1)
    return np.where(top > 0, err / np.where(top > 0, top, 1.0), err)


# ------------------------------------------------------------------ mel
def hz_to_mel(f, scale):
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * 27.0 / math.log(6.4), 3.0 * f / 200.0)


def mel_to_hz(m, scale):
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp(math.log(6.4) / 27.0 * (m - 15.0)), 200.0 * m / 3.0)


def mel_corners(sr, n_mels, f_min=0.0, f_max=None, scale="htk"):
    f_max = sr / 2.0 if f_max is None else f_max
    return mel_to_hz(np.linspace(hz_to_mel(f_min, scale), hz_to_mel(f_max, scale), n_mels + 2), scale)


def filterbank64(sr, n_fft, n_mels, f_min=0.0, f_max=None, scale="htk", norm=None) -> np.ndarray:
    """[n_mels, n_fft / 2 + 1] float64: max(0, min((f - f_m) / (f_{m+1} - f_m), (f_{m+2} - f) / (f_{m+2} - f_{m+1})))"""
    f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    c = mel_corners(sr, n_mels, f_min, f_max, scale)
    fb = np.zeros((n_mels, f.size))
    for m in range(n_mels):
        fb[m] = np.maximum(0.0, np.minimum((f - c[m]) / (c[m + 1] - c[m]), (c[m + 2] - f) / (c[m + 2] - c[m + 1])))
        if norm == "slaney":
            fb[m] *= 2.0 / (c[m + 2] - c[m])
    return fb


def apply_log(v: np.ndarray, log, floor: float) -> np.ndarray:
    if log is None:
        return v
    v = np.maximum(v, v.dtype.type(floor))
    return np.log(v) if log == "log" else 10.0 * np.log10(v)


# ------------------------------------------------------------------ distances
def distances(X: np.ndarray, Y: np.ndarray, floor: float):
    """(sc, log_mag) per row of two spectrograms [rows, bins, frames] (complex), in their own precision: X the test, Y the reference"""
    ax, ay = np.abs(X), np.abs(Y)
    real = ax.dtype.type
    sc = np.sqrt(((ax - ay) ** 2).sum(axis=(1, 2)) / (ay ** 2).sum(axis=(1, 2)))
    lm = np.abs(np.log(np.maximum(ax, real(floor))) - np.log(np.maximum(ay, real(floor)))).mean(axis=(1, 2))
    return sc, lm


def log_mel_l1(X: np.ndarray, Y: np.ndarray, fb: np.ndarray, floor: float, power: float = 2.0) -> np.ndarray:
    """per row: mean |log max(fb @ |X|^p, floor) - log max(fb @ |Y|^p, floor)| in the precision of X"""
    real = np.abs(X).dtype.type
    fbp = fb.astype(np.abs(X).dtype)
    mx = np.einsum("mk,rkt->rmt", fbp, np.abs(X) ** real(power))
    my = np.einsum("mk,rkt->rmt", fbp, np.abs(Y) ** real(power))
    return np.abs(np.log(np.maximum(mx, real(floor))) - np.log(np.maximum(my, real(floor)))).mean(axis=(1, 2))
