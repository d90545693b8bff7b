"""The float64 restatement the resampler's tests compare against: torchaudio's default windowed-sinc resampler in its DENSE form, written
literally from the formulas (the zero-padded signal and the K-tap rows), independent of the compact table of jen1_amd/audio.py.

    g = gcd(sr, target_sr);  o = sr // g;  n = target_sr // g
    base = min(o, n) * 0.99;  w = ceil(6 * o / base);  K = 2 * w + o
    t[p][k] = ((k - w) / o - p / n) * base, clamped to [-6, 6]
    h[p][k] = (1 if t == 0 else sin(pi t) / (pi t)) * cos(pi t / 12)**2 * (base / o)
    xp[i] = x[i - w], zero outside [0, L);   y[j n + p] = sum_k h[p][k] * xp[j o + k];   len(y) = ceil(n L / o)
"""
import math

import numpy as np

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 88200, 96000)
PAIRS_INTO_48K = tuple((r, 48000) for r in RATES)
ALL_PAIRS = PAIRS_INTO_48K + tuple((48000, r) for r in RATES)


def geometry(sr, target_sr):
    """(o, n, w, K)"""
    g = math.gcd(sr, target_sr)
    o, n = sr // g, target_sr // g
    base = min(o, n) * 0.99
    w = int(math.ceil(6 * o / base))
    return o, n, w, 2 * w + o


def dense_table(sr, target_sr, dtype=np.float32):
    """h [n, K]: evaluated in float64, rounded to ``dtype`` once"""
    o, n, w, K = geometry(sr, target_sr)
    base = min(o, n) * 0.99
    h = np.empty((n, K), np.float64)
    for p in range(n):
        t = np.clip(((np.arange(K, dtype=np.float64) - w) / o - p / n) * base, -6.0, 6.0)
        safe = np.where(t == 0, 1.0, t)
        h[p] = np.where(t == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe)) * np.cos(np.pi * t / 12) ** 2 * (base / o)
    return h.astype(dtype)


def dense_resample(x, sr, target_sr, table=None):
    """x [..., L] -> float64 [..., ceil(n L / o)] with the dense K-tap rows (``table``: default the float64 one), sums in float64"""
    o, n, w, K = geometry(sr, target_sr)
    h = (dense_table(sr, target_sr, np.float64) if table is None else table).astype(np.float64)
    x = np.asarray(x, np.float64)
    L = x.shape[-1]
    n_out = -(-n * L // o)
    frames = -(-n_out // n)
    xp = np.zeros(x.shape[:-1] + ((frames - 1) * o + K + w,), np.float64)          # xp[i] = x[i - w]
    xp[..., w:w + L] = x
    y = np.empty(x.shape[:-1] + (frames, n), np.float64)
    for j in range(frames):
        y[..., j, :] = xp[..., j * o:j * o + K] @ h.T
    return y.reshape(x.shape[:-1] + (frames * n,))[..., :n_out]


def mix_channels(x, c_out):
    """the channel rule of encodec.utils.convert_audio on float32 [..., C, L]: the mean is formed in float32, (l + r) * 0.5f"""
    x = np.asarray(x, np.float32)
    c_in = x.shape[-2]
    if c_out == 1:
        return x if c_in == 1 else ((x[..., 0:1, :] + x[..., 1:2, :]) * np.float32(0.5)).astype(np.float32)
    if c_out == 2:
        return x if c_in == 2 else np.concatenate([x, x], axis=-2)
    raise RuntimeError("impossible channel conversion")
