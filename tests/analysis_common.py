"""Oracle of the tempo / key analyser (jen1_amd/analysis.py, include/jen1_analysis.h), restated without the package in numpy float64 from
the definitions alone: the chroma map, the onset flux and chromagram on ``torch.stft`` (CPU, float64), the autocorrelation tempo
estimator and the Krumhansl-Kessler key estimator.  ``features(..., dtype=torch.float32)`` is the same chain in float32 on the CPU and
serves only to size tolerances: a kernel is allowed 8x the error that chain makes on the same input (spectral_common.TOL_FACTOR)."""
import functools
import math

import numpy as np
import torch

import spectral_common as SC

SR = 48000
KK_MAJOR = np.array([6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88])
KK_MINOR = np.array([6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17])
KEY_NAMES = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
KEY_NAMES = KEY_NAMES + [k + "m" for k in KEY_NAMES]
BPMS = (60, 90, 120, 128, 174)
PASSAGES = (("C", 0, 0), ("G", 7, 7), ("Eb", 3, 3), ("Am", 0, 21), ("F#m", -3, 18))       # (name, transposition in semitones, key index)


# ------------------------------------------------------------------ tables
def chroma_matrix(sr, n_fft, a440=440.0, centre_octave=5.0, octave_width=2.0):
    bins = n_fft // 2 + 1
    pit = np.zeros(bins)
    for k in range(1, bins):
        pit[k] = 12.0 * math.log2((k * sr / n_fft) / (a440 / 16.0))
    pit[0] = pit[1] - 18.0
    width = np.ones(bins)
    for k in range(bins - 1):
        width[k] = max(pit[k + 1] - pit[k], 1.0)
    W = np.zeros((12, bins))
    for p in range(12):
        D = np.mod(pit - p + 6.0 + 120.0, 12.0) - 6.0
        W[p] = np.exp(-0.5 * (2.0 * D / width) ** 2)
    W = W / np.sqrt((W ** 2).sum(axis=0))[None, :]
    W = W * np.exp(-0.5 * ((pit / 12.0 - centre_octave) / octave_width) ** 2)[None, :]
    return np.roll(W, -3, axis=0)


def key_table():
    return np.stack([np.roll(KK_MAJOR if j < 12 else KK_MINOR, j % 12) for j in range(24)])


# ------------------------------------------------------------------ features
def features(x, sr, n_fft, hop, n_mels, gamma=1.0, center=True, dtype=torch.float64):
    """(onset [rows, F], chroma [rows, 12, F]) of x [rows, n] in ``dtype`` on the CPU"""
    S = np.abs(SC.stft_cpu(x, n_fft, hop, n_fft, center, dtype))
    real = S.dtype.type
    mel = np.einsum("mk,rkt->rmt", SC.filterbank64(sr, n_fft, n_mels).astype(S.dtype), S)
    Y = np.log1p(real(gamma) * mel)
    onset = np.zeros((S.shape[0], S.shape[2]), dtype=S.dtype)
    onset[:, 1:] = np.maximum(real(0), Y[:, :, 1:] - Y[:, :, :-1]).sum(axis=1) / real(n_mels)
    chroma = np.einsum("pk,rkt->rpt", chroma_matrix(sr, n_fft).astype(S.dtype), S * S)
    return onset, chroma


# ------------------------------------------------------------------ tempo
def lag_range(fps, bpm_min=40.0, bpm_max=240.0):
    return int(math.ceil(60.0 * fps / bpm_max)), int(math.floor(60.0 * fps / bpm_min))


def tempo(onset, fps, F=None, bpm_min=40.0, bpm_max=240.0, prior_bpm=120.0, prior_octaves=1.0):
    """one row.  dict: tempo, strength, lag (None when undecided), acf {lag: r}, terms {lag: sum |u u|}, s {lag: weighted}, gap (the
    relative distance of the best from the second-best weighted value)"""
    F = len(onset) if F is None else int(F)
    o = np.asarray(onset[:F], dtype=np.float64)
    lo, hi = lag_range(fps, bpm_min, bpm_max)
    out = {"tempo": 0.0, "strength": 0.0, "lag": None, "acf": {}, "terms": {}, "s": {}, "gap": None}
    u = o - o.mean() if F > 0 else o
    for l in [0] + list(range(lo - 1, hi + 2)):
        prod = u[:F - l] * u[l:F] if l < F else np.zeros(0)
        out["acf"][l] = float(prod.sum())
        out["terms"][l] = float(np.abs(prod).sum())
    for l in range(lo - 1, hi + 2):
        out["s"][l] = out["acf"][l] * math.exp(-0.5 * ((math.log2(60.0 * fps / l) - math.log2(prior_bpm)) / prior_octaves) ** 2)
    cand = list(range(lo, min(hi, F - 2) + 1))
    if not cand or out["acf"][0] == 0.0:
        return out
    L = cand[0]
    for l in cand:
        if out["s"][l] > out["s"][L]:
            L = l
    a, b, c = out["s"][L - 1], out["s"][L], out["s"][L + 1]
    d = a - 2.0 * b + c
    ls = L + 0.5 * (a - c) / d if d < 0 else float(L)
    rest = sorted((out["s"][l] for l in cand if l != L), reverse=True)
    out.update(tempo=60.0 * fps / ls, strength=out["acf"][L] / out["acf"][0], lag=L,
               gap=None if not rest else (b - rest[0]) / abs(b))
    return out


# ------------------------------------------------------------------ key
def key(chroma, F=None):
    """one row [12, frames].  dict: key, strength, profile [12], terms [12] (sum |c|), corr [24], gap (best - second best)"""
    F = chroma.shape[1] if F is None else int(F)
    c = np.asarray(chroma[:, :F], dtype=np.float64)
    prof = c.sum(axis=1)
    out = {"key": -1, "strength": 0.0, "profile": prof, "terms": np.abs(c).sum(axis=1), "corr": np.zeros(24), "gap": None}
    if prof.max() == prof.min():
        return out
    x = prof - prof.mean()
    for j, k in enumerate(key_table()):
        y = k - k.mean()
        out["corr"][j] = float((x * y).sum() / math.sqrt((x * x).sum() * (y * y).sum()))
    best = int(np.argmax(out["corr"]))
    order = np.sort(out["corr"])[::-1]
    out.update(key=best, strength=float(out["corr"][best]), gap=float(order[0] - order[1]))
    return out


# ------------------------------------------------------------------ signals
def click_track(bpm, seconds=4.0, sr=SR, seed=0):
    """float32 [n]: decaying 1.5 kHz bursts on the beats over noise at 1e-3"""
    n = int(seconds * sr)
    rng = np.random.default_rng([seed, int(bpm)])
    x = 1e-3 * rng.standard_normal(n)
    t = np.arange(int(0.05 * sr)) / sr
    burst = 0.8 * np.sin(2 * np.pi * 1500.0 * t) * np.exp(-t / 0.01)
    beat = 0.0
    while True:
        i = int(round(beat * sr))
        if i >= n:
            break
        m = min(len(burst), n - i)
        x[i:i + m] += burst[:m]
        beat += 60.0 / bpm
    return x.astype(np.float32)


def tone(midi, n, sr=SR):
    f = 440.0 * 2.0 ** ((midi - 69) / 12.0)
    t = np.arange(n) / sr
    env = np.minimum(1.0, np.minimum(np.arange(n), n - 1 - np.arange(n)) / (0.01 * sr))
    return env * sum(a * np.sin(2 * np.pi * f * h * t) for h, a in ((1, 1.0), (2, 0.5), (3, 0.25)))


def passage(name, seconds=4.0, sr=SR):
    """float32 [n]: a scale passage of three-harmonic tones that dwells on the tonic triad -- C major from middle C, or A natural minor from
    A3 -- transposed by the semitones PASSAGES names"""
    _, shift, index = next(p for p in PASSAGES if p[0] == name)
    minor = index >= 12
    scale = [0, 2, 3, 5, 7, 8, 10, 12] if minor else [0, 2, 4, 5, 7, 9, 11, 12]
    root = (57 if minor else 60) + shift
    third = scale[2]
    steps = scale + scale[-2::-1] + [0, third, 7, third, 0, 7, 0, 12, 7, third, 0, 0, 7, 0, third, 0, 0]
    n = int(seconds * sr)
    each = n // len(steps)
    x = np.zeros(n)
    for i, s in enumerate(steps):
        x[i * each:(i + 1) * each] = 0.3 * tone(root + s, each, sr)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def click_features(n_fft=2048, hop=512, n_mels=128):
    """the oracle's onset envelopes float64 [5, F] of the five click tracks"""
    x = np.stack([click_track(b) for b in BPMS])
    return features(x, SR, n_fft, hop, n_mels)[0]


@functools.lru_cache(maxsize=None)
def passage_features(n_fft=2048, hop=512, n_mels=128):
    """the oracle's chromagrams float64 [5, 12, F] of the five passages"""
    x = np.stack([passage(p[0]) for p in PASSAGES])
    return features(x, SR, n_fft, hop, n_mels)[1]
