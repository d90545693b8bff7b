"""Tempo and key of waveforms on libjen1_hip.so (include/jen1_analysis.h; csrc/spectral.hip: jen1_music_features, csrc/analysis.hip:
jen1_tempo, jen1_key): the two global controls the conditioners take ("tempo", "key"), measured from audio.  Not in the reference.

    features    one pass over the waveform: the onset-strength envelope -- Y[b,t] = log1p(gamma * mel[b,t]) on the magnitude spectrum,
                onset[t] = mean_b max(0, Y[b,t] - Y[b,t-1]) -- and the 12-class chromagram chroma[p,t] = sum_k W[p,k] |X[k,t]|^2, both
                formed while the spectrum is in LDS; no spectrogram is written
    tempo       the autocorrelation of the mean-free envelope (float64), weighted by a log-normal prior around ``prior_bpm``; the best lag
                in [bpm_min, bpm_max], refined by a parabola through its neighbours; strength = r[L] / r[0]
    key         the chroma summed over time (float64) against the 24 rotated Krumhansl-Kessler profiles: key j has tonic j % 12 (0 = C)
                and is minor for j >= 12; strength = the winning correlation
    undecided   tempo 0 (silence, or too few frames for any lag) and key -1 (a profile without variance), with strength 0

Everything between the waveform and the four results runs on the HIP kernels, in fixed-order sums: the same bits on every run, wherever
in the batch a row sits.  There is no autograd and no fallback; neither ``torch.stft`` nor any ATen op forms a value.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import audio_host as H
from . import lib as L
from . import spectral

KEY_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B",
             "Cm", "C#m", "Dm", "D#m", "Em", "Fm", "F#m", "Gm", "G#m", "Am", "A#m", "Bm")
KK_MAJOR = (6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88)
KK_MINOR = (6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17)
TEMPO_TOLERANCE = 0.04                      # MIREX accuracy 1
OCTAVE_FACTORS = (1.0, 2.0, 3.0, 0.5, 1.0 / 3.0)
ANALYZE = ("tempo", "key")


# ------------------------------------------------------------------------------------------------------------- host tables
def chroma_filterbank(sr: float, n_fft: int, a440: float = 440.0, centre_octave: float = 5.0, octave_width: float = 2.0) -> np.ndarray:
    """float64 [12, n_fft / 2 + 1], class 0 = C: the usual STFT chroma map.  Bin k >= 1 has the pitch ``pit[k] = 12 log2(f_k / (a440 / 16))``
    in semitones (``pit[0] = pit[1] - 18``) and the width ``max(pit[k+1] - pit[k], 1)`` (the last: 1); class p gets
    ``exp(-0.5 (2 D / width)^2)`` with D the distance of pit[k] from p folded into [-6, 6); every column has unit L2 norm before the octave
    weight ``exp(-0.5 ((pit / 12 - centre_octave) / octave_width)^2)``; the rows are rolled by -3 (the pitch scale starts at A)."""
    H.check_n_fft(n_fft)
    if not float(sr) > 0 or not float(a440) > 0 or not float(octave_width) > 0:
        raise ValueError(f"chroma_filterbank needs positive sr, a440 and octave_width, not {sr}, {a440}, {octave_width}")
    n_fft = int(n_fft)
    bins = n_fft // 2 + 1
    pit = np.empty(bins, dtype=np.float64)
    pit[1:] = 12.0 * np.log2(np.arange(1, bins, dtype=np.float64) * float(sr) / n_fft / (float(a440) / 16.0))
    pit[0] = pit[1] - 18.0
    width = np.ones(bins, dtype=np.float64)
    width[:-1] = np.maximum(pit[1:] - pit[:-1], 1.0)
    D = np.mod(pit[None, :] - np.arange(12, dtype=np.float64)[:, None] + 6.0 + 120.0, 12.0) - 6.0
    W = np.exp(-0.5 * (2.0 * D / width[None, :]) ** 2)
    W /= np.sqrt((W * W).sum(axis=0, keepdims=True))
    W *= np.exp(-0.5 * ((pit / 12.0 - float(centre_octave)) / float(octave_width)) ** 2)[None, :]
    return np.roll(W, -3, axis=0)


def key_profiles() -> np.ndarray:
    """float64 [24, 12]: the Krumhansl-Kessler profile of key j -- major for j < 12, minor above -- rotated to the tonic j % 12"""
    return np.stack([np.roll(np.asarray(KK_MAJOR if j < 12 else KK_MINOR, dtype=np.float64), j % 12) for j in range(24)])


def frame_lengths(lengths, n: int, n_fft: int, hop: int, center: bool = True) -> np.ndarray:
    """int32 [B]: the frames of ``spectral.frame_count`` for clips of ``lengths`` samples inside a row of n (0 for a clip too short to frame)"""
    total = spectral.frame_count(n, n_fft, hop, center)
    out = []
    for v in np.asarray(lengths, dtype=np.int64).reshape(-1):
        v = max(0, min(int(v), int(n)))
        f = (1 + v // hop) if center else (1 + (v - n_fft) // hop if v >= n_fft else 0)
        out.append(max(0, min(f if v > 0 else 0, total)))
    return np.asarray(out, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------- device side
def _chroma_w(sr, n_fft: int, dev: torch.device) -> torch.Tensor:
    return H.device_table(dev, ("chroma", float(sr), int(n_fft)), lambda: torch.from_numpy(chroma_filterbank(sr, n_fft).astype(np.float32)).to(dev))


def _mono(wav: torch.Tensor, sr: int, dev: torch.device, what: str) -> torch.Tensor:
    """[B, C, n] or [B, n] -> float32 [B, n] on dev; two channels are averaged by ``audio.convert_audio``"""
    spectral.check_wave(wav, what)
    if wav.dim() not in (2, 3):
        raise ValueError(f"{what} takes [B, C, n] or [B, n], not {tuple(wav.shape)}")
    x = wav.to(dev)
    if x.dim() == 3:
        if int(x.shape[1]) != 1:
            from . import audio
            x = audio.convert_audio(x, sr, sr, 1, device=dev)
        x = x[:, 0]
    return x


def _frames_arg(frames, rows: int, stride: int, dev: torch.device) -> torch.Tensor:
    if frames is None:
        return torch.from_numpy(np.full((rows,), stride, dtype=np.int32)).to(dev)
    if torch.is_tensor(frames):
        if frames.dtype != torch.int32 or tuple(frames.shape) != (rows,):
            raise ValueError(f"frames must be int32 [{rows}], not {frames.dtype} {tuple(frames.shape)}")
        return frames.to(dev).contiguous()
    f = np.asarray(frames, dtype=np.int64).reshape(-1)
    if f.size != rows or (f < 0).any() or (f > stride).any():
        raise ValueError(f"frames must be {rows} counts in [0, {stride}], not {f.tolist()}")
    return torch.from_numpy(f.astype(np.int32)).to(dev)


def music_features(wav: torch.Tensor, sr: int, n_fft: int = 2048, hop: int = 512, n_mels: int = 128, gamma: float = 1.0,
                   device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """(onset float32 [B, F], chroma float32 [B, 12, F]) of ``wav`` ([B, C, n] or [B, n] at rate ``sr``) on ``device``: periodic Hann window
    of n_fft, center=True framing, the mel matrix of ``spectral.mel_filterbank(sr, n_fft, n_mels)`` in banded form and
    ``chroma_filterbank(sr, n_fft)``; one launch"""
    if not float(gamma) > 0.0:
        raise ValueError(f"gamma = {gamma} must be positive")
    spectral.check_wave(wav, "music_features")
    dev = H.gpu_device(device, "music_features")
    x = _mono(wav, sr, dev, "music_features")
    fr = H.framing(n_fft, hop, None, "hann", True, n=int(x.shape[-1]))
    most = int(L.load().jen1_music_features_max_bands(fr.n_fft))
    if int(n_mels) > most:
        raise ValueError(f"n_mels = {n_mels}: at most {most} bands fit next to a transform of {fr.n_fft}")
    x, rows, n, stride = H.rows_of(x, dev)
    bands = spectral.mel_bands(sr, fr.n_fft, n_mels, 0.0, None, "htk", None, dev)
    onset = torch.empty((rows, fr.frames), dtype=torch.float32, device=dev)
    chroma = torch.empty((rows, 12, fr.frames), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_music_features", x.data_ptr(), stride, onset.data_ptr(), chroma.data_ptr(), *H.frame_tables(fr, "hann", dev), *bands.abi(),
             _chroma_w(sr, fr.n_fft, dev).data_ptr(), float(gamma), *fr.abi(rows, n))
    return onset, chroma


def tempo(onset: torch.Tensor, fps: float, frames=None, bpm_min: float = 40.0, bpm_max: float = 240.0, prior_bpm: float = 120.0,
          prior_octaves: float = 1.0, return_acf: bool = False):
    """(tempo float32 [B] in BPM, strength float32 [B]) of onset envelopes float32 [B, F] on a GPU, ``fps`` frames per second; ``frames``:
    the valid frames per row (int32 tensor or a sequence; None: all).  ``return_acf``: also the autocorrelation float64 [B, lags] and
    the lag of its first column."""
    if not torch.is_tensor(onset) or onset.dtype != torch.float32 or onset.dim() != 2 or int(onset.shape[1]) < 1:
        raise ValueError(f"tempo takes a float32 [B, F] envelope, not {getattr(onset, 'dtype', type(onset))} {tuple(getattr(onset, 'shape', ()))}")
    dev = H.gpu_device(onset.device, "tempo")
    lib = L.load()
    lags = int(lib.jen1_tempo_lags(float(fps), float(bpm_min), float(bpm_max)))
    if lags < 1 or not float(prior_bpm) > 0 or not float(prior_octaves) > 0:
        raise ValueError(f"tempo: no lags for fps {fps}, bpm range [{bpm_min}, {bpm_max}], prior {prior_bpm} bpm over {prior_octaves} octaves")
    o = onset if onset.stride(1) == 1 and (onset.stride(0) >= onset.shape[1] or onset.shape[0] == 1) else onset.contiguous()
    rows, stride = int(o.shape[0]), int(o.stride(0)) if o.shape[0] > 1 else int(o.shape[1])
    fr = _frames_arg(frames, rows, int(o.shape[1]), dev)
    out = torch.empty((2, rows), dtype=torch.float32, device=dev)
    acf = torch.empty((rows, lags), dtype=torch.float64, device=dev) if return_acf else None
    nbytes = int(lib.jen1_tempo_workspace_bytes(rows, float(fps), float(bpm_min), float(bpm_max)))
    work = H.workspace(nbytes, dev)
    H.launch(dev, "jen1_tempo", o.data_ptr(), stride, fr.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), None if acf is None else acf.data_ptr(),
             rows, float(fps), float(bpm_min), float(bpm_max), float(prior_bpm), float(prior_octaves), work.data_ptr(), nbytes)
    if return_acf:
        return out[0], out[1], acf, int(np.ceil(60.0 * float(fps) / float(bpm_max))) - 1
    return out[0], out[1]


def key(chroma: torch.Tensor, frames=None, return_profile: bool = False):
    """(key int32 [B], strength float32 [B]) of chromagrams float32 [B, 12, F] on a GPU; ``return_profile``: also the time sums float64
    [B, 12] and the 24 correlations float32 [B, 24]"""
    if not torch.is_tensor(chroma) or chroma.dtype != torch.float32 or chroma.dim() != 3 or int(chroma.shape[1]) != 12 or int(chroma.shape[2]) < 1:
        raise ValueError(f"key takes a float32 [B, 12, F] chromagram, not {getattr(chroma, 'dtype', type(chroma))} {tuple(getattr(chroma, 'shape', ()))}")
    dev = H.gpu_device(chroma.device, "key")
    c = chroma.contiguous()
    rows, stride = int(c.shape[0]), int(c.shape[2])
    fr = _frames_arg(frames, rows, stride, dev)
    k = torch.empty((rows,), dtype=torch.int32, device=dev)
    st = torch.empty((rows,), dtype=torch.float32, device=dev)
    prof = torch.empty((rows, 12), dtype=torch.float64, device=dev)
    corr = torch.empty((rows, 24), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_key", c.data_ptr(), stride, fr.data_ptr(), k.data_ptr(), st.data_ptr(), prof.data_ptr(), corr.data_ptr(), rows)
    return (k, st, prof, corr) if return_profile else (k, st)


def analyze(wav: torch.Tensor, sr: int, lengths=None, n_fft: int = 2048, hop: int = 512, n_mels: int = 128, gamma: float = 1.0,
            bpm_min: float = 40.0, bpm_max: float = 240.0, prior_bpm: float = 120.0, prior_octaves: float = 1.0, device="cuda") -> dict:
    """``{"tempo", "tempo_strength", "key", "key_strength"}`` of ``wav`` ([B, C, n] or [B, n] at rate ``sr``): device tensors [B], four
    launches and no host synchronisation.  ``lengths``: the valid samples of every row (a sequence), mapped to frames as
    ``spectral.frame_count`` maps n, so that the zero padding of short clips stays out of both estimates."""
    onset, chroma = music_features(wav, sr, n_fft, hop, n_mels, gamma, device)
    frames = None
    if lengths is not None:
        n = int(wav.shape[-1])
        frames = torch.from_numpy(frame_lengths(lengths, n, n_fft, hop)).to(onset.device)
        if int(frames.numel()) != int(onset.shape[0]):
            raise ValueError(f"lengths must have one entry per row ({onset.shape[0]}), not {int(frames.numel())}")
    t, ts = tempo(onset, float(sr) / float(hop), frames, bpm_min, bpm_max, prior_bpm, prior_octaves)
    k, ks = key(chroma, frames)
    return {"tempo": t, "tempo_strength": ts, "key": k, "key_strength": ks}


# ------------------------------------------------------------------------------------------------------------- the control report
def tempo_verdict(measured: float, target: float) -> dict:
    """``tempo_ratio`` and the two MIREX verdicts of one measured tempo against its target"""
    if not float(target) > 0:
        raise ValueError(f"a tempo target must be positive, not {target}")
    ratio = float(measured) / float(target)
    near = lambda f: float(measured) > 0 and abs(ratio / f - 1.0) <= TEMPO_TOLERANCE
    return {"tempo_ratio": ratio, "tempo_match": bool(near(1.0)), "tempo_match_octave": bool(any(near(f) for f in OCTAVE_FACTORS))}


def key_verdict(measured: int, target: int) -> dict:
    """``key_match`` (exact) and ``key_related`` (exact, the relative major / minor, or a fifth apart in the same mode)"""
    measured, target = int(measured), int(target)
    if not 0 <= target < 24:
        raise ValueError(f"a key target is in [0, 24), not {target}")
    if not 0 <= measured < 24:
        return {"key_match": False, "key_related": False}
    relative = (target + 9) % 12 + 12 if target < 12 else (target - 12 + 3) % 12
    fifths = {(target % 12 + s) % 12 + 12 * (target // 12) for s in (7, 5)}
    return {"key_match": measured == target, "key_related": measured == target or measured == relative or measured in fifths}


def control_report(wav: torch.Tensor, sr: int, tempo=None, key=None, device="cuda", analyzer=None) -> dict:
    """How ``wav`` ([B, C, n] or [B, n] at rate ``sr``, as ``analyze`` takes it) follows its controls: the measured
    ``tempo``, ``tempo_strength``, ``key``, ``key_strength`` (lists, one entry per row) and ``key_name``; with a target ``tempo`` (BPM) also
    ``tempo_ratio``, ``tempo_match`` (within 4 %) and ``tempo_match_octave`` (within 4 % of the target times 1, 2, 3, 1/2 or 1/3); with a
    target ``key`` (0 .. 23) also ``key_match`` and ``key_related``.  A target is one value or one per row.  ``analyzer``: a stand-in for
    ``analyze`` (tests)."""
    res = (analyze if analyzer is None else analyzer)(wav, sr, device=device)
    got = {k: [v.item() for v in torch.as_tensor(res[k]).reshape(-1).cpu()] for k in ("tempo", "tempo_strength", "key", "key_strength")}
    rows = len(got["tempo"])
    out = dict(got)
    out["key"] = [int(k) for k in got["key"]]
    out["key_name"] = [KEY_NAMES[k] if 0 <= k < 24 else None for k in out["key"]]

    def per_row(target, what):
        t = list(target) if isinstance(target, (list, tuple)) else [target] * rows
        if len(t) != rows:
            raise ValueError(f"{what}: {len(t)} targets for {rows} rows")
        return t
    if tempo is not None:
        verdicts = [tempo_verdict(m, t) for m, t in zip(got["tempo"], per_row(tempo, "tempo"))]
        for name in ("tempo_ratio", "tempo_match", "tempo_match_octave"):
            out[name] = [v[name] for v in verdicts]
    if key is not None:
        verdicts = [key_verdict(m, t) for m, t in zip(out["key"], per_row(key, "key"))]
        for name in ("key_match", "key_related"):
            out[name] = [v[name] for v in verdicts]
    return out
