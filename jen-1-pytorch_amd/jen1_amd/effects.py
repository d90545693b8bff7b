"""Tempo and pitch changes of waveforms on libjen1_hip.so, and the training augmentation that keeps ``tempo`` and ``key`` metadata true.
Not in the reference.

    time_stretch(wav, rate)             rate > 1 plays faster: round(n / rate) samples at the same pitch
    pitch_shift(wav, sr, semitones)     the same length, every frequency times p / q = semitone_ratio(semitones)
    stretch_and_shift(wav, sr, ...)     both at once: one ``spectral.stft``, one ``spectral.phase_vocoder`` pass at rate / (p / q), one
                                        ``spectral.istft``, one ``audio.resample(y, p, q)``; cropped or zero-padded to round(n / rate)

The pitch factor is the rational p / q nearest to 2 ** (semitones / 12) with q <= 128, because the polyphase resampler works on
rational rate pairs and its table grows with them: within 2 cents of equal temperament for every whole step up to an octave, and a
filter table of a few KiB.  This is the textbook phase vocoder: no phase locking, no transient handling, no formant preservation, and
with the reflect padding of ``center=True`` the first frames of a slowed-down clip are quieter than the rest.
There is no autograd and no CPU fallback: off the GPU every function raises ``Jen1HipError``; only "nothing to do" (rate 1 with 0
semitones) returns its input as it is.

``Augment`` draws a (rate, semitones) pair per clip from its own ``random.Random(seed)``; ``dataset.LatentCollate(augment=...)`` applies
the draws in front of the analyser, the level normaliser and the codec, and moves the labels with them (``transform_metadata``).
"""
from __future__ import annotations

import math
import random
from fractions import Fraction
from typing import Sequence, Tuple

import torch

from . import audio_host as H

MAX_DENOMINATOR = 128


def semitone_ratio(semitones: float) -> Fraction:
    """the frequency factor of ``semitones`` as the nearest fraction with a denominator of at most 128"""
    return Fraction(2.0 ** (float(semitones) / 12.0)).limit_denominator(MAX_DENOMINATOR)


def _check(wav: torch.Tensor, rate: float, n_fft: int, what: str) -> None:
    from . import spectral
    spectral.check_wave(wav, what)
    if not (float(rate) > 0.0 and math.isfinite(float(rate))):
        raise ValueError(f"{what}: rate = {rate} must be positive and finite")
    H.check_n_fft(n_fft)


def _fit(y: torch.Tensor, n: int) -> torch.Tensor:
    """the last axis cropped or zero-padded to n samples"""
    have = int(y.shape[-1])
    if have == n:
        return y
    if have > n:
        return y[..., :n].contiguous()
    out = torch.zeros(tuple(y.shape[:-1]) + (n,), dtype=y.dtype, device=y.device)
    out[..., :have] = y
    return out


def stretch_and_shift(wav: torch.Tensor, sr: int, rate: float = 1.0, semitones: float = 0.0, n_fft: int = 2048, hop: int = 512,
                      device="cuda") -> torch.Tensor:
    """``wav`` float32 ``[..., n]`` played ``rate`` times faster and ``semitones`` higher: float32 ``[..., round(n / rate)]`` on
    ``device``.  ``sr`` only names the rate of the input, which is also the rate of the result."""
    from . import audio, spectral
    _check(wav, rate, n_fft, "stretch_and_shift")
    if int(sr) <= 0:
        raise ValueError(f"sample rates must be positive, not {sr}")
    f = semitone_ratio(semitones)
    if float(rate) == 1.0 and f == 1:
        return wav
    dev = H.gpu_device(device, "stretch_and_shift")
    n = int(wav.shape[-1])
    n_out = max(1, int(round(n / float(rate))))
    step = float(rate) * f.denominator / f.numerator            # frames of the input per frame of the output
    spec = spectral.stft(wav, n_fft, hop, device=dev)
    if step != 1.0:
        spec = spectral.phase_vocoder(spec, step, hop, device=dev)
    y = spectral.istft(spec, n_fft, hop, length=max(1, int(round(n / step))), device=dev)
    if f != 1:
        y = audio.resample(y, f.numerator, f.denominator, device=dev)
    return _fit(y, n_out)


def time_stretch(wav: torch.Tensor, rate: float, n_fft: int = 2048, hop: int = 512, device="cuda") -> torch.Tensor:
    """``stretch_and_shift`` without a pitch change: ``round(n / rate)`` samples"""
    return stretch_and_shift(wav, 1, rate=rate, semitones=0.0, n_fft=n_fft, hop=hop, device=device)


def pitch_shift(wav: torch.Tensor, sr: int, semitones: float, n_fft: int = 2048, hop: int = 512, device="cuda") -> torch.Tensor:
    """``stretch_and_shift`` without a tempo change: the same length, ``semitones`` higher"""
    return stretch_and_shift(wav, sr, rate=1.0, semitones=semitones, n_fft=n_fft, hop=hop, device=device)


class Augment:
    """Tempo and pitch augmentation for ``dataset.LatentCollate``: with probability ``p`` a clip gets one of ``tempo_rates`` and one of
    ``semitones`` (whole steps, so that a key stays a key), otherwise (1.0, 0).  ``draw`` uses the instance's own generator, so a seed
    fixes the whole sequence of draws whatever else uses ``random``."""

    def __init__(self, tempo_rates: Sequence[float] = (1.0,), semitones: Sequence[int] = (0,), p: float = 1.0, seed: int = 0):
        self.tempo_rates = tuple(float(r) for r in tempo_rates)
        if not self.tempo_rates or any(not (r > 0.0 and math.isfinite(r)) for r in self.tempo_rates):
            raise ValueError(f"tempo_rates = {tuple(tempo_rates)} must be positive and finite, and not empty")
        if not semitones or any(isinstance(s, bool) or float(s) != int(s) for s in semitones):
            raise ValueError(f"semitones = {tuple(semitones)} must be whole numbers, and not empty: a key moves in semitone steps")
        self.semitones = tuple(int(s) for s in semitones)
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"p = {p} must be in [0, 1]")
        self.p, self.seed = float(p), seed
        self._rng = random.Random(seed)

    def draw(self) -> Tuple[float, int]:
        """(rate, semitones) of the next clip"""
        if self._rng.random() >= self.p:
            return 1.0, 0
        return self._rng.choice(self.tempo_rates), self._rng.choice(self.semitones)

    @staticmethod
    def transform_metadata(md: dict, rate: float, semitones: int) -> dict:
        """a copy of ``md`` with ``tempo`` times ``rate`` and ``key`` (0..11 major, 12..23 minor) moved by ``semitones`` within its mode;
        entries that are absent stay absent"""
        out = dict(md)
        if "tempo" in out and out["tempo"] is not None:
            out["tempo"] = float(out["tempo"]) * float(rate)
        if "key" in out and out["key"] is not None:
            key = int(out["key"])
            out["key"] = (key % 12 + int(semitones)) % 12 + 12 * (key // 12)
        return out
