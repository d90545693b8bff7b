"""Spectral metrics of waveforms on libjen1_hip.so (csrc/spectral.hip, include/jen1_spectral.h): the short-time Fourier transform in the
framing and layout of ``torch.stft``, log-mel spectrograms, and the two objective distances that sit on them -- the multi-resolution
STFT distance (spectral convergence + log-magnitude L1, as in Parallel WaveGAN) and the log-mel L1.  Not in the reference, which has no
evaluation of its output at all.

    frames      center=True: reflect padding of n_fft / 2 on either side, 1 + n // hop frames; center=False: 1 + (n - n_fft) // hop
    window      "hann" (periodic, ``torch.hann_window(win_length)``) or a 1-D tensor of win_length values; shorter than n_fft it is centred
                in the frame with (n_fft - win_length) // 2 zeros on its left
    stft        complex64 [..., n_fft / 2 + 1, frames], not normalised, one-sided
    istft       ``torch.istft`` of that layout: the windowed inverse frames overlap-added in a fixed order and divided by the summed
                squared window (refused where that sum vanishes: NOLA); float32 [..., length]
    vocoder     ``phase_vocoder`` resamples the frame axis by ``rate`` (the textbook phase vocoder, as ``torchaudio.functional.phase_vocoder``):
                magnitudes interpolated, phase advances accumulated exactly; complex64 [..., n_fft / 2 + 1, len(arange(0, frames, rate))]
    mel         ``mel_filterbank`` restates ``torchaudio.functional.melscale_fbanks`` (htk / slaney scale, optional slaney norm) in float64;
                the kernel gets it as a banded matrix (per band a bin range and its weights) and knows nothing of mel
    distances   sc = sqrt(sum (|X| - |Y|)^2 / sum |Y|^2),  log_mag = mean |log max(|X|, floor) - log max(|Y|, floor)|  over bins and frames,
                X of the test signal and Y of the reference; three float64 sums per row leave the GPU, in a fixed order (the same bits on
                every run, wherever in the batch a row sits)

Inputs are float32 ``[n]``, ``[C, n]`` or ``[B, C, n]`` (any leading axes); CPU tensors are moved to ``device`` and results stay there.
These are metrics, not losses: there is no autograd, and an input that requires grad is refused.  There is no fallback: everything
runs on the HIP kernels.  Neither torchaudio nor ``torch.stft`` is used.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import audio_host as H
from . import lib as L
from .audio_host import N_FFTS, frame_count, hann_window, twiddle_table     # the framing primitives: public names of this module too

RESOLUTIONS_48K = ((1024, 100, 480), (2048, 240, 1200), (4096, 480, 2400))        # (n_fft, hop, win_length): Parallel WaveGAN's set, doubled
LOGS = (None, "log", "db")


# ------------------------------------------------------------------------------------------------------------- host tables
def hz_to_mel(f, mel_scale: str = "htk"):
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    if mel_scale != "slaney":
        raise ValueError(f"unknown mel_scale {mel_scale!r}: 'htk' or 'slaney'")
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    logstep = math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m, mel_scale: str = "htk"):
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if mel_scale != "slaney":
        raise ValueError(f"unknown mel_scale {mel_scale!r}: 'htk' or 'slaney'")
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_points(sr: int, n_mels: int, f_min: float = 0.0, f_max: Optional[float] = None, mel_scale: str = "htk") -> np.ndarray:
    """the n_mels + 2 corner frequencies in Hz, equally spaced on the mel scale between f_min and f_max (sr / 2 by default)"""
    f_max = float(sr) / 2.0 if f_max is None else float(f_max)
    if int(n_mels) < 1 or not 0.0 <= float(f_min) < f_max:
        raise ValueError(f"mel bands need n_mels >= 1 and 0 <= f_min < f_max, not n_mels {n_mels}, f_min {f_min}, f_max {f_max}")
    return mel_to_hz(np.linspace(hz_to_mel(f_min, mel_scale), hz_to_mel(f_max, mel_scale), int(n_mels) + 2), mel_scale)


def mel_filterbank(sr: int, n_fft: int, n_mels: int, f_min: float = 0.0, f_max: Optional[float] = None, mel_scale: str = "htk",
                   norm: Optional[str] = None) -> np.ndarray:
    """float64 [n_mels, n_fft / 2 + 1]: the triangles of ``torchaudio.functional.melscale_fbanks`` (transposed: one row per band) on the
    bin frequencies ``linspace(0, sr / 2, n_fft / 2 + 1)``; ``norm="slaney"`` scales band m by 2 / (f_{m+2} - f_m)"""
    if norm not in (None, "slaney"):
        raise ValueError(f"unknown norm {norm!r}: None or 'slaney'")
    n_freq = int(n_fft) // 2 + 1
    freqs = np.linspace(0.0, float(sr) / 2.0, n_freq)
    f = mel_points(sr, n_mels, f_min, f_max, mel_scale)
    up = (freqs[None, :] - f[:-2, None]) / (f[1:-1] - f[:-2])[:, None]
    down = (f[2:, None] - freqs[None, :]) / (f[2:] - f[1:-1])[:, None]
    fb = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        fb = fb * (2.0 / (f[2:] - f[:-2]))[:, None]
    return fb


def banded(matrix: np.ndarray):
    """a dense [bands, bins] matrix as (lo int32 [bands], hi int32 [bands], off int32 [bands], weights [sum (hi - lo)]): row b is
    ``weights[off[b] : off[b] + hi[b] - lo[b]]`` on the bins [lo[b], hi[b]) and zero elsewhere; an all-zero row has lo = hi = 0.  The
    weights keep the matrix's dtype, so the form is exact."""
    m = np.asarray(matrix)
    if m.ndim != 2:
        raise ValueError(f"a filterbank is a [bands, bins] matrix, not {m.shape}")
    nz = m != 0
    some = nz.any(axis=1)
    lo = np.where(some, np.argmax(nz, axis=1), 0).astype(np.int32)
    hi = np.where(some, m.shape[1] - np.argmax(nz[:, ::-1], axis=1), 0).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(hi - lo)[:-1]]).astype(np.int32)
    parts = [m[b, lo[b]:hi[b]] for b in range(m.shape[0])]
    weights = np.concatenate(parts) if parts and int((hi - lo).sum()) else np.zeros((0,), dtype=m.dtype)
    return lo, hi, off, weights


def unbanded(lo, hi, off, weights, bins: int) -> np.ndarray:
    """the dense matrix of a banded form"""
    out = np.zeros((len(lo), int(bins)), dtype=np.asarray(weights).dtype)
    for b in range(len(lo)):
        out[b, lo[b]:hi[b]] = weights[off[b]:off[b] + hi[b] - lo[b]]
    return out


# ------------------------------------------------------------------------------------------------------------- arguments
def check_wave(wav: torch.Tensor, what: str) -> None:
    if not torch.is_tensor(wav) or wav.dtype != torch.float32:
        raise TypeError(f"{what}: waveforms are float32 tensors, not {getattr(wav, 'dtype', type(wav))}")
    if wav.requires_grad:
        raise ValueError(f"{what}: a metric, not a loss -- there is no autograd; detach the input")
    if wav.dim() < 1 or int(wav.shape[-1]) < 1:
        raise ValueError(f"{what}: audio needs a time axis that is not empty, not shape {tuple(wav.shape)}")


def mel_bands(sr, n_fft, n_mels, f_min, f_max, mel_scale, norm, dev: torch.device) -> H.Bands:
    """the mel filterbank on ``dev`` in banded form"""
    def make():
        lo, hi, off, w = banded(mel_filterbank(sr, n_fft, n_mels, f_min, f_max, mel_scale, norm))
        if w.size == 0:
            raise ValueError(f"the mel filterbank (sr {sr}, n_fft {n_fft}, n_mels {n_mels}, f_min {f_min}, f_max {f_max}) has no bin in any band")
        return H.Bands.on(dev, lo, hi, off, w)
    return H.device_table(dev, ("mel", int(sr), int(n_fft), int(n_mels), float(f_min), None if f_max is None else float(f_max), mel_scale, norm), make)


def _kind(power: float) -> int:
    if float(power) == 2.0:
        return L.SPEC_POWER
    if float(power) == 1.0:
        return L.SPEC_MAGNITUDE
    raise ValueError(f"power = {power} must be 2.0 (power) or 1.0 (magnitude)")


# ------------------------------------------------------------------------------------------------------------- transforms
def _stft(wav, n_fft, hop, win_length, window, center, kind, device, what):
    check_wave(wav, what)
    fr = H.framing(n_fft, hop, win_length, window, center, n=int(wav.shape[-1]))
    dev = H.gpu_device(device, what)
    x, rows, n, stride = H.rows_of(wav, dev)
    shape = tuple(wav.shape[:-1]) + (fr.n_fft // 2 + 1, fr.frames)
    out = torch.empty(shape + ((2,) if kind == L.SPEC_COMPLEX else ()), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_stft", x.data_ptr(), stride, out.data_ptr(), *H.frame_tables(fr, window, dev), *fr.abi(rows, n), kind)
    return torch.view_as_complex(out) if kind == L.SPEC_COMPLEX else out


def stft(wav: torch.Tensor, n_fft: int, hop: Optional[int] = None, win_length: Optional[int] = None, window="hann", center: bool = True,
         device="cuda") -> torch.Tensor:
    """``torch.stft(wav, n_fft, hop, win_length, window, center=center, pad_mode="reflect", return_complex=True)``: complex64
    ``[..., n_fft / 2 + 1, frames]`` on ``device``.  ``hop`` defaults to n_fft / 4 and ``win_length`` to n_fft, as there."""
    return _stft(wav, n_fft, hop, win_length, window, center, L.SPEC_COMPLEX, device, "stft")


def spectrogram(wav: torch.Tensor, n_fft: int, hop: Optional[int] = None, win_length: Optional[int] = None, power: float = 2.0, window="hann",
                center: bool = True, device="cuda") -> torch.Tensor:
    """``|stft|^2`` (power=2.0) or ``|stft|`` (power=1.0): float32 ``[..., n_fft / 2 + 1, frames]``, formed in the transform's launch"""
    return _stft(wav, n_fft, hop, win_length, window, center, _kind(power), device, "spectrogram")


def mel_spectrogram(wav: torch.Tensor, sr: int, n_fft: int = 2048, hop: int = 512, win_length: Optional[int] = None, n_mels: int = 128,
                    f_min: float = 0.0, f_max: Optional[float] = None, power: float = 2.0, mel_scale: str = "htk", norm: Optional[str] = None,
                    log: Optional[str] = None, floor: float = 1e-10, window="hann", center: bool = True, device="cuda") -> torch.Tensor:
    """``mel_filterbank(...) @ spectrogram(wav, ..., power)``: float32 ``[..., n_mels, frames]``, the filterbank applied while the spectrum
    is in LDS.  ``log``: None, ``"log"`` = log(max(v, floor)) or ``"db"`` = 10 log10(max(v, floor))."""
    if log not in LOGS:
        raise ValueError(f"unknown log {log!r}: one of {LOGS}")
    if log is not None and not float(floor) > 0.0:
        raise ValueError(f"floor = {floor} must be positive under a logarithm")
    check_wave(wav, "mel_spectrogram")
    kind = _kind(power)
    fr = H.framing(n_fft, hop, win_length, window, center, n=int(wav.shape[-1]))
    dev = H.gpu_device(device, "mel_spectrogram")
    x, rows, n, stride = H.rows_of(wav, dev)
    bands = mel_bands(sr, fr.n_fft, n_mels, f_min, f_max, mel_scale, norm, dev)
    out = torch.empty(tuple(wav.shape[:-1]) + (int(n_mels), fr.frames), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_mel", x.data_ptr(), stride, out.data_ptr(), *H.frame_tables(fr, window, dev), *bands.abi(), *fr.abi(rows, n), kind,
             LOGS.index(log), float(floor))
    return out


def _check_spec(spec: torch.Tensor, what: str) -> int:
    """n_fft of a complex64 spectrogram [..., n_fft / 2 + 1, frames]"""
    if not torch.is_tensor(spec) or spec.dtype != torch.complex64:
        raise TypeError(f"{what}: spectrograms are complex64 tensors, not {getattr(spec, 'dtype', type(spec))}")
    if spec.requires_grad:
        raise ValueError(f"{what}: there is no autograd; detach the input")
    if spec.dim() < 2 or int(spec.shape[-1]) < 1:
        raise ValueError(f"{what}: a spectrogram needs a bin axis and a frame axis that is not empty, not shape {tuple(spec.shape)}")
    n_fft = 2 * (int(spec.shape[-2]) - 1)
    if n_fft not in N_FFTS:
        raise ValueError(f"{what}: {int(spec.shape[-2])} bins are not n_fft / 2 + 1 of an n_fft in {N_FFTS}")
    return n_fft


def vocoder_frame_count(frames: int, rate: float) -> int:
    """frames of ``phase_vocoder`` for ``frames`` input frames: ``len(numpy.arange(0, frames, rate))``, by the library's own rule"""
    if not (float(rate) > 0.0 and math.isfinite(float(rate))):
        raise ValueError(f"rate = {rate} must be positive and finite")
    count = int(L.load().jen1_vocoder_frames(int(frames), float(rate)))
    if count < 1:
        raise ValueError(f"rate = {rate} gives no usable frame count from {frames} frames")
    return count


def istft(spec: torch.Tensor, n_fft: int, hop: Optional[int] = None, win_length: Optional[int] = None, window="hann", center: bool = True,
          length: Optional[int] = None, device="cuda") -> torch.Tensor:
    """``torch.istft(spec, n_fft, hop, win_length, window, center=center, length=length)`` of a one-sided complex64 ``[..., n_fft / 2 + 1,
    frames]``: float32 ``[..., length]`` on ``device``.  ``length`` defaults to ``hop * (frames - 1)`` (plus n_fft with center=False);
    a longer one is filled with zeros past the last frame.  A window whose squared overlap-add vanishes somewhere (NOLA) is refused."""
    got = _check_spec(spec, "istft")
    H.check_n_fft(n_fft)
    if got != int(n_fft):
        raise ValueError(f"istft: the input has {int(spec.shape[-2])} bins, n_fft = {n_fft} needs {int(n_fft) // 2 + 1}")
    fr = H.framing(n_fft, hop, win_length, window, center, frames=int(spec.shape[-1]))
    host = window.detach().to("cpu", torch.float32).contiguous().numpy() if torch.is_tensor(window) else hann_window(fr.win_length)
    length = fr.hop * (fr.frames - 1) + (0 if center else fr.n_fft) if length is None else int(length)
    if length < 1:
        raise ValueError(f"istft: length = {length} must be positive ({fr.frames} frames at hop {fr.hop})")
    dev = H.gpu_device(device, "istft")
    lead = tuple(spec.shape[:-2])
    x = torch.view_as_real(spec.to(dev).contiguous())
    out = torch.empty(lead + (length,), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_istft", x.data_ptr(), out.data_ptr(), length, H.window_on(window, fr.win_length, dev).data_ptr(), host.ctypes.data,
             H.twiddle_on(fr.n_fft, dev).data_ptr(), math.prod(lead), fr.frames, length, fr.n_fft, fr.hop, fr.win_length, int(fr.center))
    return out


def phase_vocoder(spec: torch.Tensor, rate: float, hop: int, device="cuda") -> torch.Tensor:
    """``torchaudio.functional.phase_vocoder(spec, rate, 2 pi hop k / n_fft)``: the frame axis of a complex64 ``[..., n_fft / 2 + 1,
    frames]`` resampled at steps of ``rate`` frames (rate > 1: fewer frames, faster), complex64 ``[..., n_fft / 2 + 1, J]`` on ``device``.
    ``hop`` is the hop the spectrogram was taken with."""
    n_fft = _check_spec(spec, "phase_vocoder")
    H.check_hop(hop, n_fft)
    frames = int(spec.shape[-1])
    if not (float(rate) > 0.0 and math.isfinite(float(rate))):
        raise ValueError(f"rate = {rate} must be positive and finite")
    dev = H.gpu_device(device, "phase_vocoder")
    count = vocoder_frame_count(frames, rate)
    x = torch.view_as_real(spec.to(dev).contiguous())
    out = torch.empty(tuple(spec.shape[:-1]) + (count, 2), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_phase_vocoder", x.data_ptr(), out.data_ptr(), math.prod(spec.shape[:-2]), frames, n_fft, int(hop), float(rate))
    return torch.view_as_complex(out)


# ------------------------------------------------------------------------------------------------------------- distances
def _pair(test: torch.Tensor, reference: torch.Tensor, what: str) -> None:
    check_wave(test, what)
    check_wave(reference, what)
    if tuple(test.shape) != tuple(reference.shape):
        raise ValueError(f"{what}: test {tuple(test.shape)} and reference {tuple(reference.shape)} must have the same shape")


def _distance_sums(test, reference, n_fft, hop, win_length, window, center, bands, kind, floor, dev):
    """float64 [..., 3] on ``dev``: the three sums of ``jen1_spectral_distance`` per row, and the frame count"""
    fr = H.framing(n_fft, hop, win_length, window, center, n=int(test.shape[-1]))
    if not float(floor) > 0.0:
        raise ValueError(f"floor = {floor} must be positive")
    x, rows, n, xs = H.rows_of(test, dev)
    y, _, _, ys = H.rows_of(reference, dev)
    nbytes = int(L.load().jen1_spectral_distance_workspace_bytes(rows, n, fr.n_fft, fr.hop, int(fr.center)))
    work = H.workspace(nbytes, dev)
    out = torch.empty(tuple(test.shape[:-1]) + (3,), dtype=torch.float64, device=dev)
    H.launch(dev, "jen1_spectral_distance", x.data_ptr(), xs, y.data_ptr(), ys, out.data_ptr(), *H.frame_tables(fr, window, dev), *bands.abi(),
             *fr.abi(rows, n), kind, float(floor), work.data_ptr(), nbytes)
    return out, fr.frames


def _bc(t: torch.Tensor) -> torch.Tensor:
    """[n] -> [1, 1, n], [C, n] -> [1, C, n]; [B, C, n] as it is"""
    if t.dim() > 3:
        raise ValueError(f"distances take [n], [C, n] or [B, C, n], not {tuple(t.shape)}")
    return t.reshape((1,) * (3 - t.dim()) + tuple(t.shape))


def mrstft_distance(test: torch.Tensor, reference: torch.Tensor, resolutions: Sequence[Tuple[int, int, int]] = RESOLUTIONS_48K,
                    floor: float = 1e-5, window="hann", center: bool = True, device="cuda") -> Dict[str, torch.Tensor]:
    """The multi-resolution STFT distance of ``test`` from ``reference`` (``[n]``, ``[C, n]`` or ``[B, C, n]``, same shape): ``{"sc", "log_mag"}``
    float64 ``[B, C, n_res]`` and ``"total"`` ``[B]``, the mean over channels and resolutions of sc + log_mag.  One launch pair per
    resolution ``(n_fft, hop, win_length)``; a silent reference gives sc = inf or nan, as the definition does."""
    _pair(test, reference, "mrstft_distance")
    if len(resolutions) < 1:
        raise ValueError("mrstft_distance needs at least one resolution")
    if not float(floor) > 0.0:
        raise ValueError(f"floor = {floor} must be positive")
    for n_fft, hop, win_length in resolutions:                  # every refusal before anything runs
        H.framing(n_fft, hop, win_length, window, center, n=int(test.shape[-1]))
    dev = H.gpu_device(device, "mrstft_distance")
    t, r = _bc(test), _bc(reference)
    sc, lm = [], []
    for n_fft, hop, win_length in resolutions:
        sums, frames = _distance_sums(t, r, n_fft, hop, win_length, window, center, H.NO_BANDS, L.SPEC_MAGNITUDE, floor, dev)
        sc.append(torch.sqrt(sums[..., 0] / sums[..., 1]))
        lm.append(sums[..., 2] / float((int(n_fft) // 2 + 1) * frames))
    sc, lm = torch.stack(sc, dim=-1), torch.stack(lm, dim=-1)
    return {"sc": sc, "log_mag": lm, "total": (sc + lm).mean(dim=(1, 2))}


def mel_distance(test: torch.Tensor, reference: torch.Tensor, sr: int, n_fft: int = 2048, hop: int = 512, win_length: Optional[int] = None,
                 n_mels: int = 128, f_min: float = 0.0, f_max: Optional[float] = None, power: float = 2.0, mel_scale: str = "htk",
                 norm: Optional[str] = None, floor: float = 1e-10, window="hann", center: bool = True, device="cuda") -> torch.Tensor:
    """mean over bands and frames of ``|log max(mel(test), floor) - log max(mel(reference), floor)|`` (natural log): float64 ``[B, C]``.
    The mel values never leave the workgroup that forms them."""
    _pair(test, reference, "mel_distance")
    kind = _kind(power)
    if not float(floor) > 0.0:
        raise ValueError(f"floor = {floor} must be positive")
    H.framing(n_fft, hop, win_length, window, center, n=int(test.shape[-1]))
    dev = H.gpu_device(device, "mel_distance")
    bands = mel_bands(sr, n_fft, n_mels, f_min, f_max, mel_scale, norm, dev)
    sums, frames = _distance_sums(_bc(test), _bc(reference), n_fft, hop, win_length, window, center, bands, kind, floor, dev)
    return sums[..., 2] / float(int(n_mels) * frames)


def audio_report(test: torch.Tensor, reference: torch.Tensor, sr: int, device="cuda") -> dict:
    """how far ``test`` is from ``reference`` (``[B, C, n]`` or ``[C, n]``, C in {1, 2}, at rate ``sr``), everything on ``device``:
    ``mrstft_total [B]``, ``sc`` / ``log_mag [B, C, n_res]`` (``mrstft_distance`` at RESOLUTIONS_48K), ``log_mel_l1 [B, C]`` (``mel_distance``
    with its defaults) and ``lufs_test`` / ``lufs_reference [B]`` (``audio.loudness``)"""
    from . import audio
    _pair(test, reference, "audio_report")
    dev = H.gpu_device(device, "audio_report")
    t, r = _bc(test).to(dev), _bc(reference).to(dev)
    d = mrstft_distance(t, r, device=dev)
    return {"mrstft_total": d["total"], "sc": d["sc"], "log_mag": d["log_mag"], "log_mel_l1": mel_distance(t, r, sr, device=dev),
            "lufs_test": audio.loudness(t, sr, device=dev), "lufs_reference": audio.loudness(r, sr, device=dev)}
