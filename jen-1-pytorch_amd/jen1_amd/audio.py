"""Sample-rate and channel conversion of waveforms on libjen1_hip.so (csrc/audio.hip: ``jen1_resample``).

What the reference gets from ``encodec.utils.convert_audio(wav, sr, target_sr, target_channels)`` in front of the Encodec encoder
(generation.py:95, dataset/dataloader.py:106): the channel rule (-> 1: mean over the channels; -> 2: mono duplicated, stereo kept;
anything else is an error), then ``torchaudio.transforms.Resample(sr, target_sr)``, i.e. ``torchaudio.functional.resample`` with its
defaults (Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99), restated here from its formulas:

    g = gcd(sr, target_sr);  o = sr // g;  n = target_sr // g
    base = min(o, n) * 0.99;  w = ceil(6 * o / base);  K = 2 * w + o
    t[p][k] = ((k - w) / o - p / n) * base, clamped to [-6, 6]                       p in [0, n), k in [0, K)
    h[p][k] = sinc(t) * cos(pi t / 12)**2 * (base / o)                               float64, rounded to float32 once
    xp[i] = x[i - w], zero outside [0, L);  y[j n + p] = sum_k h[p][k] * xp[j o + k];  len(y) = ceil(n L / o)

``h[p]`` is exactly zero outside a short run of taps (the clamp parks the rest on the window's zero), so the kernel gets the compact
form: ``taps [n, W]`` and ``first [n]`` with ``h[p][first[p] + t] = taps[p][t]`` and zeros elsewhere.  Neither torchaudio nor encodec is
a dependency: parity with the packages themselves is not pinned.

There is no fallback: whatever needs arithmetic runs on the HIP kernel of ``device``; only "nothing to do" returns without it.

Behind the decoder (and in front of the encoder, for training clips) the same file sets the LEVEL of a waveform, which the reference
never does: ``loudness`` (ITU-R BS.1770-4 integrated loudness) and ``normalize_audio`` (gain to a target + limiter) on
csrc/loudness.hip; see the second half of this file and DESIGN.md section 10e.  The last part is the other half of BS.1770: ``true_peak``
(Annex 2: the level between the samples) and ``limit_true_peak`` (a look-ahead limiter under a true-peak ceiling, ``limit="truepeak"`` of
``normalize_audio``) on csrc/limiter.hip; DESIGN.md section 10k.
"""
from __future__ import annotations

import math
import numpy as np
import torch

from . import audio_host as H
from . import lib as L

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99
TABLE_MAX_BYTES = 256 * 1024     # cap on taps [n, W] float32: the table is meant to stay in L2; also keeps one frame's window within LDS


def tile_frames(o: int, n: int) -> int:
    """frames (o inputs -> n outputs each) one workgroup of the kernel owns for this rate pair: the library's own rule"""
    return int(L.load().jen1_resample_tile_frames(int(o), int(n)))


def resample_table(sr: int, target_sr: int):
    """(o, n, w, taps float32 [n, W], first int32 [n]): the compact polyphase filter of ``sr -> target_sr``.  Host only (numpy, float64,
    rounded to float32 once).  ``first[p]`` is the first non-zero tap of phase p in the dense row of K = 2 w + o taps, moved down where
    the W-tap row would otherwise run past K (the taps in front are zeros of the dense row).  Equal rates give the identity filter
    (o = n = 1, w = 0, one tap of 1.0)."""
    sr, target_sr = int(sr), int(target_sr)
    if sr <= 0 or target_sr <= 0:
        raise ValueError(f"sample rates must be positive, not {sr} -> {target_sr}")
    if sr == target_sr:
        return 1, 1, 0, np.ones((1, 1), np.float32), np.zeros((1,), np.int32)
    g = math.gcd(sr, target_sr)
    o, n = sr // g, target_sr // g
    base = min(o, n) * ROLLOFF
    w = int(math.ceil(LOWPASS_FILTER_WIDTH * o / base))
    K = 2 * w + o
    # |t| < 6 only for the k within 6 o / base of the phase's centre w + p o / n; everywhere else the clamp puts the window at
    # cos(pi / 2)**2 ~ 4e-33 and the product rounds to 0 in float32.  So only a band of Kb taps per phase is ever evaluated.
    half = LOWPASS_FILTER_WIDTH * o / base
    Kb = min(K, int(2 * half) + 6)
    if n * (Kb - 6) * 4 > TABLE_MAX_BYTES:
        raise ValueError(f"resample {sr} -> {target_sr}: the filter table ({n} phases of about {Kb - 5} taps) exceeds {TABLE_MAX_BYTES} bytes")
    pi = np.arange(n, dtype=np.int64)
    k0 = np.clip(w + (pi * o) // n - int(half) - 3, 0, K - Kb)          # first tap of the band of phase p
    k = (k0[:, None] + np.arange(Kb, dtype=np.int64)[None, :]).astype(np.float64)
    p = pi.astype(np.float64)[:, None]
    t = np.clip(((k - w) / o - p / n) * base, -LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    tz = np.where(t == 0, 1.0, t)
    sinc = np.where(t == 0, 1.0, np.sin(np.pi * tz) / (np.pi * tz))
    h = (sinc * np.cos(np.pi * t / (2 * LOWPASS_FILTER_WIDTH)) ** 2 * (base / o)).astype(np.float32)
    nz = h != 0
    lo = np.argmax(nz, axis=1)
    hi = Kb - np.argmax(nz[:, ::-1], axis=1)               # one past the last non-zero tap
    W = int((hi - lo).max())
    if n * W * 4 > TABLE_MAX_BYTES:
        raise ValueError(f"resample {sr} -> {target_sr}: the filter table ({n} x {W} float32) exceeds {TABLE_MAX_BYTES} bytes")
    lo = np.minimum(lo, Kb - W)
    taps = np.take_along_axis(h, lo[:, None] + np.arange(W)[None, :], axis=1)
    return o, n, w, np.ascontiguousarray(taps), (k0 + lo).astype(np.int32)


def _tables(sr: int, target_sr: int, device: torch.device):
    """(o, n, w, W, taps, first) of ``resample_table`` with the two arrays on ``device``"""
    def make():
        o, n, w, taps, first = resample_table(sr, target_sr)
        return o, n, w, taps.shape[1], torch.from_numpy(taps).to(device), torch.from_numpy(first).to(device)
    g = math.gcd(int(sr), int(target_sr))
    return H.device_table(device, ("resample", int(sr) // g, int(target_sr) // g), make)


def _run(wav: torch.Tensor, sr: int, target_sr: int, c_out: int, device) -> torch.Tensor:
    """wav [..., C, L] float32 -> [..., c_out, ceil(n L / o)] on the kernel of ``device``, returned on wav's device"""
    if wav.dtype != torch.float32:
        raise TypeError(f"waveforms are float32, not {wav.dtype}")
    dev = H.gpu_device(device, "the resampler")
    lead, c_in, n_in = tuple(wav.shape[:-2]), int(wav.shape[-2]), int(wav.shape[-1])
    o, n, w, W, taps, first = _tables(sr, target_sr, dev)
    n_out = -(-n * n_in // o)
    x = wav.to(dev).contiguous()
    y = torch.empty(lead + (c_out, n_out), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_resample", x.data_ptr(), y.data_ptr(), taps.data_ptr(), first.data_ptr(), math.prod(lead), c_in, c_out, n_in, n_out,
             o, n, w, W)
    return y.to(wav.device)


def resample(wav: torch.Tensor, sr: int, target_sr: int, device="cuda") -> torch.Tensor:
    """``torchaudio.functional.resample(wav, sr, target_sr)`` over the last axis of a float32 tensor with any leading axes.  Equal rates
    return ``wav`` itself."""
    if int(sr) <= 0 or int(target_sr) <= 0:
        raise ValueError(f"sample rates must be positive, not {sr} -> {target_sr}")
    if int(sr) == int(target_sr):
        return wav
    if wav.dim() < 1:
        raise ValueError("resample needs a time axis")
    return _run(wav.unsqueeze(-2), sr, target_sr, 1, device).squeeze(-2)


def convert_audio(wav: torch.Tensor, sr: int, target_sr: int, target_channels: int, device="cuda") -> torch.Tensor:
    """``encodec.utils.convert_audio``: wav [..., C, L] with C in {1, 2} -> [..., target_channels, ceil(n L / o)].  The channel rule is
    applied in front of the filter, in the same launch.  Same rate and same channel count: ``wav`` itself, nothing is loaded."""
    if wav.dim() < 2:
        raise RuntimeError("convert_audio: audio must have at least a channel and a time axis")
    c_in = int(wav.shape[-2])
    if c_in not in (1, 2):
        raise RuntimeError(f"convert_audio: audio must have one or two channels, not {c_in}")
    if target_channels not in (1, 2):
        raise RuntimeError(f"convert_audio: impossible to convert from {c_in} to {target_channels} channels")
    if int(sr) <= 0 or int(target_sr) <= 0:
        raise ValueError(f"sample rates must be positive, not {sr} -> {target_sr}")
    if int(sr) == int(target_sr) and c_in == target_channels:
        return wav
    return _run(wav, sr, target_sr, int(target_channels), device)


# ---------------------------------------------------------------------------------------------------------------- loudness
#
# ITU-R BS.1770-4 integrated loudness with every channel weight 1.0 (mono and stereo), and the gain + limiter that bring a waveform
# to a target (csrc/loudness.hip: jen1_kweight_energy, jen1_loudness_gate, jen1_gain_apply).  Not in the reference, whose output
# has whatever level the decoder gives it (Encodec 48 kHz: unit RMS per segment, peaks far above full scale).
STRATEGIES = ("loudness", "peak", "rms", "clip")
LIMITS = ("none", "clip", "tanh", "truepeak")     # the first three are JEN1_LIMIT_* of jen1_gain_apply; "truepeak" is jen1_limit_true_peak behind it
DEFAULT_HEADROOM_DB = {"loudness": 0.0, "peak": 1.0, "rms": 18.0, "clip": 0.0}


def k_weighting(sr: int) -> np.ndarray:
    """the K-weighting cascade at sample rate ``sr`` as float64 second-order sections ``[2, 6]``: rows (b0, b1, b2, 1, a1, a2) of the
    high shelf and of the high-pass behind it.  The analogue prototypes of BS.1770 through the bilinear transform with pre-warping
    (K = tan(pi f0 / sr)); at 48 kHz this reproduces the standard's tables to 1e-15.  Host only (numpy)."""
    sr = int(sr)
    if sr <= 0:
        raise ValueError(f"sample rate must be positive, not {sr}")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, high], dtype=np.float64)


def hop_samples(sr: int) -> int:
    """the 100 ms hop of the meter's 400 ms blocks in samples; the rate must give a whole number"""
    sr = int(sr)
    if sr <= 0 or sr % 10 != 0:
        raise ValueError(f"the loudness meter needs a positive sample rate that is a multiple of 10 (a whole 100 ms hop), not {sr}")
    return sr // 10


def chunk_samples(hop: int) -> int:
    """samples per chunk of the time-parallel K-weighting filter for this hop: the library's own rule"""
    return int(L.load().jen1_kweight_chunk(int(hop)))


def _check_wave(wav: torch.Tensor, what: str) -> None:
    if wav.dtype != torch.float32:
        raise TypeError(f"waveforms are float32, not {wav.dtype}")
    if wav.dim() < 2:
        raise ValueError(f"{what}: audio must have at least a channel and a time axis")
    if int(wav.shape[-2]) not in (1, 2):
        raise ValueError(f"{what}: audio must have one or two channels, not {int(wav.shape[-2])}")
    if int(wav.shape[-1]) < 1:
        raise ValueError(f"{what}: the time axis is empty")


def _measure(x: torch.Tensor, sr: int, gate: bool = True):
    """x [rows, C, L] float32, contiguous, on a GPU -> (lufs float64 [rows] or None, stats float64 [rows, 2]): the four launches of
    jen1_kweight_energy and, with ``gate``, jen1_loudness_gate behind them on the current stream of x's device"""
    rows, C, n = (int(s) for s in x.shape)
    hop = hop_samples(sr)
    blocks = n // hop
    dev = x.device
    nbytes = int(L.load().jen1_kweight_energy_workspace_bytes(rows, C, n, hop))
    work = H.workspace(nbytes, dev)
    e = torch.empty((rows, C, blocks), dtype=torch.float64, device=dev)
    stats = torch.empty((rows, 2), dtype=torch.float64, device=dev)
    sos = k_weighting(sr)
    coef = (L.C.c_double * 10)(*sos[0, [0, 1, 2, 4, 5]], *sos[1, [0, 1, 2, 4, 5]])
    H.launch(dev, "jen1_kweight_energy", x.data_ptr(), e.data_ptr() if blocks else None, stats.data_ptr(), coef, rows, C, n, hop, work.data_ptr(),
             nbytes)
    if not gate:
        return None, stats
    lufs = torch.empty((rows,), dtype=torch.float64, device=dev)
    H.launch(dev, "jen1_loudness_gate", e.data_ptr() if blocks else None, lufs.data_ptr(), rows, C, blocks, hop)
    return lufs, stats


def loudness(wav: torch.Tensor, sr: int, device="cuda") -> torch.Tensor:
    """BS.1770-4 integrated loudness in LUFS of ``wav [..., C, L]`` (float32, C in {1, 2}, channel weights 1.0): float64 ``[...]`` on
    wav's device.  ``-inf`` for a row shorter than one 400 ms block or with nothing above the gates."""
    _check_wave(wav, "loudness")
    hop_samples(sr)
    dev = H.gpu_device(device, "the loudness meter")
    lufs, _ = _measure(wav.to(dev).contiguous().reshape((-1,) + tuple(wav.shape[-2:])), sr)
    return lufs.reshape(tuple(wav.shape[:-2])).to(wav.device)


def normalize_audio(wav: torch.Tensor, sr: int, strategy: str = "loudness", target_lufs=-14.0, headroom_db=None, limit: str = "clip",
                    energy_floor: float = 2e-3, device="cuda", return_gain: bool = False, ceiling_dbtp: float = -1.0,
                    lookahead_ms: float = 1.5, release_ms: float = 100.0):
    """``limit(g * wav)`` over ``wav [..., C, L]`` (float32, C in {1, 2}) with one gain per row ``[...]``, formed on the device (nothing is
    read back on the way) and rounded to float32 once:

        "loudness"  10^((target_lufs - loudness) / 20); 1 for a row whose loudness is -inf or whose RMS is below ``energy_floor`` (such a
                    row comes back bit for bit)
        "peak"      10^(-headroom_db / 20) / max |wav| (headroom_db: 1 by default); 1 for an all-zero row
        "rms"       10^(-headroom_db / 20) / rms (headroom_db: 18 by default); 1 for an all-zero row
        "clip"      1

    ``target_lufs``: a float or a tensor ``[...]``, one target per row.  ``limit``: "none", "clip" (clamp to [-1, 1]), "tanh", or "truepeak":
    the gain with no limit, then ``limit_true_peak`` with ``ceiling_dbtp`` / ``lookahead_ms`` / ``release_ms`` (read by this limit alone).
    The result is a new tensor on wav's device; ``return_gain=True`` returns ``(result, gain float32 [...])``."""
    if strategy not in STRATEGIES:
        raise ValueError(f"unknown strategy {strategy!r}: one of {STRATEGIES}")
    if limit not in LIMITS:
        raise ValueError(f"unknown limit {limit!r}: one of {LIMITS}")
    _check_wave(wav, "normalize_audio")
    hop_samples(sr)
    plan = limiter_plan(sr, ceiling_dbtp, lookahead_ms, release_ms) if limit == "truepeak" else None
    lead = tuple(wav.shape[:-2])
    if torch.is_tensor(target_lufs) and tuple(target_lufs.shape) != lead:
        raise ValueError(f"target_lufs {tuple(target_lufs.shape)} must have one entry per row {lead}")
    dev = H.gpu_device(device, "normalize_audio")
    x = wav.to(dev).contiguous().reshape((-1,) + tuple(wav.shape[-2:]))
    rows, C, n = (int(s) for s in x.shape)
    if torch.is_tensor(target_lufs):
        target = target_lufs.to(dev, torch.float64).contiguous().reshape(-1)
    else:
        target = torch.full((rows,), float(target_lufs), dtype=torch.float64, device=dev)
    headroom = DEFAULT_HEADROOM_DB[strategy] if headroom_db is None else float(headroom_db)
    lufs, stats = (None, None) if strategy == "clip" else _measure(x, sr, gate=strategy == "loudness")
    y = torch.empty_like(x)
    gain = torch.empty((rows,), dtype=torch.float32, device=dev)
    H.launch(dev, "jen1_gain_apply", x.data_ptr(), y.data_ptr(), gain.data_ptr(), None if lufs is None else lufs.data_ptr(),
             None if stats is None else stats.data_ptr(), target.data_ptr(), rows, C, n, STRATEGIES.index(strategy),
             L.LIMIT_NONE if plan is not None else LIMITS.index(limit), headroom, float(energy_floor))
    if plan is not None:
        _limit_rows(y, y, sr, plan)
    y = y.reshape(tuple(wav.shape)).to(wav.device)
    return (y, gain.reshape(lead).to(wav.device)) if return_gain else y


# -------------------------------------------------------------------------------------------------------------- true peak
#
# ITU-R BS.1770-4 Annex 2: the peak of a waveform BETWEEN its samples, read from an oversampled copy, and a look-ahead limiter that
# holds a waveform under a true-peak ceiling (csrc/limiter.hip: jen1_true_peak, jen1_limit_true_peak).  Not in the reference.  The
# limiter is offline: the whole row is there, so it looks ahead without delay.
TRUE_PEAK_TAPS = 16              # taps per phase of the interpolator


def true_peak_factor(sr: int) -> int:
    """the oversampling factor: 4 below 80 kHz, 2 below 160 kHz, else 1 -- at least about 192 kHz after oversampling, as in Annex 2"""
    sr = int(sr)
    if sr <= 0:
        raise ValueError(f"sample rate must be positive, not {sr}")
    return 4 if sr < 80000 else 2 if sr < 160000 else 1


def true_peak_prototype(F: int) -> np.ndarray:
    """``h[i] = sinc((i - F T / 2) / F) kaiser(F T + 1, beta = 8)[i]``, i = 0 .. F T: the interpolator before it is cut into phases.
    float64; symmetric, 1 at its centre and 0 (to rounding) at every other multiple of F."""
    n = int(F) * TRUE_PEAK_TAPS
    i = np.arange(n + 1, dtype=np.float64)
    return np.sinc((i - n / 2) / F) * np.kaiser(n + 1, 8.0)


def true_peak_filter(sr: int):
    """(F, taps float64 [F - 1, T]) at sample rate ``sr``, T = 16: phase p = 1 .. F - 1 of the prototype, ``taps[p - 1][k] = h[p + k F]``.
    Phase 0 is the identity by construction (``o[n F] = x[n]``), so it is neither stored nor filtered and a reading never falls below
    the sample peak.  The oversampled signal is ``o[n F + p] = sum_{k < T} taps[p - 1][k] x[n + T / 2 - k]`` with zeros outside the row."""
    F = true_peak_factor(sr)
    h = true_peak_prototype(F)
    taps = np.stack([h[p:p + F * TRUE_PEAK_TAPS:F] for p in range(1, F)]) if F > 1 else np.zeros((0, TRUE_PEAK_TAPS))
    return F, np.ascontiguousarray(taps, dtype=np.float64)


def true_peak_tile() -> int:
    """samples of a row one workgroup of the meter and of the limiter owns: the library's own figure"""
    return int(L.load().jen1_true_peak_tile())


def max_lookahead() -> int:
    """the longest look-ahead of ``limit_true_peak`` in samples: what a tile of the limiter keeps of its neighbour in LDS"""
    return int(L.load().jen1_limiter_max_lookahead())


def attack_window(A: int) -> np.ndarray:
    """float64 [A + 1]: ``w[j] ~ sin^2(pi (j + 1) / (A + 2))``, normalised to sum 1 -- the weights that spread a step of the held
    reduction over the look-ahead"""
    j = np.arange(int(A) + 1, dtype=np.float64)
    w = np.sin(np.pi * (j + 1.0) / (int(A) + 2.0)) ** 2
    return w / w.sum()


def _envelope(x: torch.Tensor, sr: int, want_env: bool):
    """x [rows, C, L] float32, contiguous, on a GPU -> (env float64 [rows, L] or None, peak float64 [rows], linear): the two launches of
    jen1_true_peak on the current stream of x's device"""
    rows, C, n = (int(s) for s in x.shape)
    dev = x.device
    F, taps = true_peak_filter(sr)
    nbytes = int(L.load().jen1_true_peak_workspace_bytes(rows, C, n))
    work = H.workspace(nbytes, dev)
    env = torch.empty((rows, n), dtype=torch.float64, device=dev) if want_env else None
    peak = torch.empty((rows,), dtype=torch.float64, device=dev)
    H.launch(dev, "jen1_true_peak", x.data_ptr(), None if env is None else env.data_ptr(), n, peak.data_ptr(),
             taps.ctypes.data_as(L.C.POINTER(L.C.c_double)) if F > 1 else None, F, rows, C, n, work.data_ptr(), nbytes)
    return env, peak


def true_peak(wav: torch.Tensor, sr: int, device="cuda") -> torch.Tensor:
    """BS.1770-4 Annex 2 true peak in dBTP of ``wav [..., C, L]`` (float32, C in {1, 2}), the larger of the channels: float64 ``[...]`` on
    wav's device, ``-inf`` for silence.  Any positive ``sr`` (there is no hop rule).  Nothing is read back on the way."""
    _check_wave(wav, "true_peak")
    true_peak_factor(sr)
    dev = H.gpu_device(device, "the true-peak meter")
    _, peak = _envelope(wav.to(dev).contiguous().reshape((-1,) + tuple(wav.shape[-2:])), sr, False)
    return (20.0 * torch.log10(peak)).reshape(tuple(wav.shape[:-2])).to(wav.device)


def limiter_plan(sr: int, ceiling_dbtp, lookahead_ms, release_ms):
    """(c, A, rho) of ``limit_true_peak`` from its keywords, or the ValueError; nothing touches a device"""
    true_peak_factor(sr)
    ceiling_dbtp, lookahead_ms, release_ms = float(ceiling_dbtp), float(lookahead_ms), float(release_ms)
    if not math.isfinite(ceiling_dbtp):
        raise ValueError(f"ceiling_dbtp must be finite, not {ceiling_dbtp}")
    if not (math.isfinite(lookahead_ms) and lookahead_ms >= 0.0):
        raise ValueError(f"lookahead_ms must be finite and not negative, not {lookahead_ms}")
    if not (math.isfinite(release_ms) and release_ms >= 0.0):
        raise ValueError(f"release_ms must be finite and not negative, not {release_ms}")
    A = int(round(lookahead_ms * int(sr) / 1000.0))
    if A > max_lookahead():
        raise ValueError(f"lookahead_ms = {lookahead_ms} is {A} samples at {int(sr)} Hz: the limiter looks ahead {max_lookahead()} samples at most")
    c = 10.0 ** (ceiling_dbtp / 20.0)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"ceiling_dbtp = {ceiling_dbtp} is not a level a float64 holds")
    tau = release_ms * int(sr) / 1000.0
    return c, A, (math.exp(-1.0 / tau) if tau > 0.0 else 0.0)


def _limit_rows(x: torch.Tensor, y: torch.Tensor, sr: int, plan, want_reduction: bool = False):
    """x [rows, C, L] -> y (the same shape; may be x itself), both float32, contiguous, on one GPU: the meter's two launches and the
    limiter's four on the current stream.  Returns ``1 - s`` float64 [rows, L], or None"""
    c, A, rho = plan
    rows, C, n = (int(s) for s in x.shape)
    dev = x.device
    env, _ = _envelope(x, sr, True)
    window = H.device_table(dev, ("attack", A), lambda: torch.from_numpy(attack_window(A)).to(dev))
    nbytes = int(L.load().jen1_limiter_workspace_bytes(rows, n, A))
    work = H.workspace(nbytes, dev)
    red = torch.empty((rows, n), dtype=torch.float64, device=dev) if want_reduction else None
    H.launch(dev, "jen1_limit_true_peak", x.data_ptr(), y.data_ptr(), C * n, None if red is None else red.data_ptr(), n, env.data_ptr(), n,
             window.data_ptr(), rows, C, n, A, c, rho, work.data_ptr(), nbytes)
    return red


def limit_true_peak(wav: torch.Tensor, sr: int, ceiling_dbtp: float = -1.0, lookahead_ms: float = 1.5, release_ms: float = 100.0,
                    device="cuda", return_reduction: bool = False):
    """``s * wav`` over ``wav [..., C, L]`` (float32, C in {1, 2}) with one gain ``s [..., L] <= 1`` for every channel of a row, such that the
    true peak of the result stays at ``ceiling_dbtp``.  With ``env`` the linked envelope of the oversampled row (``true_peak_filter``),
    ``c = 10^(ceiling_dbtp / 20)``, ``A = round(lookahead_ms sr / 1000)`` and ``rho = exp(-1 / (release_ms sr / 1000))`` (0 for 0 ms):

        q[n] = 1 - min(1, c / env[n])                                     the reduction wanted
        Q[i] = max q[max(i, 0) .. min(i + A, L - 1)],  i = -A .. L - 1       held over the look-ahead (A samples of silence in front)
        d[i] = max(Q[i], rho d[i - 1]),  d[-A - 1] = 0                      released
        s[n] = 1 - sum_{j <= A} w[j] d[n - j],  w = attack_window(A)         attacked: every step of d is spread over A + 1 samples

    in float64, and ``float32(s[n] * float64(wav[n]))`` at the store.  By construction ``s[n] <= min(1, c / env[n])`` (to the rounding of
    ``sum w``), and a row whose true peak is at or under the ceiling comes back bit for bit.  ``A`` may be 0; above ``max_lookahead()``
    samples the call is refused.  A new tensor on wav's device; ``return_reduction=True`` returns ``(result, 1 - s float64 [..., L])``."""
    _check_wave(wav, "limit_true_peak")
    plan = limiter_plan(sr, ceiling_dbtp, lookahead_ms, release_ms)
    dev = H.gpu_device(device, "the true-peak limiter")
    x = wav.to(dev).contiguous().reshape((-1,) + tuple(wav.shape[-2:]))
    y = torch.empty_like(x)
    red = _limit_rows(x, y, sr, plan, return_reduction)
    y = y.reshape(tuple(wav.shape)).to(wav.device)
    return (y, red.reshape(tuple(wav.shape[:-2]) + (int(wav.shape[-1]),)).to(wav.device)) if return_reduction else y
