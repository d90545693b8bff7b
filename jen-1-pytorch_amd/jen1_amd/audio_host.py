"""Host layer of the waveform tools (``audio``, ``spectral``, ``analysis``, ``effects``, ``fad``, ``normalizer``): what they share between a
checked argument and a launch.  It imports nothing of the package but ``lib``.

    gpu_device      a device spec or a tensor's device -> ``torch.device("cuda", index)``, or the one refusal of a CPU
    rows_of         the leading axes of a tensor as one row axis, without a copy where the rows are evenly spaced
    device_table    the one cache of per-device constants (filter taps, twiddles, windows, filterbanks)
    Framing         (n_fft, hop, win_length, center, frames) from the one validator ``framing``; ``abi`` in the order of ``lib._SPEC_FRAMING``
    Bands           a banded filterbank on a device (``spectral.banded``); ``NO_BANDS`` where a kernel applies none
    launch          device guard, current stream, ``lib.check``; ``workspace`` for the float64 scratch a kernel asks for

Plain functions and two records; every helper but ``gpu_device`` works on any device, so the host tests run them on the CPU.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, NamedTuple, Optional

import numpy as np
import torch

from . import lib as L

N_FFTS = (256, 512, 1024, 2048, 4096)
_tables: Dict[tuple, object] = {}


# ------------------------------------------------------------------------------------------------------------- device, rows, launch
def gpu_device(where, what: str) -> torch.device:
    dev = torch.device(where)
    if dev.type != "cuda":
        raise L.Jen1HipError(f"{what} runs on a GPU, not on {dev}: there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def rows_of(t: torch.Tensor, dev: torch.device):
    """(x on dev, rows, n, row stride in elements): the leading axes as one row axis, without a copy where the rows are evenly spaced"""
    x = t.to(dev)
    n = int(x.shape[-1])
    rows = math.prod(x.shape[:-1])
    even = x.stride(-1) == 1 or n == 1
    for d in range(x.dim() - 2):
        even = even and (x.shape[d] == 1 or x.stride(d) == x.stride(d + 1) * x.shape[d + 1])
    if x.dim() >= 2 and even and (x.stride(-2) >= n or rows == 1):
        return x, rows, n, int(x.stride(-2)) if rows > 1 else n
    x = x.contiguous()
    return x, rows, n, n


def device_table(dev: torch.device, key: tuple, make: Callable[[], object]):
    """``make()`` on the first use of ``key`` on ``dev`` (by its string, as every table was cached), the same object afterwards"""
    hit = _tables.get((key, str(dev)))
    if hit is None:
        hit = _tables[(key, str(dev))] = make()
    return hit


def workspace(nbytes: int, dev: torch.device) -> torch.Tensor:
    """float64 scratch of at least ``nbytes`` bytes (never empty: the kernels take its pointer)"""
    return torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)


def launch(dev: torch.device, name: str, *args) -> None:
    """``lib.<name>(*args, stream)`` on the current stream of ``dev``, with ``dev`` current; a non-zero status raises ``Jen1HipError``"""
    with torch.cuda.device(dev):
        L.check(getattr(L.load(), name)(*args, torch.cuda.current_stream(dev).cuda_stream), name)


def host_ints(values, count: int, what: str) -> list:
    """host integers, one per row (a sequence, or a tensor that is read back), as a checked list"""
    vals = [int(v) for v in (values.tolist() if torch.is_tensor(values) else values)]
    if len(vals) != count:
        raise ValueError(f"{what} has {len(vals)} entries, the batch has {count} rows")
    return vals


def c_ints(vals):
    return (L.c_int * len(vals))(*vals)


# ------------------------------------------------------------------------------------------------------------- framing
def check_n_fft(n_fft) -> None:
    if int(n_fft) not in N_FFTS:
        raise ValueError(f"n_fft = {n_fft} is not one of {N_FFTS}")


def check_hop(hop, n_fft: int) -> None:
    if not 1 <= int(hop) <= n_fft:
        raise ValueError(f"hop = {hop} must be in [1, n_fft = {n_fft}]")


def twiddle_table(n_fft: int) -> np.ndarray:
    """float32 [n_fft, 2]: (cos, -sin)(2 pi m / n_fft), formed in float64 and rounded once"""
    check_n_fft(n_fft)
    a = 2.0 * np.pi * np.arange(int(n_fft), dtype=np.float64) / int(n_fft)
    return np.stack([np.cos(a), -np.sin(a)], axis=1).astype(np.float32)


def hann_window(win_length: int) -> np.ndarray:
    """the periodic Hann window of ``torch.hann_window(win_length)``: float32, from float64"""
    if int(win_length) < 1:
        raise ValueError(f"win_length must be positive, not {win_length}")
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(win_length), dtype=np.float64) / int(win_length))).astype(np.float32)


def frame_count(n: int, n_fft: int, hop: int, center: bool = True) -> int:
    """frames of ``torch.stft`` for n samples; the ValueErrors of ``stft`` for a signal too short to frame"""
    n, n_fft, hop = int(n), int(n_fft), int(hop)
    check_n_fft(n_fft)
    check_hop(hop, n_fft)
    if center:
        if n <= n_fft // 2:
            raise ValueError(f"center=True needs more than n_fft / 2 = {n_fft // 2} samples for the reflect padding, not {n}")
        return 1 + n // hop
    if n < n_fft:
        raise ValueError(f"center=False needs at least n_fft = {n_fft} samples, not {n}")
    return 1 + (n - n_fft) // hop


class Framing(NamedTuple):
    n_fft: int
    hop: int
    win_length: int
    center: bool
    frames: int

    def abi(self, rows: int, n: int) -> tuple:
        """rows, n, n_fft, hop, win_length, center: ``lib._SPEC_FRAMING``"""
        return rows, n, self.n_fft, self.hop, self.win_length, int(self.center)


def framing(n_fft: int, hop: Optional[int], win_length: Optional[int], window, center: bool, n: Optional[int] = None,
            frames: Optional[int] = None) -> Framing:
    """the defaults of ``torch.stft`` filled in and every refusal raised; the frames of ``n`` samples (``frame_count``), or the ``frames`` a
    spectrogram already has"""
    check_n_fft(n_fft)
    n_fft = int(n_fft)
    if win_length is None:
        win_length = int(window.numel()) if torch.is_tensor(window) else n_fft
    win_length = int(win_length)
    if win_length > n_fft or win_length < 1:
        raise ValueError(f"win_length = {win_length} must be in [1, n_fft = {n_fft}]")
    hop = n_fft // 4 if hop is None else int(hop)
    if frames is not None:
        check_hop(hop, n_fft)                       # of a spectrogram: before the window, as ``istft`` always refused
    if torch.is_tensor(window):
        if window.dim() != 1 or int(window.numel()) != win_length:
            raise ValueError(f"window of shape {tuple(window.shape)} must be 1-D with win_length = {win_length} values")
    elif window != "hann":
        raise ValueError(f"unknown window {window!r}: 'hann' or a 1-D tensor")
    if frames is None:
        frames = frame_count(n, n_fft, hop, center)
    return Framing(n_fft, hop, win_length, bool(center), int(frames))


def twiddle_on(n_fft: int, dev: torch.device) -> torch.Tensor:
    return device_table(dev, ("twiddle", int(n_fft)), lambda: torch.from_numpy(twiddle_table(n_fft)).to(dev))


def window_on(window, win_length: int, dev: torch.device) -> torch.Tensor:
    if torch.is_tensor(window):
        return window.detach().to(dev, torch.float32).contiguous()
    return device_table(dev, ("hann", int(win_length)), lambda: torch.from_numpy(hann_window(win_length)).to(dev))


def frame_tables(fr: Framing, window, dev: torch.device) -> tuple:
    """the window and twiddle pointers of a framing on ``dev``, in the order every framed kernel takes them"""
    return window_on(window, fr.win_length, dev).data_ptr(), twiddle_on(fr.n_fft, dev).data_ptr()


# ------------------------------------------------------------------------------------------------------------- filterbanks
class Bands(NamedTuple):
    """a banded [bands, bins] matrix on a device: band b is ``w[off[b] : off[b] + hi[b] - lo[b]]`` on the bins [lo[b], hi[b])"""
    lo: Optional[torch.Tensor]
    hi: Optional[torch.Tensor]
    off: Optional[torch.Tensor]
    w: Optional[torch.Tensor]
    n_bands: int
    n_weights: int

    @classmethod
    def on(cls, dev: torch.device, lo: np.ndarray, hi: np.ndarray, off: np.ndarray, w: np.ndarray) -> "Bands":
        """the four arrays of ``spectral.banded`` moved to ``dev``, the weights rounded to float32"""
        up = lambda a: torch.from_numpy(a).to(dev)
        return cls(up(lo), up(hi), up(off), up(w.astype(np.float32)), len(lo), int(w.size))

    def abi(self) -> tuple:
        """lo, hi, off, weights, n_bands, n_weights: the band arguments of include/jen1_spectral.h"""
        ptr = lambda t: None if t is None else t.data_ptr()
        return ptr(self.lo), ptr(self.hi), ptr(self.off), ptr(self.w), self.n_bands, self.n_weights


NO_BANDS = Bands(None, None, None, None, 0, 0)
