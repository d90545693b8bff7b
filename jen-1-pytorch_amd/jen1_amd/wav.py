"""RIFF/WAVE files in and out on the host (numpy only): what the reference gets from ``torchaudio.load`` / ``torchaudio.save`` /
``torchaudio.info`` for ``.wav`` (dataset/dataloader.py:41,86; generation.py:212).

Read: PCM at 8, 16, 24 and 32 bits, IEEE float32, and ``WAVE_FORMAT_EXTENSIBLE`` wrapping either; chunks other than ``fmt `` and ``data``
are skipped, odd-sized chunks carry their pad byte.  Integer samples are scaled by ``1 / 2^(bits - 1)`` (8-bit is unsigned with an offset
of 128), which is torchaudio's ``normalize=True``.  Write: 16-bit PCM (clipped to [-1, 1), rounded to nearest) or float32.
"""
from __future__ import annotations

import os
import struct
from typing import BinaryIO, Tuple

import numpy as np

FORMAT_PCM, FORMAT_FLOAT, FORMAT_EXTENSIBLE = 0x0001, 0x0003, 0xFFFE


def _refuse_other_containers(path) -> None:
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".mp3":
        raise ValueError(f"{path}: .mp3 files are not supported (no decoder on this path); convert the file to .wav")
    if ext not in (".wav", ".wave", ""):
        raise ValueError(f"{path}: only RIFF/WAVE (.wav) files are supported, not {ext!r}")


def _header(f: BinaryIO, path) -> Tuple[int, int, int, int, int, int]:
    """walks the chunks up to ``data``: (format tag, channels, sample rate, bits, data offset, data bytes); the file is left at the data"""
    head = f.read(12)
    if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    fmt = None
    while True:
        ck = f.read(8)
        if len(ck) < 8:
            raise ValueError(f"{path}: no data chunk")
        name, size = ck[:4], struct.unpack("<I", ck[4:])[0]
        if name == b"fmt ":
            body = f.read(size)
            if len(body) < 16:
                raise ValueError(f"{path}: fmt chunk of {len(body)} bytes")
            tag, channels, rate, _byte_rate, _align, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == FORMAT_EXTENSIBLE:
                if len(body) < 40:
                    raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE with a {len(body)}-byte fmt chunk")
                tag = struct.unpack("<H", body[24:26])[0]                   # the first two bytes of the SubFormat GUID
            fmt = (tag, channels, rate, bits)
            if size & 1:
                f.seek(1, os.SEEK_CUR)
        elif name == b"data":
            if fmt is None:
                raise ValueError(f"{path}: data chunk before the fmt chunk")
            tag, channels, rate, bits = fmt
            if (tag, bits) not in ((FORMAT_PCM, 8), (FORMAT_PCM, 16), (FORMAT_PCM, 24), (FORMAT_PCM, 32), (FORMAT_FLOAT, 32)):
                raise ValueError(f"{path}: unsupported WAVE format tag {tag:#06x} at {bits} bits")
            if channels < 1 or rate < 1:
                raise ValueError(f"{path}: {channels} channels at {rate} Hz")
            offset = f.tell()
            rest = os.fstat(f.fileno()).st_size - offset
            return tag, channels, rate, bits, offset, min(size, rest)       # a streamed file may leave size at 0xFFFFFFFF
        else:
            f.seek(size + (size & 1), os.SEEK_CUR)


def info(path) -> Tuple[int, int, int]:
    """(frames, sample rate, channels) from the header alone"""
    _refuse_other_containers(path)
    with open(path, "rb") as f:
        _tag, channels, rate, bits, _off, nbytes = _header(f, path)
    return nbytes // (channels * (bits // 8)), rate, channels


def load(path) -> Tuple[np.ndarray, int]:
    """(float32 [channels, frames], sample rate)"""
    _refuse_other_containers(path)
    with open(path, "rb") as f:
        tag, channels, rate, bits, _off, nbytes = _header(f, path)
        step = channels * (bits // 8)
        raw = np.frombuffer(f.read(nbytes - nbytes % step), dtype=np.uint8)
    if tag == FORMAT_FLOAT:
        x = raw.view("<f4").astype(np.float32)
    elif bits == 8:
        x = (raw.astype(np.float32) - 128.0) / 128.0
    elif bits == 16:
        x = raw.view("<i2").astype(np.float32) / 32768.0
    elif bits == 24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
    else:
        x = (raw.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    return np.ascontiguousarray(x.reshape(-1, channels).T), rate


def save(path, audio, sr: int, encoding: str = "pcm16") -> None:
    """audio [channels, frames] or [1, channels, frames] (numpy array or torch tensor, any float type) -> a WAVE file"""
    _refuse_other_containers(path)
    if encoding not in ("pcm16", "float32"):
        raise ValueError(f"encoding must be 'pcm16' or 'float32', not {encoding!r}")
    if hasattr(audio, "detach"):
        audio = audio.detach().to("cpu").numpy()
    x = np.asarray(audio, dtype=np.float32)
    if x.ndim == 3 and x.shape[0] == 1:
        x = x[0]
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[0] > 65535:
        raise ValueError(f"audio must be [channels, frames] or [1, channels, frames], not {tuple(np.shape(audio))}")
    channels = x.shape[0]
    if encoding == "pcm16":
        tag, bits = FORMAT_PCM, 16
        body = np.clip(np.rint(x.T.astype(np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes()
    else:
        tag, bits = FORMAT_FLOAT, 32
        body = np.ascontiguousarray(x.T).astype("<f4").tobytes()
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", tag, channels, int(sr), int(sr) * align, align, bits)
    pad = b"\0" * (len(body) & 1)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(body) + len(pad)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(body)) + body + pad)
