"""jen1_amd/wav.py on the host: files written by ``save`` and files built here byte by byte (PCM 8 / 16 / 24 / 32, float32, mono and stereo,
the extensible header, an odd-sized LIST chunk in front of ``data``) read back to the values they hold; against ``scipy.io.wavfile.read``
where scipy knows the format."""
import struct

import numpy as np
import pytest
import torch

from jen1_amd import wav

GUID_TAIL = bytes.fromhex("000000001000800000AA00389B71")          # KSDATAFORMAT_SUBTYPE_*: the 14 bytes after the format tag


def _ints(bits: int, channels: int, frames: int, seed: int) -> np.ndarray:
    """[frames, channels] integers covering the whole range of the width, with both extremes, 0 and -1 in front"""
    lo, hi = (0, 255) if bits == 8 else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    g = np.random.default_rng(seed)
    v = g.integers(lo, hi, size=(frames, channels), endpoint=True, dtype=np.int64)
    head = [lo, hi, 128 if bits == 8 else 0, 127 if bits == 8 else -1]
    v.reshape(-1)[:4] = head
    return v


def _pack(v: np.ndarray, bits: int) -> bytes:
    flat = v.reshape(-1)
    if bits == 8:
        return flat.astype(np.uint8).tobytes()
    if bits == 24:
        u = (flat & 0xFFFFFF).astype(np.uint32)
        return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    return flat.astype({16: "<i2", 32: "<i4"}[bits]).tobytes()


def _file(path, tag: int, channels: int, rate: int, bits: int, body: bytes, extensible: bool = False, extra: bytes = b"") -> None:
    align = channels * bits // 8
    base = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        base += struct.pack("<HHI", 22, bits, (1 << channels) - 1) + struct.pack("<H", tag) + GUID_TAIL
        assert len(base) == 40
    chunks = b"fmt " + struct.pack("<I", len(base)) + base + extra + b"data" + struct.pack("<I", len(body)) + body + b"\0" * (len(body) & 1)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


ODD_LIST = b"LIST" + struct.pack("<I", 13) + b"INFOICMT\x01\x00\x00\x00x" + b"\0"          # 13 bytes of body + the pad byte


@pytest.mark.parametrize("extra", [b"", ODD_LIST], ids=["plain", "odd-LIST"])
@pytest.mark.parametrize("extensible", [False, True], ids=["basic", "extensible"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_hand_built_pcm(tmp_path, bits, channels, extensible, extra):
    frames, rate = 37, 44100
    v = _ints(bits, channels, frames, 10 * bits + channels)
    path = tmp_path / "x.wav"
    _file(path, wav.FORMAT_PCM, channels, rate, bits, _pack(v, bits), extensible, extra)
    x, sr = wav.load(path)
    want = ((v - 128) / 128.0 if bits == 8 else v / float(1 << (bits - 1))).T
    assert sr == rate and x.dtype == np.float32 and x.shape == (channels, frames) and x.flags["C_CONTIGUOUS"]
    assert np.array_equal(x, want.astype(np.float32))                    # x / 2^(bits - 1), rounded once to float32
    assert wav.info(path) == (frames, rate, channels)
    assert x.min() == -1.0 and (x.max() < 1.0 if bits < 32 else x.max() == 1.0)      # (2^31 - 1) / 2^31 rounds to 1.0 in float32
    wavfile = pytest.importorskip("scipy.io.wavfile")
    sr2, y = wavfile.read(path)
    y = y.reshape(frames, channels).astype(np.int64)
    if bits == 24:
        y = y >> 8                                                       # scipy left-justifies 24-bit samples in int32
    assert sr2 == rate and np.array_equal(y, v)


@pytest.mark.parametrize("extensible", [False, True], ids=["basic", "extensible"])
@pytest.mark.parametrize("channels", [1, 2])
def test_hand_built_float32(tmp_path, channels, extensible):
    frames, rate = 41, 48000
    v = np.random.default_rng(channels).standard_normal((frames, channels)).astype(np.float32)
    v[0, 0], v[1, 0] = 1.5, -3.0                                         # float files are not clipped
    path = tmp_path / "f.wav"
    _file(path, wav.FORMAT_FLOAT, channels, rate, 32, v.astype("<f4").tobytes(), extensible, ODD_LIST)
    x, sr = wav.load(path)
    assert sr == rate and x.dtype == np.float32 and np.array_equal(x, v.T)
    assert wav.info(path) == (frames, rate, channels)
    wavfile = pytest.importorskip("scipy.io.wavfile")
    sr2, y = wavfile.read(path)
    assert sr2 == rate and np.array_equal(y.reshape(frames, channels), v)


@pytest.mark.parametrize("shape", [(1, 100), (2, 99), (1, 2, 50)], ids=str)
@pytest.mark.parametrize("encoding", ["pcm16", "float32"])
def test_save_round_trip(tmp_path, encoding, shape):
    x = (np.random.default_rng(3).random(shape) * 1.8 - 0.9).astype(np.float32)
    path = tmp_path / "s.wav"
    wav.save(path, torch.from_numpy(x) if len(shape) == 3 else x, 32000, encoding)
    y, sr = wav.load(path)
    flat = x.reshape(shape[-2:])
    assert sr == 32000 and y.shape == flat.shape and wav.info(path) == (shape[-1], 32000, shape[-2])
    if encoding == "float32":
        assert np.array_equal(y, flat)
    else:
        assert np.abs(y - flat).max() <= 0.5 / 32768 + 1e-9
        wav.save(path, y, 32000)                                         # what pcm16 holds survives a second trip exactly
        assert np.array_equal(wav.load(path)[0], y)
    wavfile = pytest.importorskip("scipy.io.wavfile")
    sr2, z = wavfile.read(path)
    assert sr2 == 32000 and z.dtype == (np.float32 if encoding == "float32" else np.int16)


def test_pcm16_clips_and_rounds_to_nearest(tmp_path):
    lsb = 1.0 / 32768
    x = np.array([[1.0, -1.0, 2.0, -2.0, 1.0 - lsb, 0.49 * lsb, 0.51 * lsb, -0.49 * lsb, -0.51 * lsb, 1.0 - 0.49 * lsb, -1.0 + 0.49 * lsb,
                   100.4 * lsb, 100.6 * lsb, 0.5 * lsb, 1.5 * lsb, -0.5 * lsb]], dtype=np.float64)
    path = tmp_path / "c.wav"
    wav.save(path, x, 8000)
    y, _ = wav.load(path)
    got = np.rint(y[0].astype(np.float64) * 32768).astype(int).tolist()
    # [-1, 1): +1.0 and beyond is the largest code; exact halves go to the even neighbour (IEEE round-half-even)
    assert got == [32767, -32768, 32767, -32768, 32767, 0, 1, 0, -1, 32767, -32768, 100, 101, 0, 2, 0]


def test_save_audio_tensor(tmp_path):
    from jen1_amd.generation import save_audio_tensor
    x = torch.rand((1, 2, 480)) * 0.5 - 0.25
    path = str(tmp_path / "samples.wav")
    save_audio_tensor(x, path)
    y, sr = wav.load(path)
    assert sr == 48000 and y.shape == (2, 480) and np.abs(y - x[0].numpy()).max() <= 0.5 / 32768 + 1e-9
    save_audio_tensor(x[0], path, sample_rate=44100)
    assert wav.info(path) == (480, 44100, 2)


def test_refusals(tmp_path):
    with pytest.raises(ValueError, match="mp3"):
        wav.load(tmp_path / "song.mp3")
    with pytest.raises(ValueError, match="mp3"):
        wav.info(tmp_path / "song.mp3")
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"RIFF\x04\0\0\0WAVX")
    with pytest.raises(ValueError, match="RIFF/WAVE"):
        wav.load(bad)
    _file(bad, 0x0055, 2, 44100, 16, b"\0" * 8)                          # MPEG layer 3 inside a WAVE container
    with pytest.raises(ValueError, match="unsupported"):
        wav.load(bad)
    with pytest.raises(ValueError, match="encoding"):
        wav.save(tmp_path / "e.wav", np.zeros((1, 4), dtype=np.float32), 8000, "pcm24")
