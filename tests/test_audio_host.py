"""Host side of the resampler / channel converter (jen1_amd/audio.py) and its place in ``Jen1``: the compact filter table against the
dense restatement of tests/audio_common.py, the restatement itself against an analytic sine, and the paths that need no kernel.

Behind them, the host layer the waveform tools share (jen1_amd/audio_host.py): the row view, the framing record and its one validator,
the banded filterbank record, the device-table cache, the refusal of a CPU, and the rule that no module reaches into another's private
names.  Everything runs on the CPU: every helper but ``gpu_device`` takes any device."""
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

from audio_common import ALL_PAIRS, dense_resample, dense_table, geometry

from jen1_amd import audio
from jen1_amd import audio_host as H
from jen1_amd import fad
from jen1_amd import lib as L
from jen1_amd import spectral as S
from jen1_amd.config import tiny_model_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.mark.parametrize("sr,target,want,w_max", [(44100, 48000, (147, 160, 7), 13), (96000, 48000, (2, 1, 13), 25),
                                                  (48000, 44100, (160, 147, 7), 14)])
def test_table_geometry(sr, target, want, w_max):
    o, n, w, taps, first = audio.resample_table(sr, target)
    assert (o, n, w) == want == geometry(sr, target)[:3]
    assert taps.dtype == np.float32 and first.dtype == np.int32 and taps.shape[0] == n and first.shape == (n,)
    assert taps.shape[1] <= w_max


@pytest.mark.parametrize("sr,target", ALL_PAIRS)
def test_compact_table_is_the_dense_table(sr, target):
    """scattering taps / first back into [n, K] gives the dense float32 table exactly; the dense table is 0 outside [first, first + W)"""
    o, n, w, taps, first = audio.resample_table(sr, target)
    h = dense_table(sr, target)
    K, W = h.shape[1], taps.shape[1]
    assert K == 2 * w + o and 1 <= W <= K and taps.nbytes <= audio.TABLE_MAX_BYTES
    assert int(first.min()) >= 0 and int((first + W).max()) <= K
    back = np.zeros_like(h)
    outside = np.ones(h.shape, bool)
    for p in range(n):
        back[p, first[p]:first[p] + W] = taps[p]
        outside[p, first[p]:first[p] + W] = False
    assert np.array_equal(back, h)
    assert not h[outside].any()
    assert int((h != 0).sum(axis=1).max()) <= W == int(max(np.flatnonzero(r)[-1] - np.flatnonzero(r)[0] + 1 for r in h))


def test_table_refusals_and_identity():
    for bad in ((0, 48000), (48000, -1)):
        with pytest.raises(ValueError):
            audio.resample_table(*bad)
    with pytest.raises(ValueError, match="bytes"):
        audio.resample_table(44101, 48000)            # 48000 phases x 13 taps: over TABLE_MAX_BYTES (and never built densely)
    o, n, w, taps, first = audio.resample_table(48000, 48000)
    assert (o, n, w) == (1, 1, 0) and taps.tolist() == [[1.0]] and first.tolist() == [0]


@pytest.mark.parametrize("sr,target", [(44100, 48000), (32000, 48000), (96000, 48000), (22050, 48000), (48000, 44100)])
def test_restatement_resamples_a_sine(sr, target):
    """the dense float64 restatement against something that does not share its formula: a 1 kHz sine of 3000 samples must come out as
    the same sine sampled at the new rate, within 1e-3 (the filter's pass-band gain is 1.00004 .. 1.0009), 200 samples off each end"""
    L, f = 3000, 1000.0
    x = np.sin(2 * np.pi * f * np.arange(L) / sr)
    y = dense_resample(x, sr, target)
    o, n, _, _ = geometry(sr, target)
    assert y.shape == (-(-n * L // o),)
    want = np.sin(2 * np.pi * f * np.arange(y.shape[0]) / target)
    err = float(np.abs(y - want)[200:-200].max())
    print(f"{sr} -> {target}: max error against the analytic sine {err:.2e}")
    assert err <= 1e-3


def test_rows_of_the_441_to_48_table_sum_to_one():
    sums = dense_table(44100, 48000).astype(np.float64).sum(axis=1)
    assert float(sums.min()) >= 1.0 and float(sums.max()) <= 1.001


def test_convert_audio_paths_without_a_kernel():
    wav = torch.randn((2, 2, 100))
    assert audio.convert_audio(wav, 48000, 48000, 2, device="cpu") is wav
    mono = torch.randn((1, 100))
    assert audio.convert_audio(mono, 44100, 44100, 1) is mono
    assert audio.resample(mono, 44100, 44100) is mono
    with pytest.raises(RuntimeError):
        audio.convert_audio(torch.randn((3, 100)), 44100, 48000, 2)
    with pytest.raises(RuntimeError):
        audio.convert_audio(torch.randn((2, 100)), 44100, 48000, 3)
    with pytest.raises(RuntimeError):
        audio.convert_audio(torch.randn((2, 100)), 48000, 48000, 3)


def test_jen1_default_convert_audio_passes_matching_audio_through():
    from jen1_amd.generation import Jen1

    class Enc:
        channels = 2
    j = Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda md, dev: {}, model_config=tiny_model_config())
    batched = torch.randn((3, 2, 4800))
    for sr in (48000, None):
        wav, placeholder, prefix = j._known_audio("music_inpaint", batched, sr, 3, 4800)
        assert wav is batched and not placeholder and prefix == 4800
    own = Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda md, dev: {}, model_config=tiny_model_config(),
               convert_audio=lambda wav, sr, target_sr, ch: wav[..., ::2])
    assert own._known_audio("music_inpaint", batched, 96000, 3, 2400)[0].shape == (3, 2, 2400)     # a caller's own callable still wins


def test_generate_has_output_sr():
    from jen1_amd.generation import Jen1
    p = inspect.signature(Jen1.generate).parameters
    assert p["output_sr"].default is None
    assert list(p).index("output_sr") > list(p).index("inpainting_scope")          # behind every parameter of the reference


# ================================================================== the shared host layer (jen1_amd/audio_host.py)
def header_parameters(header: str, entry: str):
    """the parameter names of ``entry`` as include/<header> declares them, in order"""
    text = open(os.path.join(ROOT, "include", header)).read()
    decl = re.search(r"\bint " + entry + r"\((.*?)\);", text, re.S).group(1)
    return [re.split(r"[\s*]+", p.strip())[-1] for p in decl.split(",")]


# ------------------------------------------------------------------ rows_of
ROW_VIEWS = [                       # input, rows, n, stride, same memory: what spectral's row view gave on these before it moved here
    ("b", lambda b: b, 6, 4, 4, True),
    ("arange(5.)", lambda b: torch.arange(5.0), 1, 5, 5, True),
    ("b[..., :3]", lambda b: b[..., :3], 6, 3, 4, True),
    ("b[:, :2]", lambda b: b[:, :2], 4, 4, 4, False),
    ("arange(4.).expand(3, 4)", lambda b: torch.arange(4.0).expand(3, 4), 3, 4, 4, False),
    ("b.transpose(1, 2)", lambda b: b.transpose(1, 2), 8, 3, 3, False),
    ("b[..., :1]", lambda b: b[..., :1], 6, 1, 4, True),
    ("b[..., ::2]", lambda b: b[..., ::2], 6, 2, 2, False),
    ("b[:1, :1, :3]", lambda b: b[:1, :1, :3], 1, 3, 3, True),
]


@pytest.mark.parametrize("name,view,rows,n,stride,same", ROW_VIEWS, ids=[v[0] for v in ROW_VIEWS])
def test_rows_of_reproduces_the_row_view(name, view, rows, n, stride, same):
    t = view(torch.arange(24.0).reshape(2, 3, 4))
    assert t.dtype == torch.float32
    x, got_rows, got_n, got_stride = H.rows_of(t, CPU)
    assert (got_rows, got_n, got_stride) == (rows, n, stride)
    assert (x.data_ptr() == t.data_ptr()) == same
    # whatever the view, element i of row r lies r * stride + i elements behind x's first
    assert torch.equal(torch.as_strided(x, (rows, n), (stride, 1)), t.reshape(rows, n))


# ------------------------------------------------------------------ Framing
def test_framing_abi_is_the_headers_order():
    abi = H.framing(1024, 100, 480, "hann", False, n=5000).abi(7, 5000)
    assert len(abi) == len(L._SPEC_FRAMING)
    assert abi == (7, 5000, 1024, 100, 480, 0) and all(type(v) is int for v in abi)
    assert H.framing(1024, 100, 480, "hann", True, n=5000).abi(1, 5000)[-1] == 1
    for header, entry in (("jen1_spectral.h", "jen1_stft"), ("jen1_spectral.h", "jen1_mel"), ("jen1_spectral.h", "jen1_spectral_distance"),
                          ("jen1_analysis.h", "jen1_music_features")):
        params = header_parameters(header, entry)
        at = params.index("rows")
        assert params[at:at + 6] == ["rows", "n", "n_fft", "hop", "win_length", "center"], entry


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("n_fft", [256, 4096])
def test_framing_counts_frames_as_frame_count_does(n_fft, center):
    for hop in (1, n_fft):
        for n in (n_fft, n_fft + 1, 3 * n_fft + 17):
            fr = H.framing(n_fft, hop, None, "hann", center, n=n)
            assert fr.frames == S.frame_count(n, n_fft, hop, center)
            assert (fr.n_fft, fr.hop, fr.win_length, fr.center) == (n_fft, hop, n_fft, center)
    assert H.framing(n_fft, None, None, "hann", center, n=n_fft).hop == n_fft // 4
    assert H.framing(n_fft, None, None, torch.ones(100), center, n=n_fft).win_length == 100


@pytest.mark.parametrize("n_fft", [256, 4096])
def test_framing_bounds_on_the_signal_length(n_fft):
    assert H.framing(n_fft, None, None, "hann", True, n=n_fft // 2 + 1).frames == 1 + (n_fft // 2 + 1) // (n_fft // 4)
    assert H.framing(n_fft, None, None, "hann", False, n=n_fft).frames == 1
    with pytest.raises(ValueError, match="center=True needs more than"):
        H.framing(n_fft, None, None, "hann", True, n=n_fft // 2)
    with pytest.raises(ValueError, match="center=False needs at least"):
        H.framing(n_fft, None, None, "hann", False, n=n_fft - 1)


BAD_FRAMINGS = [
    (dict(win_length=300), "win_length = 300 must be in [1, n_fft = 256]"),
    (dict(win_length=0), "win_length = 0 must be in [1, n_fft = 256]"),
    (dict(hop=0), "hop = 0 must be in [1, n_fft = 256]"),
    (dict(hop=257), "hop = 257 must be in [1, n_fft = 256]"),
    (dict(window="hamming"), "unknown window 'hamming': 'hann' or a 1-D tensor"),
    (dict(window=torch.ones(100), win_length=128), "window of shape (100,) must be 1-D with win_length = 128 values"),
    (dict(window=torch.ones(2, 128)), "window of shape (2, 128) must be 1-D with win_length = 256 values"),
]


@pytest.mark.parametrize("bad,text", BAD_FRAMINGS, ids=[f"{'-'.join(sorted(b[0]))}-{i}" for i, b in enumerate(BAD_FRAMINGS)])
def test_stft_and_istft_refuse_a_bad_framing_alike(bad, text):
    """both build their framing through ``audio_host.framing``: the same type and the same text, before any device is looked at"""
    with pytest.raises(ValueError) as forward:
        S.stft(torch.zeros(2, 1000), 256, **bad)
    with pytest.raises(ValueError) as inverse:
        S.istft(torch.zeros((2, 129, 16), dtype=torch.complex64), 256, **bad)
    assert str(forward.value) == str(inverse.value) == text
    assert type(forward.value) is type(inverse.value) is ValueError


def test_two_refusals_at_once_keep_each_transforms_own_order():
    """a bad hop and a bad window together: ``stft`` names the window (its hop is checked with the frame count), ``istft`` the hop;
    ``phase_vocoder`` prints the hop it was given"""
    spec = torch.zeros((2, 129, 16), dtype=torch.complex64)
    with pytest.raises(ValueError, match=r"^unknown window 'boxcar': 'hann' or a 1-D tensor$"):
        S.stft(torch.zeros(2, 1000), 256, hop=0, window="boxcar")
    with pytest.raises(ValueError, match=r"^hop = 0 must be in \[1, n_fft = 256\]$"):
        S.istft(spec, 256, hop=0, window="boxcar")
    with pytest.raises(ValueError, match=r"^hop = 300\.5 must be in \[1, n_fft = 256\]$"):
        S.phase_vocoder(spec, 1.5, 300.5)


# ------------------------------------------------------------------ Bands
def test_bands_abi_is_the_headers_order():
    lo, hi, off, w = S.banded(np.array([[0.0, 1.0, 2.0, 0.0], [0.0, 0.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0]]))
    b = H.Bands.on(CPU, lo, hi, off, w)
    assert b.abi() == (b.lo.data_ptr(), b.hi.data_ptr(), b.off.data_ptr(), b.w.data_ptr(), 3, 4)
    assert b.w.dtype == torch.float32 and b.lo.dtype == b.hi.dtype == b.off.dtype == torch.int32
    for header, entry in (("jen1_spectral.h", "jen1_mel"), ("jen1_spectral.h", "jen1_spectral_distance"), ("jen1_analysis.h", "jen1_music_features")):
        params = header_parameters(header, entry)
        at = params.index("band_lo")
        assert params[at:at + 6] == ["band_lo", "band_hi", "band_off", "band_w", "n_bands", "n_weights"], entry


def test_no_bands_is_the_empty_form():
    assert H.NO_BANDS.n_bands == 0 and H.NO_BANDS.n_weights == 0
    assert H.NO_BANDS.abi() == (None, None, None, None, 0, 0)


def test_the_banks_round_trip_to_their_dense_matrices():
    mel = (32000, 512, 40, 50.0, 14000.0, "slaney", "slaney")
    for bands, dense in ((fad.vggish_bands(CPU), fad.vggish_mel_matrix()), (S.mel_bands(*mel, CPU), S.mel_filterbank(*mel))):
        assert bands.n_bands == dense.shape[0] and bands.n_weights == int(bands.w.numel())
        back = S.unbanded(bands.lo.numpy(), bands.hi.numpy(), bands.off.numpy(), bands.w.numpy(), dense.shape[1])
        assert back.dtype == np.float32 and np.array_equal(back, dense.astype(np.float32))
    assert fad.vggish_bands(CPU) is fad.vggish_bands(CPU) and S.mel_bands(*mel, CPU) is S.mel_bands(*mel, CPU)


# ------------------------------------------------------------------ device_table, workspace, host integers
def test_device_table_makes_once_per_key_and_device():
    made = []

    def make(tag):
        def f():
            made.append(tag)
            return torch.zeros(3)
        return f
    key = ("test_audio_host", 1)
    a = H.device_table(CPU, key, make("a"))
    assert H.device_table(CPU, key, make("again")) is a and H.device_table(torch.device("cpu"), key, make("again")) is a
    b = H.device_table(torch.device("cpu", 0), key, make("b"))              # "cpu:0": another device string
    c = H.device_table(CPU, ("test_audio_host", 2), make("c"))
    assert b is not a and c is not a and c is not b
    assert H.device_table(torch.device("cpu", 0), key, make("again")) is b
    assert made == ["a", "b", "c"]
    assert H.twiddle_on(256, CPU) is H.twiddle_on(256, CPU) and H.twiddle_on(256, CPU) is not H.twiddle_on(512, CPU)
    assert H.window_on("hann", 256, CPU) is H.window_on("hann", 256, CPU)
    assert np.array_equal(H.twiddle_on(256, CPU).numpy(), S.twiddle_table(256))
    assert np.array_equal(H.window_on("hann", 256, CPU).numpy(), S.hann_window(256))


def test_workspace_is_never_empty():
    assert H.workspace(0, CPU).numel() == 1 and H.workspace(8, CPU).numel() == 1 and H.workspace(808, CPU).numel() == 101
    assert H.workspace(0, CPU).dtype == torch.float64


def test_host_ints_are_checked():
    assert H.host_ints(torch.tensor([3, 4]), 2, "lengths") == [3, 4] and H.host_ints((5,), 1, "lengths") == [5]
    with pytest.raises(ValueError, match="lengths has 2 entries, the batch has 3 rows"):
        H.host_ints([1, 2], 3, "lengths")
    assert list(H.c_ints([3, 0, 7])) == [3, 0, 7]


# ------------------------------------------------------------------ gpu_device
@pytest.mark.parametrize("where", ["cpu", torch.device("cpu"), torch.zeros(1).device], ids=["string", "device", "tensor"])
def test_gpu_device_refuses_a_cpu(where):
    with pytest.raises(L.Jen1HipError) as e:
        H.gpu_device(where, "the tool")
    assert str(e.value) == "the tool runs on a GPU, not on cpu: there is no CPU fallback"


# ------------------------------------------------------------------ layering
def test_no_module_reaches_into_anothers_private_names():
    pattern = re.compile(r"(spectral|audio|fad|analysis)\._[a-z]")
    hits = []
    for path in sorted(glob.glob(os.path.join(ROOT, "jen-1-pytorch_amd", "jen1_amd", "*.py"))):
        for i, line in enumerate(open(path), 1):
            if pattern.search(line):
                hits.append(f"{os.path.basename(path)}:{i}: {line.strip()}")
    assert not hits, "\n".join(hits)
