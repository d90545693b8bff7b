"""Host side of the resampler / channel converter (jen1_amd/audio.py) and its place in ``Jen1``: the compact filter table against the
dense restatement of tests/audio_common.py, the restatement itself against an analytic sine, and the paths that need no kernel."""
import inspect

import numpy as np
import pytest
import torch

from audio_common import ALL_PAIRS, dense_resample, dense_table, geometry

from jen1_amd import audio
from jen1_amd.config import tiny_model_config


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
