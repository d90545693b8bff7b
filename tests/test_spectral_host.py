"""Host side of the spectral metrics (jen1_amd/spectral.py, include/jen1_spectral.h): the mel filterbank and its banded form, the frame
arithmetic against ``torch.stft``, the twiddle table, every ValueError, and every refusal of the C entry points -- none of which needs a
GPU (a refused call returns before it touches the device)."""
import os
import re

import numpy as np
import pytest
import torch

import spectral_common as O

from jen1_amd import lib as L
from jen1_amd import spectral as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANKS = [(48000, 2048, 128, 0.0, None), (48000, 1024, 16, 0.0, None), (32000, 512, 40, 50.0, 14000.0), (48000, 4096, 128, 20.0, 20000.0)]


# ------------------------------------------------------------------ mel filterbank
@pytest.mark.parametrize("norm", [None, "slaney"])
@pytest.mark.parametrize("scale", ["htk", "slaney"])
@pytest.mark.parametrize("sr,n_fft,n_mels,f_min,f_max", BANKS)
def test_mel_filterbank_against_the_restatement(sr, n_fft, n_mels, f_min, f_max, scale, norm):
    fb = S.mel_filterbank(sr, n_fft, n_mels, f_min, f_max, mel_scale=scale, norm=norm)
    want = O.filterbank64(sr, n_fft, n_mels, f_min, f_max, scale, norm)
    assert fb.dtype == np.float64 and fb.shape == (n_mels, n_fft // 2 + 1)
    assert float(np.abs(fb - want).max()) <= 1e-12 * float(want.max())
    corners = O.mel_corners(sr, n_mels, f_min, f_max, scale)
    assert float(np.abs(S.mel_points(sr, n_mels, f_min, f_max, scale) - corners).max()) <= 1e-9
    f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    eps = 1e-9                     # bins within 1e-9 Hz of a corner may fall on either side
    for m in range(n_mels):        # the band of row m is exactly (f_m, f_{m+2})
        assert np.all(fb[m][(f > corners[m] + eps) & (f < corners[m + 2] - eps)] > 0), m
        assert np.all(fb[m][(f < corners[m] - eps) | (f > corners[m + 2] + eps)] == 0), m


@pytest.mark.parametrize("scale", ["htk", "slaney"])
@pytest.mark.parametrize("sr,n_fft,n_mels,f_min,f_max", BANKS)
def test_mel_triangles_sum_to_one_between_the_peaks(sr, n_fft, n_mels, f_min, f_max, scale):
    """without a norm every triangle peaks at 1 (at f_{m+1}) and its neighbours take over linearly: at every bin between the first and the
    last peak the bands add up to 1, and no weight exceeds 1"""
    fb = S.mel_filterbank(sr, n_fft, n_mels, f_min, f_max, mel_scale=scale)
    corners = O.mel_corners(sr, n_mels, f_min, f_max, scale)
    f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    inside = (f >= corners[1]) & (f <= corners[n_mels])
    assert inside.any() or n_mels == 1
    assert float(np.abs(fb[:, inside].sum(axis=0) - 1.0).max(initial=0.0)) <= 1e-12
    assert float(fb.max()) <= 1.0
    up = (corners[1:-1] - corners[:-2]) / (corners[1:-1] - corners[:-2])          # the formula at the peak itself
    assert np.all(up == 1.0)


def test_slaney_norm_scales_every_band():
    sr, n_fft, n_mels = 48000, 2048, 64
    corners = O.mel_corners(sr, n_mels, scale="slaney")
    plain = S.mel_filterbank(sr, n_fft, n_mels, mel_scale="slaney")
    normed = S.mel_filterbank(sr, n_fft, n_mels, mel_scale="slaney", norm="slaney")
    assert np.allclose(normed, plain * (2.0 / (corners[2:] - corners[:-2]))[:, None], rtol=1e-14, atol=0)


@pytest.mark.parametrize("sr,n_fft,n_mels,f_min,f_max", BANKS)
def test_banded_form_is_the_dense_matrix_bit_for_bit(sr, n_fft, n_mels, f_min, f_max):
    fb = S.mel_filterbank(sr, n_fft, n_mels, f_min, f_max)
    for m in (fb, fb.astype(np.float32)):
        lo, hi, off, w = S.banded(m)
        assert lo.dtype == hi.dtype == off.dtype == np.int32 and w.dtype == m.dtype
        assert np.all(lo <= hi) and np.all(hi <= m.shape[1]) and w.size == int((hi - lo).sum())
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(hi - lo)[:-1]]))
        assert np.array_equal(S.unbanded(lo, hi, off, w, m.shape[1]), m)
    # rows without a bin (more bands than bins below f_max) stay empty, and an interior zero stays inside its band
    tight = np.zeros((3, 9))
    tight[0, 2:6] = [0.5, 0.0, 0.25, 1.0]
    tight[2, 8] = 2.0
    lo, hi, off, w = S.banded(tight)
    assert lo.tolist() == [2, 0, 8] and hi.tolist() == [6, 0, 9] and off.tolist() == [0, 4, 4] and w.tolist() == [0.5, 0.0, 0.25, 1.0, 2.0]
    assert np.array_equal(S.unbanded(lo, hi, off, w, 9), tight)


# ------------------------------------------------------------------ framing
@pytest.mark.parametrize("n_fft,hop,win,n,rows,center", O.SHAPES)
def test_frame_count_is_torch_stft_s(n_fft, hop, win, n, rows, center):
    want = O.stft_cpu(np.zeros((1, n), np.float32), n_fft, hop, win, center).shape
    assert want == (1, n_fft // 2 + 1, S.frame_count(n, n_fft, hop, center)) == (1, n_fft // 2 + 1, O.frames_of(n, n_fft, hop, center))
    lib = L.load()
    assert lib.jen1_stft_frames(n, n_fft, hop, int(center)) == want[2]


def test_frame_count_at_the_edges():
    lib = L.load()
    for n_fft in S.N_FFTS:
        assert S.frame_count(n_fft // 2 + 1, n_fft, 1, True) == n_fft // 2 + 2 == lib.jen1_stft_frames(n_fft // 2 + 1, n_fft, 1, 1)
        assert S.frame_count(n_fft, n_fft, n_fft, False) == 1 == lib.jen1_stft_frames(n_fft, n_fft, n_fft, 0)
        assert lib.jen1_stft_frames(n_fft // 2, n_fft, 1, 1) == -1 and lib.jen1_stft_frames(n_fft - 1, n_fft, 1, 0) == -1
        assert lib.jen1_stft_tile_frames(n_fft) == 2 * lib.jen1_spectral_distance_tile_frames(n_fft) > 0
    assert lib.jen1_stft_tile_frames(384) == 0 and lib.jen1_stft_frames(1000, 384, 96, 1) == -1
    assert lib.jen1_spectral_distance_workspace_bytes(2, 1000, 256, 64, 1) == 2 * -(-16 // lib.jen1_spectral_distance_tile_frames(256)) * 24
    assert lib.jen1_spectral_distance_workspace_bytes(2, 100, 256, 64, 1) == 0


def test_window_placement_matches_torch_stft():
    """win_length < n_fft: the window sits (n_fft - win_length) // 2 from the left, also when the difference is odd -- read off torch.stft
    with an impulse at every offset of one frame"""
    n_fft, win = 256, 101
    left = (n_fft - win) // 2
    x = np.zeros((1, n_fft), np.float32)
    x[0, left] = 1.0
    first = O.stft_cpu(x, n_fft, n_fft, win, False)[0, 0, 0]
    x[:] = 0
    x[0, left + 1] = 1.0
    second = O.stft_cpu(x, n_fft, n_fft, win, False)[0, 0, 0]
    w = O.window64(win).numpy()
    assert abs(first.real - w[0]) <= 1e-15 and abs(second.real - w[1]) <= 1e-15 and w[0] == 0.0 and w[1] > 0
    assert float(np.abs(S.hann_window(win).astype(np.float64) - w).max()) <= 2.0 ** -24


@pytest.mark.parametrize("n_fft", S.N_FFTS)
def test_twiddle_table(n_fft):
    tw = S.twiddle_table(n_fft)
    a = 2.0 * np.pi * np.arange(n_fft) / n_fft
    assert tw.dtype == np.float32 and tw.shape == (n_fft, 2)
    assert float(np.abs(tw[:, 0] - np.cos(a)).max()) <= 2.0 ** -25 and float(np.abs(tw[:, 1] + np.sin(a)).max()) <= 2.0 ** -25
    assert tw[0].tolist() == [1.0, 0.0] and tw[n_fft // 2, 0] == -1.0 and tw[n_fft // 4, 1] == -1.0


# ------------------------------------------------------------------ ValueErrors (raised before a device is asked for)
def test_value_errors():
    x = torch.zeros((2, 2, 1000))
    with pytest.raises(ValueError, match="384"):
        S.stft(x, 384)
    with pytest.raises(ValueError, match=r"win_length = 600.*512"):
        S.stft(x, 512, win_length=600)
    with pytest.raises(ValueError, match=r"1024.*1000"):
        S.stft(x, 2048)                                   # center=True, n <= n_fft / 2
    with pytest.raises(ValueError, match=r"128.*128"):
        S.stft(torch.zeros(128), 256)
    with pytest.raises(ValueError, match=r"1024.*1000"):
        S.stft(x, 1024, center=False)                      # center=False, n < n_fft
    with pytest.raises(ValueError, match=r"hop = 0"):
        S.stft(x, 256, hop=0)
    with pytest.raises(ValueError, match=r"hop = 257"):
        S.spectrogram(x, 256, hop=257)
    with pytest.raises(ValueError, match="power"):
        S.spectrogram(x, 256, power=3.0)
    with pytest.raises(ValueError, match="window"):
        S.stft(x, 256, window="hamming")
    with pytest.raises(ValueError, match="window"):
        S.stft(x, 256, win_length=200, window=torch.ones(100))
    with pytest.raises(ValueError, match="autograd"):
        S.stft(torch.zeros((2, 1000), requires_grad=True), 256)
    with pytest.raises(TypeError):
        S.stft(x.double(), 256)
    with pytest.raises(ValueError, match=r"\(2, 2, 1000\).*\(2, 2, 999\)"):
        S.mrstft_distance(x, x[:, :, :999])
    with pytest.raises(ValueError, match=r"\(2, 2, 1000\).*\(2, 1, 1000\)"):
        S.mel_distance(x, x[:, :1], 48000)
    with pytest.raises(ValueError, match="384"):
        S.mrstft_distance(x, x, resolutions=((384, 96, 384),))
    with pytest.raises(ValueError, match=r"1024.*1000"):
        S.mrstft_distance(x, x)                           # the 2048-point resolution cannot pad 1000 samples
    with pytest.raises(ValueError, match="autograd"):
        S.mrstft_distance(torch.zeros((2, 3000), requires_grad=True), torch.zeros((2, 3000)))
    with pytest.raises(ValueError, match="384"):
        S.mel_spectrogram(x, 48000, n_fft=384)
    with pytest.raises(ValueError, match="log"):
        S.mel_spectrogram(x, 48000, n_fft=256, hop=64, log="ln")
    with pytest.raises(ValueError, match="floor"):
        S.mel_spectrogram(x, 48000, n_fft=256, hop=64, log="db", floor=0.0)
    with pytest.raises(ValueError, match="mel_scale"):
        S.mel_filterbank(48000, 256, 16, mel_scale="bark")
    with pytest.raises(ValueError, match="norm"):
        S.mel_filterbank(48000, 256, 16, norm="area")
    with pytest.raises(ValueError, match="384"):
        S.twiddle_table(384)
    with pytest.raises(ValueError, match=r"\(2, 2, 1000\).*\(2, 2, 999\)"):
        S.audio_report(x, x[:, :, :999], 48000)


def test_codec_report_needs_the_segment_codec():
    from jen1_amd.config import GDMConfig, tiny_model_config
    from jen1_amd.generation import Jen1

    class Stub:
        channels, sample_rate = 2, 48000

    j = Jen1(None, device="cpu", audio_encoder=Stub(), conditioner=lambda md, device: {}, model_config=tiny_model_config(),
             diffusion_config=GDMConfig(), compute_dtype="f32")
    with pytest.raises(ValueError, match=r"needs an audio_encoder with encode_latents \(jen1_amd.encodec.EncodecHIP\)"):
        j.codec_report(torch.zeros((2, 48000)))
    Stub.encode_latents = lambda self, a: None
    with pytest.raises(ValueError, match=r"needs an audio_encoder with decode_latents \(jen1_amd.encodec.EncodecHIP\)"):
        j.codec_report(torch.zeros((2, 48000)))


# ------------------------------------------------------------------ the C ABI
def test_header_declares_what_lib_binds():
    import jen1_amd
    text = open(os.path.join(ROOT, "include", "jen1_spectral.h")).read()
    names = re.findall(r"^(?:int|int64_t) (jen1_\w+)\(", text, flags=re.M)
    assert sorted(names) == sorted(L.SPECTRAL_SYMBOLS) and len(names) == 7
    assert "spectral.hip" in L.SOURCES and L.ABI_VERSION == 2
    so = L.load()
    assert so.jen1_abi_version() == 2
    for n in names:
        assert hasattr(so, n), n
    for const in ("SPEC_COMPLEX", "SPEC_MAGNITUDE", "SPEC_POWER", "SPEC_LOG_NONE", "SPEC_LOG_E", "SPEC_LOG_DB"):
        assert re.search(rf"#define JEN1_{const} {getattr(L, const)}\b", text), const
    assert jen1_amd.spectral is S and "spectral" in jen1_amd.__all__


FAKE = 0x10000          # a non-null "device pointer": a refused call never dereferences or launches on it


def _stft_call(lib, **kw):
    a = dict(x=FAKE, stride=1000, out=FAKE, window=FAKE, twiddle=FAKE, rows=2, n=1000, n_fft=256, hop=64, win=256, center=1, kind=0)
    a.update(kw)
    return lib.jen1_stft(a["x"], a["stride"], a["out"], a["window"], a["twiddle"], a["rows"], a["n"], a["n_fft"], a["hop"], a["win"], a["center"],
                         a["kind"], None)


def _mel_call(lib, **kw):
    a = dict(x=FAKE, stride=1000, out=FAKE, window=FAKE, twiddle=FAKE, lo=FAKE, hi=FAKE, off=FAKE, w=FAKE, n_bands=16, n_weights=100, rows=2,
             n=1000, n_fft=256, hop=64, win=256, center=1, kind=2, log=0, floor=1e-10)
    a.update(kw)
    return lib.jen1_mel(a["x"], a["stride"], a["out"], a["window"], a["twiddle"], a["lo"], a["hi"], a["off"], a["w"], a["n_bands"], a["n_weights"],
                        a["rows"], a["n"], a["n_fft"], a["hop"], a["win"], a["center"], a["kind"], a["log"], a["floor"], None)


def _distance_call(lib, **kw):
    a = dict(x=FAKE, xs=1000, y=FAKE, ys=1000, out=FAKE, window=FAKE, twiddle=FAKE, lo=None, hi=None, off=None, w=None, n_bands=0, n_weights=0,
             rows=2, n=1000, n_fft=256, hop=64, win=256, center=1, kind=1, floor=1e-5, work=FAKE, nbytes=1 << 20)
    a.update(kw)
    return lib.jen1_spectral_distance(a["x"], a["xs"], a["y"], a["ys"], a["out"], a["window"], a["twiddle"], a["lo"], a["hi"], a["off"], a["w"],
                                      a["n_bands"], a["n_weights"], a["rows"], a["n"], a["n_fft"], a["hop"], a["win"], a["center"], a["kind"],
                                      a["floor"], a["work"], a["nbytes"], None)


COMMON_REFUSALS = [(dict(x=None), "null"), (dict(window=None), "null"), (dict(twiddle=None), "null"), (dict(out=None), "null"),
                   (dict(n_fft=384), "n_fft = 384"), (dict(hop=0), "hop = 0"), (dict(hop=257), "hop = 257"), (dict(win=257), "win_length = 257"),
                   (dict(win=0), "win_length = 0"), (dict(center=2), "center = 2"), (dict(n=128), "n_fft / 2"), (dict(n=0), "bad shape"),
                   (dict(rows=-1), "bad shape"), (dict(center=0, n=255), "n >= n_fft")]


def _refused(lib, call, bad, word):
    assert call(lib, **bad) != 0, bad
    msg = lib.jen1_last_error().decode()
    assert word in msg, (bad, msg)


def test_c_entry_points_refuse_bad_arguments():
    lib = L.load()
    for bad, word in COMMON_REFUSALS + [(dict(kind=3), "kind = 3"), (dict(stride=999), "stride")]:
        _refused(lib, _stft_call, bad, word)
        assert "jen1_stft" in lib.jen1_last_error().decode()
    for bad, word in COMMON_REFUSALS + [(dict(kind=0), "kind = 0"), (dict(log=3), "log_mode = 3"), (dict(log=1, floor=0.0), "floor"),
                                        (dict(lo=None), "null"), (dict(w=None), "null"), (dict(n_bands=0), "n_bands = 0"),
                                        (dict(n_weights=0), "n_weights")]:
        _refused(lib, _mel_call, bad, word)
        assert "jen1_mel" in lib.jen1_last_error().decode()
    for bad, word in COMMON_REFUSALS + [(dict(y=None), "null"), (dict(work=None), "null"), (dict(floor=0.0), "floor"), (dict(nbytes=8), "workspace"),
                                        (dict(work=FAKE + 4), "aligned"), (dict(ys=10), "stride"), (dict(n_bands=-1), "n_bands"),
                                        (dict(n_bands=4, n_weights=10), "null"), (dict(n_bands=4, n_weights=10, lo=FAKE, hi=FAKE, off=FAKE, w=FAKE,
                                                                                       kind=0), "kind = 0")]:
        _refused(lib, _distance_call, bad, word)
        assert "jen1_spectral_distance" in lib.jen1_last_error().decode()
    # rows = 0 is a valid call that has nothing to do
    assert _stft_call(lib, rows=0) == 0 and _mel_call(lib, rows=0) == 0 and _distance_call(lib, rows=0) == 0
