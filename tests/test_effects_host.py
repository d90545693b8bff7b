"""Host side of the inverse STFT, the phase vocoder and the tempo / pitch effects (include/jen1_vocoder.h, jen1_amd/spectral.py,
jen1_amd/effects.py): the C ABI and every refusal of its entry points (a refused call returns before it touches the device), the frame
rule of the vocoder, the rational pitch factors, the metadata rule, and ``LatentCollate(augment=...)`` with stubs.  None needs a GPU."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import vocoder_common as V

from jen1_amd import audio
from jen1_amd import effects as E
from jen1_amd import lib as L
from jen1_amd import spectral as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a non-null "device pointer": a refused call never dereferences or launches on it


# ------------------------------------------------------------------ the C ABI
def test_header_declares_what_lib_binds():
    import jen1_amd
    text = open(os.path.join(ROOT, "include", "jen1_vocoder.h")).read()
    names = re.findall(r"^(?:int|int64_t) (jen1_\w+)\(", text, flags=re.M)
    assert sorted(names) == sorted(L.VOCODER_SYMBOLS) and len(names) == 6
    assert "vocoder.hip" in L.SOURCES and L.ABI_VERSION == 2
    so = L.load()
    assert so.jen1_abi_version() == 2
    for n in names:
        assert hasattr(so, n), n
    assert jen1_amd.effects is E and "effects" in jen1_amd.__all__ and "spectral" in jen1_amd.__all__
    assert os.path.exists(os.path.join(ROOT, "jen-1-pytorch_amd", "csrc", "spec_fft.h"))


def test_tile_queries():
    lib = L.load()
    for n_fft in S.N_FFTS:
        run, per = lib.jen1_istft_tile_samples(n_fft), lib.jen1_istft_tile_frames(n_fft)
        assert run >= n_fft and run % n_fft == 0 and per == lib.jen1_stft_tile_frames(n_fft)
        buffers = (per // 2) * (n_fft + 1) * 8
        lds = lambda r: buffers + (r + r // 64 + 1) * 4
        assert lds(run) <= 160 * 1024 and (run == 8192 or lds(2 * run) > 160 * 1024), "the longest run up to 8192 that fits a CU's LDS"
    assert lib.jen1_istft_tile_samples(384) == 0 and lib.jen1_istft_tile_frames(384) == 0
    assert lib.jen1_phase_vocoder_tile_frames() == 64


def _istft_call(lib, host_window=None, **kw):
    w = np.ascontiguousarray(S.hann_window(256) if host_window is None else host_window, dtype=np.float32)
    a = dict(spec=FAKE, out=FAKE, stride=None, window=FAKE, host=w.ctypes.data, twiddle=FAKE, rows=2, frames=16, length=960, n_fft=256, hop=64,
             win=len(w), center=1)
    a.update(kw)
    a["stride"] = a["length"] + 7 if a["stride"] is None else a["stride"]
    return lib.jen1_istft(a["spec"], a["out"], a["stride"], a["window"], a["host"], a["twiddle"], a["rows"], a["frames"], a["length"], a["n_fft"],
                          a["hop"], a["win"], a["center"], None)


def _vocoder_call(lib, **kw):
    a = dict(spec=FAKE, out=FAKE, rows=2, frames=16, n_fft=256, hop=64, rate=1.25)
    a.update(kw)
    return lib.jen1_phase_vocoder(a["spec"], a["out"], a["rows"], a["frames"], a["n_fft"], a["hop"], a["rate"], None)


def _refused(lib, call, bad, word, who):
    assert call(lib, **bad) != 0, bad
    msg = lib.jen1_last_error().decode()
    assert word in msg and who in msg, (bad, msg)


def test_c_entry_points_refuse_bad_arguments():
    lib = L.load()
    for bad, word in [(dict(n_fft=384), "n_fft = 384"), (dict(hop=0), "hop = 0"), (dict(hop=257), "hop = 257"), (dict(win=257), "win_length = 257"),
                      (dict(center=2), "center = 2"), (dict(frames=0), "bad shape"), (dict(rows=-1), "bad shape"), (dict(length=0), "length = 0"),
                      (dict(length=-5), "length = -5"), (dict(stride=959), "stride"), (dict(spec=None), "null"), (dict(out=None), "null"),
                      (dict(window=None), "null"), (dict(host=None), "null"), (dict(twiddle=None), "null"), (dict(spec=FAKE + 4), "aligned"),
                      (dict(hop=256, length=3840), "NOLA")]:                  # a Hann window of 256 at hop 256: zero wherever two frames meet
        _refused(lib, _istft_call, bad, word, "jen1_istft")
    # a window that never vanishes overlap-adds at any hop; a short window leaves gaps between frames at a hop beyond its length
    lifted = np.full(256, 0.5, np.float32)
    assert _istft_call(lib, host_window=lifted, hop=256, length=3840, rows=0) == 0
    _refused(lib, _istft_call, dict(host_window=np.ones(100, np.float32), hop=128, length=1920), "NOLA", "jen1_istft")
    # center = 0 starts under the window's first value, which is zero for a periodic Hann
    _refused(lib, _istft_call, dict(center=0, length=1216), "NOLA", "jen1_istft")
    assert _istft_call(lib, host_window=lifted, center=0, length=1216, rows=0) == 0
    # samples past the frames' reach are zeros by definition and stay out of the check: 16 frames hold 256 + 15 * 64 - 128 = 1088 samples
    assert _istft_call(lib, length=5000, rows=0) == 0
    for bad, word in [(dict(n_fft=384), "n_fft = 384"), (dict(hop=0), "hop = 0"), (dict(hop=257), "hop = 257"), (dict(rate=0.0), "rate = 0"),
                      (dict(rate=-1.0), "rate = -1"), (dict(rate=float("nan")), "rate"), (dict(rate=float("inf")), "rate"),
                      (dict(rate=1e-12), "too many"), (dict(frames=0), "bad shape"), (dict(rows=-1), "bad shape"), (dict(spec=None), "null"),
                      (dict(out=None), "null"), (dict(out=FAKE + 4), "aligned")]:
        _refused(lib, _vocoder_call, bad, word, "jen1_phase_vocoder")
    assert _vocoder_call(lib, rows=0) == 0 and _istft_call(lib, rows=0) == 0


@pytest.mark.parametrize("T", [1, 3, 94, 3001])
@pytest.mark.parametrize("rate", V.RATES)
def test_vocoder_frames_is_numpy_arange(T, rate):
    lib = L.load()
    want = len(np.arange(0, T, rate))
    assert lib.jen1_vocoder_frames(T, rate) == want == V.vocoder_frames(T, rate) == S.vocoder_frame_count(T, rate)
    assert (want - 1) * rate < T <= want * rate, "the number of j >= 0 with j * rate < T"


def test_vocoder_frames_refusals():
    lib = L.load()
    assert lib.jen1_vocoder_frames(0, 1.0) == -1 and lib.jen1_vocoder_frames(10, 0.0) == -1 and lib.jen1_vocoder_frames(10, -2.0) == -1
    assert lib.jen1_vocoder_frames(10, float("nan")) == -1 and lib.jen1_vocoder_frames(10, 1e-10) == -1
    assert lib.jen1_vocoder_frames(10, 100.0) == 1
    with pytest.raises(ValueError, match="rate"):
        S.vocoder_frame_count(10, 0.0)


# ------------------------------------------------------------------ ValueErrors and the missing GPU
def test_value_errors_come_before_the_device():
    spec = torch.zeros((2, 129, 16), dtype=torch.complex64)
    with pytest.raises(TypeError, match="complex64"):
        S.istft(torch.zeros((2, 129, 16)), 256)
    with pytest.raises(ValueError, match="384"):
        S.istft(spec, 384)
    with pytest.raises(ValueError, match=r"129 bins.*512"):
        S.istft(spec, 512)
    with pytest.raises(ValueError, match="hop = 0"):
        S.istft(spec, 256, hop=0)
    with pytest.raises(ValueError, match="win_length = 300"):
        S.istft(spec, 256, win_length=300)
    with pytest.raises(ValueError, match="window"):
        S.istft(spec, 256, window="hamming")
    with pytest.raises(ValueError, match="length = 0"):
        S.istft(spec[:, :, :1], 256)
    with pytest.raises(ValueError, match="bins"):
        S.phase_vocoder(torch.zeros((2, 100, 16), dtype=torch.complex64), 1.25, 64)
    with pytest.raises(ValueError, match="rate = 0"):
        S.phase_vocoder(spec, 0.0, 64)
    with pytest.raises(ValueError, match="hop = 300"):
        S.phase_vocoder(spec, 1.25, 300)
    x = torch.zeros((2, 4000))
    with pytest.raises(ValueError, match="rate = -1"):
        E.time_stretch(x, -1.0)
    with pytest.raises(TypeError):
        E.pitch_shift(x.double(), 48000, 2)
    with pytest.raises(ValueError, match="384"):
        E.time_stretch(x, 1.25, n_fft=384)


def test_no_cpu_fallback_and_nothing_to_do():
    x = torch.zeros((2, 4000))
    spec = torch.zeros((2, 129, 16), dtype=torch.complex64)
    for call in (lambda: S.istft(spec, 256, device="cpu"), lambda: S.phase_vocoder(spec, 1.25, 64, device="cpu"),
                 lambda: E.time_stretch(x, 1.25, device="cpu"), lambda: E.pitch_shift(x, 48000, 2, device="cpu"),
                 lambda: E.stretch_and_shift(x, 48000, 0.9, -2, device="cpu")):
        with pytest.raises(L.Jen1HipError, match="no CPU fallback"):
            call()
    assert E.stretch_and_shift(x, 48000, device="cpu") is x and E.time_stretch(x, 1.0, device="cpu") is x and E.pitch_shift(x, 48000, 0, device="cpu") is x


# ------------------------------------------------------------------ pitch factors
def test_semitone_ratio_is_within_two_cents_and_every_table_builds():
    worst = 0.0
    for s in range(-12, 13):
        f = E.semitone_ratio(s)
        assert f.denominator <= 128 and f > 0
        cents = abs(1200.0 * math.log2(float(f)) - 100.0 * s)
        worst = max(worst, cents)
        assert cents < 2.0, (s, f, cents)
        o, n, w, taps, first = audio.resample_table(f.numerator, f.denominator)
        assert (o, n) == (f.numerator, f.denominator) and taps.nbytes < 9 * 1024 < audio.TABLE_MAX_BYTES, (s, f, taps.nbytes)
    assert E.semitone_ratio(0) == 1 and E.semitone_ratio(12) == 2 and E.semitone_ratio(-12) == Fraction(1, 2) and E.semitone_ratio(7) == Fraction(3, 2)
    assert 1.9 < worst < 2.0, "the worst case is the fifth, 3/2"


# ------------------------------------------------------------------ Augment
def test_transform_metadata():
    T = E.Augment.transform_metadata
    md = {"prompt": "x", "tempo": 120, "key": 7}
    out = T(md, 1.1, 2)
    assert out == {"prompt": "x", "tempo": 120 * 1.1, "key": 9} and md == {"prompt": "x", "tempo": 120, "key": 7} and out is not md
    for key in range(24):
        for s in range(-12, 13):
            moved = T({"key": key}, 1.0, s)["key"]
            assert moved // 12 == key // 12, "major stays major, minor stays minor"
            assert moved % 12 == (key + s) % 12, "the tonic moves by s modulo 12"
    assert T({"key": 11}, 1.0, 2) == {"key": 1} and T({"key": 12}, 1.0, -3) == {"key": 21} and T({"key": 23}, 1.0, 1) == {"key": 12}
    assert T({"prompt": "y"}, 0.9, -2) == {"prompt": "y"}, "absent entries stay absent"
    assert T({"tempo": 100.0}, 0.9, 5) == {"tempo": 90.0} and T({"key": 3}, 0.9, 0) == {"key": 3}


def test_augment_draws():
    kw = dict(tempo_rates=(0.9, 1.0, 1.1), semitones=(-2, 0, 2), p=0.7)
    a, b, c = E.Augment(seed=5, **kw), E.Augment(seed=5, **kw), E.Augment(seed=6, **kw)
    import random
    random.seed(0)
    da = [a.draw() for _ in range(200)]
    random.seed(1)                                     # the global generator is not the one that draws
    db = [b.draw() for _ in range(200)]
    assert da == db and da != [c.draw() for _ in range(200)]
    assert set(da) <= {(r, s) for r in kw["tempo_rates"] for s in kw["semitones"]} and len(set(da)) == 9
    plain = sum(d == (1.0, 0) for d in da)
    assert 200 * (0.3 + 0.7 / 9) * 0.6 < plain < 200 * (0.3 + 0.7 / 9) * 1.4
    assert all(type(s) is int and type(r) is float for r, s in da)
    assert [E.Augment(p=0.0, tempo_rates=(2.0,), semitones=(5,)).draw() for _ in range(5)] == [(1.0, 0)] * 5
    assert E.Augment().draw() == (1.0, 0)
    for bad in (dict(semitones=(0.5,)), dict(semitones=()), dict(tempo_rates=(0.0,)), dict(tempo_rates=()), dict(p=1.5), dict(semitones=(True,))):
        with pytest.raises(ValueError):
            E.Augment(**bad)
    assert E.Augment(semitones=(2.0, -3)).semitones == (2, -3)


# ------------------------------------------------------------------ LatentCollate(augment=...)
class StubEncoder:
    sample_rate, channels = 48000, 2

    def __init__(self):
        self.calls = []

    def encode_latents(self, wav):
        self.calls.append(wav.clone())
        return (wav[:, :1, ::320].repeat(1, 128, 1) * 2.0,)


class FixedDraws:
    """an Augment whose draws are given"""

    def __init__(self, draws):
        self.draws, self.at = list(draws), 0

    def draw(self):
        self.at += 1
        return self.draws[self.at - 1]

    transform_metadata = staticmethod(E.Augment.transform_metadata)


def _batch():
    g = torch.Generator().manual_seed(3)
    clip = lambda n: torch.rand((2, n), generator=g) - 0.5
    return [(clip(48000), 48000, {"prompt": "a", "tempo": 100, "key": 11}),
            (clip(48000), 48000, {"prompt": "b"}),
            (clip(24000), 48000, {"prompt": "c", "key": 14}),
            (clip(48000), 48000, {"prompt": "d", "tempo": 80.0}),
            (clip(30000), 48000, {"prompt": "e", "tempo": 60, "key": 0})]


def test_latent_collate_augment_with_stubs():
    from jen1_amd.dataset import LatentCollate
    same = lambda wav, sr, target_sr, ch: wav
    calls, seen = [], []

    def stretch(wav, sr, rate=1.0, semitones=0.0):
        """a stand-in with the right length: the clip's samples at steps of ``rate``, marked with the shift"""
        calls.append((wav.clone(), sr, rate, semitones))
        n = int(round(wav.shape[-1] / rate))
        idx = torch.clamp((torch.arange(n) * rate).long(), max=wav.shape[-1] - 1)
        return wav[..., idx] + 0.001 * semitones

    def analyser(wav, rate, lengths=None):
        seen.append((wav.clone(), list(lengths)))
        B = wav.shape[0]
        return {"tempo": torch.full((B,), 111.0), "tempo_strength": torch.ones(B), "key": torch.full((B,), 5, dtype=torch.int32),
                "key_strength": torch.ones(B)}

    batch = _batch()
    before = [dict(md) for _c, _s, md in batch]
    draws = [(1.25, 2), (0.8, -3), (1.25, 2), (1.0, 0), (0.8, -3)]
    enc = StubEncoder()
    fn = LatentCollate(enc, device="cpu", sample_duration=1, convert_audio=same, analyze=("tempo", "key"), analyzer=analyser, augment=FixedDraws(draws),
                       augmenter=stretch, with_lengths=True)
    emb, meta, lengths = fn(batch)
    plain_enc = StubEncoder()
    plain = LatentCollate(plain_enc, device="cpu", sample_duration=1, convert_audio=same)(batch)
    base = plain_enc.calls[0]
    # grouping: one call per distinct draw that changes anything, each with the rows of its items, in the batch's order
    assert len(calls) == 2 and [(c[2], c[3]) for c in calls] == [(1.25, 2), (0.8, -3)] and all(c[1] == 48000 for c in calls)
    assert torch.equal(calls[0][0], base[[0, 2]]) and torch.equal(calls[1][0], base[[1, 4]])
    fed = enc.calls[0]
    assert fed.shape == base.shape == (5, 2, 48000) and emb.shape == plain[0].shape, "the batch keeps its shape"
    assert torch.equal(fed[3], base[3]), "the (1.0, 0) draw is left alone"
    fast = stretch(base[[0, 2]], 48000, 1.25, 2)                               # 38400 samples: zero-padded
    assert torch.equal(fed[[0, 2], :, :38400], fast) and not fed[[0, 2], :, 38400:].any()
    slow = stretch(base[[1, 4]], 48000, 0.8, -3)                               # 60000 samples: cropped
    assert torch.equal(fed[[1, 4]], slow[:, :, :48000])
    # valid lengths: min(n_out, round(valid / rate)), in front of the analyser and in the latent frame counts
    want_valid = [38400, 48000, 19200, 48000, 37500]
    assert len(seen) == 1 and seen[0][1] == want_valid and torch.equal(seen[0][0], fed), "measured on the augmented batch"
    assert lengths == [fn.valid_frames(v, 48000, emb.shape[-1]) for v in want_valid]
    # entries of the JSON move with the draw; measured entries are taken from the augmented audio as they are
    assert meta[0] == {"prompt": "a", "tempo": 125.0, "key": 1}
    assert meta[1] == {"prompt": "b", "tempo": 111.0, "key": 5}
    assert meta[2] == {"prompt": "c", "key": 16, "tempo": 111.0}
    assert meta[3] == {"prompt": "d", "tempo": 80.0, "key": 5}
    assert meta[4] == {"prompt": "e", "tempo": 48.0, "key": 9}
    assert [md for _c, _s, md in batch] == before, "the input dicts are not mutated"


def test_latent_collate_without_augment_is_unchanged():
    from jen1_amd.dataset import LatentCollate, get_dataloaders
    import inspect
    same = lambda wav, sr, target_sr, ch: wav
    batch = _batch()
    e0, e1, e2 = StubEncoder(), StubEncoder(), StubEncoder()
    boom = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the augmenter must not run"))
    a = LatentCollate(e0, device="cpu", sample_duration=1, convert_audio=same)(batch)
    b = LatentCollate(e1, device="cpu", sample_duration=1, convert_audio=same, augment=None, augmenter=boom)(batch)
    c = LatentCollate(e2, device="cpu", sample_duration=1, convert_audio=same, augment=E.Augment(p=0.0, tempo_rates=(1.5,)), augmenter=boom)(batch)
    for other, enc in ((b, e1), (c, e2)):
        assert torch.equal(a[0], other[0]) and torch.equal(e0.calls[0], enc.calls[0])
    assert all(m is item[2] for m, item in zip(b[1], batch)), "augment=None hands the dicts on as before"
    # the content of the batch, spelled out: clips zero-padded to one second, encoded by the stub
    want = torch.zeros((5, 2, 48000))
    for i, (clip, _sr, _md) in enumerate(batch):
        want[i, :, :clip.shape[-1]] = clip
    assert torch.equal(e0.calls[0], want) and torch.equal(a[0], want[:, :1, ::320].repeat(1, 128, 1) * 2.0)
    sig = inspect.signature(LatentCollate.__init__).parameters
    assert sig["augment"].default is None and sig["augmenter"].default is None
    assert inspect.signature(get_dataloaders).parameters["augment"].default is None
