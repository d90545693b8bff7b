"""Host side of the true-peak meter and limiter (include/jen1_limiter.h, jen1_amd/audio.py: true_peak, limit_true_peak,
normalize_audio(limit="truepeak")): the C ABI and every refusal of its entry points (a refused call returns before it touches the
device), the interpolator's table against the float64 oracle of tests/limiter_common.py, the keywords and their defaults, and the
oracle itself on signals whose answer is known.  None needs a GPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import limiter_common as O

from jen1_amd import audio
from jen1_amd import lib as L
from jen1_amd.config import tiny_model_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000          # a non-null, 8-byte aligned "device pointer": a refused call never dereferences or launches on it


# ------------------------------------------------------------------ the C ABI
def test_header_declares_what_lib_binds():
    text = open(os.path.join(ROOT, "include", "jen1_limiter.h")).read()
    names = re.findall(r"^(?:int|int64_t) (jen1_\w+)\(", text, flags=re.M)
    assert sorted(names) == sorted(L.LIMITER_SYMBOLS) and len(names) == 7
    assert not set(names) & set(L.SYMBOLS), "the new entry points stay out of the table of the old headers"
    assert "limiter.hip" in L.SOURCES and L.ABI_VERSION == 2
    so = L.load()
    assert so.jen1_abi_version() == 2
    for n in names:
        assert hasattr(so, n), n
    assert os.path.exists(os.path.join(ROOT, "jen-1-pytorch_amd", "csrc", "limiter.hip"))


def test_size_queries():
    lib = L.load()
    tile, chunk, cap = lib.jen1_true_peak_tile(), lib.jen1_limiter_chunk(), lib.jen1_limiter_max_lookahead()
    assert tile == audio.true_peak_tile() and cap == audio.max_lookahead()
    assert tile >= 256 and tile % chunk == 0 and tile // chunk == 256, "a tile is one chunk per thread of a 256-thread workgroup"
    assert (tile + cap) * 8 + (cap + 1) * 8 <= 64 * 1024, "the tile and its look-ahead halo in float64, and the window, fit 64 KiB of LDS"
    assert cap >= 288, "1.5 ms at 192 kHz"
    assert lib.jen1_true_peak_workspace_bytes(3, 2, 1) == 3 * 8 and lib.jen1_true_peak_workspace_bytes(3, 2, tile + 1) == 3 * 2 * 8
    for bad in ((-1, 2, 10), (1, 3, 10), (1, 0, 10), (1, 2, 0)):
        assert lib.jen1_true_peak_workspace_bytes(*bad) == 0, bad
    assert lib.jen1_limiter_workspace_bytes(2, tile, 0) == 2 * (tile + 2) * 8
    assert lib.jen1_limiter_workspace_bytes(2, tile, 1) == 2 * (tile + 1 + 4) * 8, "the hold's domain is L + A samples"
    for bad in ((-1, 10, 0), (1, 0, 0), (1, 10, -1), (1, 10, cap + 1)):
        assert lib.jen1_limiter_workspace_bytes(*bad) == 0, bad
    assert lib.jen1_limiter_workspace_bytes(1, 10, cap) > 0


def _meter_call(lib, **kw):
    _, taps = audio.true_peak_filter(48000)
    a = dict(x=FAKE, env=FAKE, stride=None, peak=FAKE, taps=taps, F=4, rows=2, C=2, L=5000, work=FAKE, nbytes=None)
    a.update(kw)
    a["stride"] = a["L"] + 3 if a["stride"] is None else a["stride"]
    a["nbytes"] = lib.jen1_true_peak_workspace_bytes(2, 2, 5000) if a["nbytes"] is None else a["nbytes"]
    t = a["taps"]
    tp = None if t is None else np.ascontiguousarray(t, dtype=np.float64).ctypes.data_as(L.C.POINTER(L.C.c_double))
    return lib.jen1_true_peak(a["x"], a["env"], a["stride"], a["peak"], tp, a["F"], a["rows"], a["C"], a["L"], a["work"], a["nbytes"], None)


def _limiter_call(lib, **kw):
    a = dict(x=FAKE, y=FAKE + 0x100000, ys=None, red=FAKE, rs=None, env=FAKE, es=None, window=FAKE, rows=2, C=2, L=5000, A=72, c=0.89, rho=0.999,
             work=FAKE, nbytes=None)
    a.update(kw)
    a["ys"] = a["C"] * a["L"] + 5 if a["ys"] is None else a["ys"]
    a["rs"] = a["L"] + 3 if a["rs"] is None else a["rs"]
    a["es"] = a["L"] + 3 if a["es"] is None else a["es"]
    a["nbytes"] = lib.jen1_limiter_workspace_bytes(2, 5000, 72) if a["nbytes"] is None else a["nbytes"]
    return lib.jen1_limit_true_peak(a["x"], a["y"], a["ys"], a["red"], a["rs"], a["env"], a["es"], a["window"], a["rows"], a["C"], a["L"], a["A"],
                                    a["c"], a["rho"], a["work"], a["nbytes"], None)


def _refused(lib, call, bad, word, who):
    assert call(lib, **bad) != 0, bad
    msg = lib.jen1_last_error().decode()
    assert word in msg and who in msg, (bad, msg)


def test_c_entry_points_refuse_bad_arguments():
    lib = L.load()
    cap = lib.jen1_limiter_max_lookahead()
    nan_taps = audio.true_peak_filter(48000)[1].copy()
    nan_taps[2, 5] = math.nan
    for bad, word in [(dict(C=3), "C = 3"), (dict(C=0), "C = 0"), (dict(F=3), "F = 3"), (dict(F=0), "F = 0"), (dict(rows=-1), "bad shape"),
                      (dict(L=0), "bad shape"), (dict(x=None), "null"), (dict(peak=None), "null"), (dict(work=None), "null"), (dict(taps=None), "null"),
                      (dict(stride=4999), "env_stride"), (dict(env=FAKE + 4), "aligned"), (dict(peak=FAKE + 4), "aligned"),
                      (dict(taps=nan_taps), "taps[37]"), (dict(nbytes=8), "workspace")]:
        _refused(lib, _meter_call, bad, word, "jen1_true_peak")
    assert _meter_call(lib, rows=0) == 0 and _meter_call(lib, rows=0, env=None, stride=0) == 0 and _meter_call(lib, rows=0, F=1, taps=None) == 0
    for bad, word in [(dict(C=3), "C = 3"), (dict(rows=-1), "bad shape"), (dict(L=0), "bad shape"), (dict(A=-1), "A = -1"), (dict(A=cap + 1), f"A = {cap + 1}"),
                      (dict(c=0.0), "ceiling"), (dict(c=-1.0), "ceiling"), (dict(c=math.inf), "ceiling"), (dict(c=math.nan), "ceiling"),
                      (dict(rho=1.0), "rho"), (dict(rho=-0.1), "rho"), (dict(rho=math.nan), "rho"), (dict(x=None), "null"), (dict(y=None), "null"),
                      (dict(env=None), "null"), (dict(window=None), "null"), (dict(work=None), "null"), (dict(ys=9999), "y_stride"),
                      (dict(y=FAKE, ys=10005), "in place"), (dict(es=4999), "env_stride"), (dict(rs=4999), "red_stride"),
                      (dict(env=FAKE + 4), "aligned"), (dict(window=FAKE + 4), "aligned"), (dict(red=FAKE + 4), "aligned"),
                      (dict(nbytes=lib.jen1_limiter_workspace_bytes(2, 5000, 72) - 8), "workspace")]:
        _refused(lib, _limiter_call, bad, word, "jen1_limit_true_peak")
    assert _limiter_call(lib, rows=0) == 0 and _limiter_call(lib, rows=0, red=None, rs=0) == 0 and _limiter_call(lib, rows=0, y=FAKE, ys=10000) == 0
    assert _limiter_call(lib, rows=0, A=cap, nbytes=1 << 30) == 0 and _limiter_call(lib, rows=0, A=0, rho=0.0) == 0


# ------------------------------------------------------------------ the interpolator
@pytest.mark.parametrize("sr,F", [(44100, 4), (48000, 4), (79999, 4), (80000, 2), (96000, 2), (159999, 2), (160000, 1), (192000, 1), (8000, 4)])
def test_factor_rule_and_table(sr, F):
    assert audio.true_peak_factor(sr) == F == O.factor(sr)
    got_F, taps = audio.true_peak_filter(sr)
    assert got_F == F and taps.shape == (F - 1, 16) and taps.dtype == np.float64 and audio.TRUE_PEAK_TAPS == O.TAPS == 16
    if F > 1:
        assert float(np.abs(taps - O.phases(F)).max()) <= 1e-15
    h, want = audio.true_peak_prototype(F), O.prototype(F)
    assert h.shape == (16 * F + 1,) and float(np.abs(h - want).max()) <= 1e-15
    assert np.array_equal(h, h[::-1]) and np.array_equal(want, want[::-1]), "h is symmetric"
    assert h[8 * F] == 1.0 and float(np.abs(np.delete(h[::F], 8)).max()) <= 1e-16, "phase 0 is the identity"
    for p in range(1, F):
        assert np.array_equal(taps[p - 1], h[p:p + 16 * F:F]) and np.array_equal(taps[p - 1], taps[F - 1 - p][::-1]), "phase p mirrors phase F - p"
        assert abs(float(taps[p - 1].sum()) - 1.0) <= 2e-3, "unity gain at DC"


def test_attack_window():
    for A in (0, 1, 2, 72, audio.max_lookahead()):
        w = audio.attack_window(A)
        assert w.shape == (A + 1,) and w.dtype == np.float64 and bool((w > 0).all()) and abs(float(w.sum()) - 1.0) <= 1e-15
        assert float(np.abs(w - O.window(A)).max()) <= 1e-15 and float(np.abs(w - w[::-1]).max()) <= 1e-15
    assert audio.attack_window(0)[0] == 1.0


# ------------------------------------------------------------------ refusals in Python
def test_argument_errors():
    x = torch.zeros((2, 4800))
    cap = audio.max_lookahead()
    for fn in (audio.true_peak, audio.limit_true_peak):
        with pytest.raises(ValueError, match="one or two channels"):
            fn(torch.zeros((3, 4800)), 48000)
        with pytest.raises(ValueError, match="channel and a time axis"):
            fn(torch.zeros((4800,)), 48000)
        with pytest.raises(TypeError, match="float32"):
            fn(x.double(), 48000)
        with pytest.raises(ValueError, match="positive"):
            fn(x, 0)
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros((2, 0)), 48000)
    over = (cap + 1) * 1000.0 / 48000
    for call in (lambda **kw: audio.limit_true_peak(x, 48000, **kw), lambda **kw: audio.normalize_audio(x, 48000, limit="truepeak", **kw)):
        with pytest.raises(ValueError, match="lookahead_ms"):
            call(lookahead_ms=-1.0)
        with pytest.raises(ValueError, match="lookahead_ms"):
            call(lookahead_ms=math.nan)
        with pytest.raises(ValueError, match=f"{cap} samples at most"):
            call(lookahead_ms=over)
        with pytest.raises(ValueError, match="release_ms"):
            call(release_ms=-0.5)
        with pytest.raises(ValueError, match="release_ms"):
            call(release_ms=math.inf)
        for bad in (math.nan, math.inf, -math.inf):
            with pytest.raises(ValueError, match="ceiling_dbtp"):
                call(ceiling_dbtp=bad)
    assert audio.limiter_plan(48000, -1.0, cap * 1000.0 / 48000, 100.0)[1] == cap, "the cap itself is accepted"
    c, A, rho = audio.limiter_plan(48000, -1.0, 1.5, 100.0)
    assert A == 72 == O.lookahead(1.5, 48000) and c == 10.0 ** (-1.0 / 20.0) and rho == math.exp(-1.0 / 4800.0) == O.rho_of(100.0, 48000)
    assert audio.limiter_plan(44100, 0.0, 0.0, 0.0) == (1.0, 0, 0.0) and audio.limiter_plan(44100, 0.0, 1.5, 1.0)[1] == 66
    # the other limits do not read the new keywords
    with pytest.raises(L.Jen1HipError, match="no CPU fallback"):
        audio.normalize_audio(x, 48000, limit="clip", lookahead_ms=-1.0, device="cpu")
    with pytest.raises(ValueError, match="limit"):
        audio.normalize_audio(x, 48000, limit="soft")


def test_there_is_no_cpu_fallback():
    x = torch.zeros((2, 4800))
    for call in (lambda: audio.true_peak(x, 48000, device="cpu"), lambda: audio.limit_true_peak(x, 48000, device="cpu"),
                 lambda: audio.normalize_audio(x, 48000, limit="truepeak", device="cpu")):
        with pytest.raises(L.Jen1HipError, match="no CPU fallback"):
            call()


def test_keywords_and_defaults():
    assert audio.LIMITS == ("none", "clip", "tanh", "truepeak")
    p = inspect.signature(audio.limit_true_peak).parameters
    assert [(k, p[k].default) for k in list(p)[2:]] == [("ceiling_dbtp", -1.0), ("lookahead_ms", 1.5), ("release_ms", 100.0), ("device", "cuda"),
                                                       ("return_reduction", False)]
    assert inspect.signature(audio.true_peak).parameters["device"].default == "cuda"
    from jen1_amd.dataset import LatentCollate
    from jen1_amd.generation import Jen1, save_audio_tensor
    for fn in (audio.normalize_audio, Jen1.generate, save_audio_tensor):
        q = inspect.signature(fn).parameters
        assert [q[k].default for k in ("limit", "ceiling_dbtp", "lookahead_ms", "release_ms")] == ["clip", -1.0, 1.5, 100.0], fn.__qualname__
    assert "ceiling_dbtp" not in inspect.signature(LatentCollate.__init__).parameters, "the collate keeps its hard-wired clip"


def test_generate_refuses_before_it_touches_a_device():
    from jen1_amd.generation import Jen1

    class Enc:
        channels = 2
    j = Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda md, dev: {}, model_config=tiny_model_config())
    with pytest.raises(ValueError, match="lookahead_ms"):
        j.generate("y", normalize="loudness", limit="truepeak", lookahead_ms=-1.0)
    with pytest.raises(ValueError, match="ceiling_dbtp"):
        j.generate("y", normalize="loudness", limit="truepeak", ceiling_dbtp=math.nan)
    with pytest.raises(ValueError, match="samples at most"):       # 5 ms fit at the model's 48 kHz and not at the 192 kHz the caller receives
        j.generate("y", normalize="loudness", limit="truepeak", lookahead_ms=5.0, output_sr=192000)
    with pytest.raises(ValueError, match="limit"):
        j.generate("y", normalize="peak", limit="soft")


# ------------------------------------------------------------------ the oracle on known answers
def test_oracle_pieces():
    """the oversampler against the polyphase formula of the issue, the hold against its definition, the release against a scalar loop"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 50))
    for F in (2, 4):
        o, h = O.oversample(x, F), O.phases(F)
        xp = np.concatenate([np.zeros((2, 16)), x, np.zeros((2, 16))], axis=1)
        for n in (0, 1, 7, 8, 25, 42, 49):
            assert np.array_equal(o[:, n * F], x[:, n])
            for p in range(1, F):
                want = sum(h[p - 1][k] * xp[:, 16 + n + 8 - k] for k in range(16))
                assert float(np.abs(o[:, n * F + p] - want).max()) <= 1e-14
    q = rng.random((1, 40))
    for A in (0, 1, 5):
        Q = O.hold(q, A)
        assert Q.shape == (1, 40 + A)
        for i in range(-A, 40):
            assert Q[0, i + A] == q[0, max(i, 0):min(i + A, 39) + 1].max()
    d, s = O.release(q, 0.9)[0], 0.0
    for i in range(40):
        s = max(q[0, i], 0.9 * s)
        assert d[i] == s
    assert np.array_equal(O.release(q, 0.0), q)


def test_oracle_tones():
    """a full-scale tone at fs / 4 sampled 45 degrees off its crests shows -3.01 dBFS in its samples and 0 dBTP between them"""
    quarter = O.faded_tone(12000.0, math.pi / 4)
    assert abs(float(O.db(np.abs(quarter).max())) + 3.0103) <= 1e-3
    tp = O.true_peak(quarter[None], 48000)
    print(f"fs/4 at 45 degrees: {tp:+.4f} dBTP")
    assert abs(tp) <= 0.005
    tp = O.true_peak(O.faded_tone(997.0)[None], 48000)
    print(f"997 Hz: {tp:+.6f} dBTP")
    assert abs(tp) <= 0.001
    assert O.true_peak(np.zeros((2, 100)), 48000) == -math.inf


def test_oracle_overshoot():
    """the limited signal, read again by the same meter, stays within 0.01 dB of the ceiling: the gain moves slowly against the 16 taps"""
    sig = O.loud_signals()
    for name, u in (("uniform noise 12 dB over", sig[0:1]), ("Gaussian noise", sig[1:2]), ("50 Hz + 15 kHz", sig[2:3]), ("stereo", sig[0:2])):
        before = O.true_peak(u, 48000)
        y, g, env = O.limit(u, 48000, ceiling_dbtp=-1.0, A=72, release_ms=100.0)
        after = O.true_peak(y, 48000)
        print(f"{name}: {before:+.3f} dBTP -> {after:+.5f} dBTP (ceiling -1)")
        assert before > 3.0 and after <= -1.0 + 0.01 and after >= -1.5
        c = 10.0 ** (-1.0 / 20.0)
        assert float(g.min()) >= 0.0 and float(g.max()) <= 1.0
        with np.errstate(divide="ignore"):
            assert bool(np.all(1.0 - g <= np.minimum(1.0, c / env) * (1.0 + 1e-14))), "s <= min(1, c / env)"
        assert float(np.abs(y).max()) <= c * (1.0 + 2.0 ** -23)
    quiet = (sig[0:2] * np.float32(0.01))
    y, g, _ = O.limit(quiet, 48000)
    assert np.array_equal(y, quiet) and not g.any(), "a row under the ceiling comes back bit for bit"
