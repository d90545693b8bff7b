"""-m gpu: the true-peak meter and the look-ahead limiter (csrc/limiter.hip: jen1_true_peak, jen1_limit_true_peak) against the float64
oracle of tests/limiter_common.py, and their place in ``audio.true_peak`` / ``audio.limit_true_peak`` / ``audio.normalize_audio``,
``Jen1.generate`` and ``save_audio_tensor``.

Every signal is at most 2.5 tiles + 37 samples long, a tile taken from the library's own query (2048 samples: 5157).  Outputs lie
between guard bands of a sentinel and their rows have a padded pitch; the pads must come back untouched.  The oracle's envelope is
formed once per rate and shared; its release loop runs once per parameter set over all rows at once.

Bounds.  Envelope and peak: 1e-12 max(1, peak) -- float64 sums of at most 16 products that differ from the oracle's only in order.
Reduction 1 - s: 1e-12.  Output: 2^-23 |y_ref| + 1e-12 |u| (one rounding to float32 of a product whose factor is good to 1e-12).
Measured on an MI355X (the figures the tests print): see DESIGN.md section 10k."""
import contextlib
import math

import numpy as np
import pytest
import torch

import limiter_common as O

from jen1_amd import synth
from jen1_amd.config import GDMConfig, tiny_model_config

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PAD = 37


@pytest.fixture(scope="module")
def audio():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import audio as A
    return A


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import lib as L
    L.build()
    return L.load()


def long_length(lib):
    return (5 * lib.jen1_true_peak_tile()) // 2 + 37


def taps_pointer(sr):
    import ctypes
    F = O.factor(sr)
    taps = np.ascontiguousarray(O.phases(F).reshape(-1)) if F > 1 else np.zeros(1)
    return F, taps, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def call_meter(lib, x, sr, want_env=True):
    """jen1_true_peak on x [rows, C, L] (numpy float32): env with a row pitch of L + 5 and peak carved out of one float64 buffer full of a
    sentinel.  Returns env [rows, L] (or None), peak [rows] (numpy) and whether the guard bands and the pitch pads are intact"""
    rows, C, n = x.shape
    pitch = n + 5
    ne = rows * pitch
    buf = torch.full((PAD + ne + PAD + rows + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    env, peak = buf[PAD:PAD + ne], buf[PAD + ne + PAD:PAD + ne + PAD + rows]
    nbytes = lib.jen1_true_peak_workspace_bytes(rows, C, n)
    assert nbytes > 0
    work = torch.full((nbytes // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    xd = torch.from_numpy(np.array(x)).cuda()
    F, keep, tp = taps_pointer(sr)
    rc = lib.jen1_true_peak(xd.data_ptr(), env.data_ptr() if want_env else None, pitch, peak.data_ptr(), tp, F, rows, C, n, work.data_ptr(), nbytes,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    e = host[PAD:PAD + ne].reshape(rows, pitch)
    guards = np.concatenate([host[:PAD], host[PAD + ne:PAD + ne + PAD], host[PAD + ne + PAD + rows:], e[:, n:].reshape(-1)])
    if not want_env:
        guards = np.concatenate([guards, e.reshape(-1)])
    return (e[:, :n].copy() if want_env else None), host[PAD + ne + PAD:PAD + ne + PAD + rows].copy(), bool((guards == SENTINEL).all())


def call_limiter(lib, u, env, A, c, rho, want_red=True, in_place=False):
    """jen1_limit_true_peak on u [rows, C, L] (numpy float32) and env [rows, L] (numpy float64): y with a row pitch of C L + 3 (C L in
    place) and 1 - s with one of L + 5, each between guard bands.  Returns y, 1 - s (or None) and whether guards and pads are intact"""
    rows, C, n = u.shape
    yp, rp = (C * n if in_place else C * n + 3), n + 5
    ybuf = torch.full((PAD + rows * yp + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    rbuf = torch.full((PAD + rows * rp + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    y, red = ybuf[PAD:PAD + rows * yp], rbuf[PAD:PAD + rows * rp]
    ud = torch.from_numpy(np.array(u)).cuda()
    if in_place:
        y.copy_(ud.reshape(-1))
    ed = torch.from_numpy(np.array(env)).cuda()
    wd = torch.from_numpy(O.window(A)).cuda()
    nbytes = lib.jen1_limiter_workspace_bytes(rows, n, A)
    assert nbytes > 0
    work = torch.full((nbytes // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.jen1_limit_true_peak(y.data_ptr() if in_place else ud.data_ptr(), y.data_ptr(), yp, red.data_ptr() if want_red else None, rp,
                                  ed.data_ptr(), n, wd.data_ptr(), rows, C, n, A, c, rho, work.data_ptr(), nbytes,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    yh, rh = ybuf.cpu().numpy(), rbuf.cpu().numpy()
    yr, rr = yh[PAD:PAD + rows * yp].reshape(rows, yp), rh[PAD:PAD + rows * rp].reshape(rows, rp)
    guards = [yh[:PAD], yh[PAD + rows * yp:], yr[:, C * n:].reshape(-1), rh[:PAD], rh[PAD + rows * rp:], rr[:, n:].reshape(-1)]
    if not want_red:
        guards.append(rr.reshape(-1))
    intact = all(bool((g == SENTINEL).all()) for g in guards)
    return yr[:, :C * n].reshape(rows, C, n).copy(), (rr[:, :n].copy() if want_red else None), intact


# ------------------------------------------------------------------ 1. the meter against the oracle
_METER = {}


def meter_rows(lib, sr):
    """x float32 [6, L] (rows of 3 x 2 channels, or 3 x 1 from the first three) at three levels, and the oracle's per-channel envelopes"""
    if sr not in _METER:
        rng = np.random.default_rng(sr)
        x = ((rng.random((6, long_length(lib))) * 2.0 - 1.0) * np.array([1.0, 3.0, 0.01, 0.5, 2.0, 0.02])[:, None]).astype(np.float32)
        F = O.factor(sr)
        chan = np.abs(O.oversample(x, F)).reshape(6, -1, F).max(axis=2)
        x.setflags(write=False)
        chan.setflags(write=False)
        _METER[sr] = (x, chan)
    return _METER[sr]


def meter_case(lib, sr, C, n):
    x6, chan = meter_rows(lib, sr)
    if n == x6.shape[1]:
        x, ref = x6[:3 * C], chan[:3 * C]
    else:                                                      # a cut changes the last 8 samples' neighbours: the oracle again
        x = x6[:3 * C, :n]
        F = O.factor(sr)
        ref = np.abs(O.oversample(x, F)).reshape(3 * C, n, F).max(axis=2)
    return np.ascontiguousarray(x.reshape(3, C, n)), ref.reshape(3, C, n).max(axis=1)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("sr", [48000, 96000, 192000])
def test_meter_against_the_oracle(lib, sr, C):
    worst = 0.0
    for n in (long_length(lib), 1, 2, 7, 8, 9, lib.jen1_true_peak_tile(), lib.jen1_true_peak_tile() + 1):
        x, ref = meter_case(lib, sr, C, n)
        env, peak, intact = call_meter(lib, x, sr)
        assert intact, f"L = {n}: the kernels wrote outside env / peak"
        bound = 1e-12 * np.maximum(1.0, ref.max(axis=1))
        err = np.abs(env - ref).max(axis=1)
        worst = max(worst, float((err / bound).max()) * 1e-12)
        assert bool((err <= bound).all()), f"L = {n}: |env - ref| = {err} (bound {bound})"
        assert bool((np.abs(peak - ref.max(axis=1)) <= bound).all()) and np.array_equal(peak, env.max(axis=1))
        sample_peak = np.abs(x.astype(np.float64)).max(axis=(1, 2))
        assert bool((peak >= sample_peak).all()) and bool((env >= np.abs(x.astype(np.float64)).max(axis=1)).all()), "never below the sample peak"
        if sr == 192000:
            assert np.array_equal(env, np.abs(x.astype(np.float64)).max(axis=1)), "F = 1: the envelope is |x|"
        elif n == long_length(lib):
            assert bool((peak > sample_peak).all()), "noise peaks between its samples"
        env2, peak2, _ = call_meter(lib, x, sr)
        assert np.array_equal(env, env2) and np.array_equal(peak, peak2), f"L = {n}: two runs differ"
        env1, peak1, ok1 = call_meter(lib, x[1:2], sr)
        assert ok1 and np.array_equal(env1[0], env[1]) and peak1[0] == peak[1], f"L = {n}: a row alone differs from the row in a batch"
        none, peak3, ok3 = call_meter(lib, x, sr, want_env=False)
        assert ok3 and none is None and np.array_equal(peak3, peak), "the peak alone: env = NULL writes nothing else"
    print(f"sr {sr}, C {C}: worst |env - ref| / max(1, peak) = {worst:.3e} (bound 1e-12)")


def test_true_peak_silence_tones_axes_and_devices(audio, lib):
    z = torch.zeros((2, 2, 1000))
    got = audio.true_peak(z, 48000)
    assert got.dtype == torch.float64 and got.shape == (2,) and got.device.type == "cpu" and bool(torch.isinf(got).all()) and bool((got < 0).all())
    quarter = torch.from_numpy(O.faded_tone(12000.0, math.pi / 4).astype(np.float32))
    low = torch.from_numpy(O.faded_tone(997.0).astype(np.float32))
    zero = torch.zeros_like(low)
    tp = audio.true_peak(torch.stack([torch.stack([quarter, quarter]), torch.stack([zero, quarter]), torch.stack([low, zero])]), 48000)
    mono = audio.true_peak(quarter[None], 48000)
    print(f"fs/4 at 45 degrees: {float(tp[0]):+.5f} dBTP (one channel {float(tp[1]):+.5f}, mono {float(mono):+.5f}); 997 Hz: {float(tp[2]):+.6f} dBTP")
    assert mono.shape == () and abs(float(tp[0])) <= 0.005 and float(tp[1]) == float(tp[0]) == float(mono) and abs(float(tp[2])) <= 0.001
    assert abs(float(20.0 * torch.log10(quarter.abs().max())) + 3.0103) <= 1e-3, "3 dB under in its samples"
    x = torch.from_numpy(meter_rows(lib, 48000)[0][:6].reshape(3, 2, -1).copy())
    base = audio.true_peak(x, 48000)
    want = np.array([O.db(meter_rows(lib, 48000)[1][2 * r:2 * r + 2].max()) for r in range(3)])
    assert float(np.abs(base.numpy() - want).max()) <= 1e-9, "1e-12 of an envelope whose peak is 0.01 at the least: 8.7e-10 dB"
    assert torch.equal(audio.true_peak(x.reshape(1, 3, 1, 2, -1), 48000), base.reshape(1, 3, 1))
    wide = torch.zeros((3, 2, 2 * x.shape[2]))
    wide[:, :, ::2] = x
    assert torch.equal(audio.true_peak(wide[:, :, ::2], 48000), base)
    on_gpu = audio.true_peak(x.cuda(), 48000)
    assert on_gpu.device.type == "cuda" and torch.equal(on_gpu.cpu(), base)
    assert float(audio.true_peak(x[0], 44100)) == float(base[0]) and float(audio.true_peak(x[0], 11)) == float(base[0]), "any positive rate"


# ------------------------------------------------------------------ 2. the limiter against the oracle
_ROWS = {}


def limiter_rows(lib, sr):
    """u float32 [9, 2, L], the oracle's envelope [9, L] and the row names.  The hold's domain is shifted by the look-ahead (sample n is
    b = n + A), so the bursts are placed for A = 72: their last sample's hold ends on the last sample of a tile (the carry between
    launches) and of the 64th chunk of a tile (the carry inside a workgroup, between two waves)"""
    if sr not in _ROWS:
        tile, chunk, n = lib.jen1_true_peak_tile(), lib.jen1_limiter_chunk(), long_length(lib)
        rng = np.random.default_rng(7 + sr)
        u = np.zeros((9, 2, n), dtype=np.float32)
        names = ["uniform noise 12 dB over", "under the ceiling", "impulse at 0", "impulse at the last sample", "impulse at tile - 1", "impulse at tile",
                 "burst before a tile boundary", "burst before a chunk boundary", "both channels, one louder"]
        u[0] = ((rng.random((2, n)) * 2.0 - 1.0) * 10.0 ** (12.0 / 20.0)).astype(np.float32)
        u[1] = ((rng.random((2, n)) * 2.0 - 1.0) * 0.2).astype(np.float32)
        for r, at in ((2, 0), (3, n - 1), (4, tile - 1), (5, tile)):
            u[r, r % 2, at] = 3.0
        for r, end in ((6, tile - 72), (7, tile + 64 * chunk - 72)):
            u[r, :, end - 16:end] = (4.0 * (rng.random((2, 16)) - 0.5) + np.array([[3.0], [-3.0]])).astype(np.float32)
        u[8] = u[0] * np.array([[0.05], [1.0]], dtype=np.float32)
        u[8, 0, tile // 2] = 9.0
        env = np.stack([O.envelope(u[r], sr) for r in range(9)])
        u.setflags(write=False)
        env.setflags(write=False)
        _ROWS[sr] = (u, env, names)
    return _ROWS[sr]


_WORST = {"red": 0.0, "y": 0.0}


@pytest.mark.parametrize("ceiling", [0.0, -6.0])
@pytest.mark.parametrize("release_ms", [0.0, 100.0])
@pytest.mark.parametrize("A", [0, 1, 72, "cap"])
@pytest.mark.parametrize("sr", [48000, 44100])
def test_limiter_against_the_oracle(lib, sr, A, release_ms, ceiling):
    A = lib.jen1_limiter_max_lookahead() if A == "cap" else A
    u, env_ref, names = limiter_rows(lib, sr)
    c, rho = 10.0 ** (ceiling / 20.0), O.rho_of(release_ms, sr)
    env, peak, intact = call_meter(lib, u, sr)
    assert intact and bool((np.abs(env - env_ref) <= 1e-12 * np.maximum(1.0, env_ref.max(axis=1, keepdims=True))).all())
    y, red, intact = call_limiter(lib, u, env, A, c, rho)
    assert intact, "the kernels wrote outside y / 1 - s"
    g_ref, d_ref = O.reduction(env_ref, c, A, rho)
    y_ref = ((1.0 - g_ref)[:, None, :] * u.astype(np.float64)).astype(np.float32)
    ud = np.abs(u.astype(np.float64))
    for r, name in enumerate(names):
        e_red = float(np.abs(red[r] - g_ref[r]).max())
        over = np.abs(y[r].astype(np.float64) - y_ref[r].astype(np.float64)) - (2.0 ** -23 * np.abs(y_ref[r].astype(np.float64)) + 1e-12 * ud[r])
        _WORST["red"] = max(_WORST["red"], e_red)
        assert e_red <= 1e-12, f"{name}: |(1 - s) - ref| = {e_red:.3e}"
        assert float(over.max()) <= 0.0, f"{name}: y misses 2^-23 |y_ref| + 1e-12 |u| by {float(over.max()):.3e}"
        assert float(red[r].min()) >= 0.0 and float(red[r].max()) <= 1.0, name
        assert float(np.abs(y[r]).max()) <= c * (1.0 + 2.0 ** -23), f"{name}: max |y| = {float(np.abs(y[r]).max())} over the ceiling {c}"
        # one gain for both channels: the bits of float32((1 - (1 - s)) * u) formed on the host from the returned reduction
        assert np.array_equal(y[r], ((1.0 - red[r])[None, :] * u[r].astype(np.float64)).astype(np.float32)), name
    assert np.array_equal(y[1], u[1]) and not red[1].any(), "a row under the ceiling comes back bit for bit"
    assert float(red[0].max()) > 0.5, "12 dB over: where the noise peaks, s <= c / env < 1 / 2"
    if release_ms > 0:                                          # the release is carried: across the tile boundary, across the chunk boundary
        tile, chunk = lib.jen1_true_peak_tile(), lib.jen1_limiter_chunk()
        for r, end in ((6, tile - 72), (7, tile + 64 * chunk - 72)):
            tail = red[r, end + 200:end + 200 + tile]
            assert float(tail.min()) > 0.3 * float(red[r].max()) > 0.0 and bool((np.diff(tail) < 0).all()), f"{names[r]}: the tail decays through the next tile"
    else:
        assert red[6].any() and not red[6, lib.jen1_true_peak_tile() - 72 + A:].any(), "no release: nothing behind the burst and its look-ahead"
    if A == 72 and release_ms > 0:
        y2, red2, _ = call_limiter(lib, u, env, A, c, rho)
        assert np.array_equal(y, y2) and np.array_equal(red, red2), "two runs differ"
        y1, red1, ok = call_limiter(lib, u[6:7], env[6:7], A, c, rho)
        assert ok and np.array_equal(y1[0], y[6]) and np.array_equal(red1[0], red[6]), "a row alone differs from the row in a batch"
        y3, none, ok = call_limiter(lib, u, env, A, c, rho, want_red=False)
        assert ok and none is None and np.array_equal(y3, y), "without the reduction: red = NULL writes nothing else"
        y4, red4, ok = call_limiter(lib, u, env, A, c, rho, in_place=True)
        assert ok and np.array_equal(y4, y) and np.array_equal(red4, red), "y == x gives the bits of the call with two buffers"
        mono_y, mono_red, ok = call_limiter(lib, u[:, :1], np.ascontiguousarray(env), A, c, rho)
        assert ok and np.array_equal(mono_y[:, 0], y[:, 0]) and np.array_equal(mono_red, red), "C = 1 on the same envelope"
    print(f"sr {sr}, A {A}, release {release_ms} ms, ceiling {ceiling} dBTP: worst |(1 - s) - ref| so far {_WORST['red']:.3e} (bound 1e-12)")


@pytest.mark.parametrize("n", [1, 2, 9, 300])
def test_limiter_on_short_rows(lib, n):
    """rows shorter than the look-ahead, than the filter and than a chunk"""
    rng = np.random.default_rng(n)
    u = ((rng.random((2, 2, n)) * 2.0 - 1.0) * 3.0).astype(np.float32)
    env_ref = np.stack([O.envelope(u[r], 48000) for r in range(2)])
    env, _, intact = call_meter(lib, u, 48000)
    assert intact and float(np.abs(env - env_ref).max()) <= 1e-12 * max(1.0, float(env_ref.max()))
    for A in (0, 72, lib.jen1_limiter_max_lookahead()):
        c, rho = 10.0 ** (-1.0 / 20.0), O.rho_of(100.0, 48000)
        y, red, intact = call_limiter(lib, u, env, A, c, rho)
        g_ref, _ = O.reduction(env_ref, c, A, rho)
        y_ref = ((1.0 - g_ref)[:, None, :] * u.astype(np.float64)).astype(np.float32)
        assert intact and float(np.abs(red - g_ref).max()) <= 1e-12
        assert bool((np.abs(y.astype(np.float64) - y_ref) <= 2.0 ** -23 * np.abs(y_ref.astype(np.float64)) + 1e-12 * np.abs(u.astype(np.float64))).all())


# ------------------------------------------------------------------ 3. audio.limit_true_peak
def test_limit_true_peak_properties(audio, lib):
    u, env_ref, names = limiter_rows(lib, 48000)
    x = torch.from_numpy(u.copy())
    y, red = audio.limit_true_peak(x, 48000, return_reduction=True)
    assert y.shape == x.shape and y.dtype == torch.float32 and red.shape == (9, x.shape[2]) and red.dtype == torch.float64 and y.device.type == "cpu"
    c = 10.0 ** (-1.0 / 20.0)
    g_ref, _ = O.reduction(env_ref, c, 72, O.rho_of(100.0, 48000))
    assert float(np.abs(red.numpy() - g_ref).max()) <= 1e-12
    assert torch.equal(y, ((1.0 - red)[:, None, :] * x.double()).float()), "both channels share one gain"
    assert float(red.min()) >= 0.0 and float(red.max()) <= 1.0 and float(y.abs().max()) <= c * (1.0 + 2.0 ** -23)
    assert torch.equal(y[1], x[1]), "under the ceiling: bit for bit"
    before, after = audio.true_peak(x, 48000), audio.true_peak(y, 48000)
    print(f"true peak before {[round(v, 3) for v in before.tolist()]}\n          after  {[round(v, 5) for v in after.tolist()]} (ceiling -1)")
    assert float(before[0]) > 12.0 and float(after[0]) <= -1.0 + 0.01, "uniform noise 12 dB over: read again, it stays within 0.01 dB of the ceiling"
    assert float(after[0]) >= -1.5 and float(after[1]) == float(before[1])
    assert torch.equal(audio.limit_true_peak(x, 48000), y)
    assert torch.equal(audio.limit_true_peak(x.reshape(3, 1, 3, 2, -1), 48000), y.reshape(3, 1, 3, 2, -1))
    on_gpu, red_gpu = audio.limit_true_peak(x.cuda(), 48000, return_reduction=True)
    assert on_gpu.device.type == "cuda" and red_gpu.device.type == "cuda" and torch.equal(on_gpu.cpu(), y) and torch.equal(red_gpu.cpu(), red)
    mono, mono_red = audio.limit_true_peak(x[0, :1], 48000, ceiling_dbtp=-3.0, lookahead_ms=0.0, release_ms=0.0, return_reduction=True)
    want, _ = O.reduction(O.envelope(u[0, :1], 48000)[None], 10.0 ** (-3.0 / 20.0), 0, 0.0)
    assert mono.shape == (1, x.shape[2]) and mono_red.shape == (x.shape[2],) and float(np.abs(mono_red.numpy() - want[0]).max()) <= 1e-12
    for sr in (96000, 192000):                                # the other two factors, through the same calls
        ys, rs = audio.limit_true_peak(x[:2], sr, return_reduction=True)
        want, _ = O.reduction(np.stack([O.envelope(u[r], sr) for r in range(2)]), c, O.lookahead(1.5, sr), O.rho_of(100.0, sr))
        assert float(np.abs(rs.numpy() - want).max()) <= 1e-12 and float(audio.true_peak(ys, sr)[0]) <= -1.0 + 0.01


def test_limiter_in_a_captured_graph(audio, lib):
    """nothing inside the calls allocates outside torch or synchronises: meter and limiter replay from one captured graph on new data"""
    from jen1_amd import graphs
    u = torch.from_numpy(limiter_rows(lib, 48000)[0][:4].copy())
    first, second = u.cuda(), (u * 0.5).flip(0).contiguous().cuda()
    want = [(audio.limit_true_peak(d, 48000, return_reduction=True), audio.true_peak(d, 48000)) for d in (first, second)]
    torch.cuda.synchronize()
    static = first.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with graphs.capture(g):
            y, red = audio.limit_true_peak(static, 48000, return_reduction=True)
            tp = audio.true_peak(static, 48000)
    torch.cuda.current_stream().wait_stream(s)
    for data, ((wy, wr), wt) in ((first, want[0]), (second, want[1]), (first, want[0])):
        static.copy_(data)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, wy) and torch.equal(red, wr) and torch.equal(tp, wt)


# ------------------------------------------------------------------ 4. normalize_audio, Jen1.generate, save_audio_tensor
def test_normalize_audio_truepeak(audio, lib):
    u = torch.from_numpy(limiter_rows(lib, 48000)[0][[0, 1, 8]].copy()).repeat(1, 1, 5) * 0.05          # 0.54 s: the loudness meter needs 0.4 s
    for kw in (dict(), dict(ceiling_dbtp=-3.0, lookahead_ms=0.5, release_ms=20.0)):
        for strategy, extra in (("loudness", dict(target_lufs=-3.0)), ("peak", dict(headroom_db=-6.0)), ("clip", dict())):
            got, g = audio.normalize_audio(u, 48000, strategy=strategy, limit="truepeak", return_gain=True, **extra, **kw)
            plain, g0 = audio.normalize_audio(u, 48000, strategy=strategy, limit="none", return_gain=True, **extra)
            assert torch.equal(g, g0) and torch.equal(got, audio.limit_true_peak(plain, 48000, **kw)), (strategy, kw)
            ceiling = kw.get("ceiling_dbtp", -1.0)
            assert float(audio.true_peak(got, 48000).max()) <= ceiling + 0.01
            if strategy != "clip":
                assert float(audio.true_peak(plain, 48000).max()) > ceiling + 1.0 and not torch.equal(got, plain), "the limiter had work to do"
    # the three old limits do not read the new keywords
    for limit in ("none", "clip", "tanh"):
        assert torch.equal(audio.normalize_audio(u, 48000, target_lufs=-3.0, limit=limit, ceiling_dbtp=-20.0, lookahead_ms=0.0, release_ms=0.0),
                           audio.normalize_audio(u, 48000, target_lufs=-3.0, limit=limit))
    on_gpu = audio.normalize_audio(u.cuda(), 48000, target_lufs=-3.0, limit="truepeak")
    assert on_gpu.device.type == "cuda" and torch.equal(on_gpu.cpu(), audio.normalize_audio(u, 48000, target_lufs=-3.0, limit="truepeak"))


HOP = 320


class _Quantizer:
    def __init__(self, n_q=4, bins=64, dim=128):
        g = torch.Generator().manual_seed(11)
        self.tables = torch.randn((n_q, bins, dim), generator=g) * 0.3

    def decode(self, codes):
        out = 0
        for q in range(codes.shape[0]):
            out = out + self.tables.to(codes.device)[q][codes[q]]
        return out.transpose(1, 2)


class StubAudioEncoder:
    """the slice of ``encodec.EncodecModel`` generation.py touches (test_gpu_loudness.py's)"""
    channels = 2
    sample_rate = 48000

    def __init__(self):
        self.quantizer = _Quantizer()

    def encode(self, audio):
        B, _, n = audio.shape
        frames = audio[:, :, : n // HOP * HOP].reshape(B, 2, n // HOP, HOP).mean(dim=(1, 3))
        base = (frames * 1000).round().long().abs() % 64
        return [(torch.stack([(base + 7 * q) % 64 for q in range(4)], dim=1), None)]

    def decoder(self, emb):
        assert emb.device.type == "cpu"
        return torch.tanh(emb[:, :2].repeat_interleave(HOP, dim=2))


@pytest.fixture(scope="module")
def jen1(audio):
    from jen1_amd.generation import Jen1
    cond = synth.conditioning(8, 300, "text_guided")
    emb = torch.from_numpy(cond["cross_attn_cond"]).cuda()
    msk = torch.from_numpy(cond["cross_attn_masks"]).cuda()

    def conditioner(batch_metadata, device):
        n = len(batch_metadata)
        return {"prompt": (emb[:n].to(device), msk[:n].to(device))}

    return Jen1(None, device="cuda", audio_encoder=StubAudioEncoder(), conditioner=conditioner, model_config=tiny_model_config(),
                diffusion_config=GDMConfig(), compute_dtype="f32")


@contextlib.contextmanager
def fixed_order(m, on):
    """the sampler's bit-reproducible mode (no float-atomic statistics), as in test_gpu_known_blend.py"""
    old = m.deterministic
    m.deterministic = bool(on)
    try:
        yield
    finally:
        m.deterministic = old


def test_generate_truepeak(jen1, audio):
    steps = 3
    _, model = jen1.get_model_and_diffusion(steps, True)
    kw = dict(seed=3, steps=steps, batch_size=2, seconds=2, use_gdm=True)
    loud = dict(normalize="loudness", target_lufs=0.0)
    with fixed_order(model, True):
        plain = jen1.generate("y", **kw)
        ignored = jen1.generate("y", limit="truepeak", ceiling_dbtp=-20.0, **kw)
        clip = jen1.generate("y", ceiling_dbtp=-20.0, lookahead_ms=0.0, release_ms=0.0, **loud, **kw)
        same_rate = jen1.generate("y", limit="truepeak", **loud, **kw)
        got = jen1.generate("y", limit="truepeak", ceiling_dbtp=-2.0, output_sr=44100, **loud, **kw)
    assert torch.equal(ignored, plain), "a limit acts with normalize alone, as before"
    assert torch.equal(clip, audio.normalize_audio(plain, 48000, target_lufs=0.0)), "the old limits do not read the new keywords"
    assert torch.equal(same_rate, audio.normalize_audio(plain, 48000, target_lufs=0.0, limit="truepeak"))
    resampled = audio.resample(audio.normalize_audio(plain, 48000, target_lufs=0.0, limit="none"), 48000, 44100)
    assert got.device == plain.device and torch.equal(got, audio.limit_true_peak(resampled, 44100, ceiling_dbtp=-2.0)), "the limiter runs last, at 44.1 kHz"
    before, after = audio.true_peak(resampled, 44100), audio.true_peak(got, 44100)
    print(f"generate at 44.1 kHz: {before.tolist()} dBTP -> {after.tolist()} dBTP (ceiling -2)")
    assert float(before.max()) > -1.5 and float(after.max()) <= -2.0 + 0.01 and not torch.equal(got, resampled), "the limiter had work to do"


def test_save_audio_tensor_truepeak(audio, lib, tmp_path):
    from jen1_amd import wav
    from jen1_amd.generation import save_audio_tensor
    u = torch.from_numpy(limiter_rows(lib, 48000)[0][0].copy()).repeat(1, 5) * 0.05
    a, b, c = (str(tmp_path / f"{k}.wav") for k in "abc")
    save_audio_tensor(u.unsqueeze(0), a, 48000, normalize="loudness", target_lufs=-3.0, limit="truepeak", ceiling_dbtp=-2.0)
    wav.save(b, audio.normalize_audio(u, 48000, target_lufs=-3.0, limit="truepeak", ceiling_dbtp=-2.0), 48000)
    save_audio_tensor(u, c, 48000, normalize="loudness", target_lufs=-3.0, limit="none")
    assert open(a, "rb").read() == open(b, "rb").read() != open(c, "rb").read()
    back, sr = wav.load(a)
    assert sr == 48000 and float(np.abs(back).max()) <= 10.0 ** (-2.0 / 20.0) + 2.0 ** -15


# ------------------------------------------------------------------ 5. argument errors (no launch)
def test_c_abi_argument_errors(lib):
    import ctypes
    rows, C, n, A = 2, 2, 3000, 72
    s = torch.cuda.current_stream().cuda_stream
    x = torch.ones((rows, C, n), device="cuda")
    fill = lambda shape, dtype=torch.float64: torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
    env, peak, red, y = fill((rows, n)), fill((rows,)), fill((rows, n)), fill((rows, C, n), torch.float32)
    nb_m, nb_l = lib.jen1_true_peak_workspace_bytes(rows, C, n), lib.jen1_limiter_workspace_bytes(rows, n, A)
    work_m, work_l = fill((nb_m // 8,)), fill((nb_l // 8,))
    window = torch.from_numpy(O.window(A)).cuda()
    F, keep, tp = taps_pointer(48000)
    meter = lambda **kw: lib.jen1_true_peak(kw.get("x", x.data_ptr()), kw.get("env", env.data_ptr()), kw.get("stride", n), kw.get("peak", peak.data_ptr()),
                                            kw.get("taps", tp), kw.get("F", F), rows, kw.get("C", C), kw.get("L", n), kw.get("work", work_m.data_ptr()),
                                            kw.get("nbytes", nb_m), s)
    for bad, word in ((dict(x=None), "null"), (dict(peak=None), "null"), (dict(taps=None), "null"), (dict(work=None), "null"), (dict(C=3), "C = 3"),
                      (dict(F=3), "F = 3"), (dict(L=0), "bad shape"), (dict(stride=n - 1), "env_stride"), (dict(nbytes=nb_m - 8), "workspace"),
                      (dict(env=env.data_ptr() + 4), "aligned")):
        assert meter(**bad) != 0, bad
        assert word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    real_env = torch.full((rows, n), 2.0, dtype=torch.float64, device="cuda")
    limiter = lambda **kw: lib.jen1_limit_true_peak(kw.get("x", x.data_ptr()), kw.get("y", y.data_ptr()), kw.get("ys", C * n), kw.get("red", red.data_ptr()),
                                                    kw.get("rs", n), kw.get("env", real_env.data_ptr()), kw.get("es", n), kw.get("window", window.data_ptr()),
                                                    rows, kw.get("C", C), n, kw.get("A", A), kw.get("c", 0.5), kw.get("rho", 0.999),
                                                    kw.get("work", work_l.data_ptr()), kw.get("nbytes", nb_l), s)
    cap = lib.jen1_limiter_max_lookahead()
    for bad, word in ((dict(x=None), "null"), (dict(y=None), "null"), (dict(env=None), "null"), (dict(window=None), "null"), (dict(work=None), "null"),
                      (dict(C=3), "C = 3"), (dict(A=-1), "A = -1"), (dict(A=cap + 1), "lookahead"), (dict(c=0.0), "ceiling"), (dict(c=math.nan), "ceiling"),
                      (dict(rho=1.0), "rho"), (dict(ys=C * n - 1), "y_stride"), (dict(rs=n - 1), "red_stride"), (dict(es=n - 1), "env_stride"),
                      (dict(nbytes=nb_l - 8), "workspace"), (dict(red=red.data_ptr() + 4), "aligned")):
        assert limiter(**bad) != 0, bad
        assert word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    torch.cuda.synchronize()
    for t in (env, peak, red, y, work_m, work_l):
        assert bool((t == SENTINEL).all()), "a refused call launched something"
    assert meter() == 0 and limiter() == 0
    torch.cuda.synchronize()
    assert bool((env >= 1.0).all()) and bool((env < 1.2).all()) and torch.equal(peak, env.amax(dim=1)), "a constant 1 reads 1 at its samples, and no less between them"
    assert bool((y == 0.25).all()) and float((red - 0.75).abs().max()) <= 1e-15, "env = 2 under a ceiling of 0.5: every sample is turned down to a quarter"
