"""-m gpu: the loudness meter and normaliser (csrc/loudness.hip: jen1_kweight_energy, jen1_loudness_gate, jen1_gain_apply) against the
float64 oracle of tests/loudness_common.py, and their place in ``audio.loudness`` / ``audio.normalize_audio``, ``Jen1.generate`` and
``LatentCollate``.

The reference filter runs once over all signals (``loudness_common.bank``); a signal cut to its first L samples is checked against the
first L samples of that pass (the filter is causal).  Those signals are at most 2 s at 48 kHz; at 8 kHz the one length that must cover
2.5 staging tiles of the kernel is 4 s, because a tile is counted in samples (32 087 of them).  The known-answer tones are the 5 s the
answers were computed for; the one reference pass over them (under a second) serves the check of their distance from the gates.

Measured on an MI355X (the figures the tests print): see DESIGN.md section 10e."""
import contextlib
import math

import numpy as np
import pytest
import torch

import loudness_common as O

from jen1_amd import synth
from jen1_amd.config import GDMConfig, tiny_model_config

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PAD = 37
RATES = (48000, 8000)


@pytest.fixture(scope="module")
def audio():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import audio as A
    return A


@pytest.fixture(scope="module")
def lib():
    from jen1_amd import lib as L
    L.build()
    return L.load()


def long_length(lib, sr):
    """at least 2.5 staging tiles of chunks (the library's own rules) and a tail that ends inside a chunk and inside a hop"""
    hop = sr // 10
    N, T = lib.jen1_kweight_chunk(hop), lib.jen1_kweight_tile_chunks(hop)
    L = (5 * T * N) // 2 + N // 2 + 37
    assert L % N != 0 and L % hop != 0 and L >= 2.5 * T * N
    return L


@pytest.fixture(scope="module")
def bank(lib):
    return O.bank({sr: long_length(lib, sr) for sr in RATES})


def coef_array(sr):
    import ctypes
    sos = O.coefficients(sr)
    return (ctypes.c_double * 10)(*sos[0, [0, 1, 2, 4, 5]], *sos[1, [0, 1, 2, 4, 5]])


def call_energy(lib, x, sr):
    """jen1_kweight_energy on x [rows, C, L] (numpy float32) with e and stats carved out of one float64 buffer full of a sentinel:
    returns e [rows, C, H], stats [rows, 2] (numpy) and whether the three guard bands are intact"""
    rows, C, L = x.shape
    hop = sr // 10
    H = L // hop
    ne, ns = rows * C * H, rows * 2
    buf = torch.full((PAD + ne + PAD + ns + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    e, stats = buf[PAD:PAD + ne], buf[PAD + ne + PAD:PAD + ne + PAD + ns]
    nbytes = lib.jen1_kweight_energy_workspace_bytes(rows, C, L, hop)
    assert nbytes > 0
    work = torch.full((nbytes // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rc = lib.jen1_kweight_energy(xd.data_ptr(), e.data_ptr(), stats.data_ptr(), coef_array(sr), rows, C, L, hop, work.data_ptr(), nbytes,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    guards = np.concatenate([host[:PAD], host[PAD + ne:PAD + ne + PAD], host[PAD + ne + PAD + ns:]])
    return host[PAD:PAD + ne].reshape(rows, C, H).copy(), host[PAD + ne + PAD:PAD + ne + PAD + ns].reshape(rows, 2).copy(), bool((guards == SENTINEL).all())


def energy_ratio(e, e_ref, x, hop):
    """worst |e - e_ref| / max(e_ref, 1e-6 hop max|x|^2) over the hops, max|x| per channel: the test's bound is 1e-8 of that"""
    if e_ref.size == 0:
        return 0.0
    floor = 1e-6 * hop * (np.abs(x.astype(np.float64)).max(axis=-1, keepdims=True) ** 2)
    return float((np.abs(e - e_ref) / np.maximum(e_ref, floor)).max())


def check_stats(stats, x):
    """sum of x^2 within n 2^-53 of the float64 sum (n positive terms, one rounding per add), max |x| exactly"""
    xd = x.astype(np.float64).reshape(x.shape[0], -1)
    want = (xd ** 2).sum(axis=1)
    assert np.all(np.abs(stats[:, 0] - want) <= xd.shape[1] * 2.0 ** -53 * want + 1e-300), (stats[:, 0], want)
    assert np.array_equal(stats[:, 1], np.abs(xd).max(axis=1))


# ------------------------------------------------------------------ 1. energies against the oracle
_WORST = {"ratio": 0.0}


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("sr", RATES)
def test_energies_against_the_oracle(lib, bank, sr, rows, C):
    hop = sr // 10
    base, y = bank[("base", sr)]
    lengths = [1, hop - 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 5 * hop + 37, long_length(lib, sr)]
    assert lengths[-1] <= base.shape[1]
    for kind, first in (("uniform", 0), ("quiet middle", 6)):
        for L in lengths:
            x = base[first:first + rows * C, :L].reshape(rows, C, L)
            e_ref = O.hop_energies(y[first:first + rows * C, :L], hop).reshape(rows, C, L // hop)
            e, stats, intact = call_energy(lib, x, sr)
            assert intact, f"{kind}, L = {L}: the kernels wrote outside e / stats"
            r = energy_ratio(e, e_ref, x, hop)
            _WORST["ratio"] = max(_WORST["ratio"], r)
            assert r <= 1e-8, f"{kind}, L = {L}: |e - e_ref| is {r:.3e} of max(e_ref, 1e-6 hop max|x|^2)"
            check_stats(stats, x)
            if L in (5 * hop + 37, lengths[-1]):
                e2, stats2, _ = call_energy(lib, x, sr)
                assert np.array_equal(e, e2) and np.array_equal(stats, stats2), f"{kind}, L = {L}: two runs differ"
    print(f"sr {sr}, rows {rows}, C {C}: worst |e - e_ref| / max(e_ref, floor) so far {_WORST['ratio']:.3e} (bound 1e-8)")


# ------------------------------------------------------------------ 2. the carry
def test_the_state_is_carried_across_chunks(lib, bank):
    """an impulse at sample 0 and a constant 0.5, 2 s each: everything behind the first chunk is the filter's memory.  A kernel that
    restarted chunks from zero state would return 0 behind the impulse's chunk and a transient of order 0.25 hop in every chunk of
    the constant."""
    sr, hop = 48000, 4800
    x2, y = bank["carry"]
    x = x2.reshape(2, 1, -1)
    e_ref = O.hop_energies(y, hop).reshape(2, 1, -1)
    e, stats, intact = call_energy(lib, x, sr)
    assert intact
    r = energy_ratio(e, e_ref, x, hop)
    print(f"impulse / constant: |e - e_ref| is {r:.3e} of max(e_ref, floor) (bound 1e-8)")
    assert r <= 1e-8
    check_stats(stats, x)
    # the ringing of the high-pass (a double pole at radius 0.995: e^-24 per hop) is far below the floor of the bound above, so here it
    # is checked RELATIVE to itself over the hops whose energy is still a normal float64.  Behind the impulse both sides are homogeneous
    # float64 recurrences whose rounding errors decay with the signal; through a (nearly) double pole they grow like n^2 2^-53 / 6 at
    # the worst, 3e-8 at n = 9 hops (two forms of the filter differ by 3e-10 there on a CPU), and the kernel also puts the state through
    # 40 products with A^N per hop, whose entries nearly cancel.  This is a check of the ORDER of the ringing, not of accuracy (that is the
    # bound above): 1e-3, where a restart gives exactly 0 and a carry off by one sample per chunk changes the decay by r^40 = 18 % per hop.
    # Measured: 1.2e-6 at hop 8.
    tail, tail_ref = e[0, 0, 1:9], e_ref[0, 0, 1:9]
    assert np.all(tail_ref > 1e-200) and np.all(tail > 0)
    rel = float(np.abs(tail / tail_ref - 1.0).max())
    print(f"impulse, hops 1..8 (energies {tail_ref[0]:.3e} .. {tail_ref[-1]:.3e}): worst relative error {rel:.3e}")
    assert rel <= 1e-3
    assert e[1, 0, 0] > 1.0 and float(e[1, 0, 1:].max()) < 1e-6               # the constant is filtered away after the first hop


# ------------------------------------------------------------------ 3. the gate
def gate_cases():
    hop = 4800
    loud = np.concatenate([np.full(10, 1e-9), np.full(4, 0.1), np.full(16, 1e-5)]) * hop
    stripes = np.where((np.arange(300) // 40) % 2 == 0, 0.1, 1e-4) * hop
    return hop, {
        "H = 0": np.zeros((2, 0)), "H = 3": np.full((2, 3), 0.01 * hop), "H = 4": np.full((1, 4), 0.01 * hop),
        "H = 5": np.array([[0.01, 0.02, 0.005, 0.01, 0.03]]) * hop, "zeros": np.zeros((2, 20)),
        "one loud block among quiet ones": loud[None], "the same, split over two channels": np.stack([0.3 * loud, 0.7 * loud]),
        "more blocks than threads": np.stack([stripes, 0.5 * stripes]),
    }


def call_gate(lib, e, hop):
    rows, C, H = e.shape
    ed = torch.from_numpy(np.ascontiguousarray(e)).cuda()
    out = torch.full((PAD + rows + PAD,), SENTINEL, dtype=torch.float64, device="cuda")
    rc = lib.jen1_loudness_gate(ed.data_ptr() if H else None, out[PAD:].data_ptr(), rows, C, H, hop, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.all(host[:PAD] == SENTINEL) and np.all(host[PAD + rows:] == SENTINEL)
    return host[PAD:PAD + rows]


def test_gate_on_hand_made_energies(lib):
    hop, cases = gate_cases()
    got = {}
    for name, e in cases.items():
        assert O.gate_margin(e, hop) >= 0.1 and O.gate_margin(0.5 * e, hop) >= 0.1, f"{name}: a block within 0.1 LU of a threshold"
        rows = np.stack([e, 0.5 * e])                                          # a second row 3.01 LU down: rows are independent
        got[name] = call_gate(lib, rows, hop)
        for r in range(2):
            want = O.gate(rows[r], hop)
            if math.isinf(want):
                assert got[name][r] == -np.inf, (name, r, got[name][r])
            else:
                assert abs(got[name][r] - want) <= 1e-9, (name, r, got[name][r], want)
    assert got["H = 0"][0] == got["H = 3"][0] == got["zeros"][0] == -np.inf
    assert abs(got["H = 4"][0] - (-0.691 - 20.0)) <= 1e-9
    assert abs(got["one loud block among quiet ones"][0] - got["the same, split over two channels"][0]) <= 1e-9
    _, l, gamma = O.gate(cases["one loud block among quiet ones"], hop, details=True)
    assert (l <= O.ABSOLUTE_GATE).any() and ((l > O.ABSOLUTE_GATE) & (l <= gamma)).any() and (l > gamma).any()     # both gates drop blocks


# ------------------------------------------------------------------ 4. audio.loudness
def test_loudness_known_answers(audio):
    k = O.kat_energies()
    for name in ("tone23", "tone0", "gating"):
        assert O.gate_margin(np.stack([k[name], k[name]]), 4800) >= 5.0 and O.gate_margin(k[name][None], 4800) >= 5.0
    t23 = torch.from_numpy(O.tone(10 ** (-23 / 20)).astype(np.float32))
    t0 = torch.from_numpy(O.tone(1.0).astype(np.float32))
    g = torch.from_numpy(O.gating_signal().astype(np.float32))
    z = torch.zeros_like(t23)
    stereo = audio.loudness(torch.stack([torch.stack([t23, t23]), torch.stack([t23, z]), torch.stack([z, t0]), torch.stack([g, g])]), 48000)
    mono = audio.loudness(t23[None], 48000)
    print(f"tone at -23 dBFS: stereo {float(stereo[0]):.5f}, one channel {float(stereo[1]):.5f}, mono {float(mono):.5f}; full scale in one "
          f"channel {float(stereo[2]):.5f}; gating signal {float(stereo[3]):.5f}")
    assert stereo.dtype == torch.float64 and stereo.shape == (4,) and mono.shape == () and stereo.device.type == "cpu"
    assert abs(float(stereo[0]) + 23.0) <= 0.01
    assert abs(float(stereo[1]) + 26.0103) <= 1e-3 and abs(float(mono) + 26.0103) <= 1e-3
    assert abs(float(stereo[2]) + 3.0103) <= 1e-3
    assert abs(float(stereo[3]) + 20.6037) <= 1e-3


def test_loudness_axes_strides_devices_and_short_input(audio, bank):
    sr, hop = 48000, 4800
    base, y = bank[("base", sr)]
    L = 5 * hop + 37
    x = torch.from_numpy(base[:12, :L].reshape(6, 2, L).copy())
    e_ref = O.hop_energies(y[:12, :L], hop).reshape(6, 2, -1)
    want = np.array([O.gate(e_ref[r], hop) for r in range(6)])
    assert all(O.gate_margin(e_ref[r], hop) >= 0.1 for r in range(6))
    got = audio.loudness(x, sr)
    # energies within 1e-8 move a loudness by at most 10 log10(1 + 1e-8) = 4.4e-8 LU
    assert got.shape == (6,) and float(np.abs(got.numpy() - want).max()) <= 1e-7
    assert torch.equal(audio.loudness(x.reshape(1, 3, 2, 2, L), sr), got.reshape(1, 3, 2))
    wide = torch.zeros((6, 2, 2 * L))
    wide[:, :, ::2] = x
    assert torch.equal(audio.loudness(wide[:, :, ::2], sr), got)
    on_gpu = audio.loudness(x.cuda(), sr)
    assert on_gpu.device.type == "cuda" and torch.equal(on_gpu.cpu(), got)
    mono = audio.loudness(x[:, :1], sr)
    assert float(np.abs(mono.numpy() - np.array([O.gate(e_ref[r, :1], hop) for r in range(6)])).max()) <= 1e-7
    short = audio.loudness(x[:, :, :4 * hop - 1], sr)
    assert bool(torch.isinf(short).all()) and bool((short < 0).all())
    assert float(audio.loudness(x[0, :, :1], sr)) == -math.inf


# ------------------------------------------------------------------ 5. normalize_audio
@pytest.fixture(scope="module")
def rows4(bank):
    """[4, 2, L]: a row, a row 12 dB down, a row below the energy floor (2^-10: powers of two scale the reference exactly), zeros"""
    sr, hop = 48000, 4800
    base, y = bank[("base", sr)]
    L = 5 * hop + 37
    scale = np.array([1.0, 0.25, 2.0 ** -10, 0.0])
    x = np.zeros((4, 2, L), dtype=np.float32)
    e = np.zeros((4, 2, L // hop))
    for r in range(3):
        x[r] = base[2 * r:2 * r + 2, :L] * np.float32(scale[r])
        e[r] = O.hop_energies(y[2 * r:2 * r + 2, :L], hop) * scale[r] ** 2
    lufs = [O.gate(e[r], hop) for r in range(4)]
    assert all(O.gate_margin(e[r], hop) >= 0.1 for r in range(3)) and lufs[3] == -math.inf
    assert math.sqrt(float((x[2].astype(np.float64) ** 2).mean())) < 2e-3 < math.sqrt(float((x[1].astype(np.float64) ** 2).mean()))
    return torch.from_numpy(x), lufs


def host_limit(p, limit):
    return p.clamp(-1.0, 1.0) if limit == "clip" else p


@pytest.mark.parametrize("strategy", ["loudness", "peak", "rms", "clip"])
def test_normalize_gain_and_bits(audio, rows4, strategy):
    """the gain against the oracle's to 1e-7 (one rounding to float32, 6e-8, on top of a meter that is good to 1e-8), and the output the
    bits of clamp(float32(g) * x) formed on the host from the returned gain"""
    x, lufs = rows4
    for limit, target in (("none", -14.0), ("clip", 0.0), ("clip", -14.0)):
        y, g = audio.normalize_audio(x, 48000, strategy=strategy, target_lufs=target, limit=limit, return_gain=True)
        assert y.shape == x.shape and y.dtype == torch.float32 and g.shape == (4,) and g.dtype == torch.float32 and y.device.type == "cpu"
        for r in range(4):
            want = O.gain(strategy, x[r].numpy(), lufs=lufs[r], target=target)
            assert abs(float(g[r]) - want) <= 1e-7 * want, (strategy, r, float(g[r]), want)
        assert torch.equal(y, host_limit(g[:, None, None] * x, limit)), (strategy, limit, target)
    if strategy == "loudness":
        assert float(g[2]) == 1.0 and float(g[3]) == 1.0 and torch.equal(y[2:], x[2:])              # below the floor, and silence: bit for bit
        assert float(g[0]) != 1.0 and float(g[1]) != 1.0
        big = audio.normalize_audio(x, 48000, target_lufs=0.0, limit="none")
        assert float(big.abs().max()) > 1.0 and float(audio.normalize_audio(x, 48000, target_lufs=0.0).abs().max()) == 1.0     # the clamp does work
    if strategy in ("peak", "rms"):
        assert float(g[3]) == 1.0 and torch.equal(y[3], x[3]) and float(g[2]) > 100.0
        y2, g2 = audio.normalize_audio(x, 48000, strategy=strategy, headroom_db=6.0, limit="none", return_gain=True)
        for r in range(3):
            want = O.gain(strategy, x[r].numpy(), headroom_db=6.0)
            assert abs(float(g2[r]) - want) <= 1e-7 * want
    if strategy == "clip":
        assert torch.equal(g, torch.ones(4)) and torch.equal(y, x.clamp(-1.0, 1.0))


def test_normalize_tanh_limit(audio, rows4):
    x, _ = rows4
    y, g = audio.normalize_audio(x, 48000, target_lufs=0.0, limit="tanh", return_gain=True)
    p = (g[:, None, None] * x).numpy()
    assert float(np.abs(p).max()) > 1.0
    err = float(np.abs(y.numpy().astype(np.float64) - np.tanh(p.astype(np.float64))).max())
    print(f"tanh limiter: max |y - tanh(g x)| = {err:.3e} (bound 1e-6)")
    assert err <= 1e-6 and float(y.abs().max()) <= 1.0


def test_normalize_per_row_targets_leading_axes_and_round_trip(audio, rows4):
    x, lufs = rows4
    targets = torch.tensor([-14.0, -20.0, -30.0, -9.0], dtype=torch.float64)
    y, g = audio.normalize_audio(x, 48000, target_lufs=targets, limit="none", return_gain=True)
    for r in range(2):
        want = O.gain("loudness", x[r].numpy(), lufs=lufs[r], target=float(targets[r]))
        assert abs(float(g[r]) - want) <= 1e-7 * want
    assert torch.equal(y, g[:, None, None] * x)
    y22, g22 = audio.normalize_audio(x.reshape(2, 2, 2, -1), 48000, target_lufs=targets.reshape(2, 2), limit="none", return_gain=True)
    assert torch.equal(y22, y.reshape(2, 2, 2, -1)) and torch.equal(g22, g.reshape(2, 2))
    on_gpu = audio.normalize_audio(x.cuda(), 48000, target_lufs=targets.cuda(), limit="none")
    assert on_gpu.device.type == "cuda" and torch.equal(on_gpu.cpu(), y)
    back = audio.loudness(audio.normalize_audio(x[:2], 48000, limit="none", target_lufs=-30.0), 48000)
    print(f"loudness of the audio normalised to -30 LUFS: {back.tolist()}")
    assert float((back + 30.0).abs().max()) <= 1e-3


def test_gain_apply_in_place(audio, lib, rows4):
    """y == x at the C ABI: the bits of the call with two buffers; odd row lengths put every row at another alignment"""
    x, _ = rows4
    for L in (x.shape[2], 4801, 3):
        src = x[:, :, :L].contiguous().cuda()
        lufs = torch.tensor([-20.0, -30.0, -math.inf, -25.0], dtype=torch.float64, device="cuda")
        stats = torch.stack([(src.double() ** 2).sum(dim=(1, 2)), src.abs().amax(dim=(1, 2)).double()], dim=1).contiguous()
        target = torch.full((4,), -14.0, dtype=torch.float64, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        out, g = torch.full_like(src, SENTINEL), torch.empty(4, device="cuda")
        assert lib.jen1_gain_apply(src.data_ptr(), out.data_ptr(), g.data_ptr(), lufs.data_ptr(), stats.data_ptr(), target.data_ptr(), 4, 2, L,
                                   0, 1, 0.0, 2e-3, s) == 0, lib.jen1_last_error()
        buf = torch.full((PAD + src.numel() + PAD,), SENTINEL, device="cuda")
        inplace = buf[PAD:PAD + src.numel()]
        inplace.copy_(src.reshape(-1))
        g2 = torch.empty(4, device="cuda")
        assert lib.jen1_gain_apply(inplace.data_ptr(), inplace.data_ptr(), g2.data_ptr(), lufs.data_ptr(), stats.data_ptr(), target.data_ptr(), 4, 2,
                                   L, 0, 1, 0.0, 2e-3, s) == 0, lib.jen1_last_error()
        torch.cuda.synchronize()
        assert torch.equal(inplace.view_as(out), out) and torch.equal(g, g2)
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + src.numel():] == SENTINEL).all())
        assert torch.equal(out.cpu(), (g.cpu()[:, None, None] * x[:, :, :L]).clamp(-1.0, 1.0))
        assert float(g[2]) == 1.0 and float(g[3]) == 1.0               # -inf, and a silent row


def test_normalize_in_a_captured_graph(audio, rows4):
    """nothing inside the calls allocates outside torch or synchronises: meter, gate and gain replay from one captured graph on new data"""
    from jen1_amd import graphs
    x, _ = rows4
    first, second = x.cuda(), (x * 0.5).flip(0).contiguous().cuda()
    want = [audio.normalize_audio(d, 48000, target_lufs=-20.0, return_gain=True) for d in (first, second)]
    torch.cuda.synchronize()
    static = first.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with graphs.capture(g):
            y, gain = audio.normalize_audio(static, 48000, target_lufs=-20.0, return_gain=True)
    torch.cuda.current_stream().wait_stream(s)
    for data, (wy, wg) in ((first, want[0]), (second, want[1]), (first, want[0])):
        static.copy_(data)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, wy) and torch.equal(gain, wg)


# ------------------------------------------------------------------ 6. Jen1.generate
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
    """the slice of ``encodec.EncodecModel`` generation.py touches (test_gpu_audio.py's)"""
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


def test_generate_normalize(jen1, audio):
    steps = 3
    _, model = jen1.get_model_and_diffusion(steps, True)
    kw = dict(seed=3, steps=steps, batch_size=2, seconds=2, use_gdm=True)
    with fixed_order(model, True):
        plain = jen1.generate("y", **kw)
        off = jen1.generate("y", normalize=None, **kw)
        loud = jen1.generate("y", normalize="loudness", **kw)
        tanh = jen1.generate("y", normalize="loudness", target_lufs=-20.0, limit="tanh", output_sr=44100, **kw)
    assert torch.equal(off, plain)
    want, g = audio.normalize_audio(plain, 48000, return_gain=True)
    assert bool((g != 1.0).all()) and loud.device == plain.device and torch.equal(loud, want)
    assert abs(float(audio.loudness(audio.normalize_audio(plain, 48000, limit="none"), 48000)[0]) + 14.0) <= 1e-3
    assert torch.equal(tanh, audio.resample(audio.normalize_audio(plain, 48000, target_lufs=-20.0, limit="tanh"), 48000, 44100))


def test_generate_target_input(jen1, audio):
    """music_cont with ``target_lufs="input"``: every row is brought to the measured loudness of the converted prefix"""
    B, seconds, steps = 2, 2, 3
    prefix = torch.rand((1, 24000), generator=torch.Generator().manual_seed(4)) * 0.2 - 0.1            # 1 s at 24 kHz, mono
    _, model = jen1.get_model_and_diffusion(steps, True)
    kw = dict(seed=3, steps=steps, batch_size=B, seconds=seconds, use_gdm=True, task="music_cont", init_audio=prefix, init_audio_sr=24000)
    with fixed_order(model, True):
        plain = jen1.generate("y", **kw)
        got = jen1.generate("y", normalize="loudness", target_lufs="input", limit="none", **kw)
    converted = audio.convert_audio(prefix.unsqueeze(0).expand(B, -1, -1), 24000, 48000, 2)
    target = audio.loudness(converted, 48000)
    assert target.shape == (B,) and bool(torch.isfinite(target).all())
    assert torch.equal(got, audio.normalize_audio(plain, 48000, target_lufs=target, limit="none"))
    assert float((audio.loudness(got, 48000) - target).abs().max()) <= 1e-3


# ------------------------------------------------------------------ 7. LatentCollate
class RecordingEncoder:
    """``encode_latents`` of a codec, reduced to something cheap that depends on every sample: frame means as latents"""
    sample_rate = 48000
    channels = 2

    def __init__(self):
        self.seen = []

    def encode_latents(self, wav):
        self.seen.append(wav.clone())
        B, C, n = wav.shape
        return wav[:, :, :n // HOP * HOP].reshape(B, C, n // HOP, HOP).mean(dim=3), None, None


def test_latent_collate_normalize(audio):
    from jen1_amd.dataset import LatentCollate
    g = torch.Generator().manual_seed(8)
    batch = [(torch.rand((2, 48000), generator=g) * 0.1 - 0.05, 48000, {"i": 0}), (torch.rand((1, 12000), generator=g) - 0.5, 24000, {"i": 1}),
             (torch.zeros((2, 30000)), 48000, {"i": 2})]
    enc = RecordingEncoder()
    plain, meta = LatentCollate(enc, "cuda", sample_duration=1)(batch)
    same, _ = LatentCollate(enc, "cuda", sample_duration=1, normalize=None)(batch)
    loud, meta2 = LatentCollate(enc, "cuda", sample_duration=1, normalize="loudness", target_lufs=-20.0)(batch)
    assert meta == meta2 == [{"i": 0}, {"i": 1}, {"i": 2}]
    assert torch.equal(enc.seen[0], enc.seen[1]) and torch.equal(plain, same)                       # the default is unchanged
    by_hand = audio.normalize_audio(enc.seen[0], 48000, strategy="loudness", target_lufs=-20.0, limit="clip")
    assert torch.equal(enc.seen[2], by_hand) and torch.equal(loud, enc.encode_latents(by_hand)[0])
    assert not torch.equal(enc.seen[2][:2], enc.seen[0][:2]) and torch.equal(enc.seen[2][2], enc.seen[0][2])     # silence stays silence
    level = audio.loudness(enc.seen[2][:1], 48000)
    assert abs(float(level) + 20.0) <= 1e-3


# ------------------------------------------------------------------ 8. argument errors (no launch)
def test_c_abi_argument_errors(lib):
    sr, hop, rows, C, L = 48000, 4800, 2, 2, 2 * 4800 + 5
    s = torch.cuda.current_stream().cuda_stream
    x = torch.zeros((rows, C, L), device="cuda")
    e = torch.full((rows, C, 2), SENTINEL, dtype=torch.float64, device="cuda")
    stats = torch.full((rows, 2), SENTINEL, dtype=torch.float64, device="cuda")
    nbytes = lib.jen1_kweight_energy_workspace_bytes(rows, C, L, hop)
    work = torch.full((nbytes // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    coef = coef_array(sr)
    energy = lambda **kw: lib.jen1_kweight_energy(kw.get("x", x.data_ptr()), kw.get("e", e.data_ptr()), stats.data_ptr(), kw.get("coef", coef), rows,
                                                  kw.get("C", C), L, kw.get("hop", hop), kw.get("work", work.data_ptr()), kw.get("nbytes", nbytes), s)
    for bad, word in ((dict(x=None), "null"), (dict(e=None), "null"), (dict(coef=None), "null"), (dict(work=None), "null"), (dict(C=3), "C = 3"),
                      (dict(hop=0), "hop"), (dict(hop=-4800), "hop"), (dict(nbytes=nbytes - 8), "workspace")):
        assert energy(**bad) != 0, bad
        assert word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    lufs = torch.full((rows,), SENTINEL, dtype=torch.float64, device="cuda")
    gate = lambda **kw: lib.jen1_loudness_gate(kw.get("e", e.data_ptr()), kw.get("lufs", lufs.data_ptr()), rows, kw.get("C", C), 2, kw.get("hop", hop), s)
    for bad, word in ((dict(e=None), "null"), (dict(lufs=None), "null"), (dict(C=3), "C = 3"), (dict(hop=0), "hop")):
        assert gate(**bad) != 0, bad
        assert word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    y = torch.full((rows, C, L), SENTINEL, device="cuda")
    gain = torch.full((rows,), SENTINEL, device="cuda")
    target = torch.zeros((rows,), dtype=torch.float64, device="cuda")
    apply = lambda **kw: lib.jen1_gain_apply(kw.get("x", x.data_ptr()), y.data_ptr(), kw.get("gain", gain.data_ptr()), kw.get("lufs", lufs.data_ptr()),
                                             kw.get("stats", stats.data_ptr()), target.data_ptr(), rows, kw.get("C", C), L, kw.get("strategy", 0),
                                             kw.get("limit", 1), 0.0, 2e-3, s)
    for bad, word in ((dict(x=None), "null"), (dict(gain=None), "null"), (dict(lufs=None), "null"), (dict(stats=None), "null"), (dict(C=3), "C = 3"),
                      (dict(strategy=4), "strategy"), (dict(limit=3), "limit")):
        assert apply(**bad) != 0, bad
        assert word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    torch.cuda.synchronize()
    for t in (e, stats, work, lufs, y, gain):
        assert bool((t == SENTINEL).all()), "a refused call launched something"
    assert energy() == 0 and gate() == 0
    torch.cuda.synchronize()
    assert bool((e == 0).all()) and bool((stats == 0).all()) and bool(torch.isinf(lufs).all())
