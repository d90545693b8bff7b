"""-m gpu: the spectral kernels (csrc/spectral.hip: jen1_stft, jen1_mel, jen1_spectral_distance) against the float64 oracle of
tests/spectral_common.py, and their place in ``jen1_amd.spectral`` and ``Jen1.codec_report``.

Tolerances are not fixed numbers: for the same input every test first measures what float32 ``torch.stft`` on the CPU (and the float32
chain behind it) loses against float64, and the kernel is allowed 8x that (its butterfly order and table-rounded twiddles differ from
pocketfft's, and float32 FFT error grows with log N).  Every test prints the figures it measured; DESIGN.md section 10f records them.
No signal is longer than 0.5 s (24 000 samples)."""
import functools

import numpy as np
import pytest
import torch

import spectral_common as O

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PAD = 37
STARTS = [0, 3, 5, 0, 0, 2, 1, 1, 2]           # which of O.KINDS the first row of every case of O.SHAPES gets (the rest follow in order)
CASES = [pytest.param(i, id="-".join(str(int(v)) for v in O.SHAPES[i])) for i in range(len(O.SHAPES))]
MEL_KINDS = ("noise", "tone", "chirp", "quiet", "zeros")          # the impulse's silent frames would all sit on the floor of a log
MEL_FLOOR = 1e-14


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import spectral
    return spectral


@pytest.fixture(scope="module")
def lib():
    from jen1_amd import lib as L
    L.build()
    return L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def rotated(start):
    return tuple(O.KINDS[(start + i) % len(O.KINDS)] for i in range(len(O.KINDS)))


@functools.lru_cache(maxsize=None)
def case_data(i):
    """signals of case i, their float64 STFT and what float32 torch.stft reaches against it (complex, magnitude, power), computed once"""
    n_fft, hop, win, n, rows, center = O.SHAPES[i]
    x = O.signals(n, rows, rotated(STARTS[i]))
    s64 = O.stft_cpu(x, n_fft, hop, win, center)
    s32 = O.stft_cpu(x, n_fft, hop, win, center, torch.float32)
    figure = {0: float(O.row_error(s32, s64).max()), 1: float(O.row_error(np.abs(s32), np.abs(s64)).max()),
              2: float(O.row_error(np.abs(s32) ** 2, np.abs(s64) ** 2).max())}
    return x, s64, figure


def guarded(numel, dtype=torch.float32, pad=PAD):
    buf = torch.full((pad + numel + pad,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + numel]


def intact(buf, numel, pad=PAD):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + numel:] == SENTINEL).all())


def tables(S, n_fft, win):
    return torch.from_numpy(S.hann_window(win)).cuda(), torch.from_numpy(S.twiddle_table(n_fft)).cuda()


def call_stft(lib, S, x, n_fft, hop, win, center, kind, stride=None):
    """jen1_stft on x [rows, n] (a CUDA tensor, rows ``stride`` apart) into a sentinel-guarded buffer -> (numpy result, guards intact)"""
    rows, n = x.shape
    frames, bins = O.frames_of(n, n_fft, hop, center), n_fft // 2 + 1
    per = 2 if kind == 0 else 1
    numel = rows * bins * frames * per
    pad = PAD + 1 if kind == 0 else PAD            # complex pairs are stored as 8-byte words
    buf, out = guarded(numel, pad=pad)
    w, tw = tables(S, n_fft, win)
    rc = lib.jen1_stft(x.data_ptr(), x.stride(0) if stride is None else stride, out.data_ptr(), w.data_ptr(), tw.data_ptr(), rows, n, n_fft, hop, win,
                       int(center), kind, stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    got = got.reshape(rows, bins, frames, 2) if kind == 0 else got.reshape(rows, bins, frames)
    return (got[..., 0] + 1j * got[..., 1]).astype(np.complex64) if kind == 0 else got, intact(buf, numel, pad)


# ------------------------------------------------------------------ 1. the transform against float64
@pytest.mark.parametrize("i", CASES)
def test_stft_against_float64(lib, S, i):
    n_fft, hop, win, n, rows, center = O.SHAPES[i]
    x, s64, figure = case_data(i)
    kinds = rotated(STARTS[i])
    if (n_fft, n) == (2048, 24000):
        assert s64.shape[2] > 2 * lib.jen1_stft_tile_frames(n_fft), "the frame count must span more than two frame tiles"
    if i == 0:
        assert s64.shape[2] == 3, "an odd frame count: the last pair of frames is a lone frame"
    xd = torch.from_numpy(x).cuda()
    for kind, want in ((0, s64), (1, np.abs(s64)), (2, np.abs(s64) ** 2)):
        got, ok = call_stft(lib, S, xd, n_fft, hop, win, center, kind)
        assert ok, f"kind {kind}: the kernel wrote outside its output"
        err = O.row_error(got, want)
        bound = O.TOL_FACTOR * figure[kind]
        print(f"case {O.SHAPES[i]}, kind {kind}: max|S - S64| / max|S64| per row {[f'{e:.2e}' for e in err]}; float32 torch.stft on the CPU "
              f"{figure[kind]:.2e}, bound {bound:.2e}")
        assert figure[kind] > 0
        for r in range(rows):
            if kinds[r % len(kinds)] == "zeros":
                assert not got[r].any(), f"kind {kind}: the all-zero row {r} is not exactly zero"
            else:
                assert err[r] <= bound, (kind, r, err[r], bound)
        if kind == 0:
            api = S.stft(torch.from_numpy(x), n_fft, hop, win, center=center)
            assert api.dtype == torch.complex64 and api.device.type == "cuda" and tuple(api.shape) == s64.shape
            assert np.array_equal(api.cpu().numpy(), got)
            again, _ = call_stft(lib, S, xd, n_fft, hop, win, center, kind)
            assert np.array_equal(again, got), "two runs differ"
        else:
            api = S.spectrogram(xd, n_fft, hop, win, power=float(kind), center=center)
            assert api.dtype == torch.float32 and np.array_equal(api.cpu().numpy(), got)


def test_stft_axes_strides_and_windows(lib, S):
    """[n], [C, n] and [B, C, n]; a [B, C, n] view whose rows are further apart than n; a window given as a tensor"""
    n_fft, hop, win, n = 256, 64, 256, 1000
    x = torch.from_numpy(O.signals(n, 6, rotated(0))).cuda()
    flat = S.stft(x, n_fft, hop)
    assert torch.equal(S.stft(x.reshape(3, 2, n), n_fft, hop), flat.reshape(3, 2, 129, -1))
    assert torch.equal(S.stft(x[4], n_fft, hop), flat[4]) and S.stft(x[4], n_fft, hop).dim() == 2
    wide = torch.full((3, 2, n + 13), SENTINEL, device="cuda")
    wide[:, :, :n] = x.reshape(3, 2, n)
    view = wide[:, :, :n]
    assert view.stride() == (2 * (n + 13), n + 13, 1)
    assert torch.equal(S.stft(view, n_fft, hop), flat.reshape(3, 2, 129, -1))
    got, ok = call_stft(lib, S, wide.reshape(6, n + 13)[:, :n], n_fft, hop, win, True, 2, stride=n + 13)
    assert ok and np.array_equal(got, S.spectrogram(x, n_fft, hop).cpu().numpy())
    assert torch.equal(S.stft(x[:, ::2], n_fft, hop), S.stft(x[:, ::2].contiguous(), n_fft, hop))            # not unit stride: copied
    hann = torch.from_numpy(S.hann_window(200))
    assert torch.equal(S.stft(x, n_fft, hop, window=hann), S.stft(x, n_fft, hop, win_length=200))
    ones = S.stft(x, n_fft, hop, window=torch.ones(n_fft), center=False)
    want = torch.stft(x.cpu().double(), n_fft, hop, window=torch.ones(n_fft, dtype=torch.float64), center=False, return_complex=True).numpy()
    assert float(O.row_error(ones.cpu().numpy(), want).max()) <= 2e-6


@pytest.mark.parametrize("N,hop,n", [(256, 64, 2048), (2048, 512, 24000), (4096, 1024, 24000)])
def test_known_answers(S, N, hop, n):
    """periodic Hann, win_length = n_fft = N, frames that touch no padding: a sine at the exact bin k0 with amplitude A has magnitude A N / 4
    at k0, A N / 8 at k0 +- 1 and nothing elsewhere; a constant c has c N / 2 at bin 0 and c N / 4 at bin 1"""
    t = np.arange(n, dtype=np.float64)
    k0, A, c = 20, 0.7, 0.3
    x = np.stack([A * np.sin(2 * np.pi * k0 * t / N + 0.4), np.full(n, c)]).astype(np.float32)
    mag = S.spectrogram(torch.from_numpy(x), N, hop, N, power=1.0).cpu().numpy().astype(np.float64)
    frames = [f for f in range(mag.shape[2]) if f * hop - N // 2 >= 0 and f * hop + N // 2 <= n]
    assert len(frames) >= 3
    sine, const = mag[0][:, frames], mag[1][:, frames]
    rel = lambda got, want: float(np.abs(got / want - 1.0).max())
    figures = (rel(sine[k0], A * N / 4), rel(sine[k0 - 1], A * N / 8), rel(sine[k0 + 1], A * N / 8), rel(const[0], c * N / 2), rel(const[1], c * N / 4))
    rest = np.delete(sine, [k0 - 1, k0, k0 + 1], axis=0)
    print(f"N {N}: relative error of the five known magnitudes {[f'{v:.2e}' for v in figures]} (bound 1e-5); largest other bin of the sine "
          f"{rest.max() / (A * N):.2e} of A N (bound 1e-5)")
    assert max(figures) <= 1e-5
    assert float(rest.max()) < 1e-5 * A * N
    assert float(const[2:].max()) < 1e-5 * c * N


# ------------------------------------------------------------------ 2. mel
MEL_CASES = [(256, 64, 256, 1000, 16), (1024, 100, 480, 5000, 16), (4096, 480, 2400, 24000, 128)]


@functools.lru_cache(maxsize=None)
def mel_data(n_fft, hop, win, n):
    x = O.signals(n, len(MEL_KINDS), MEL_KINDS, seed=1)
    s64 = O.stft_cpu(x, n_fft, hop, win, True)
    s32 = O.stft_cpu(x, n_fft, hop, win, True, torch.float32)
    return x, np.abs(s64) ** 2, (np.abs(s32) ** 2).astype(np.float32)


def call_mel(lib, S, x, sr, n_fft, hop, win, n_mels, scale, norm, log, floor):
    rows, n = x.shape
    frames = O.frames_of(n, n_fft, hop, True)
    numel = rows * n_mels * frames
    buf, out = guarded(numel)
    w, tw = tables(S, n_fft, win)
    lo, hi, off, wt = S.banded(S.mel_filterbank(sr, n_fft, n_mels, mel_scale=scale, norm=norm))
    d = [torch.from_numpy(a).cuda() for a in (lo, hi, off, wt.astype(np.float32))]
    rc = lib.jen1_mel(x.data_ptr(), x.stride(0), out.data_ptr(), w.data_ptr(), tw.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                      d[3].data_ptr(), n_mels, wt.size, rows, n, n_fft, hop, win, 1, 2, (None, "log", "db").index(log), floor, stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(rows, n_mels, frames), intact(buf, numel)


@pytest.mark.parametrize("log", [None, "log", "db"])
@pytest.mark.parametrize("scale,norm", [("htk", None), ("slaney", "slaney")])
@pytest.mark.parametrize("n_fft,hop,win,n,n_mels", MEL_CASES)
def test_mel_against_float64(lib, S, n_fft, hop, win, n, n_mels, scale, norm, log):
    x, p64, p32 = mel_data(n_fft, hop, win, n)
    fb = O.filterbank64(O.SR, n_fft, n_mels, scale=scale, norm=norm)
    want = np.einsum("mk,rkt->rmt", fb, p64)
    cpu32 = np.einsum("mk,rkt->rmt", fb.astype(np.float32), p32)
    got, ok = call_mel(lib, S, torch.from_numpy(x).cuda(), O.SR, n_fft, hop, win, n_mels, scale, norm, log, MEL_FLOOR)
    assert ok, "the kernel wrote outside its output"
    zero = MEL_KINDS.index("zeros")
    live = [r for r in range(len(MEL_KINDS)) if r != zero]
    if log is None:
        assert not got[zero].any()
        fig32, err = O.row_error(cpu32[live], want[live]), O.row_error(got[live], want[live])
    else:
        keep = want[live] > 100.0 * MEL_FLOOR
        dropped = 1.0 - keep.reshape(len(live), -1).mean(axis=1)
        assert float(dropped.max()) < 0.01, f"the floor hides {dropped} of the oracle's own values"
        silent = np.float32(np.log(np.float64(np.float32(MEL_FLOOR)))) if log == "log" else np.float32(10.0 * np.log10(np.float64(np.float32(MEL_FLOOR))))
        assert np.all(got[zero] == silent), f"the all-zero row is not exactly log(floor) = {silent}"
        w64 = np.where(keep, O.apply_log(want[live], log, MEL_FLOOR), 0.0)
        fig32 = O.row_error(np.where(keep, O.apply_log(cpu32[live], log, MEL_FLOOR), 0.0), w64)
        err = O.row_error(np.where(keep, got[live], 0.0), w64)
    bound = O.TOL_FACTOR * float(fig32.max())
    print(f"mel n_fft {n_fft}, {n_mels} bands, {scale}/{norm}, log {log}: per row {[f'{e:.2e}' for e in err]} of the row maximum; float32 chain on "
          f"the CPU {float(fig32.max()):.2e}, bound {bound:.2e}")
    assert float(err.max()) <= bound
    api = S.mel_spectrogram(torch.from_numpy(x), O.SR, n_fft, hop, win, n_mels=n_mels, mel_scale=scale, norm=norm, log=log, floor=MEL_FLOOR)
    assert api.device.type == "cuda" and np.array_equal(api.cpu().numpy(), got)


def test_mel_magnitude_mode(S):
    n_fft, hop, win, n = 1024, 100, 480, 5000
    x, _, _ = mel_data(n_fft, hop, win, n)
    mag = S.spectrogram(torch.from_numpy(x), n_fft, hop, win, power=1.0).cpu().numpy().astype(np.float64)
    fb = O.filterbank64(O.SR, n_fft, 16)
    want = np.einsum("mk,rkt->rmt", fb, mag)
    got = S.mel_spectrogram(torch.from_numpy(x), O.SR, n_fft, hop, win, n_mels=16, power=1.0).cpu().numpy()
    # the banded sums alone, on the kernel's own magnitudes: weights rounded to float32 (2^-24) and a chain of K float32 fmas of positive
    # terms (K 2^-24 at the worst), K the widest band
    K = int((fb > 0).sum(axis=1).max())
    assert float(O.row_error(got, want).max()) <= (K + 1) * 2.0 ** -24


# ------------------------------------------------------------------ 3. distances
DIST_KINDS = ("noise", "tone", "chirp", "quiet", "impulse")
N_DIST = 24000


@functools.lru_cache(maxsize=None)
def pair():
    """reference [3, 2, n]: the signals without the zero row (six rows: the sixth is a second noise); test = reference + 5 % noise"""
    ref = O.signals(N_DIST, 6, DIST_KINDS, seed=2)
    rng = np.random.default_rng(77)
    test = (ref + 0.05 * np.abs(ref).max(axis=1, keepdims=True) * rng.standard_normal(ref.shape)).astype(np.float32)
    return test.reshape(3, 2, N_DIST), ref.reshape(3, 2, N_DIST)


@functools.lru_cache(maxsize=None)
def pair_spectra(n_fft, hop, win):
    test, ref = pair()
    t, r = test.reshape(6, -1), ref.reshape(6, -1)
    return tuple(O.stft_cpu(a, n_fft, hop, win, True, dt) for dt in (torch.float64, torch.float32) for a in (t, r))


def call_distance(lib, S, x, y, n_fft, hop, win, bank=None, floor=1e-5, kind=1):
    """jen1_spectral_distance on x, y [rows, n] (CUDA) -> (float64 [rows, 3] numpy, guards intact)"""
    rows, n = x.shape
    buf, out = guarded(rows * 3, torch.float64)
    w, tw = tables(S, n_fft, win)
    nbytes = lib.jen1_spectral_distance_workspace_bytes(rows, n, n_fft, hop, 1)
    assert nbytes > 0
    wbuf, work = guarded(nbytes // 8, torch.float64)
    b = [None] * 4 if bank is None else [t.data_ptr() for t in bank[:4]]
    rc = lib.jen1_spectral_distance(x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), out.data_ptr(), w.data_ptr(), tw.data_ptr(), *b,
                                    0 if bank is None else int(bank[0].numel()), 0 if bank is None else bank[4], rows, n, n_fft, hop, win, 1, kind,
                                    floor, work.data_ptr(), nbytes, stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(rows, 3).copy(), intact(buf, rows * 3) and intact(wbuf, nbytes // 8)


def test_mrstft_distance_against_float64(lib, S):
    from jen1_amd.spectral import RESOLUTIONS_48K
    assert RESOLUTIONS_48K == ((1024, 100, 480), (2048, 240, 1200), (4096, 480, 2400))
    test, ref = pair()
    floor = 1e-5
    got = S.mrstft_distance(torch.from_numpy(test), torch.from_numpy(ref), floor=floor)
    assert got["sc"].dtype == got["log_mag"].dtype == got["total"].dtype == torch.float64 and got["sc"].device.type == "cuda"
    assert tuple(got["sc"].shape) == tuple(got["log_mag"].shape) == (3, 2, 3) and tuple(got["total"].shape) == (3,)
    assert torch.equal(got["total"], (got["sc"] + got["log_mag"]).mean(dim=(1, 2)))
    for j, (n_fft, hop, win) in enumerate(RESOLUTIONS_48K):
        t64, r64, t32, r32 = pair_spectra(n_fft, hop, win)
        sc64, lm64 = O.distances(t64, r64, floor)
        sc32, lm32 = O.distances(t32, r32, floor)
        f_sc, f_lm = np.abs(sc32 / sc64 - 1.0), np.abs(lm32 / lm64 - 1.0)
        assert float(max(f_sc.max(), f_lm.max())) <= 1e-4, "the float32 chain itself is off on a row: change that row's bed, not the bound"
        e_sc = np.abs(got["sc"][..., j].cpu().numpy().reshape(6) / sc64 - 1.0)
        e_lm = np.abs(got["log_mag"][..., j].cpu().numpy().reshape(6) / lm64 - 1.0)
        print(f"n_fft {n_fft}: sc relative error per row {[f'{e:.2e}' for e in e_sc]} (float32 chain {f_sc.max():.2e}, bound {8 * f_sc.max():.2e}); "
              f"log-mag {[f'{e:.2e}' for e in e_lm]} (float32 chain {f_lm.max():.2e}, bound {8 * f_lm.max():.2e})")
        assert float(e_sc.max()) <= O.TOL_FACTOR * float(f_sc.max())
        assert float(e_lm.max()) <= O.TOL_FACTOR * float(f_lm.max())


def test_mel_distance_against_float64(S):
    test, ref = pair()
    floor = 1e-10
    got = S.mel_distance(torch.from_numpy(test), torch.from_numpy(ref), O.SR, floor=floor)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 2) and got.device.type == "cuda"
    t64, r64, t32, r32 = pair_spectra(2048, 512, 2048)
    fb = O.filterbank64(O.SR, 2048, 128)
    want, cpu32 = O.log_mel_l1(t64, r64, fb, floor), O.log_mel_l1(t32, r32, fb, floor)
    fig, err = np.abs(cpu32 / want - 1.0), np.abs(got.cpu().numpy().reshape(6) / want - 1.0)
    print(f"log-mel L1 relative error per row {[f'{e:.2e}' for e in err]} (float32 chain {fig.max():.2e}, bound {8 * fig.max():.2e})")
    assert float(fig.max()) <= 1e-4 and float(err.max()) <= O.TOL_FACTOR * float(fig.max())


def test_distance_sums_are_deterministic_and_independent_of_the_batch(lib, S):
    test, ref = pair()
    t, r = torch.from_numpy(test.reshape(6, -1)).cuda(), torch.from_numpy(ref.reshape(6, -1)).cuda()
    fb = S.banded(S.mel_filterbank(O.SR, 2048, 128))
    bank = [torch.from_numpy(a).cuda() for a in fb[:3]] + [torch.from_numpy(fb[3].astype(np.float32)).cuda(), int(fb[3].size)]
    for n_fft, hop, win, bk, kind, floor in ((1024, 100, 480, None, 1, 1e-5), (4096, 480, 2400, None, 1, 1e-5), (2048, 512, 2048, bank, 2, 1e-10)):
        four, ok = call_distance(lib, S, t[:4], r[:4], n_fft, hop, win, bk, floor, kind)
        assert ok, "the kernels wrote outside their output or workspace"
        again, _ = call_distance(lib, S, t[:4], r[:4], n_fft, hop, win, bk, floor, kind)
        assert np.array_equal(four, again), "two calls differ"
        alone, ok = call_distance(lib, S, t[2:3], r[2:3], n_fft, hop, win, bk, floor, kind)
        assert ok and np.array_equal(alone[0], four[2]), "a row's sums depend on its place in the batch"
        assert np.all(four[:, :2] > 0) and np.all(np.isfinite(four))
        same, _ = call_distance(lib, S, r[:4], r[:4], n_fft, hop, win, bk, floor, kind)
        # a signal against itself: the two halves of a packed transform round differently, so the distance is tiny, not zero
        assert np.all(same[:, 0] <= 1e-10 * same[:, 1]) and np.all(same[:, 1] > 0)
    wide = torch.full((6, N_DIST + 5), SENTINEL, device="cuda")
    wide[:, :N_DIST] = t
    strided, _ = call_distance(lib, S, wide[:, :N_DIST], r, 1024, 100, 480)
    plain, _ = call_distance(lib, S, t, r, 1024, 100, 480)
    assert np.array_equal(strided, plain)


# ------------------------------------------------------------------ 4. the report
def test_audio_report(S):
    from jen1_amd import audio
    test, ref = pair()
    t, r = torch.from_numpy(test), torch.from_numpy(ref)
    rep = S.audio_report(t, r, O.SR)
    assert sorted(rep) == ["log_mag", "log_mel_l1", "lufs_reference", "lufs_test", "mrstft_total", "sc"]
    assert all(v.device.type == "cuda" and v.dtype == torch.float64 for v in rep.values())
    d = S.mrstft_distance(t, r)
    assert torch.equal(rep["mrstft_total"], d["total"]) and torch.equal(rep["sc"], d["sc"]) and torch.equal(rep["log_mag"], d["log_mag"])
    assert torch.equal(rep["log_mel_l1"], S.mel_distance(t, r, O.SR))
    assert torch.equal(rep["lufs_test"].cpu(), audio.loudness(t, O.SR)) and torch.equal(rep["lufs_reference"].cpu(), audio.loudness(r, O.SR))
    assert tuple(rep["lufs_test"].shape) == (3,) and bool(torch.isfinite(rep["lufs_test"][0]))
    two = S.audio_report(t[1], r[1], O.SR)                     # [C, n]: a batch of one
    assert torch.equal(two["sc"], rep["sc"][1:2]) and torch.equal(two["log_mel_l1"], rep["log_mel_l1"][1:2])


def _codec():
    """a random-weight EncodecHIP, built as tests/test_gpu_codec_segments.py builds its own"""
    import codec_segments_common as CC
    from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in CC.dec_params().items()}, compute_dtype="bf16")
    enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in CC.enc_params().items()}, compute_dtype="bf16")
    return EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(CC.tables(16))), encoder=enc)


def _jen1(encoder):
    from jen1_amd.config import GDMConfig, tiny_model_config
    from jen1_amd.generation import Jen1
    return Jen1(None, device="cuda", audio_encoder=encoder, conditioner=lambda md, device: {}, model_config=tiny_model_config(),
                diffusion_config=GDMConfig(), compute_dtype="bf16")


def test_codec_report(S):
    codec = _codec()
    j = _jen1(codec)
    g = torch.Generator().manual_seed(5)
    wav = (torch.rand((1, 2, 48000), generator=g) - 0.5) * 0.4 + 0.3 * torch.sin(torch.arange(48000) * (2 * np.pi * 440.0 / 48000))
    seen = {}
    inner = codec.decode_latents
    codec.decode_latents = lambda z, counts, **kw: seen.setdefault("y", (inner(z, counts, **kw), list(counts), kw))[0]
    try:
        rep = j.codec_report(wav)
    finally:
        codec.decode_latents = inner
    y, counts, kw = seen["y"]
    assert tuple(y.shape) == (1, 2, 48000) and kw["length"] == 48000 and counts == codec.segment_frames(48000)
    want = S.audio_report(y, wav, 48000)
    assert sorted(rep) == sorted(want)
    for k in want:
        assert torch.equal(rep[k], want[k]), k
    assert bool(torch.isfinite(rep["mrstft_total"]).all()) and float(rep["mrstft_total"]) > 0
    # the same by hand: encode, decode, report (the codec's own kernels may add in another order from run to run)
    z, seg, scales = codec.encode_latents(wav.cuda())
    by_hand = S.audio_report(codec.decode_latents(z, seg, scales=scales, length=48000), wav, 48000)
    assert abs(float(by_hand["mrstft_total"]) / float(rep["mrstft_total"]) - 1.0) <= 1e-2
    half = j.codec_report(wav[0, :1, ::2].contiguous(), sr=24000)           # [C, n] mono at another rate: converted as generate converts
    assert tuple(half["sc"].shape) == (1, 2, 3)

    class Stub:
        channels, sample_rate = 2, 48000

    with pytest.raises(ValueError, match=r"needs an audio_encoder with encode_latents \(jen1_amd.encodec.EncodecHIP\)"):
        _jen1(Stub()).codec_report(wav)


# ------------------------------------------------------------------ 5. refused calls launch nothing
def test_refused_calls_launch_nothing(lib, S):
    n_fft, hop, win, n, rows = 256, 64, 256, 1000, 2
    x = torch.from_numpy(O.signals(n, rows)).cuda()
    w, tw = tables(S, n_fft, win)
    frames = O.frames_of(n, n_fft, hop, True)
    out = torch.full((rows * 129 * frames * 2,), SENTINEL, device="cuda")
    sums = torch.full((rows * 3,), SENTINEL, dtype=torch.float64, device="cuda")
    nbytes = lib.jen1_spectral_distance_workspace_bytes(rows, n, n_fft, hop, 1)
    work = torch.full((nbytes // 8,), SENTINEL, dtype=torch.float64, device="cuda")
    stft = lambda **k: lib.jen1_stft(k.get("x", x.data_ptr()), n, out.data_ptr(), k.get("w", w.data_ptr()), tw.data_ptr(), rows, n, k.get("n_fft", n_fft),
                                     k.get("hop", hop), k.get("win", win), 1, 0, stream())
    dist = lambda **k: lib.jen1_spectral_distance(x.data_ptr(), n, k.get("y", x.data_ptr()), n, sums.data_ptr(), w.data_ptr(), tw.data_ptr(), None, None,
                                                  None, None, 0, 0, rows, n, k.get("n_fft", n_fft), k.get("hop", hop), k.get("win", win), 1, 1, 1e-5,
                                                  work.data_ptr(), k.get("nbytes", nbytes), stream())
    for bad, word in ((dict(x=None), "null"), (dict(w=None), "null"), (dict(n_fft=384), "n_fft = 384"), (dict(hop=0), "hop = 0"), (dict(win=257), "win_length")):
        assert stft(**bad) != 0 and word in lib.jen1_last_error().decode(), bad
    for bad, word in ((dict(y=None), "null"), (dict(n_fft=384), "n_fft = 384"), (dict(hop=0), "hop = 0"), (dict(win=257), "win_length"),
                      (dict(nbytes=nbytes - 8), "workspace")):
        assert dist(**bad) != 0 and word in lib.jen1_last_error().decode(), bad
    torch.cuda.synchronize()
    for t in (out, sums, work):
        assert bool((t == SENTINEL).all()), "a refused call launched something"
    assert stft() == 0 and dist() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()) and not bool((sums == SENTINEL).any())
