"""-m gpu: the inverse STFT and the phase vocoder (csrc/vocoder.hip: jen1_istft, jen1_phase_vocoder) against the float64 oracles of
tests/vocoder_common.py, the effects built on them (``jen1_amd.effects``) through the analyser and a spectral peak, and the augmentation
hook of ``LatentCollate``.

Tolerances are measured, not fixed: the inverse transform is allowed 8x (spectral_common.TOL_FACTOR) what float32 ``torch.istft`` on the
CPU loses against float64 on the same complex64 input; the vocoder is allowed 8x what the float64 oracle loses when only its magnitudes
and its result are rounded to float32, and it is fed the GPU's own complex64 spectrogram, so the comparison is about the kernel and not
about the ill-conditioned angles of near-empty bins.  No amplitude of a stretched signal is asserted: the textbook vocoder's first
frames under ``center=True`` are quieter at rates below 1.  Every test prints the figures it measured."""
import functools

import numpy as np
import pytest
import torch

import analysis_common as AC
import spectral_common as O
import vocoder_common as V

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PAD = 38            # even: complex pairs are stored as 8-byte words
ROWS = 6            # one row of every kind of O.KINDS


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


def guarded(numel, pad=PAD):
    buf = torch.full((pad + numel + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[pad:pad + numel]


def intact(buf, numel, pad=PAD):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + numel:] == SENTINEL).all())


def as_pairs(spec):
    """complex64 numpy [rows, bins, frames] -> float32 CUDA tensor [rows, bins, frames, 2]"""
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(spec.astype(np.complex64)))).contiguous().cuda()


def call_istft(lib, S, spec, n_fft, hop, win, center, length, lifted=False, slack=0):
    """jen1_istft on complex64 numpy [rows, bins, frames] into a sentinel-guarded buffer whose rows are ``length + slack`` apart ->
    (numpy [rows, length], guards and the slack between the rows intact)"""
    rows = spec.shape[0]
    stride = length + slack
    buf, out = guarded(rows * stride)
    host = np.ascontiguousarray(V.window_of(win, lifted).numpy().astype(np.float32))
    w, tw = torch.from_numpy(host).cuda(), torch.from_numpy(S.twiddle_table(n_fft)).cuda()
    x = as_pairs(spec)
    rc = lib.jen1_istft(x.data_ptr(), out.data_ptr(), stride, w.data_ptr(), host.ctypes.data, tw.data_ptr(), rows, spec.shape[2], length, n_fft, hop,
                        win, int(center), stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(rows, stride)
    return got[:, :length].copy(), intact(buf, rows * stride) and bool((got[:, length:] == SENTINEL).all())


def call_vocoder(lib, spec, n_fft, hop, rate):
    rows, bins, T = spec.shape
    J = int(lib.jen1_vocoder_frames(T, rate))
    assert J == V.vocoder_frames(T, rate)
    buf, out = guarded(rows * bins * J * 2)
    x = as_pairs(spec)
    rc = lib.jen1_phase_vocoder(x.data_ptr(), out.data_ptr(), rows, T, n_fft, hop, float(rate), stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(rows, bins, J, 2)
    return (got[..., 0] + 1j * got[..., 1]).astype(np.complex64), intact(buf, rows * bins * J * 2)


@functools.lru_cache(maxsize=None)
def spectrum(n_fft, hop, win, n, center=True, rows=ROWS):
    """the six signals (rows of O.KINDS in order: row 4 is all zero) and their complex64 spectrogram from float64 torch.stft, computed once"""
    x = O.signals(n, rows)
    return x, O.stft_cpu(x, n_fft, hop, win, center).astype(np.complex64)


def check_rows(got, want, bound, what):
    err = O.row_error(got, want)
    print(f"{what}: max|y - y64| / max|y64| per row {[f'{e:.2e}' for e in err]}, bound {bound:.2e}")
    for r in range(got.shape[0]):
        if O.KINDS[r % len(O.KINDS)] == "zeros":
            assert not got[r].any(), f"{what}: the all-zero row {r} is not exactly zero"
        else:
            assert err[r] <= bound, (what, r, err[r], bound)
    return err


# ------------------------------------------------------------------ 1. the inverse transform against float64 torch.istft
# center=False starts under w[0], which is zero for a periodic Hann, and at n_fft = 2048 its last value squared (5.5e-12) is under the
# NOLA threshold wherever the last frame stands alone: torch.istft refuses both, so these cases use the lifted window
ISTFT_CASES = [pytest.param(*s, True, None, False, id="-".join(map(str, s))) for s in V.ISTFT_SHAPES] + [
    pytest.param(256, 64, 256, 1216, False, None, True, id="center-false"),
    pytest.param(256, 64, 256, 1000, True, 700, False, id="length-shorter"),
    pytest.param(256, 64, 256, 1000, True, 1300, False, id="length-longer"),
    pytest.param(2048, 512, 2048, 24000, True, 30000, True, id="2048-length-longer"),         # its last output run holds no frame at all
]


@pytest.mark.parametrize("n_fft,hop,win,n,center,length,lifted", ISTFT_CASES)
def test_istft_against_float64(lib, S, n_fft, hop, win, n, center, length, lifted):
    x, spec = spectrum(n_fft, hop, win, n, center)
    frames = spec.shape[2]
    natural = hop * (frames - 1) + (0 if center else n_fft)
    L = natural if length is None else length
    want = V.istft_cpu(spec, n_fft, hop, win, center, L, torch.float64, lifted)
    f32 = V.istft_cpu(spec, n_fft, hop, win, center, L, torch.float32, lifted)
    figure = float(O.row_error(f32, want).max())
    assert figure > 0 and want.shape == (ROWS, L)
    run, per = lib.jen1_istft_tile_samples(n_fft), lib.jen1_istft_tile_frames(n_fft)
    if (n_fft, n, length) == (2048, 24000, None):
        assert L > 2 * run and frames > 2 * per and (run + n_fft) // hop > 2 * per, "more than two output runs and more than two frame passes"
    if n == 129:
        assert frames == 3, "a lone last frame"
    got, ok = call_istft(lib, S, spec, n_fft, hop, win, center, L, lifted, slack=5)
    assert ok, "the kernel wrote outside its rows"
    check_rows(got, want, O.TOL_FACTOR * figure, f"istft {(n_fft, hop, win, n, center, length)} (float32 torch.istft on the CPU {figure:.2e})")
    if length is not None and length > natural:
        held = n_fft + hop * (frames - 1) - (n_fft // 2 if center else 0)
        assert not got[:, held:].any() and not want[:, held:].any(), "samples past the last frame's reach are exact zeros"
        if n_fft == 2048:
            assert held <= (-(-L // run) - 1) * run, "the last run lies past every frame"
    again, _ = call_istft(lib, S, spec, n_fft, hop, win, center, L, lifted)
    assert np.array_equal(again, got), "two runs differ"
    for r in (0, 2):
        alone, ok = call_istft(lib, S, spec[r:r + 1], n_fft, hop, win, center, L, lifted)
        assert ok and np.array_equal(alone[0], got[r]), f"row {r} alone and inside the batch differ"
    if lifted:
        window = V.window_of(win, True).float()
    else:
        window = "hann"
    api = S.istft(torch.from_numpy(spec).reshape(3, 2, *spec.shape[1:]), n_fft, hop, win, window=window, center=center, length=length)
    assert api.dtype == torch.float32 and api.device.type == "cuda" and tuple(api.shape) == (3, 2, L)
    assert np.array_equal(api.cpu().numpy().reshape(ROWS, L), got)


@pytest.mark.parametrize("n_fft,hop,win,n", V.ISTFT_SHAPES)
def test_round_trip(S, n_fft, hop, win, n):
    """istft(stft(x)) against x: allowed 8x what the float32 round trip of torch on the CPU loses"""
    x = O.signals(n, ROWS)
    w32 = O.window64(win).float()
    xt = torch.from_numpy(x)
    back = torch.istft(torch.stft(xt, n_fft, hop_length=hop, win_length=win, window=w32, center=True, pad_mode="reflect", return_complex=True), n_fft,
                       hop_length=hop, win_length=win, window=w32, center=True, length=n).numpy()
    L = hop * (n // hop)                     # a sample past the last frame's centre is held by no full overlap in either implementation
    figure = float(O.row_error(back[:, :L], x[:, :L].astype(np.float64)).max())
    got = S.istft(S.stft(xt, n_fft, hop, win), n_fft, hop, win, length=n).cpu().numpy()
    assert got.shape == (ROWS, n) and figure > 0
    check_rows(got[:, :L], x[:, :L].astype(np.float64), O.TOL_FACTOR * figure, f"round trip {(n_fft, hop, win, n)} (float32 torch on the CPU {figure:.2e})")


def test_istft_refuses_nola_through_the_api(S):
    from jen1_amd.lib import Jen1HipError
    spec = torch.zeros((2, 129, 16), dtype=torch.complex64)
    with pytest.raises(Jen1HipError, match="NOLA"):
        S.istft(spec, 256, hop=256)
    with pytest.raises(Jen1HipError, match="NOLA"):
        S.istft(spec, 256, hop=64, center=False)


# ------------------------------------------------------------------ 2. the phase vocoder against the float64 oracle
def vocoder_case(lib, S, x, n_fft, hop, rate, what):
    spec = S.stft(torch.from_numpy(x), n_fft, hop).cpu().numpy()            # the GPU's own complex64 spectrogram
    want = V.phase_vocoder64(spec, rate, hop, n_fft)
    figure = float(O.row_error(V.phase_vocoder64(spec, rate, hop, n_fft, float32_magnitudes=True), want).max())
    assert figure > 0
    got, ok = call_vocoder(lib, spec, n_fft, hop, rate)
    assert ok, "the kernel wrote outside its output"
    assert got.shape == want.shape
    bound = O.TOL_FACTOR * figure
    check_rows(got, want, bound, f"vocoder {what} rate {rate:.4f} (float32 magnitudes and result alone {figure:.2e})")
    return spec, got, want, bound


@pytest.mark.parametrize("rate", V.RATES)
def test_vocoder_against_float64(lib, S, rate):
    step = lib.jen1_phase_vocoder_tile_frames()
    for n_fft, hop, n in ((256, 64, 129), (256, 64, 17000), (2048, 512, 24000)):
        x = O.signals(n, ROWS)
        spec, got, want, bound = vocoder_case(lib, S, x, n_fft, hop, rate, (n_fft, hop, n))
        T = spec.shape[2]
        if n == 129:
            assert T == 3
        if n == 17000:
            assert T > 2 * step and got.shape[2] > 2 * step, "the scan carries its sum across more than two steps at every rate"
        again, _ = call_vocoder(lib, spec, n_fft, hop, rate)
        assert np.array_equal(again, got), "two runs differ"
        alone, ok = call_vocoder(lib, spec[2:3], n_fft, hop, rate)
        assert ok and np.array_equal(alone[0], got[2]), "a row alone and inside the batch differ"
        api = S.phase_vocoder(torch.from_numpy(spec).reshape(3, 2, *spec.shape[1:]), rate, hop)
        assert api.dtype == torch.complex64 and api.device.type == "cuda" and tuple(api.shape) == (3, 2) + got.shape[1:]
        assert np.array_equal(api.cpu().numpy().reshape(got.shape), got)
        if rate == 1.0:
            check_rows(got, spec.astype(np.complex128), bound, f"vocoder {(n_fft, hop, n)} at rate 1 against its input")


@pytest.mark.parametrize("rate", [0.8, 2.0 ** (1.0 / 12.0)])
def test_vocoder_long_row(lib, S, rate):
    """3001 frames at n_fft 256, hop 64: the top bin advances by 800 rad per frame, and a float32 sum of the phase has lost it long before
    the end (4e-2 after 118 frames); the exact sum keeps the rounding of the result alone"""
    x = O.signals(192000, 1, kinds=("chirp",))
    spec, got, want, bound = vocoder_case(lib, S, x, 256, 64, rate, "long row")
    assert spec.shape[2] == 3001
    tail = slice(got.shape[2] - 64, None)
    last = float(np.abs(got[:, :, tail] - want[:, :, tail]).max() / np.abs(want).max())
    print(f"long row, rate {rate:.4f}: the last 64 frames {last:.2e} of max|Y|")
    assert last <= bound, "the last frames are as good as the first"


# ------------------------------------------------------------------ 3. properties through the public API
@pytest.fixture(scope="module")
def FX(S):
    from jen1_amd import effects
    return effects


@pytest.fixture(scope="module")
def analyze(S):
    from jen1_amd import analysis
    return analysis.analyze


def test_tempo_follows_the_stretch(FX, analyze):
    pairs = ((90, 0.8), (90, 1.25), (120, 0.9), (128, 1.1))
    for bpm, r in pairs:
        x = torch.from_numpy(AC.click_track(bpm))[None]
        y = FX.time_stretch(x, r)
        assert y.device.type == "cuda" and tuple(y.shape) == (1, int(round(x.shape[-1] / r)))
        got = float(analyze(y, AC.SR)["tempo"][0])
        print(f"click track {bpm} bpm stretched by {r}: measured {got:.2f}, expected {bpm * r:.2f}")
        assert abs(got - bpm * r) <= 0.04 * bpm * r, (bpm, r, got)


def test_key_follows_the_shift(FX, analyze):
    index = {name: key for name, _shift, key in AC.PASSAGES}
    for name, s in (("G", 2), ("Eb", 2), ("Am", -3), ("F#m", 5), ("G", 5)):
        x = torch.from_numpy(AC.passage(name))[None]
        y = FX.pitch_shift(x, AC.SR, s)
        assert tuple(y.shape) == tuple(x.shape)
        want = FX.Augment.transform_metadata({"key": index[name]}, 1.0, s)["key"]
        got = int(analyze(y, AC.SR)["key"][0])
        print(f"passage in {name} shifted by {s:+d}: measured {AC.KEY_NAMES[got] if got >= 0 else got}, expected {AC.KEY_NAMES[want]}")
        assert got == want, (name, s, got, want)


def test_a_tone_keeps_or_moves_its_frequency(FX):
    sr, n = 48000, 96000
    x = torch.from_numpy((0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)).astype(np.float32))
    assert abs(V.peak_hz(x.numpy(), sr) - 1000.0) <= 0.1
    for r in (0.8, 1.25):
        y = FX.time_stretch(x, r)
        assert tuple(y.shape) == (int(round(n / r)),)
        f = V.peak_hz(y.cpu().numpy(), sr)
        print(f"1 kHz tone stretched by {r}: peak at {f:.3f} Hz")
        assert abs(f - 1000.0) <= 1.0, (r, f)
    for s in (-2, 3):
        ratio = FX.semitone_ratio(s)
        y = FX.pitch_shift(x, sr, s)
        assert tuple(y.shape) == (n,)
        f = V.peak_hz(y.cpu().numpy(), sr)
        print(f"1 kHz tone shifted by {s:+d} semitones ({ratio}): peak at {f:.3f} Hz, expected {1000.0 * float(ratio):.3f}")
        assert abs(f - 1000.0 * float(ratio)) <= 1e-3 * 1000.0 * float(ratio), (s, f)
    both = FX.stretch_and_shift(x.reshape(1, 1, n).expand(2, 2, n), sr, rate=1.25, semitones=3)
    assert tuple(both.shape) == (2, 2, int(round(n / 1.25))) and torch.equal(both[0, 0], both[1, 1])
    assert abs(V.peak_hz(both[0, 0].cpu().numpy(), sr) - 1000.0 * float(FX.semitone_ratio(3))) <= 1e-3 * 1000.0 * float(FX.semitone_ratio(3))
    assert FX.stretch_and_shift(x, sr) is x


# ------------------------------------------------------------------ 4. the augmentation hook of LatentCollate
@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import encodec_common as EC
    import rvq_encode_common as RC
    from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in EC.dec_params().items()}, compute_dtype="f32")
    enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in EC.enc_params().items()}, compute_dtype="f32")
    return EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(RC.golden_tables(16))), encoder=enc)


def test_latent_collate_augments_on_the_gpu(FX, codec):
    from jen1_amd.dataset import LatentCollate
    clips = [AC.click_track(120, 2.0), AC.passage("G", 2.0), AC.click_track(90, 2.0), AC.passage("Am", 2.0)]
    metas = [{"prompt": "a", "tempo": 120.0}, {"prompt": "b", "key": 7}, {"prompt": "c"}, {"prompt": "d", "tempo": 100.0, "key": 21}]
    batch = [(torch.from_numpy(c)[None].repeat(2, 1), 48000, dict(m)) for c, m in zip(clips, metas)]
    kw = dict(tempo_rates=(0.9, 1.1), semitones=(-2, 2), seed=1)
    twin = FX.Augment(**kw)
    draws = [twin.draw() for _ in batch]
    fed = []
    inner = codec.encode_latents
    codec.encode_latents = lambda a: (fed.append(a.clone()), inner(a))[1]
    try:
        plain = LatentCollate(codec, "cuda", sample_duration=2)(batch)
        emb, meta, lengths = LatentCollate(codec, "cuda", sample_duration=2, augment=FX.Augment(**kw), analyze=("tempo", "key"), with_lengths=True)(batch)
    finally:
        del codec.encode_latents
    assert emb.shape == plain[0].shape and emb.dtype == plain[0].dtype and len(fed) == 2 and fed[1].shape == fed[0].shape == (4, 2, 96000)
    counter = LatentCollate(codec, "cuda", sample_duration=2)
    for i, (rate, semis) in enumerate(draws):
        assert rate in (0.9, 1.1) and semis in (-2, 2)
        valid = min(96000, int(round(96000 / rate)))
        assert lengths[i] == counter.valid_frames(valid, 96000, emb.shape[-1]), (i, rate, lengths[i])
        by_hand = FX.stretch_and_shift(fed[0][i:i + 1], 48000, rate=rate, semitones=semis)
        n = min(96000, by_hand.shape[-1])
        assert torch.equal(fed[1][i, :, :n], by_hand[0, :, :n]) and not fed[1][i, :, n:].any(), "the clip the encoder gets is the by-hand effect, padded"
        want = FX.Augment.transform_metadata(metas[i], rate, semis)
        for name in ("tempo", "key"):
            if name in metas[i]:
                assert meta[i][name] == want[name], (i, name, meta[i], want)
        assert meta[i]["prompt"] == metas[i]["prompt"]
    assert batch[0][2] == metas[0] and batch[3][2] == metas[3], "the input dicts are not mutated"
    print(f"draws {draws}, metadata {meta}, latent lengths {lengths}")
    # measured entries are what the analyser finds in the augmented audio itself, with the augmented valid lengths; nothing is transformed
    from jen1_amd import analysis
    valid = [min(96000, int(round(96000 / rate))) for rate, _s in draws]
    measured = analysis.analyze(fed[1], 48000, lengths=valid)
    for i, md in enumerate(metas):
        bpm, key = float(measured["tempo"][i]), int(measured["key"][i])
        if "tempo" not in md:
            assert meta[i].get("tempo") == (bpm if bpm > 0 else None), (i, meta[i], bpm)
        if "key" not in md:
            assert meta[i].get("key") == (key if key >= 0 else None), (i, meta[i], key)
