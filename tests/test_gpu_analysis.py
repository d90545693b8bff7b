"""-m gpu: the analyser kernels (csrc/spectral.hip: jen1_music_features; csrc/analysis.hip: jen1_tempo, jen1_key) against the float64
oracle of tests/analysis_common.py, and their place in ``jen1_amd.analysis``, ``Jen1.control_report`` and ``LatentCollate``.

Features: for the same input every case first measures what the float32 CPU chain (float32 ``torch.stft``, float32 matmuls, log1p, flux)
loses against the float64 oracle, per row, and the kernel is allowed 8x that figure (its butterfly order and table-rounded twiddles
differ from pocketfft's).  Estimators: the summation-order bound F 2^-53 sum |terms| on every float64 sum, computed from the data.  Every
test prints the figures it measured; DESIGN.md section 10i records them.  All output goes into sentinel-guarded buffers.

Measured on an MI355X: onset 1.1e-7 ... 6.4e-5 of the row maximum against 1.4e-7 ... 4.9e-5 for the float32 CPU chain (at most 0.22 of
a row's bound), chroma 3.8e-8 ... 2.9e-7 against 9.2e-8 ... 7.7e-7 (at most 0.16); autocorrelation at most 0.013 of its summation
bound, tempo at most 4.0e-8 relative and correlations at most 2.7e-8 from the oracle."""
import functools

import numpy as np
import pytest
import torch

import analysis_common as A
import spectral_common as SC

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
PAD = 37
N_MELS = 40
KINDS = ("noise", "tone", "chirp", "impulse", "zeros")
PAIRS = [(256, 64), (512, 128), (1024, 256), (2048, 512), (4096, 1024)]
TILES_IN = {256: 2, 512: 2, 1024: 2, 2048: 3, 4096: 2}          # frame counts around this multiple of the tile
FPS = A.SR / 512


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import lib as L
    L.build()
    return L.load()


@pytest.fixture(scope="module")
def AN(lib):
    from jen1_amd import analysis
    return analysis


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(numel, dtype=torch.float32, pad=PAD):
    buf = torch.full((pad + numel + pad,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[pad:pad + numel]


def intact(buf, numel, pad=PAD):
    mark = torch.tensor(SENTINEL).to(buf.dtype).item()               # an int32 buffer holds the sentinel truncated
    return bool((buf[:pad] == mark).all()) and bool((buf[pad + numel:] == mark).all())


@functools.lru_cache(maxsize=None)
def tables(n_fft, n_mels=N_MELS):
    from jen1_amd import analysis, spectral
    lo, hi, off, w = spectral.banded(spectral.mel_filterbank(A.SR, n_fft, n_mels))
    return dict(window=torch.from_numpy(spectral.hann_window(n_fft)).cuda(), tw=torch.from_numpy(spectral.twiddle_table(n_fft)).cuda(),
                lo=torch.from_numpy(lo).cuda(), hi=torch.from_numpy(hi).cuda(), off=torch.from_numpy(off).cuda(),
                w=torch.from_numpy(w.astype(np.float32)).cuda(), nw=int(w.size), n_mels=n_mels,
                chroma=torch.from_numpy(analysis.chroma_filterbank(A.SR, n_fft).astype(np.float32)).cuda())


def call_features(lib, x, n_fft, hop, center, gamma=1.0, extra_stride=0):
    """jen1_music_features on x [rows, n] (numpy) with rows ``n + extra_stride`` apart -> (onset, chroma, guards intact)"""
    rows, n = x.shape
    wide = torch.full((rows, n + extra_stride), 1e30, device="cuda")
    wide[:, :n] = torch.from_numpy(x).cuda()
    frames = SC.frames_of(n, n_fft, hop, center)
    T = tables(n_fft)
    b0, onset = guarded(rows * frames)
    b1, chroma = guarded(rows * 12 * frames)
    rc = lib.jen1_music_features(wide.data_ptr(), n + extra_stride, onset.data_ptr(), chroma.data_ptr(), T["window"].data_ptr(), T["tw"].data_ptr(),
                                 T["lo"].data_ptr(), T["hi"].data_ptr(), T["off"].data_ptr(), T["w"].data_ptr(), T["n_mels"], T["nw"],
                                 T["chroma"].data_ptr(), gamma, rows, n, n_fft, hop, n_fft, int(center), stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    ok = intact(b0, rows * frames) and intact(b1, rows * 12 * frames)
    return onset.cpu().numpy().reshape(rows, frames).copy(), chroma.cpu().numpy().reshape(rows, 12, frames).copy(), ok


# ------------------------------------------------------------------ 1. features against float64
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("n_fft,hop", PAIRS)
def test_features_against_float64(lib, n_fft, hop, center):
    tile = lib.jen1_music_features_tile_frames(n_fft)
    assert tile in (7, 15, 31)
    worst = [0.0, 0.0]
    for c, delta in enumerate((-1, 0, 1)):            # the lone frame of a last tile, a full last tile, one frame into the next
        frames = TILES_IN[n_fft] * tile + delta
        n = (frames - 1) * hop + (hop // 3 if center else n_fft)
        assert SC.frames_of(n, n_fft, hop, center) == frames and n <= (48000 if n_fft == 4096 else 24000)
        rows = 1 + (c + PAIRS.index((n_fft, hop))) % 3
        start = (2 * PAIRS.index((n_fft, hop)) + c + (3 if center else 0)) % len(KINDS)
        kinds = [KINDS[(start + r) % len(KINDS)] for r in range(rows)]
        x = np.stack([SC.signal(k, n, seed=r) for r, k in enumerate(kinds)])
        want = A.features(x, A.SR, n_fft, hop, N_MELS, center=center)
        cpu32 = A.features(x, A.SR, n_fft, hop, N_MELS, center=center, dtype=torch.float32)
        onset, chroma, ok = call_features(lib, x, n_fft, hop, center, extra_stride=11)
        assert ok, "the kernel wrote outside its output"
        for name, got, w64, w32 in (("onset", onset, want[0], cpu32[0]), ("chroma", chroma, want[1], cpu32[1])):
            fig, err = SC.row_error(w32, w64), SC.row_error(got, w64)
            print(f"n_fft {n_fft}, hop {hop}, center {center}, {frames} frames, rows {kinds}: {name} per row {[f'{e:.2e}' for e in err]} of the row "
                  f"maximum; float32 chain on the CPU {[f'{e:.2e}' for e in fig]}, bound 8x")
            for r, kind in enumerate(kinds):
                if kind == "zeros" or not w64[r].any():          # silence; an impulse only ever fades from frame to frame: no flux at all
                    assert kind != "noise" and not got[r].any(), f"{name}: row {r} ({kind}) is not exactly zero"
                else:
                    assert fig[r] > 0 and np.isfinite(got[r]).all()
                    assert err[r] <= SC.TOL_FACTOR * fig[r], (name, kind, r, err[r], fig[r])
                    worst[name == "chroma"] = max(worst[name == "chroma"], err[r] / (SC.TOL_FACTOR * fig[r]))
        assert not onset[:, 0].any(), "onset[0] is 0"
    print(f"n_fft {n_fft}, center {center}: the tightest row uses {worst[0]:.2f} (onset) and {worst[1]:.2f} (chroma) of its bound")


# ------------------------------------------------------------------ 2. tile independence
@pytest.mark.parametrize("n_fft,hop", PAIRS)
def test_a_row_does_not_depend_on_the_batch(lib, n_fft, hop):
    tile = lib.jen1_music_features_tile_frames(n_fft)
    n = (2 * tile) * hop + 5
    x = np.stack([SC.signal(k, n, seed=4) for k in ("tone", "chirp", "noise")])
    three = call_features(lib, x, n_fft, hop, True, extra_stride=3)
    alone = call_features(lib, x[2:3], n_fft, hop, True)
    assert three[2] and alone[2]
    assert np.array_equal(three[0][2], alone[0][0]) and np.array_equal(three[1][2], alone[1][0]), "row 2 of 3 differs from the row alone"
    again = call_features(lib, x, n_fft, hop, True, extra_stride=3)
    assert np.array_equal(again[0], three[0]) and np.array_equal(again[1], three[1]), "two runs differ"


@pytest.mark.parametrize("n_fft,hop", PAIRS)
def test_a_frame_does_not_depend_on_its_tile(lib, n_fft, hop):
    """the same signal delayed by one hop, center = 0: frame t becomes frame t + 1, so a frame that was the first of a tile (its flux
    taken against the extra frame in front of the tile) lies in the interior of one"""
    tile = lib.jen1_music_features_tile_frames(n_fft)
    frames = 3 * tile + 1
    n = n_fft + (frames - 1) * hop
    x = SC.signal("noise", n, seed=9) + SC.signal("chirp", n, seed=9)
    delayed = np.concatenate([SC.signal("noise", hop, seed=10), x]).astype(np.float32)
    o0, c0, ok0 = call_features(lib, x[None], n_fft, hop, False)
    o1, c1, ok1 = call_features(lib, delayed[None], n_fft, hop, False)
    assert ok0 and ok1 and o0.shape[1] == frames and o1.shape[1] == frames + 1
    firsts = [t for t in range(1, frames) if t % tile == 0]
    assert len(firsts) == 3 and all((t + 1) % tile == 1 for t in firsts)
    assert all(o0[0, t] > 0 for t in firsts)
    for t in firsts:
        assert o0[0, t] == o1[0, t + 1], f"onset[{t}], first of its tile, differs from the same frame inside a tile"
    assert np.array_equal(o0[0, 1:], o1[0, 2:]) and np.array_equal(c0[0], c1[0][:, 1:]), "a frame's values depend on where its tile starts"


# ------------------------------------------------------------------ 3. jen1_tempo
@functools.lru_cache(maxsize=None)
def tempo_rows():
    """(onset float32 [R, stride] with 1e30 behind every row's valid part, frames [R], names)"""
    clicks = A.click_features().astype(np.float32)
    F = clicks.shape[1]
    rng = np.random.default_rng(11)
    rows = [(f"click{b}", clicks[i], F) for i, b in enumerate(A.BPMS)]
    rows += [("noise", np.abs(rng.standard_normal(F)).astype(np.float32), F), ("zeros", np.zeros(F, np.float32), F), ("three", clicks[2], 3),
             ("click120/200", clicks[2], 200), ("click90/301", clicks[1], 301)]
    stride = F + 13
    data = np.full((len(rows), stride), 1e30, dtype=np.float32)
    for r, (_name, o, f) in enumerate(rows):
        data[r, :f] = o[:f]
    return data, np.array([f for _n, _o, f in rows], dtype=np.int32), [n for n, _o, _f in rows]


def test_tempo_against_float64(lib, AN):
    data, frames, names = tempo_rows()
    R, stride = data.shape
    lags = lib.jen1_tempo_lags(FPS, 40.0, 240.0)
    lo, hi = A.lag_range(FPS)
    assert lags == hi - lo + 3
    d, fr = torch.from_numpy(data).cuda(), torch.from_numpy(frames).cuda()
    b0, tempo = guarded(R)
    b1, strength = guarded(R)
    b2, acf = guarded(R * lags, torch.float64)
    nbytes = lib.jen1_tempo_workspace_bytes(R, FPS, 40.0, 240.0)
    assert nbytes == R * (lags + 1) * 8
    b3, work = guarded(nbytes // 8, torch.float64)
    rc = lib.jen1_tempo(d.data_ptr(), stride, fr.data_ptr(), tempo.data_ptr(), strength.data_ptr(), acf.data_ptr(), R, FPS, 40.0, 240.0, 120.0, 1.0,
                        work.data_ptr(), nbytes, stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    assert intact(b0, R) and intact(b1, R) and intact(b2, R * lags) and intact(b3, nbytes // 8), "the kernels wrote outside their output or workspace"
    tempo, strength, acf = tempo.cpu().numpy(), strength.cpu().numpy(), acf.cpu().numpy().reshape(R, lags)
    assert np.isfinite(acf).all(), "the garbage behind frames[r] was read"
    for r, name in enumerate(names):
        F = int(frames[r])
        want = A.tempo(data[r], FPS, F)
        bound = np.array([F * 2.0 ** -53 * want["terms"][lo - 1 + i] for i in range(lags)])
        err = np.abs(acf[r] - np.array([want["acf"][lo - 1 + i] for i in range(lags)]))
        used = float((err / np.where(bound > 0, bound, 1.0)).max())
        if want["lag"] is None:
            print(f"{name}: undecided; acf uses {used:.3f} of its summation bound")
            assert name in ("zeros", "three") and tempo[r] == 0.0 and strength[r] == 0.0
        else:
            rel = abs(float(tempo[r]) / want["tempo"] - 1.0)
            print(f"{name}: tempo {tempo[r]:.4f} (oracle {want['tempo']:.4f}, {rel:.1e} relative), lag {want['lag']}, strength {strength[r]:.4f}, oracle gap "
                  f"{want['gap']:.2e}; acf uses {used:.3f} of its summation bound")
            assert want["gap"] >= 1e-6, "the input does not separate the best lag from the second best: change the input"
            assert rel <= 1e-6 and abs(float(strength[r]) / want["strength"] - 1.0) <= 1e-6
            assert abs(60.0 * FPS / float(tempo[r]) - want["lag"]) <= 0.5 + 1e-6, "the parabola's vertex lies within half a lag of the chosen lag"
        assert np.all(err <= bound), (name, used)
        assert np.all(acf[r][np.arange(lags) + lo - 1 >= F] == 0.0)
    for i, b in enumerate(A.BPMS):
        assert abs(float(tempo[i]) / b - 1.0) <= 0.04
    # the module: the same bits without the acf, frames as a sequence, a row alone
    t2, s2 = AN.tempo(d[:, :stride - 13], FPS, frames=frames.tolist())
    assert np.array_equal(t2.cpu().numpy(), tempo) and np.array_equal(s2.cpu().numpy(), strength)
    t3, s3, a3, lag0 = AN.tempo(d[4:5, :stride - 13].contiguous(), FPS, return_acf=True)
    assert lag0 == lo - 1 and float(t3[0]) == tempo[4] and np.array_equal(a3.cpu().numpy()[0], acf[4]), "a row's result depends on the batch"


# ------------------------------------------------------------------ 4. jen1_key
def test_key_against_float64(lib, AN):
    ch = A.passage_features().astype(np.float32)
    F = ch.shape[2]
    rows = [(p[0], ch[i], F, p[2]) for i, p in enumerate(A.PASSAGES)]
    rows += [("constant", np.full((12, F), 0.37, np.float32), F, -1), ("G/200", ch[1], 200, None), ("empty", ch[0], 0, -1)]
    R, stride = len(rows), F + 7
    data = np.full((R, 12, stride), 1e30, dtype=np.float32)
    for r, (_n, c, f, _k) in enumerate(rows):
        data[r, :, :f] = c[:, :f]
    frames = np.array([f for _n, _c, f, _k in rows], dtype=np.int32)
    d, fr = torch.from_numpy(data).cuda(), torch.from_numpy(frames).cuda()
    b0, key = guarded(R, torch.int32)
    b1, strength = guarded(R)
    b2, profile = guarded(R * 12, torch.float64)
    b3, corr = guarded(R * 24)
    rc = lib.jen1_key(d.data_ptr(), stride, fr.data_ptr(), key.data_ptr(), strength.data_ptr(), profile.data_ptr(), corr.data_ptr(), R, stream())
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    assert intact(b0, R) and intact(b1, R) and intact(b2, R * 12) and intact(b3, R * 24), "the kernel wrote outside its output"
    key, strength = key.cpu().numpy(), strength.cpu().numpy()
    profile, corr = profile.cpu().numpy().reshape(R, 12), corr.cpu().numpy().reshape(R, 24)
    for r, (name, _c, f, index) in enumerate(rows):
        want = A.key(data[r], f)
        bound = max(f, 1) * 2.0 ** -53 * want["terms"]
        perr = np.abs(profile[r] - want["profile"])
        cerr = float(np.abs(corr[r].astype(np.float64) - want["corr"]).max())
        print(f"{name}: key {key[r]} (oracle {want['key']}), correlation {strength[r]:.4f}, oracle gap {want['gap']}; profile uses "
              f"{float((perr / np.where(bound > 0, bound, 1.0)).max()):.3f} of its summation bound, corr {cerr:.1e} from the oracle (bound 1e-5)")
        assert np.all(perr <= bound) and cerr <= 1e-5
        assert key[r] == want["key"]
        if want["key"] < 0:
            assert index == -1 and key[r] == -1 and strength[r] == 0.0
        else:
            assert want["gap"] >= 0.01 and abs(float(strength[r]) - want["strength"]) <= 1e-5
            assert index is None or key[r] == index
    k2, s2, p2, c2 = AN.key(d[:, :, :F], frames=fr, return_profile=True)
    assert np.array_equal(k2.cpu().numpy(), key) and np.array_equal(p2.cpu().numpy(), profile) and np.array_equal(c2.cpu().numpy(), corr)
    k3, s3 = AN.key(d[1:2, :, :F])
    assert int(k3[0]) == key[1] and float(s3[0]) == strength[1], "a row's result depends on the batch"


# ------------------------------------------------------------------ 5. end to end
@functools.lru_cache(maxsize=None)
def clips():
    """float32 [3, 2, n] at 48 kHz, 4 s: the 120 BPM click track, the C-major passage, and both together; the channels differ in level"""
    click, scale = A.click_track(120), A.passage("C")
    mono = np.stack([click, scale, (scale + 0.5 * click).astype(np.float32)])
    return torch.from_numpy(np.stack([mono, 0.8 * mono], axis=1).astype(np.float32))


def test_analyze_end_to_end(AN):
    from jen1_amd import audio
    x = clips()
    for sr, wav in ((48000, x), (44100, audio.convert_audio(x.cuda(), 48000, 44100, 2))):
        res = AN.analyze(wav, sr)
        assert sorted(res) == ["key", "key_strength", "tempo", "tempo_strength"]
        assert all(v.device.type == "cuda" and tuple(v.shape) == (3,) for v in res.values())
        assert res["tempo"].dtype == torch.float32 and res["key"].dtype == torch.int32
        tempo, key = res["tempo"].cpu().numpy(), res["key"].cpu().numpy()
        print(f"sr {sr}: tempo {tempo}, key {key}, strengths {res['tempo_strength'].cpu().numpy()} {res['key_strength'].cpu().numpy()}")
        assert abs(tempo[0] / 120.0 - 1.0) <= 0.04 and key[1] == 0
        assert abs(tempo[2] / 120.0 - 1.0) <= 0.04 and key[2] == 0
    # the parts by hand give the same bits; mono [B, n] is the average of the channels; lengths keep padding out
    onset, chroma = AN.music_features(x, 48000)
    assert tuple(onset.shape) == (3, 376) and tuple(chroma.shape) == (3, 12, 376)
    res = AN.analyze(x, 48000)
    assert torch.equal(AN.tempo(onset, 48000 / 512)[0], res["tempo"]) and torch.equal(AN.key(chroma)[0], res["key"])
    want = A.features(x.numpy().mean(axis=1), 48000, 2048, 512, 128)
    assert float(SC.row_error(onset.cpu().numpy(), want[0]).max()) <= 1e-4 and float(SC.row_error(chroma.cpu().numpy(), want[1]).max()) <= 1e-4
    padded = torch.cat([x, torch.zeros((3, 2, 48000))], dim=2)
    cut = AN.analyze(padded, 48000, lengths=[x.shape[2]] * 3)
    print(f"padded by 1 s of silence, lengths given: tempo {cut['tempo'].cpu().numpy()}, key {cut['key'].cpu().numpy()}")
    assert abs(float(cut["tempo"][0]) / 120.0 - 1.0) <= 0.04 and int(cut["key"][1]) == 0
    silent = AN.analyze(torch.zeros((1, 1, 48000)), 48000)
    assert float(silent["tempo"][0]) == 0.0 and int(silent["key"][0]) == -1 and float(silent["key_strength"][0]) == 0.0


class StubEncoder:
    channels, sample_rate = 2, 48000

    def encode_latents(self, wav):
        return (wav[:, :1, ::320].repeat(1, 128, 1),)


def test_control_report_of_jen1(AN):
    from jen1_amd.config import GDMConfig, tiny_model_config
    from jen1_amd.generation import Jen1
    j = Jen1(None, device="cuda", audio_encoder=StubEncoder(), conditioner=lambda md, device: {}, model_config=tiny_model_config(),
             diffusion_config=GDMConfig(), compute_dtype="bf16")
    both = clips()[2]                                   # [C, n]: a batch of one
    rep = j.control_report(both, conditions={"tempo": 120, "key": 0})
    print(rep)
    assert rep["tempo_match"] == [True] and rep["key_match"] == [True] and rep["key_related"] == [True] and rep["key_name"] == ["C"]
    assert rep["tempo_ratio"][0] == pytest.approx(rep["tempo"][0] / 120.0)
    rep = j.control_report(both, conditions={"tempo": 60})
    assert rep["tempo_match"] == [False] and rep["tempo_match_octave"] == [True] and "key_match" not in rep
    plain = j.control_report(both[:1, ::2].contiguous(), sr=24000)           # mono at another rate: converted as generate converts
    assert "tempo_match" not in plain and abs(plain["tempo"][0] / 120.0 - 1.0) <= 0.04 and plain["key"] == [0]
    direct = AN.control_report(both[None].cuda(), 48000, tempo=120, key=0)
    assert direct["tempo"] == j.control_report(both, conditions={"tempo": 120, "key": 0})["tempo"]


def test_latent_collate_fills_missing_entries(AN):
    from jen1_amd.dataset import LatentCollate
    x = clips()
    batch = [(x[2], 48000, {"prompt": "a"}), (x[2], 48000, {"prompt": "b", "tempo": 77}), (x[1][:, :96000], 48000, {"prompt": "c"}),
             (torch.zeros((2, 48000)), 48000, {"prompt": "d"})]
    plain = LatentCollate(StubEncoder(), device="cuda", sample_duration=4)(batch)
    emb, meta = LatentCollate(StubEncoder(), device="cuda", sample_duration=4, analyze=("tempo", "key"))(batch)
    print(meta)
    assert torch.equal(emb, plain[0]) and all(m is b[2] for m, b in zip(plain[1], batch))
    assert sorted(meta[0]) == ["key", "prompt", "tempo"] and abs(meta[0]["tempo"] / 120.0 - 1.0) <= 0.04 and meta[0]["key"] == 0
    assert meta[1]["tempo"] == 77 and meta[1]["key"] == 0, "the JSON's tempo stays, the missing key is measured"
    assert meta[2]["key"] == 0 and meta[3] == {"prompt": "d"}, "a 2 s clip is measured on its own samples; silence gets no entry"
    assert batch[0][2] == {"prompt": "a"} and batch[1][2] == {"prompt": "b", "tempo": 77}, "the input dicts are not mutated"
