"""Without a GPU: the C ABI of include/jen1_analysis.h, the host tables and arithmetic of ``jen1_amd.analysis``, the oracle of
tests/analysis_common.py on signals whose tempo and key are known, and ``LatentCollate(analyze=...)`` with a stub encoder and analyser."""
import os
import re

import numpy as np
import pytest
import torch

import analysis_common as A
from helpers import ROOT
from jen1_amd import analysis
from jen1_amd import lib as L


@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.load()


# ------------------------------------------------------------------ C ABI
def test_every_declared_symbol_is_exported(lib):
    src = open(os.path.join(ROOT, "include", "jen1_analysis.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(jen1_[a-z0-9_]+)\s*\(", src))
    assert declared == set(L.ANALYSIS_SYMBOLS), declared ^ set(L.ANALYSIS_SYMBOLS)
    assert {"jen1_music_features", "jen1_tempo", "jen1_key", "jen1_music_features_tile_frames"} <= declared
    for name in declared:
        assert getattr(lib, name) is not None
    assert "analysis.hip" in L.SOURCES


def test_host_queries(lib):
    assert [lib.jen1_music_features_tile_frames(n) for n in (256, 512, 1024, 2048, 4096, 384)] == [31, 31, 15, 7, 7, 0]
    for n_fft in (256, 512, 1024, 2048, 4096):
        tile, bands = lib.jen1_music_features_tile_frames(n_fft) + 1, lib.jen1_music_features_max_bands(n_fft)
        used = tile * (n_fft // 2 + 1) * 8 + 16 * 12 * tile * 8 + tile * bands * 4
        assert bands >= 128 and used <= 160 * 1024 < used + tile * 4, "the bands that fit are the bands 160 KiB of LDS leave room for"
    assert lib.jen1_music_features_max_bands(100) == 0
    lo, hi = A.lag_range(93.75)
    assert (lo, hi) == (24, 140) and lib.jen1_tempo_lags(93.75, 40.0, 240.0) == hi - lo + 3
    assert lib.jen1_tempo_lags(93.75, 240.0, 40.0) == 0 and lib.jen1_tempo_lags(0.0, 40.0, 240.0) == 0
    assert lib.jen1_tempo_lags(1.0, 40.0, 240.0) == 0, "a first lag below 2 is refused"
    assert lib.jen1_tempo_workspace_bytes(3, 93.75, 40.0, 240.0) == 3 * (hi - lo + 4) * 8 and lib.jen1_tempo_workspace_bytes(3, 1.0, 40.0, 240.0) == 0


def test_refusals_on_the_host(lib):
    """every argument is checked before anything is launched: these calls never reach a device"""
    p = 0x1000
    feat = lambda **k: lib.jen1_music_features(k.get("x", p), 1000, p, p, p, p, p, p, p, p, k.get("bands", 16), 100, k.get("cw", p), k.get("gamma", 1.0), 1, 1000,
                                               k.get("n_fft", 256), k.get("hop", 64), 256, 1, None)
    for bad, word in ((dict(x=None), "null"), (dict(cw=None), "null"), (dict(n_fft=384), "n_fft = 384"), (dict(hop=0), "hop = 0"), (dict(gamma=0.0), "gamma"),
                      (dict(bands=lib.jen1_music_features_max_bands(256) + 1), "fit in LDS"), (dict(bands=0), "n_bands")):
        assert feat(**bad) != 0 and word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    tempo = lambda **k: lib.jen1_tempo(k.get("o", p), k.get("stride", 100), p, p, p, None, 1, k.get("fps", 93.75), k.get("lo", 40.0), k.get("hi", 240.0),
                                       k.get("prior", 120.0), k.get("oct", 1.0), k.get("work", p), k.get("nbytes", 1 << 20), None)
    for bad, word in ((dict(o=None), "null"), (dict(stride=0), "frame_stride"), (dict(fps=0.0), "fps"), (dict(lo=300.0), "bpm range"), (dict(prior=0.0), "prior"),
                      (dict(oct=-1.0), "prior"), (dict(fps=1.0), "lags"), (dict(work=None), "workspace"),
                      (dict(nbytes=lib.jen1_tempo_workspace_bytes(1, 93.75, 40.0, 240.0) - 8), "workspace"), (dict(work=0x1004), "aligned")):
        assert tempo(**bad) != 0 and word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    key = lambda **k: lib.jen1_key(k.get("c", p), k.get("stride", 100), p, p, p, k.get("prof", p), p, 1, None)
    for bad, word in ((dict(c=None), "null"), (dict(stride=0), "frame_stride"), (dict(prof=0x1004), "aligned")):
        assert key(**bad) != 0 and word in lib.jen1_last_error().decode(), (bad, lib.jen1_last_error())
    assert lib.jen1_tempo(p, 100, p, p, p, None, 0, 93.75, 40.0, 240.0, 120.0, 1.0, p, 1 << 20, None) == 0, "no rows: nothing to do"


# ------------------------------------------------------------------ host tables
def test_chroma_filterbank():
    for n_fft in (256, 2048, 4096):
        W = analysis.chroma_filterbank(A.SR, n_fft)
        assert W.dtype == np.float64 and W.shape == (12, n_fft // 2 + 1) and np.isfinite(W).all() and (W >= 0).all()
        assert np.abs(W - A.chroma_matrix(A.SR, n_fft)).max() <= 1e-15
    bin_of = lambda f, n_fft: int(round(f * n_fft / A.SR))
    W = analysis.chroma_filterbank(A.SR, 4096)
    assert int(np.argmax(W[:, bin_of(440.0, 4096)])) == 9, "A"
    assert int(np.argmax(W[:, bin_of(261.63, 4096)])) == 0, "C"
    peak = [int(np.argmax(analysis.chroma_filterbank(A.SR, n)[:, bin_of(440.0, n)])) for n in (2048, 4096)]
    assert peak == [9, 9], "doubling n_fft keeps the class of the bin nearest 440 Hz"
    assert np.array_equal(analysis.chroma_filterbank(44100, 2048, a440=440.0), analysis.chroma_filterbank(44100, 2048))
    with pytest.raises(ValueError, match="n_fft"):
        analysis.chroma_filterbank(A.SR, 1000)
    with pytest.raises(ValueError, match="positive"):
        analysis.chroma_filterbank(0, 2048)


def test_key_names_and_profiles():
    assert len(analysis.KEY_NAMES) == 24 and list(analysis.KEY_NAMES) == A.KEY_NAMES
    assert analysis.KEY_NAMES[0] == "C" and analysis.KEY_NAMES[11] == "B" and analysis.KEY_NAMES[12] == "Cm" and analysis.KEY_NAMES[23] == "Bm"
    P = analysis.key_profiles()
    assert P.shape == (24, 12) and np.array_equal(P, A.key_table())
    assert P[0, 0] == 6.35 and P[7, 7] == 6.35 and P[7, 2] == 5.19 and P[21, 9] == 6.33 and P[21, 0] == 5.38


def test_frame_lengths():
    got = analysis.frame_lengths([0, 1, 511, 512, 48000, 99999], 48000, 2048, 512)
    assert got.dtype == np.int32 and got.tolist() == [0, 1, 1, 2, 94, 94]
    assert analysis.frame_lengths([100, 2048, 2560], 48000, 2048, 512, center=False).tolist() == [0, 1, 2]


# ------------------------------------------------------------------ the oracle on known signals
@pytest.mark.parametrize("i", range(len(A.BPMS)), ids=[str(b) for b in A.BPMS])
def test_oracle_tempo_of_click_tracks(i):
    bpm = A.BPMS[i]
    r = A.tempo(A.click_features()[i], A.SR / 512)
    print(f"{bpm} BPM: oracle {r['tempo']:.3f} ({r['tempo'] / bpm - 1.0:+.2e}), lag {r['lag']}, strength {r['strength']:.3f}, gap {r['gap']:.2e}")
    assert abs(r["tempo"] / bpm - 1.0) <= 0.04
    assert 0.0 < r["strength"] <= 1.0


@pytest.mark.parametrize("i", range(len(A.PASSAGES)), ids=[p[0] for p in A.PASSAGES])
def test_oracle_key_of_passages(i):
    name, _, index = A.PASSAGES[i]
    r = A.key(A.passage_features()[i])
    print(f"{name}: oracle key {r['key']} ({A.KEY_NAMES[r['key']]}), correlation {r['strength']:.3f}, gap {r['gap']:.3f}")
    assert r["key"] == index


def test_oracle_undecided_rows():
    fps = A.SR / 512
    assert A.tempo(np.zeros(200), fps)["tempo"] == 0.0 and A.tempo(np.zeros(200), fps)["lag"] is None
    assert A.tempo(np.arange(3.0), fps)["tempo"] == 0.0, "three frames: no candidate lag"
    assert A.key(np.ones((12, 50)))["key"] == -1 and A.key(np.ones((12, 50)))["strength"] == 0.0


# ------------------------------------------------------------------ control_report
def test_verdict_arithmetic():
    tv, kv = analysis.tempo_verdict, analysis.key_verdict
    assert tv(120.0, 120.0) == {"tempo_ratio": 1.0, "tempo_match": True, "tempo_match_octave": True}
    assert tv(124.7, 120.0)["tempo_match"] and not tv(125.0, 120.0)["tempo_match"] and not tv(115.0, 120.0)["tempo_match"]
    for factor in (2.0, 3.0, 0.5, 1.0 / 3.0):
        v = tv(120.0 * factor * 1.03, 120.0)
        assert not v["tempo_match"] and v["tempo_match_octave"], factor
        assert v["tempo_ratio"] == pytest.approx(factor * 1.03)
    assert not tv(120.0 * 1.5, 120.0)["tempo_match_octave"] and not tv(120.0 * 4, 120.0)["tempo_match_octave"]
    assert tv(0.0, 120.0) == {"tempo_ratio": 0.0, "tempo_match": False, "tempo_match_octave": False}
    with pytest.raises(ValueError, match="positive"):
        tv(120.0, 0.0)
    assert kv(0, 0) == {"key_match": True, "key_related": True}
    assert kv(21, 0) == {"key_match": False, "key_related": True}, "A minor is the relative minor of C major"
    assert kv(0, 21)["key_related"] and kv(3, 12)["key_related"], "and C major the relative major of A minor; Eb major of C minor"
    assert kv(7, 0)["key_related"] and kv(5, 0)["key_related"] and kv(16, 21)["key_related"] and kv(14, 21)["key_related"], "a fifth up or down, same mode"
    assert not kv(12, 0)["key_related"] and not kv(2, 0)["key_related"] and not kv(19, 0)["key_related"]
    assert kv(-1, 0) == {"key_match": False, "key_related": False}
    with pytest.raises(ValueError, match=r"\[0, 24\)"):
        kv(0, 24)


def test_control_report_with_a_stub_analyser():
    seen = {}

    def stub(wav, sr, device="cuda"):
        seen["args"] = (tuple(wav.shape), sr, device)
        return {"tempo": torch.tensor([120.5, 61.0, 0.0]), "tempo_strength": torch.tensor([0.9, 0.8, 0.0]),
                "key": torch.tensor([0, 21, -1], dtype=torch.int32), "key_strength": torch.tensor([0.7, 0.6, 0.0])}
    wav = torch.zeros((3, 1, 100))
    rep = analysis.control_report(wav, 48000, device="cpu", analyzer=stub)
    assert seen["args"] == ((3, 1, 100), 48000, "cpu")
    assert sorted(rep) == ["key", "key_name", "key_strength", "tempo", "tempo_strength"]
    assert rep["key"] == [0, 21, -1] and rep["key_name"] == ["C", "Am", None] and rep["tempo"] == [120.5, 61.0, 0.0]
    rep = analysis.control_report(wav, 48000, tempo=120, key=[0, 0, 0], device="cpu", analyzer=stub)
    assert rep["tempo_match"] == [True, False, False] and rep["tempo_match_octave"] == [True, True, False]
    assert rep["tempo_ratio"] == [pytest.approx(120.5 / 120), pytest.approx(61 / 120), 0.0]
    assert rep["key_match"] == [True, False, False] and rep["key_related"] == [True, True, False]
    with pytest.raises(ValueError, match="2 targets for 3 rows"):
        analysis.control_report(wav, 48000, tempo=[120, 120], device="cpu", analyzer=stub)


# ------------------------------------------------------------------ argument errors
def test_argument_errors():
    with pytest.raises(TypeError, match="float32"):
        analysis.music_features(torch.zeros((1, 4000), dtype=torch.float64), 48000)
    with pytest.raises(ValueError, match="gamma"):
        analysis.music_features(torch.zeros((1, 4000)), 48000, gamma=0.0)
    with pytest.raises(L.Jen1HipError, match="no CPU fallback"):
        analysis.music_features(torch.zeros((1, 4000)), 48000, device="cpu")
    with pytest.raises(L.Jen1HipError, match="no CPU fallback"):
        analysis.tempo(torch.zeros((1, 100)), 93.75)
    with pytest.raises(L.Jen1HipError, match="no CPU fallback"):
        analysis.key(torch.zeros((1, 12, 100)))
    with pytest.raises(ValueError, match=r"float32 \[B, F\]"):
        analysis.tempo(torch.zeros((100,)), 93.75)
    with pytest.raises(ValueError, match=r"float32 \[B, 12, F\]"):
        analysis.key(torch.zeros((1, 11, 100)))
    with pytest.raises(ValueError, match="unknown analyze"):
        from jen1_amd.dataset import LatentCollate
        LatentCollate(object(), analyze=("tempo", "mood"))


# ------------------------------------------------------------------ LatentCollate(analyze=...)
class StubEncoder:
    sample_rate, channels = 48000, 2

    def __init__(self):
        self.calls = []

    def encode_latents(self, wav):
        self.calls.append(wav.clone())
        return (wav[:, :1, ::320].repeat(1, 128, 1) * 2.0,)


def _batch():
    g = torch.Generator().manual_seed(3)
    clip = lambda n: torch.rand((2, n), generator=g) - 0.5
    return [(clip(48000), 48000, {"prompt": "a", "tempo": 77, "key": 4}),          # both in the JSON: they win
            (clip(48000), 48000, {"prompt": "b"}),                                  # neither: both measured
            (clip(24000), 48000, {"prompt": "c", "key": 9}),                        # short clip, tempo missing
            (clip(48000), 48000, {"prompt": "d"})]                                  # the analyser cannot decide


def test_latent_collate_analyze_with_stubs():
    from jen1_amd.dataset import LatentCollate
    seen = []

    def stub(wav, rate, lengths=None):
        seen.append((wav.clone(), rate, list(lengths)))
        return {"tempo": torch.tensor([100.0, 128.25, 90.5, 0.0]), "tempo_strength": torch.ones(4), "key": torch.tensor([1, 21, 2, -1], dtype=torch.int32),
                "key_strength": torch.ones(4)}
    same = lambda wav, sr, target_sr, ch: wav
    batch = _batch()
    before = [dict(md) for _c, _s, md in batch]
    enc0, enc1 = StubEncoder(), StubEncoder()
    plain = LatentCollate(enc0, device="cpu", sample_duration=1, convert_audio=same)(batch)
    emb, meta = LatentCollate(enc1, device="cpu", sample_duration=1, convert_audio=same, analyze=("tempo", "key"), analyzer=stub)(batch)
    assert torch.equal(emb, plain[0]) and torch.equal(enc0.calls[0], enc1.calls[0]), "the latents do not change"
    assert len(seen) == 1 and seen[0][1] == 48000 and seen[0][2] == [48000, 48000, 24000, 48000], "one call, with the valid samples of every clip"
    assert torch.equal(seen[0][0], enc1.calls[0]), "measured on the converted batch the encoder gets"
    assert meta[0] == {"prompt": "a", "tempo": 77, "key": 4}, "values of the JSON win"
    assert meta[1] == {"prompt": "b", "tempo": 128.25, "key": 21} and type(meta[1]["key"]) is int and type(meta[1]["tempo"]) is float
    assert meta[2] == {"prompt": "c", "key": 9, "tempo": 90.5}
    assert meta[3] == {"prompt": "d"}, "an undecided row gets no entry"
    assert [md for _c, _s, md in batch] == before and all(m is not b[2] for m, b in zip(meta, batch)), "the input dicts are copied, not mutated"
    assert all(m is b[2] for m, b in zip(plain[1], batch)), "analyze=() hands the dicts on as before"
    only = LatentCollate(StubEncoder(), device="cpu", sample_duration=1, convert_audio=same, analyze=("key",), analyzer=stub)(batch)[1]
    assert only[1] == {"prompt": "b", "key": 21} and only[2] == {"prompt": "c", "key": 9}
    seen.clear()
    full = [(c, s, dict(md, tempo=100, key=3)) for c, s, md in batch]
    LatentCollate(StubEncoder(), device="cpu", sample_duration=1, convert_audio=same, analyze=("tempo", "key"), analyzer=stub)(full)
    assert not seen, "nothing is measured when every item has its entries"


def test_annotate_tool_keeps_entries(tmp_path):
    """tools/annotate_dataset.py's merge rule, without the analyser"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("annotate_dataset", os.path.join(ROOT, "tools", "annotate_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    measured = {"tempo": 120.5, "tempo_strength": 0.5, "key": 9, "key_name": "A", "key_strength": 0.25}
    assert mod.merge({"prompt": "x", "tempo": 90}, measured, overwrite=False) == dict(measured, prompt="x", tempo=90)
    assert mod.merge({"prompt": "x", "tempo": 90}, measured, overwrite=True) == dict(measured, prompt="x")
    assert mod.merge({}, {"tempo": 0.0, "tempo_strength": 0.0, "key": -1, "key_name": None, "key_strength": 0.0}, overwrite=True) == {}
