"""Host side of the loudness meter and normaliser (jen1_amd/audio.py: k_weighting, loudness, normalize_audio) and of the keywords that
plug them into ``Jen1.generate``, ``save_audio_tensor``, ``LatentCollate`` and ``get_dataloaders``: the coefficients against the tables of
ITU-R BS.1770-4, the float64 oracle of tests/loudness_common.py against known answers (which pin the definition itself), and every
refusal that needs no kernel."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import loudness_common as O

from jen1_amd import audio
from jen1_amd.config import tiny_model_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ coefficients
def test_k_weighting_reproduces_the_tables_at_48k():
    sos = audio.k_weighting(48000)
    assert sos.shape == (2, 6) and sos.dtype == np.float64
    table = {(0, 0): 1.53512485958697, (0, 1): -2.69169618940638, (0, 2): 1.19839281085285, (0, 4): -1.69065929318241,
             (0, 5): 0.73248077421585, (1, 4): -1.99004745483398, (1, 5): 0.99007225036621}
    for (s, i), want in table.items():
        assert abs(sos[s, i] - want) <= 1e-12, (s, i, sos[s, i], want)
    assert sos[0, 3] == 1.0 and sos[1, 3] == 1.0 and tuple(sos[1, :3]) == (1.0, -2.0, 1.0)


@pytest.mark.parametrize("sr", [44100, 8000, 96000])
def test_k_weighting_against_the_restatement(sr):
    assert float(np.abs(audio.k_weighting(sr) - O.coefficients(sr)).max()) <= 1e-14


# ------------------------------------------------------------------ the oracle against known answers
def test_oracle_tone_at_minus_23_dbfs_in_both_channels():
    e = O.kat_energies()["tone23"]
    got = O.gate(np.stack([e, e]), 4800)
    print(f"-23 dBFS stereo tone: {got:.5f} LUFS")
    assert abs(got - (-23.0)) <= 0.01
    assert O.gate_margin(np.stack([e, e]), 4800) >= 5.0


def test_oracle_tone_in_one_channel_or_mono():
    k = O.kat_energies()
    one = O.gate(np.stack([k["tone23"], np.zeros_like(k["tone23"])]), 4800)
    mono = O.gate(k["tone23"][None], 4800)
    full = O.gate(np.stack([np.zeros_like(k["tone0"]), k["tone0"]]), 4800)
    print(f"-23 dBFS tone in one channel {one:.5f}, as mono {mono:.5f}; full scale in one channel {full:.5f}")
    assert abs(one - (-26.0103)) <= 1e-3 and abs(mono - (-26.0103)) <= 1e-3
    assert abs(full - (-3.0103)) <= 1e-3
    assert O.gate_margin(k["tone0"][None], 4800) >= 5.0


def test_oracle_gating():
    e = O.kat_energies()["gating"]
    both = np.stack([e, e])
    gated, plain = O.gate(both, 4800), O.ungated(both, 4800)
    print(f"gating signal: {gated:.5f} LUFS with the gates, {plain:.5f} without; margin {O.gate_margin(both, 4800):.2f} LU")
    assert abs(gated - (-20.6037)) <= 1e-3
    assert abs(plain - (-23.9575)) <= 1e-3
    assert O.gate_margin(both, 4800) >= 5.0


def test_oracle_gate_edge_cases():
    assert O.gate(np.zeros((2, 3)), 4800) == -np.inf and O.gate(np.zeros((1, 0)), 4800) == -np.inf
    assert O.gate(np.zeros((2, 40)), 4800) == -np.inf                                   # nothing above the absolute gate
    e = np.full((1, 4), 4800.0 * 0.01)                                                  # one block of mean square 0.01
    assert abs(O.gate(e, 4800) - (-0.691 - 20.0)) <= 1e-12


def test_oracle_gain_rules():
    x = np.array([[0.5, -0.25, 0.0, 0.25]])
    rms = np.sqrt((x ** 2).mean())
    assert O.gain("loudness", x, lufs=-20.0, target=-14.0) == pytest.approx(10 ** (6 / 20), rel=1e-15)
    assert O.gain("loudness", x, lufs=-np.inf) == 1.0 and O.gain("loudness", x * 1e-3, lufs=-60.0) == 1.0
    assert O.gain("peak", x) == pytest.approx(10 ** (-1 / 20) / 0.5, rel=1e-15)
    assert O.gain("rms", x) == pytest.approx(10 ** (-18 / 20) / rms, rel=1e-15)
    assert O.gain("peak", x * 0) == 1.0 and O.gain("rms", x * 0) == 1.0 and O.gain("clip", x) == 1.0


# ------------------------------------------------------------------ refusals that need no kernel
def test_argument_errors():
    x = torch.zeros((2, 4800))
    for fn in (audio.loudness, audio.normalize_audio):
        with pytest.raises(ValueError, match="multiple of 10"):
            fn(x, 44101)
        with pytest.raises(ValueError, match="one or two channels"):
            fn(torch.zeros((3, 4800)), 48000)
        with pytest.raises(ValueError, match="channel and a time axis"):
            fn(torch.zeros((4800,)), 48000)
        with pytest.raises(TypeError, match="float32"):
            fn(x.double(), 48000)
    with pytest.raises(ValueError, match="strategy"):
        audio.normalize_audio(x, 48000, strategy="lufs")
    with pytest.raises(ValueError, match="limit"):
        audio.normalize_audio(x, 48000, limit="soft")
    with pytest.raises(ValueError, match="one entry per row"):
        audio.normalize_audio(torch.zeros((3, 2, 4800)), 48000, target_lufs=torch.zeros(2))
    with pytest.raises(ValueError):
        audio.k_weighting(0)


def test_there_is_no_cpu_fallback():
    from jen1_amd.lib import Jen1HipError
    x = torch.zeros((2, 4800))
    with pytest.raises(Jen1HipError, match="no CPU fallback"):
        audio.loudness(x, 48000, device="cpu")
    with pytest.raises(Jen1HipError, match="no CPU fallback"):
        audio.normalize_audio(x, 48000, device="cpu")


def test_keyword_defaults():
    p = inspect.signature(audio.normalize_audio).parameters
    assert [p[k].default for k in ("strategy", "target_lufs", "headroom_db", "limit", "energy_floor", "device", "return_gain")] == \
        ["loudness", -14.0, None, "clip", 2e-3, "cuda", False]
    assert inspect.signature(audio.loudness).parameters["device"].default == "cuda"
    assert audio.DEFAULT_HEADROOM_DB == O.DEFAULT_HEADROOM_DB
    from jen1_amd.dataset import LatentCollate, get_dataloaders
    from jen1_amd.generation import Jen1, save_audio_tensor
    for fn, names in ((Jen1.generate, ("normalize", "target_lufs", "limit")), (save_audio_tensor, ("normalize", "target_lufs", "limit")),
                      (LatentCollate.__init__, ("normalize", "target_lufs")), (get_dataloaders, ("normalize", "target_lufs"))):
        q = inspect.signature(fn).parameters
        want = {"normalize": None, "target_lufs": -14.0, "limit": "clip"}
        assert [q[k].default for k in names] == [want[k] for k in names], fn.__qualname__
    names = list(inspect.signature(Jen1.generate).parameters)
    assert names[-4:] == ["normalize", "target_lufs", "limit", "preserve_known"]          # in front of preserve_known, behind the rest
    assert names.index("normalize") > names.index("window_overlap")


def _host_jen1():
    from jen1_amd.generation import Jen1

    class Enc:
        channels = 2
    return Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda md, dev: {}, model_config=tiny_model_config())


def test_generate_refuses_before_it_touches_a_device():
    j = _host_jen1()
    with pytest.raises(ValueError, match="target_lufs='input'"):
        j.generate("y", task="text_guided", normalize="loudness", target_lufs="input")
    with pytest.raises(ValueError, match="target_lufs='input'"):
        j.generate("y", task="music_cont", normalize="loudness", target_lufs="input")           # no init_audio
    with pytest.raises(ValueError, match="target_lufs"):
        j.generate("y", normalize="loudness", target_lufs="loud")
    with pytest.raises(ValueError, match="normalize"):
        j.generate("y", normalize="lufs")
    with pytest.raises(ValueError, match="limit"):
        j.generate("y", normalize="peak", limit="soft")


def test_latent_collate_refuses_an_unknown_strategy():
    from jen1_amd.dataset import LatentCollate
    with pytest.raises(ValueError, match="normalize"):
        LatentCollate(object(), normalize="lufs")
    assert LatentCollate(object()).normalize is None


# ------------------------------------------------------------------ the C ABI is declared, bound and listed
def test_entry_points_are_declared_bound_and_listed():
    from jen1_amd import lib as L
    with open(os.path.join(ROOT, "include", "jen1_hip.h")) as f:
        header = f.read()
    for name in ("jen1_kweight_energy", "jen1_kweight_energy_workspace_bytes", "jen1_kweight_chunk", "jen1_loudness_gate", "jen1_gain_apply"):
        assert re.search(r"\b(int|int64_t)\s+" + name + r"\s*\(", header), f"{name} is not declared in include/jen1_hip.h"
        assert name in L.SYMBOLS
    assert "loudness.hip" in L.SOURCES
    assert (L.GAIN_LOUDNESS, L.GAIN_PEAK, L.GAIN_RMS, L.GAIN_CLIP) == tuple(range(4)) == tuple(audio.STRATEGIES.index(s) for s in ("loudness", "peak", "rms", "clip"))
    assert (L.LIMIT_NONE, L.LIMIT_CLIP, L.LIMIT_TANH) == tuple(range(3)) == tuple(audio.LIMITS.index(s) for s in ("none", "clip", "tanh"))


@pytest.fixture(scope="module")
def lib():
    from jen1_amd import lib as L
    L.build()
    return L.load()


def test_chunk_rule(lib):
    """a chunk divides the hop; about a hundred samples where the hop allows it, never a handful"""
    got = [lib.jen1_kweight_chunk(h) for h in (4800, 4410, 800, 9600, 2 * 2399, 127, 1, 0)]
    assert got == [120, 126, 100, 128, 2399, 127, 1, 0]
    for h in (4800, 4410, 800, 1600, 2205, 3200, 9600, 19200, 2 * 2399):
        n = lib.jen1_kweight_chunk(h)
        assert h % n == 0 and n >= min(16, h)
    assert audio.chunk_samples(4800) == 120
    assert lib.jen1_kweight_tile_chunks(4800) == 128 and lib.jen1_kweight_tile_chunks(2 * 2399) == 6
    assert lib.jen1_kweight_energy_workspace_bytes(3, 2, 4800, 4800) >= 3 * 2 * (40 * 7 + 2) * 8          # 7 words per chunk, 2 per channel
    assert lib.jen1_kweight_energy_workspace_bytes(3, 3, 4800, 4800) == 0
