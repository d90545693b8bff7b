"""Host side of the Frechet Audio Distance (jen1_amd/fad.py, include/jen1_fad.h): VGGish's mel matrix, the example arithmetic, the Frechet
distance against scipy, the statistics from a hand-filled state, the weight packing and the C ABI table -- none of which needs a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import fad_common as O

from jen1_amd import fad as F
from jen1_amd import lib as L
from jen1_amd import spectral as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ mel matrix, example count
def test_mel_matrix_against_the_loop():
    m = F.vggish_mel_matrix()
    want = O.mel_matrix_loop()
    assert m.dtype == np.float64 and m.shape == (64, 257)
    assert float(np.abs(m - want).max()) <= 1e-12
    assert np.all(m[:, 0] == 0.0)
    assert np.all((m != 0).sum(axis=1) >= 1)
    assert float(m.max()) <= 1.0 and float(m.min()) >= 0.0
    assert not np.allclose(m, S.mel_filterbank(16000, 512, 64, 125.0, 7500.0))       # triangles linear in mel, not in Hz


def test_mel_matrix_banded_round_trip_is_exact():
    m = F.vggish_mel_matrix()
    lo, hi, off, w = S.banded(m)
    assert w.dtype == np.float64
    assert np.array_equal(S.unbanded(lo, hi, off, w, 257), m)
    assert np.all(hi > lo) and int(lo.min()) >= 1


@pytest.mark.parametrize("n,want", [(15599, 0), (15600, 1), (30959, 1), (30960, 2), (0, 0), (399, 0), (400, 0)])
def test_example_count(n, want):
    assert F.example_count(n) == want
    if n >= 400:
        assert F.example_count(n) == (1 + (n - 400) // 160) // 96


def test_example_count_formula_over_a_range():
    for n in range(400, 50000, 37):
        assert F.example_count(n) == (1 + (n - 400) // 160) // 96 == O.count(n)


# ------------------------------------------------------------------ statistics from a hand-filled state
def filled(e: np.ndarray) -> F.FrechetStats:
    """the state the moments kernel would leave for the rows of e, formed on the host in float64"""
    st = F.FrechetStats(e.shape[1])
    s = np.concatenate([[float(e.shape[0])], e.sum(0), (e.T @ e).reshape(-1)])
    st.state = torch.from_numpy(s)
    return st


def sets(n, d=128, seed=0, scale=1.0, shift=0.0):
    rng = np.random.default_rng([seed, n, d])
    A = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    return (rng.standard_normal((n, d)) @ A) * scale + shift


def test_mean_and_cov_equal_numpy():
    e = sets(300, 64, 1, 1.5, 0.3)
    st = filled(e)
    assert st.count == 300
    assert float(np.abs(st.mean() - e.mean(0)).max()) <= 1e-12
    c = np.cov(e, rowvar=False)
    assert float(np.abs(st.cov() - c).max()) <= 1e-12 * float(np.abs(c).max())
    assert np.array_equal(st.cov(), st.cov().T)


def test_merge_equals_the_fit_over_the_concatenation():
    a, b = sets(70, 32, 2), sets(45, 32, 3, 2.0, -1.0)
    m = filled(a).merge(filled(b))
    both = filled(np.concatenate([a, b]))
    assert m.count == 115
    assert float((m.state - both.state).abs().max()) <= 1e-9
    assert float(np.abs(m.cov() - np.cov(np.concatenate([a, b]), rowvar=False)).max()) <= 1e-12 * 10
    with pytest.raises(ValueError):
        filled(a).merge(filled(sets(10, 16, 4)))


def test_state_dict_round_trip_is_exact():
    st = filled(sets(50, 48, 5))
    sd = st.state_dict()
    back = F.FrechetStats.from_state_dict(sd)
    assert back.dim == 48 and torch.equal(back.state, st.state)
    with pytest.raises(ValueError):
        F.FrechetStats(64).load_state_dict(sd)
    with pytest.raises(ValueError):
        F.FrechetStats(100)


# ------------------------------------------------------------------ the distance against scipy
def test_frechet_distance_against_scipy_well_conditioned():
    from scipy.linalg import sqrtm
    a, b = sets(600, 128, 10), sets(500, 128, 11, 1.3, 0.2)
    got = F.frechet_distance(filled(a), filled(b))
    want = O.frechet_np(a, b, sqrtm)
    print(f"frechet_distance vs scipy, 600 / 500 samples: {got!r} vs {want!r}, relative {abs(got - want) / abs(want):.2e} (gate 1e-9)")
    assert abs(got - want) <= 1e-9 * abs(want)


def test_frechet_distance_rank_deficient_is_finite_and_near_scipy():
    from scipy.linalg import sqrtm
    a, b = sets(40, 128, 12), sets(50, 128, 13, 0.8, -0.1)
    got = F.frechet_distance(filled(a), filled(b))
    want = O.frechet_np(a, b, sqrtm)
    print(f"frechet_distance vs scipy, 40 / 50 samples: {got!r} vs {want!r}, relative {abs(got - want) / abs(want):.2e} (gate 1e-6)")
    assert np.isfinite(got)
    assert abs(got - want) <= 1e-6 * abs(want)


def test_frechet_distance_of_a_set_from_itself_and_symmetry():
    a, b = sets(600, 128, 14), sets(500, 128, 15, 1.1, 0.05)
    sa, sb = filled(a), filled(b)
    d = F.frechet_distance(sa, sa)
    print(f"d(a, a) = {d:.3e}, tr S_a = {np.trace(sa.cov()):.3e} (gate 1e-9 tr S_a)")
    assert abs(d) <= 1e-9 * float(np.trace(sa.cov()))
    ab, ba = F.frechet_distance(sa, sb), F.frechet_distance(sb, sa)
    assert ab > 0 and abs(ab - ba) <= 1e-12 * abs(ab)


def test_frechet_distance_refuses_small_sets():
    one = filled(sets(1, 128, 16))
    many = filled(sets(20, 128, 17))
    with pytest.raises(ValueError, match="at least 2"):
        F.frechet_distance(one, many)
    with pytest.raises(ValueError, match="at least 2"):
        F.frechet_distance(many, F.FrechetStats(128))
    with pytest.raises(ValueError):
        F.frechet_distance(many, filled(sets(20, 64, 18)))


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize("widths", [O.NARROW, dict(channels=(16, 80, 48, 96), hidden=64, dim=32)])
def test_from_state_dict_packs_exactly_and_infers_the_widths(widths):
    model = O.VGGishModel(**widths, seed=3)
    sd = model.state_dict()
    net = F.VGGishHIP.from_state_dict(sd, device="cpu")
    c = widths["channels"]
    assert net.channels == [c[0], c[1], c[2], c[2], c[3], c[3]] and net.widths == [widths["hidden"], widths["hidden"], widths["dim"]]
    assert net.dim == widths["dim"] and net.final_relu is False
    p = net.packed_state()
    assert torch.equal(p["conv_w"][0].t().reshape(c[0], 1, 3, 3), sd["features.0.weight"])
    for i, key in enumerate(F.CONV_KEYS):
        assert torch.equal(p["conv_b"][i], sd[key + ".bias"])
        if i:
            w = sd[key + ".weight"]
            assert p["conv_w"][i].numel() == -(-w.shape[0] // 64) * (w.shape[1] // 16) * 9 * 4 * 4 * 64
            assert torch.equal(F.unpack_conv3x3(p["conv_w"][i], w.shape[1], w.shape[0]), w)
    for j, key in enumerate(F.LINEAR_KEYS):
        assert torch.equal(p["lin_w"][j], sd[key + ".weight"]) and torch.equal(p["lin_b"][j], sd[key + ".bias"])
    assert F.VGGishHIP.from_module(model, final_relu=True, device="cpu").final_relu is True


def test_from_state_dict_names_the_key_it_refuses():
    sd = O.VGGishModel(**O.NARROW).state_dict()
    for key in ("features.8.weight", "embeddings.2.bias"):
        with pytest.raises(KeyError, match=re.escape(key)):
            F.VGGishHIP.from_state_dict({k: v for k, v in sd.items() if k != key}, device="cpu")
    bad = dict(sd)
    bad["features.6.weight"] = torch.zeros(48, 16, 3, 3)
    with pytest.raises(ValueError, match=r"features\.6\.weight"):
        F.VGGishHIP.from_state_dict(bad, device="cpu")
    bad = dict(sd)
    bad["embeddings.0.weight"] = torch.zeros(256, 100)
    with pytest.raises(ValueError, match=r"embeddings\.0\.weight"):
        F.VGGishHIP.from_state_dict(bad, device="cpu")
    bad = dict(sd)
    bad["features.3.bias"] = torch.zeros(7)
    with pytest.raises(ValueError, match=r"features\.3\.bias"):
        F.VGGishHIP.from_state_dict(bad, device="cpu")


def test_a_network_off_the_gpu_refuses_to_run():
    net = F.VGGishHIP.from_state_dict(O.VGGishModel(**O.NARROW).state_dict(), device="cpu")
    with pytest.raises(L.Jen1HipError):
        net.forward(torch.zeros(1, 96, 64))
    with pytest.raises(L.Jen1HipError):
        F.vggish_examples(torch.zeros(1, 1, 16000), 16000)
    with pytest.raises(L.Jen1HipError):
        F.FrechetStats(128).update(torch.zeros(4, 128))


# ------------------------------------------------------------------ C ABI
def test_every_symbol_of_the_header_is_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "jen1_fad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(jen1_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(L.FAD_SYMBOLS) and len(names) == 5
    L.build()
    lib = L.load()
    for n in names:
        assert hasattr(lib, n)
    assert (L.VGGISH_FRAMES, L.VGGISH_BANDS, L.CONV3X3_KC, L.CONV3X3_BN) == (96, 64, 16, 64)
    for macro, v in (("JEN1_VGGISH_FRAMES", 96), ("JEN1_VGGISH_BANDS", 64), ("JEN1_CONV3X3_KC", 16), ("JEN1_CONV3X3_BN", 64)):
        assert re.search(rf"#define {macro} {v}\b", text)


def test_launchers_refuse_bad_arguments_before_touching_the_device():
    L.build()
    lib = L.load()
    assert lib.jen1_conv3x3_packed_floats(16, 16) == 9216 and lib.jen1_conv3x3_packed_floats(512, 80) == 2 * 32 * 9216
    assert lib.jen1_conv3x3_packed_floats(8, 16) == 0 and lib.jen1_conv3x3_packed_floats(16, 528) == 0
    p = 4096                                       # a non-null, aligned address: every call below returns before it is used
    bad = [dict(cin=24), dict(cout=520), dict(N=0), dict(H=0), dict(pool=2), dict(pool=1, H=3), dict(x=None), dict(x=p + 4), dict(y=p + 64)]
    for k in bad:
        a = dict(x=p, w=p, b=p, y=p + (1 << 30), N=1, H=4, W=4, cin=16, cout=16, pool=0)
        a.update(k)
        assert lib.jen1_conv3x3(a["x"], a["w"], a["b"], a["y"], a["N"], a["H"], a["W"], a["cin"], a["cout"], a["pool"], None) != 0, k
        assert "jen1_conv3x3" in lib.jen1_last_error().decode()
    counts = (L.c_int * 2)(1, 2)
    assert lib.jen1_vggish_conv1(p, counts, 2, 191, 0, 0, 3, p, p, p, 16, None) != 0          # 2 examples need 192 frames
    assert "counts[1]" in lib.jen1_last_error().decode()
    assert lib.jen1_vggish_conv1(p, counts, 2, 192, 0, 1, 3, p, p, p, 16, None) != 0           # examples [1, 4) of 3
    assert lib.jen1_vggish_conv1(p, counts, 2, 192, 0, 0, 3, p, p, p, 20, None) != 0
    assert lib.jen1_vggish_conv1(p, counts, 2, 192, 2, 0, 3, p, p, p, 16, None) != 0
    assert lib.jen1_vggish_examples(p, (L.c_int * 2)(0, 0), 2, 192, p, None) != 0
    assert lib.jen1_vggish_examples(p, (L.c_int * 1)(-1), 1, 192, p, None) != 0
    assert lib.jen1_vggish_relu(None, 4, None) != 0 and lib.jen1_vggish_relu(p, 0, None) != 0
