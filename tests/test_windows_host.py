"""Host side of long-form sampling (jen1_amd/windows.py, csrc/windows.hip): the plan's arithmetic against the numpy restatement of
windows_common.py, every refusal, the C ABI of the two entry points, and ``Jen1.generate``'s argument checks.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT
from windows_common import np_cover, np_gather, np_k, np_merge, np_merge_rows, np_offsets


def plan(*a, **kw):
    from jen1_amd.windows import WindowPlan
    return WindowPlan(*a, **kw)


# ------------------------------------------------------------------ 1. plan arithmetic
def test_plan_offsets_and_coverage_of_the_even_case():
    p = plan(560, 300, 100)
    assert (p.W, tuple(p.offsets), p.ramp) == (4, (0, 100, 200, 260), 200)
    cover = np_cover(560, 300, p.offsets)
    assert (cover[200:260] == 3).all() and (cover[260:300] == 4).all()
    assert cover[0] == 1 and cover[99] == 1 and cover[100] == 2 and cover[559] == 1
    assert p.offsets == np_offsets(560, 300, 100)


def test_plan_pulls_the_last_window_in():
    p = plan(689, 300, 212)
    assert (p.W, tuple(p.offsets), p.ramp) == (3, (0, 212, 389), 88)
    assert p.offsets == np_offsets(689, 300, 212)
    overlaps = [a + 300 - b for a, b in zip(p.offsets, p.offsets[1:])]
    assert overlaps == [88, 123], "uneven overlaps"


def test_a_canvas_of_one_window():
    p = plan(300, 300, 100)
    assert p.W == 1 and p.offsets == [0]
    assert torch.equal(p.weights(normalised=True), torch.ones((1, 300)))
    assert plan(6750, 1500, 750).W == 8 and plan(6750, 1500, 750).offsets[-1] == 5250


@pytest.mark.parametrize("L,T,hop,ramp", [(560, 300, 100, None), (689, 300, 212, None), (70, 37, 11, 26), (70, 37, 11, 1), (70, 37, 37, None),
                                          (301, 300, 1, 7), (6750, 1500, 750, None)])
def test_weights_cover_every_frame_and_match_the_restatement(L, T, hop, ramp):
    p = plan(L, T, hop, ramp)
    assert p.offsets == np_offsets(L, T, hop)
    assert (np_cover(L, T, p.offsets) >= 1).all(), "every canvas frame is covered"
    rel = p.weights()
    assert rel.dtype == torch.float32 and tuple(rel.shape) == (p.W, T)
    assert float(rel.min()) >= 1.0 / p.ramp * (1 - 1e-6) and float(rel.max()) <= 1.0, "k(p) / ramp lies in [1 / ramp, 1]"
    assert np.allclose(rel.numpy(), np.broadcast_to(np_k(T, p.ramp) / p.ramp, (p.W, T)), rtol=1e-6)
    w = p.weights(normalised=True)
    assert w.dtype == torch.float32 and tuple(w.shape) == (p.W, T)
    k = np_k(T, p.ramp).astype(np.float64)
    total = np.zeros(L)
    for off in p.offsets:
        total[off:off + T] += k
    want = np.stack([k / total[off:off + T] for off in p.offsets])
    assert np.allclose(w.numpy(), want, rtol=1e-6, atol=0)
    # the normalised weights of the windows covering a frame sum to 1, and none is below 1 / (W ramp)
    acc = np.zeros(L)
    for j, off in enumerate(p.offsets):
        acc[off:off + T] += want[j]
    assert np.allclose(acc, 1.0, rtol=1e-12)
    assert float(w.min()) >= 1.0 / (p.W * p.ramp) * (1 - 1e-6)
    assert (np_k(T, p.ramp) >= 1).all() and (np_k(T, p.ramp) <= p.ramp).all()


def test_ramp_one_weighs_every_window_equally():
    p = plan(70, 37, 11, ramp=1)
    cover = np_cover(70, 37, p.offsets)
    assert torch.equal(p.weights(), torch.ones((p.W, 37))), "ramp = 1: all-equal weights"
    w = p.weights(normalised=True).numpy()
    for j, off in enumerate(p.offsets):
        assert np.allclose(w[j], 1.0 / cover[off:off + 37], rtol=1e-6)


def test_the_numpy_merge_is_a_weighted_mean_and_keeps_single_frames():
    rng = np.random.default_rng(3)
    offs = np_offsets(70, 37, 11)
    rows = rng.standard_normal((2 * 4, 5, 37)).astype(np.float32)
    canvas, big = np_merge(rows, 70, offs, 26)
    assert (np.abs(canvas) <= big + 1e-12).all(), "a weighted mean stays inside its values"
    same = np_gather(rng.standard_normal((2, 5, 70)).astype(np.float32), 37, offs)
    assert np.array_equal(np_merge_rows(same, 70, offs, 26), same), "crops of one canvas merge to themselves"
    merged = np_merge_rows(rows, 70, offs, 26)
    assert np.array_equal(merged[0, :, :11], rows[0, :, :11]) and not np.array_equal(merged[0, :, 11:], rows[0, :, 11:])
    assert np.array_equal(np_merge_rows(merged, 70, offs, 26)[:, :, 0], merged[:, :, 0])


def test_starts_in_seconds():
    assert plan(560, 300, 100).starts_seconds(150.0) == [0.0, 100 / 150.0, 200 / 150.0, 260 / 150.0]


# ------------------------------------------------------------------ 2. refusals
@pytest.mark.parametrize("args,kw,what", [
    ((299, 300, 100), {}, "shorter"),
    ((560, 300, 0), {}, "hop"),
    ((560, 300, -3), {}, "hop"),
    ((900, 300, 301), {}, "gap"),
    ((560, 300, 100), {"ramp": 0}, "ramp"),
    ((560, 300, 100), {"ramp": 301}, "ramp"),
])
def test_plan_refuses(args, kw, what):
    with pytest.raises(ValueError, match=what):
        plan(*args, **kw)


def test_a_table_with_a_gap_is_refused_on_the_host():
    p = plan(560, 300, 100)
    p.offsets = [0, 100, 260]                   # frames 400 .. 559 are covered, but the table no longer is the plan's
    p._check_coverage()
    p.offsets = [0, 301]
    with pytest.raises(ValueError, match="cover"):
        p._check_coverage()
    p.offsets = [0, 100, 200]                   # the end of the canvas is left out
    with pytest.raises(ValueError, match="cover"):
        p._check_coverage()


def test_merge_and_gather_check_their_tensors_before_any_launch():
    p = plan(70, 37, 11)
    with pytest.raises(ValueError):
        p.merge_(torch.zeros((3, 5, 37)))       # not a multiple of W rows
    with pytest.raises(ValueError):
        p.merge_(torch.zeros((4, 5, 36)))
    with pytest.raises(ValueError):
        p.merge_(torch.zeros((4, 5, 37)))       # not on the GPU
    with pytest.raises(ValueError):
        p.gather(torch.zeros((2, 5, 71)))
    with pytest.raises(ValueError):
        p.gather(torch.zeros((2, 5, 70)))       # not on the GPU


# ------------------------------------------------------------------ 3. the C ABI
@pytest.fixture(scope="module")
def lib():
    from jen1_amd import lib as L
    L.build()
    return L.load()


def test_entry_points_are_declared_bound_and_exported(lib):
    from jen1_amd import lib as L
    with open(os.path.join(ROOT, "include", "jen1_hip.h")) as f:
        header = f.read()
    for name in ("jen1_window_merge", "jen1_window_gather"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/jen1_hip.h"
        assert name in L.SYMBOLS and "windows.hip" in L.SOURCES
        assert getattr(lib, name) is not None, f"{name} is not exported by the built library"
    assert len(L.SYMBOLS["jen1_window_merge"][1]) == 10 and len(L.SYMBOLS["jen1_window_gather"][1]) == 10


def test_entry_points_validate_arguments_without_a_gpu(lib):
    """every refusal comes back as the error code + message before anything is launched (the pointers are never dereferenced)"""
    rows, offs, cv = 4096, 8192, 16384         # (n, W, C, T, L, ramp)
    ok = (2, 4, 5, 37, 70, 26)

    def merge(n, W, C_, T, L_, ramp, rows=rows, offs=offs, canvas=cv):
        return lib.jen1_window_merge(rows, offs, n, W, C_, T, L_, ramp, canvas, None)

    def msg():
        return lib.jen1_last_error().decode()
    bad = {
        "null": dict(rows=None), "W": (2, 0, 5, 37, 70, 26), "ramp0": (2, 4, 5, 37, 70, 0), "ramp>T": (2, 4, 5, 37, 70, 38),
        "T>L": (2, 4, 5, 71, 70, 26), "T0": (2, 4, 5, 0, 70, 1), "C0": (2, 4, 0, 37, 70, 26), "n<0": (-1, 4, 5, 37, 70, 26),
        "index": (1 << 20, 1 << 10, 1 << 10, 1 << 10, 1 << 11, 5), "weights": (1, 1 << 15, 1, 1 << 10, 1 << 11, 1 << 10),
    }
    for name, a in bad.items():
        rc = merge(*ok, **a) if isinstance(a, dict) else merge(*a)
        assert rc != 0 and "jen1_window_merge" in msg(), (name, rc, msg())
    assert merge(0, 4, 5, 37, 70, 26) == 0, "no pieces: nothing to launch"

    def gather(lead, n, W, C_, T, L_, canvas=cv, rows=rows, offs=offs):
        return lib.jen1_window_gather(canvas, rows, offs, lead, n, W, C_, T, L_, None)
    for name, a in {"null": (1, 2, 4, 5, 37, 70, None), "lead": (0, 2, 4, 5, 37, 70), "W": (1, 2, 0, 5, 37, 70), "T>L": (1, 2, 4, 5, 71, 70),
                    "index": (1 << 10, 1 << 10, 1 << 10, 1 << 10, 1 << 10, 1 << 11)}.items():
        assert gather(*a) != 0 and "jen1_window_gather" in msg(), (name, msg())
    assert gather(3, 0, 4, 5, 37, 70) == 0


# ------------------------------------------------------------------ 4. the samplers' and generate's argument checks
def test_sampler_signatures():
    from jen1_amd.diffusion import GaussianDiffusion
    from jen1_amd.vdm import VDM
    sig = inspect.signature(GaussianDiffusion.sample_windows).parameters
    assert list(sig)[1:5] == ["model", "plan", "n", "conditioning"]
    for k in ("sampler", "causal", "init_noise", "step_noises", "dropout_rows", "known", "keep_mask", "known_noise", "use_graph", "fused"):
        assert sig[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert "return_all_timesteps" not in sig
    assert inspect.signature(VDM.sample_windows).parameters["step"].default == 100
    for fn in (GaussianDiffusion._ddim_generic, GaussianDiffusion._dpm_generic, GaussianDiffusion.p_sample_loop, VDM.p_sample_loop):
        assert inspect.signature(fn).parameters["edit"].default is None, fn.__qualname__


def test_sample_windows_refuses_mismatched_rows_and_canvases_before_any_launch():
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    gd = GaussianDiffusion(steps=1000, betas=get_beta_schedule("linear", 1000)[0], objective="noise", loss_type="l2", device="cpu",
                           sampling_timesteps=3)
    p = plan(70, 37, 11)
    calls = []

    def model(x, t, **kw):
        calls.append(1)
        return x
    cond = {"cross_attn_cond": torch.zeros((7, 2, 4)), "cross_attn_masks": None, "global_cond": None, "input_concat_cond": None}
    with pytest.raises(ValueError, match="rows"):
        gd.sample_windows(model, p, 2, cond, init_noise=torch.zeros((2, 5, 70)))
    cond["cross_attn_cond"] = torch.zeros((8, 2, 4))
    with pytest.raises(ValueError, match="canvas"):
        gd.sample_windows(model, p, 2, cond, init_noise=torch.zeros((8, 5, 37)))
    with pytest.raises(ValueError, match="canvas"):
        gd.sample_windows(model, p, 2, cond, init_noise=torch.zeros((2, 5, 70)), known=torch.zeros((2, 5, 70)), keep_mask=torch.zeros((2, 5, 70)))
    with pytest.raises(ValueError, match="sampler"):
        gd.sample_windows(model, p, 2, cond, init_noise=torch.zeros((2, 5, 70)), sampler="euler")
    with pytest.raises(ValueError, match="channel"):
        gd.sample_windows(model, p, 2, cond)
    assert not calls


def test_generate_window_argument_checks():
    from jen1_amd.generation import Jen1

    class Enc:
        channels = 2
    g = Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda meta, device: {})
    kw = dict(seed=1, steps=2, seconds=4, use_gdm=True, task="text_guided")
    for overlap in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="window_overlap"):
            g.generate("a prompt", window_seconds=2, window_overlap=overlap, **kw)
    for ws in (0, -1.0):
        with pytest.raises(ValueError, match="window_seconds"):
            g.generate("a prompt", window_seconds=ws, **kw)
    sig = inspect.signature(Jen1.generate).parameters
    assert sig["window_seconds"].default is None and sig["window_overlap"].default == 0.5
    assert Jen1._check_windows(45, 10, 0.5) and not Jen1._check_windows(10, 10, 0.5) and not Jen1._check_windows(45, None, 7.0)
    # the metadata rows of a windowed call: W prompts repeated per piece, conditions per piece or per row
    rows = g._window_rows(["a", "b", "c"], 2, 3, None)
    assert [r["prompt"] for r in rows] == ["a", "b", "c", "a", "b", "c"]
    rows = g._window_rows("p", 2, 3, [{"tempo": 1}, {"tempo": 2}])
    assert [r["tempo"] for r in rows] == [1, 1, 1, 2, 2, 2] and all(r["prompt"] == "p" for r in rows)
    rows = g._window_rows("p", 2, 3, [{"k": i} for i in range(6)])
    assert [r["k"] for r in rows] == list(range(6))
    with pytest.raises(ValueError, match="W = 3"):
        g._window_rows(["a", "b"], 2, 3, None)
    with pytest.raises(ValueError, match="conditions"):
        g._window_rows("p", 2, 3, [{}] * 4)
