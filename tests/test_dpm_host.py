"""CPU-only: the DPM-Solver++(2M) sampler (GaussianDiffusion.dpm_coeff_table / dpm_sample / _dpm_generic, Jen1.generate(sampler=)).

The coefficient rows against a float64 evaluation from the same float32 ``alphas_cumprod``; the order of convergence of the literal loop
with an analytic denoiser (the evidence for "fewer steps": there are no trained weights here); the literal loop against a numpy
restatement around the oracle's model call; the argument errors; the new entry points of the C ABI without a GPU.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from dpm_common import np_dpm_loop, np_dpm_table
from helpers import ROOT, rel_err
from oracle import jen1_oracle as O

RTOL_TABLE = 2e-6       # test_diffusion_tables_and_coefficients_match_reference_goldens gives the DDIM coefficients this
GENERIC_TOL = 1e-4      # test_generic_sampler_and_loss_match_oracle_on_cpu
COND = {"cross_attn_cond": None, "cross_attn_masks": None, "global_cond": None, "input_concat_cond": None}


def _gd(S, schedule="linear", objective="noise", eta=1.0):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    betas, alphas = get_beta_schedule(schedule, 1000)
    return GaussianDiffusion(steps=1000, betas=betas, alphas=alphas, objective=objective, loss_type="l2", device="cpu",
                             cfg_dropout_proba=0.0, embedding_scale=1.0, sampling_timesteps=S, ddim_sampling_eta=eta)


# ------------------------------------------------------------------ 1. table
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("S", [10, 25, 100])
def test_dpm_table_matches_float64_restatement(S, schedule, order):
    """b0, a, b1 (slots 2, 3, 4) within RTOL_TABLE of float64 from the same float32 alphas_cumprod.  Slots 0, 1, 6, 7 are defined as
    those of ``ddim_coeff_table`` (the reference's float32 host tables, gated by its goldens) and must be those bits; 6 and 7 are also
    within RTOL_TABLE of float64 (0 and 1 carry the float32 evaluation of 1 / acp - 1 of the reference's own table)."""
    gd = _gd(S, schedule)
    rows, times = gd.dpm_coeff_table(order)
    pairs = gd.ddim_time_pairs()
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (S, 8) and times.dtype == torch.int64
    assert times.tolist() == [t for t, _ in pairs]
    ddim, dtimes = gd.ddim_coeff_table()
    assert torch.equal(times, dtimes)
    assert torch.equal(rows[:, [0, 1, 6, 7]], ddim[:, [0, 1, 6, 7]])
    acp = gd._host["alphas_cumprod"].numpy()
    assert acp.dtype == np.float32
    a64 = acp.astype(np.float64)
    want = np_dpm_table(acp, pairs, order)
    got = rows.numpy().astype(np.float64)
    worst = 0.0
    for i, w in enumerate(want[:-1]):
        assert got[i, 5] == 4.0
        np.testing.assert_allclose(got[i, 2:5], np.array(w), rtol=RTOL_TABLE, atol=0.0)
        worst = max(worst, max(abs(g - x) / abs(x) for g, x in zip(got[i, 2:5], w) if x != 0.0))
        t = pairs[i][0]
        np.testing.assert_allclose(got[i, 6:8], [np.sqrt(a64[t]), np.sqrt(1.0 - a64[t])], rtol=RTOL_TABLE)
    print(f"S={S} {schedule} order={order}: worst relative error of b0 / a / b1 {worst:.2e}")
    assert want[-1] is None and pairs[-1][1] < 0
    assert got[-1, 2:6].tolist() == [0.0, 0.0, 0.0, 1.0], "the last row is the kind-1 row"
    assert torch.equal(rows[-1], ddim[-1])
    assert got[0, 4] == 0.0, "row 0 has no history to read"
    if order == 1:
        assert (got[:, 4] == 0.0).all()
        al, sg = np.sqrt(a64), np.sqrt(1.0 - a64)
        ddim0 = np.array([al[tn] - al[t] * sg[tn] / sg[t] for t, tn in pairs[:-1]])
        np.testing.assert_allclose(got[:-1, 2], ddim0, rtol=RTOL_TABLE)
    else:
        assert (got[1:-1, 4] != 0.0).all()


# ------------------------------------------------------------------ 2. order of convergence
def _analytic(gd, s=0.2):
    acp = gd.alphas_cumprod.double()

    def model(x, t, **kw):
        a = acp[t][:, None, None]
        return (a.sqrt() * s * s / (a * s * s + (1.0 - a)) * x.double()).float()
    return model


def _errors_at_t99(S, s=0.2):
    gd = _gd(S, "linear", "x0", eta=0.0)
    shape = (2, 4, 64)
    init = torch.from_numpy(np.random.default_rng(5).standard_normal(shape).astype(np.float32))
    pairs = gd.ddim_time_pairs()
    assert pairs[0][0] == 999
    at = [i for i, (t, _) in enumerate(pairs) if t == 99]
    assert len(at) == 1, f"t = 99 is not on the grid of S = {S}"
    acp = gd._host["alphas_cumprod"].double()
    f = lambda t: float(torch.sqrt(acp[t] * s * s + 1.0 - acp[t]))
    exact = init.double() * (f(99) / f(999))
    model = _analytic(gd, s)
    dpm = gd._dpm_generic(model, shape, COND, return_all_timesteps=True, init_noise=init, order=2)
    ddim = gd._ddim_generic(model, shape, COND, True, False, None, init, None, None)
    err = lambda y: float((y[:, 1 + at[0]].double() - exact).abs().max())       # (entry 0 is the start, 1 + i the input of step i)
    assert torch.equal(dpm[:, 1], init) and torch.equal(ddim[:, 1], init)
    return err(dpm), err(ddim)


def test_second_order_convergence_with_an_analytic_denoiser():
    """data ~ N(0, s^2), s = 0.2: the exact denoiser is linear, the clip never acts, and the probability-flow solution is
    x_t = x_T f(t) / f(T) with f(t) = sqrt(acp[t] s^2 + 1 - acp[t]).  Halving the step divides a second-order error by 4 and a
    first-order error by 2."""
    e = {S: _errors_at_t99(S) for S in (10, 20, 40, 80)}
    for S, (d, i) in e.items():
        print(f"S = {S}: 2M {d:.2e}   DDIM eta=0 {i:.2e}")
    for a, b in ((20, 40), (40, 80)):
        assert e[a][0] / e[b][0] > 3.0, (a, b, e[a][0] / e[b][0])
        assert e[a][1] / e[b][1] < 2.2, (a, b, e[a][1] / e[b][1])
    for S, (d, i) in e.items():
        assert d < 0.5 * i, (S, d, i)


# ------------------------------------------------------------------ 3. generic loop against numpy
SHAPE = (2, 4, 40)


def _models(rng):
    Wm = rng.standard_normal((4, 4)).astype(np.float32) * 0.3

    def np_model(x, t, **kw):
        return np.einsum("oc,bct->bot", Wm, x).astype(np.float32) + (np.asarray(t)[:, None, None] / 1000.0).astype(np.float32)

    def th_model(x, t, **kw):
        return torch.einsum("oc,bct->bot", torch.from_numpy(Wm), x) + (t[:, None, None] / 1000.0).float()
    return np_model, th_model


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("objective", ["noise", "x0", "v"])
def test_generic_loop_matches_numpy_restatement(objective, order):
    rng = np.random.default_rng(21)
    S = 10
    np_model, th_model = _models(rng)
    init = rng.standard_normal(SHAPE).astype(np.float32)
    og = O.OracleGaussianDiffusion(steps=1000, betas=O.get_beta_schedule("linear", 1000), objective=objective, cfg_dropout_proba=0.0,
                                   embedding_scale=1.0, sampling_timesteps=S)
    ref, seen = np_dpm_loop(og, lambda x, t, **kw: np_model(x, t), SHAPE, [COND] * S, init, order=order, record=True)
    gd = _gd(S, objective=objective)
    got = gd.dpm_sample(th_model, SHAPE, COND, init_noise=torch.from_numpy(init), order=order)
    e = rel_err(got.numpy(), ref)
    print(f"{objective} order {order}: rel_err {e:.3e}")
    assert e < GENERIC_TOL
    via_sample = gd.sample(th_model, SHAPE, COND, init_noise=torch.from_numpy(init), sampler="dpmpp2m", order=order)
    assert torch.equal(via_sample, got)
    allsteps = gd.dpm_sample(th_model, SHAPE, COND, return_all_timesteps=True, init_noise=torch.from_numpy(init), order=order)
    assert allsteps.shape == (SHAPE[0], S + 1) + SHAPE[1:]
    assert rel_err(allsteps[:, S].numpy(), seen[S - 1]) < GENERIC_TOL          # the INPUT of the last step, as ddim_sample records
    # order 1 is DDIM at eta = 0 in another form -- where DDIM's noise prediction is the one of the clipped x-start (objective "noise"
    # keeps the network's own when the clip acts, gdm.py:127-129, and is another update then)
    if order == 1 and objective != "noise":
        gd0 = _gd(S, objective=objective, eta=0.0)
        ddim = gd0.ddim_sample(th_model, SHAPE, COND, init_noise=torch.from_numpy(init))
        assert rel_err(got.numpy(), ddim.numpy()) < GENERIC_TOL


def test_generic_loop_with_known_blends_x_next_only():
    from known_blend_common import blend_edits, masks, np_blend, np_levels
    rng = np.random.default_rng(22)
    S = 10
    np_model, th_model = _models(rng)
    init = rng.standard_normal(SHAPE).astype(np.float32)
    known = (rng.standard_normal(SHAPE) * 0.5).astype(np.float32)
    eps_k = rng.standard_normal(SHAPE).astype(np.float32)
    keep = masks(SHAPE[0], SHAPE[2], "inpaint")
    og = O.OracleGaussianDiffusion(steps=1000, betas=O.get_beta_schedule("linear", 1000), objective="noise", cfg_dropout_proba=0.0,
                                   embedding_scale=1.0, sampling_timesteps=S)
    start, levels = np_levels("ddim", og.alphas_cumprod, pairs=og.ddim_times())
    ref = np_dpm_loop(og, lambda x, t, **kw: np_model(x, t), SHAPE, [COND] * S, np_blend(init, known, keep, eps_k, *start),
                      edits=blend_edits(levels, known, keep, eps_k))
    th = torch.from_numpy
    gd = _gd(S)
    got = gd.dpm_sample(th_model, SHAPE, COND, init_noise=th(init), known=th(known), keep_mask=th(keep), known_noise=th(eps_k))
    assert rel_err(got.numpy(), ref) < GENERIC_TOL
    sel = np.broadcast_to(keep == 1, SHAPE)
    assert np.array_equal(got.numpy()[sel], known[sel])
    zeros = gd.dpm_sample(th_model, SHAPE, COND, init_noise=th(init), known=th(known), keep_mask=th(masks(SHAPE[0], SHAPE[2], "zeros")))
    assert torch.equal(zeros, gd.dpm_sample(th_model, SHAPE, COND, init_noise=th(init)))


# ------------------------------------------------------------------ 4. errors
def test_argument_errors():
    from jen1_amd.generation import Jen1
    rng = np.random.default_rng(23)
    _, th_model = _models(rng)
    calls = []

    def counting(x, t, **kw):
        calls.append(1)
        return th_model(x, t, **kw)
    gd = _gd(4)
    init = torch.zeros(SHAPE)
    for order in (0, 3, "2"):
        with pytest.raises(ValueError, match="order"):
            gd.dpm_sample(counting, SHAPE, COND, init_noise=init, order=order)
        with pytest.raises(ValueError, match="order"):
            gd.dpm_coeff_table(order)
    with pytest.raises(ValueError, match="known and keep_mask"):
        gd.dpm_sample(counting, SHAPE, COND, init_noise=init, known=torch.zeros(SHAPE))
    with pytest.raises(ValueError, match="unknown sampler"):
        gd.sample(counting, SHAPE, COND, init_noise=init, sampler="heun")
    assert not calls, "the errors come before anything is launched"

    class Enc:
        channels = 2
    g = Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda meta, device: {})
    with pytest.raises(ValueError, match="use_gdm"):
        g.generate("a prompt", seed=1, steps=2, seconds=1, use_gdm=False, sampler="dpmpp2m")
    with pytest.raises(ValueError, match="unknown sampler"):
        g.generate("a prompt", seed=1, steps=2, seconds=1, use_gdm=True, sampler="heun")
    import inspect
    assert inspect.signature(Jen1.generate).parameters["sampler"].default is None
    sig = inspect.signature(type(gd).dpm_sample)
    assert list(sig.parameters) == ["self", "model", "shape", "conditioning", "return_all_timesteps", "causal", "init_data", "order",
                                    "init_noise", "dropout_rows", "use_graph", "known", "keep_mask", "known_noise"]
    assert sig.parameters["order"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["order"].default == 2


# ------------------------------------------------------------------ 5. C ABI
@pytest.fixture(scope="module")
def lib():
    from jen1_amd import lib as L
    L.build()
    return L.load()


def test_multistep_entry_points_are_declared_exported_and_validate_without_a_gpu(lib):
    from jen1_amd import lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jen1_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(jen1_[a-z0-9_]+)\s*\(", src))
    for name in ("jen1_cfg_ddim_step_pack_ms", "jen1_step_tail_ms"):
        assert name in declared and name in L.SYMBOLS and getattr(lib, name) is not None
    ok = L.BlendArgs(16, 32, 48, 64)
    # (net, x, hist, coef, x_out, step_idx, ticket, rows, parts), ld_rows, B, C, T, ld, nrep, scale, scale_cfg, phi, objective, clip, dtype
    head = (256, 512, 1024, 256, 512, 256, 256, 256, 256, 128, 2, 128, 64, 128, 1, 1.0, 0, 0.7, 0, 1, L.F32)
    tail = (256, 4, None, 256, 1024)
    err = lambda: lib.jen1_last_error()
    for fn, args in ((lib.jen1_cfg_ddim_step_pack_ms, head), (lib.jen1_step_tail_ms, head + tail)):
        for blend in (None, C.byref(ok)):
            no_hist = list(args)
            no_hist[2] = None
            assert fn(*no_hist, blend, None) != 0 and b"history buffer" in err()
            no_hist[2] = 1026
            assert fn(*no_hist, blend, None) != 0 and b"4-byte aligned" in err()
            no_hist[2] = 512                                  # the latents themselves
            assert fn(*no_hist, blend, None) != 0 and b"must not be the latents" in err()
            assert fn(*((None,) + args[1:]), blend, None) != 0 and b"null" in err()
            bad_obj = list(args)
            bad_obj[18] = 7
            assert fn(*bad_obj, blend, None) != 0 and b"bad objective" in err()
            odd_c = list(args)
            odd_c[11] = 12                                    # C % 8 != 0: no vector form, no multistep row
            assert fn(*odd_c, blend, None) != 0
        b = L.BlendArgs(16, 32, None, 64)
        assert fn(*args, C.byref(b), None) != 0 and b"null known / eps_k / keep / kb" in err()
    assert lib.jen1_step_tail_ms(*head, 256, 0, None, 256, 1024, None, None) != 0 and b"sentinel table" in err()
