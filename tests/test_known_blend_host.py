"""CPU-only: the known-region blend of the samplers (inpainting / continuation with the kept frames pinned to the known latents).

The blend tables against a float64 evaluation from the reference's own ``alphas_cumprod`` (tests/golden/schedule.npz); the generic loops
(any callable model, device "cpu") against a numpy restatement around the oracle's model call; the properties a blend must have (keep = 0:
the bits of the call without it; keep = 1: the known latents exactly; a 0 / 1 mask: exact wherever it keeps); the argument errors; and the
new entry points of the C ABI without a GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import golden, rel_err
from known_blend_common import blend_edits, masks, np_blend, np_levels, oracle_loop
from oracle import jen1_oracle as O

RTOL_TABLE = 2e-6       # test_diffusion_tables_and_coefficients_match_reference_goldens gives the DDIM coefficients this
GENERIC_TOL = 1e-4      # test_generic_sampler_and_loss_match_oracle_on_cpu


def _gd(S, eta=1.0, steps=1000, objective="noise", betas=None):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    if betas is None:
        betas, _ = get_beta_schedule("linear", steps)
    return GaussianDiffusion(steps=steps, betas=betas, objective=objective, loss_type="l2", device="cpu", cfg_dropout_proba=0.0,
                             embedding_scale=1.0, sampling_timesteps=S, ddim_sampling_eta=eta)


def _vdm():
    from jen1_amd.vdm import VDM
    return VDM(loss_type="l2", device="cpu", cfg_dropout_proba=0.0, embedding_scale=1.0)


def _check_table(kb, start, want_start, want_rows):
    kb = kb.numpy()
    assert kb.dtype == np.float32 and kb.shape == (len(want_rows), 2)
    np.testing.assert_allclose(kb[:-1].astype(np.float64), np.array(want_rows[:-1]), rtol=RTOL_TABLE)
    assert kb[-1, 0] == 1.0 and kb[-1, 1] == 0.0, "the last step ends at x0: the known latents go in exactly"
    np.testing.assert_allclose(np.array(start, dtype=np.float64), np.array(want_start), rtol=RTOL_TABLE, atol=1e-7)


# ------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("S", [10, 100])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_blend_table_matches_float64_from_the_reference_schedule(S, eta):
    acp = golden("schedule")["linear.alphas_cumprod"]
    gd = _gd(S, eta)
    kb, start = gd.blend_table("ddim")
    want_start, want_rows = np_levels("ddim", acp, pairs=gd.ddim_time_pairs())
    assert [tuple(p) for p in gd.ddim_time_pairs()] == [(int(a), int(b)) for a, b in zip(golden("schedule")[f"ddim_times.{S}"][:-1],
                                                                                         golden("schedule")[f"ddim_times.{S}"][1:])]
    _check_table(kb, start, want_start, want_rows)
    coef, _ = gd.ddim_coeff_table()
    assert kb.shape[0] == coef.shape[0]


def test_ddpm_blend_table_matches_float64_from_the_reference_schedule():
    acp = golden("schedule")["linear.alphas_cumprod"]
    gd = _gd(1000)
    kb, start = gd.blend_table("ddpm")
    want_start, want_rows = np_levels("ddpm", acp)
    _check_table(kb, start, want_start, want_rows)
    assert kb.shape[0] == gd.ddpm_coeff_table()[0].shape[0] == 1000


@pytest.mark.parametrize("S", [10, 100])
def test_vdm_blend_table_is_the_next_level_of_its_own_rows(S):
    """the VDM table is defined by the sampler's own rows (alpha_{i+1}, sigma_{i+1}): bit for bit those columns; against float64 the
    entries carry the float32 rounding of ``t pi / 2`` (an absolute 1e-7 on the angle, which near cos = 0 is more than 2e-6 relative),
    so the float64 comparison has that absolute term, 2e-7 = the angle's rounding + the result's.  Measured: worst relative error 7.1e-8
    at S = 10 and 2.1e-6 at S = 100 (alpha_1 = cos(0.99 pi / 2) = 0.0157, absolute 3.3e-8); worst absolute error 1.8e-7"""
    v = _vdm()
    kb, start = v.blend_table(S)
    rows, _ = v.coeff_table(S)
    assert torch.equal(kb[:-1], rows[:-1, 2:4]) and kb[-1].tolist() == [1.0, 0.0]
    assert list(start) == rows[0, 0:2].tolist()
    assert rows[-1, 2:4].tolist() == [1.0, 0.0], "cos(0), sin(0): the sampler's own last row ends there too"
    want_start, want_rows = np_levels("vdm", S=S)
    np.testing.assert_allclose(kb.numpy().astype(np.float64), np.array(want_rows), rtol=RTOL_TABLE, atol=2e-7)
    np.testing.assert_allclose(np.array(start), np.array(want_start), rtol=RTOL_TABLE, atol=2e-7)


# ------------------------------------------------------------------ 2. / 3. generic loops
SHAPE = (2, 4, 160)
COND = {"cross_attn_cond": None, "cross_attn_masks": None, "global_cond": None, "input_concat_cond": None}


def _models(rng):
    Wm = rng.standard_normal((4, 4)).astype(np.float32) * 0.3

    def np_model(x, t, **kw):
        return np.einsum("oc,bct->bot", Wm, x).astype(np.float32) + (np.asarray(t)[:, None, None] / 1000.0).astype(np.float32)

    def th_model(x, t, **kw):
        return torch.einsum("oc,bct->bot", torch.from_numpy(Wm), x) + (t[:, None, None] / 1000.0).float()
    return np_model, th_model


def _draws(rng, S, uniform=False):
    init = rng.standard_normal(SHAPE).astype(np.float32)
    noises = [(rng.random(SHAPE) if uniform else rng.standard_normal(SHAPE)).astype(np.float32) for _ in range(S)]
    known = (rng.standard_normal(SHAPE) * 0.5).astype(np.float32)
    eps_k = rng.standard_normal(SHAPE).astype(np.float32)
    return init, noises, known, eps_k


def _run(kind, sampler, th_model, init, noises, S, **kw):
    th = lambda a: torch.from_numpy(a)
    kw = {k: (th(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    if kind == "ddim":
        return sampler.ddim_sample(th_model, SHAPE, COND, init_noise=th(init), step_noises=[th(n) for n in noises], **kw)
    if kind == "ddpm":
        return sampler.p_sample_loop(th_model, SHAPE, COND, init_noise=th(init), step_noises=[th(n) for n in noises], **kw)
    return sampler.sample(th_model, SHAPE, COND, step=S, init_noise=th(init), **kw)


def _sampler(kind, S, objective="noise"):
    from jen1_amd.diffusion import get_beta_schedule
    if kind == "ddim":
        return _gd(S, objective=objective), O.OracleGaussianDiffusion(steps=1000, betas=O.get_beta_schedule("linear", 1000), objective=objective,
                                                                      cfg_dropout_proba=0.0, embedding_scale=1.0, sampling_timesteps=S)
    if kind == "ddpm":
        betas, _ = get_beta_schedule("cosine", S)
        return (_gd(S, steps=S, objective=objective, betas=betas),
                O.OracleGaussianDiffusion(steps=S, betas=betas.numpy().astype(np.float32), objective=objective, cfg_dropout_proba=0.0,
                                          embedding_scale=1.0))
    return _vdm(), O.OracleVDM(cfg_dropout_proba=0.0, embedding_scale=1.0)


def _levels(kind, og, S):
    if kind == "ddim":
        return np_levels("ddim", og.alphas_cumprod, pairs=og.ddim_times())
    if kind == "ddpm":
        return np_levels("ddpm", og.alphas_cumprod)
    return np_levels("vdm", S=S)


@pytest.mark.parametrize("kind,objective", [("ddim", "noise"), ("ddim", "x0"), ("ddim", "v"), ("ddpm", "noise"), ("vdm", "v")])
@pytest.mark.parametrize("mask", ["inpaint", "per-sample", "fade"])
def test_generic_loops_with_known_match_numpy_restatement(kind, objective, mask):
    rng = np.random.default_rng(11)
    S = 6
    np_model, th_model = _models(rng)
    init, noises, known, eps_k = _draws(rng, S, uniform=(kind == "ddpm"))
    keep = masks(SHAPE[0], SHAPE[2], mask)
    sampler, og = _sampler(kind, S, objective)
    start, levels = _levels(kind, og, S)
    x_start = np_blend(init, known, keep, eps_k, *start)
    ref = oracle_loop(kind, og, lambda x, t, **kw: np_model(x, t), SHAPE, [COND] * S, x_start, noises,
                      edits=blend_edits(levels, known, keep, eps_k))
    got = _run(kind, sampler, th_model, init, noises, S, known=known, keep_mask=keep, known_noise=eps_k)
    e = rel_err(got.numpy(), ref)
    print(f"{kind}/{objective}/{mask}: rel_err {e:.3e}")
    assert e < GENERIC_TOL
    if mask != "fade":
        assert np.array_equal(got.numpy()[np.broadcast_to(keep == 1, SHAPE)], known[np.broadcast_to(keep == 1, SHAPE)])
    # default known noise: the start draw itself (no additional draw)
    got2 = _run(kind, sampler, th_model, init, noises, S, known=known, keep_mask=keep)
    ref2 = oracle_loop(kind, og, lambda x, t, **kw: np_model(x, t), SHAPE, [COND] * S, np_blend(init, known, keep, init, *start), noises,
                       edits=blend_edits(levels, known, keep, init))
    assert rel_err(got2.numpy(), ref2) < GENERIC_TOL


@pytest.mark.parametrize("kind", ["ddim", "ddpm", "vdm"])
def test_blend_properties_on_the_generic_loops(kind):
    rng = np.random.default_rng(12)
    S = 5
    _, th_model = _models(rng)
    init, noises, known, eps_k = _draws(rng, S, uniform=(kind == "ddpm"))
    sampler, _ = _sampler(kind, S)
    B, _, T = SHAPE
    plain = _run(kind, sampler, th_model, init, noises, S)
    zeros = _run(kind, sampler, th_model, init, noises, S, known=known, keep_mask=masks(B, T, "zeros"), known_noise=eps_k)
    assert torch.equal(zeros, plain), "keep == 0 everywhere must give the bits of the call without known"
    ones = _run(kind, sampler, th_model, init, noises, S, known=known, keep_mask=masks(B, T, "ones"), known_noise=eps_k)
    assert torch.equal(ones, torch.from_numpy(known)), "keep == 1 everywhere must return the known latents"
    for m in ("inpaint", "cont", "per-sample"):
        keep = masks(B, T, m)
        got = _run(kind, sampler, th_model, init, noises, S, known=known, keep_mask=keep, known_noise=eps_k).numpy()
        sel = np.broadcast_to(keep == 1, SHAPE)
        assert np.array_equal(got[sel], known[sel]), m
        assert not np.array_equal(got[~sel], known[~sel]), m
    allsteps = _run(kind, sampler, th_model, init, noises, S, known=known, keep_mask=masks(B, T, "ones"), known_noise=eps_k,
                    return_all_timesteps=True)
    assert allsteps.shape == (B, S + 1) + SHAPE[1:]
    assert torch.equal(allsteps[:, -1], torch.from_numpy(known)) if kind != "ddim" else True     # (DDIM records the INPUT of each step)
    assert not torch.equal(allsteps[:, 0], torch.from_numpy(init)), "the recorded start is the blended one"


# ------------------------------------------------------------------ 4. errors
@pytest.mark.parametrize("kind", ["ddim", "ddpm", "vdm"])
def test_known_argument_errors(kind):
    rng = np.random.default_rng(13)
    S = 3
    _, th_model = _models(rng)
    init, noises, known, eps_k = _draws(rng, S)
    sampler, _ = _sampler(kind, S)
    B, C_, T = SHAPE
    keep = masks(B, T, "inpaint")
    calls = []

    def counting(x, t, **kw):
        calls.append(1)
        return th_model(x, t, **kw)
    bad = [dict(known=known), dict(keep_mask=keep), dict(known=known[:, :, :-1], keep_mask=keep), dict(known=known, keep_mask=keep[:, 0]),
           dict(known=known, keep_mask=np.broadcast_to(keep, SHAPE).copy()), dict(known=known, keep_mask=keep, known_noise=eps_k[:1]),
           dict(known_noise=eps_k)]
    for kw in bad:
        with pytest.raises(ValueError):
            _run(kind, sampler, counting, init, noises, S, **kw)
    assert not calls, "the errors come before anything is launched"


def test_preserve_known_needs_known_audio():
    from jen1_amd.generation import Jen1

    class Enc:
        channels = 2
    g = Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda meta, device: {})
    with pytest.raises(ValueError, match="preserve_known"):
        g.generate("a prompt", seed=1, steps=2, seconds=1, use_gdm=True, task="text_guided", preserve_known=True)
    import inspect
    params = list(inspect.signature(Jen1.generate).parameters)
    assert params[-1] == "preserve_known" and inspect.signature(Jen1.generate).parameters["preserve_known"].default is False
    assert params[1:11] == ["prompt", "seed", "steps", "batch_size", "seconds", "use_gdm", "task", "init_audio", "init_audio_sr", "inpainting_scope"]


# ------------------------------------------------------------------ 5. C ABI
@pytest.fixture(scope="module")
def lib():
    from jen1_amd import lib as L
    L.build()
    return L.load()


def test_blend_entry_points_validate_arguments_without_a_gpu(lib):
    from jen1_amd import lib as L
    assert C.sizeof(L.BlendArgs) == 4 * C.sizeof(C.c_void_p)
    ok = L.BlendArgs(16, 32, 48, 64)
    # (net, x, noise, coef, x_out, step_idx, ticket, rows, parts), ld_rows, B, C, T, ld, nrep, scale, scale_cfg, phi, objective, clip, dtype
    head = (256, 256, None, 256, 256, 256, 256, 256, 256, 128, 2, 128, 64, 128, 1, 1.0, 0, 0.7, 0, 1, L.F32)
    tail = (256, 4, None, 256, 1024)
    err = lambda: lib.jen1_last_error()
    for fn, args in ((lib.jen1_cfg_ddim_step_pack_blend, head), (lib.jen1_step_tail_blend, head + tail)):
        assert fn(*args, None, None) != 0 and b"null blend" in err()
        for i, field in enumerate(("known", "eps_k", "keep", "kb")):
            b = L.BlendArgs(16, 32, 48, 64)
            setattr(b, field, None)
            assert fn(*args, C.byref(b), None) != 0 and b"null known / eps_k / keep / kb" in err(), field
            setattr(b, field, 16 * (i + 1) + 2)
            assert fn(*args, C.byref(b), None) != 0 and b"4-byte aligned" in err(), field
        # the checks of the entry points without the blend still hold
        assert fn(*((None,) + args[1:]), C.byref(ok), None) != 0 and b"null" in err()
        bad_obj = list(args)
        bad_obj[18] = 7
        assert fn(*bad_obj, C.byref(ok), None) != 0 and b"bad objective" in err()
        odd_c = list(args)
        odd_c[11] = 12                                   # C % 8 != 0: no vector form, no blend form
        assert fn(*odd_c, C.byref(ok), None) != 0
    assert lib.jen1_step_tail_blend(*head, 256, 0, None, 256, 1024, C.byref(ok), None) != 0 and b"sentinel table" in err()
    assert lib.jen1_step_tail_blend(*head, 256, 4, None, 256, 1000, C.byref(ok), None) != 0 and b"16-byte aligned and sized" in err()
