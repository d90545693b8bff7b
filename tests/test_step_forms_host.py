"""CPU-only: what test_gpu_step_forms.py measures the sampler step kernels with (tests/step_forms_common.py).

1. The float64 model is anchored to what the project already trusts: short trajectories of it, step by step, against the oracle's
   ddim_sample / p_sample_loop / VDM loops (known_blend_common.oracle_loop restates them one step at a time) and against
   dpm_common.np_dpm_loop, with and without known_blend_common.np_blend after every step, around one stand-in network that goes through
   the oracle's own CFG combine and std rescale.  The coefficient rows come from the product's table builders, which run on the CPU.
2. The elementwise bounds: for every case of the tables the float32 restatement, with sequential and with pairwise sums, stays inside
   half of the bound against the float64 model.
3. The case tables: every entry point meets every value it accepts; the vector cases satisfy the entry points' alignment rules and the
   scalar cases fail them.
"""
import numpy as np
import pytest

import step_forms_common as S
from dpm_common import np_dpm_loop
from helpers import rel_err
from known_blend_common import blend_edits, np_blend, oracle_loop
from oracle import jen1_oracle as O

# a float32 evaluation of a step is within ~50 ulp of its float64 value (the bounds below say so elementwise); over the at most 50 steps
# of the trajectories here, none of which amplifies an error, 1e-5 of the largest value is three orders above that and five below what
# a wrong formula or a wrong coefficient slot would give
ANCHOR_TOL = 1e-5
SHAPE = (2, 6, 9)
F = np.float32


class _Net(O.OracleUNetCFG1d):
    """the oracle's UNetCFG1d.forward (CFG pair, combine, std rescale) around a stand-in for the U-Net: a fixed channel mixing of x, one
    matrix for the conditioned rows and one for the unconditioned rows, plus the time"""

    def __init__(self, C, rng):
        self.dt = np.dtype(np.float32)
        self.p = {"fixed_embedding.embedding.weight": np.zeros((1, 4), dtype=F)}
        self.use_xattn_time = False
        self.Wc = (rng.standard_normal((C, C)) * 0.4).astype(F)
        self.Wu = (rng.standard_normal((C, C)) * 0.4).astype(F)
        self.bias = rng.standard_normal((1, C, 1)).astype(F) * F(0.3)

    def unet(self, x, t, emb, mask, ctx, causal):
        B = SHAPE[0]
        tt = (np.asarray(t, dtype=F)[:, None, None] / F(1000.0)).astype(F)
        y = np.einsum("oc,bct->bot", self.Wc, x[:B]).astype(F) + self.bias + tt[:B]
        if x.shape[0] == 2 * B:                           # the batched pair: the second half is the unconditioned one
            y = np.concatenate([y, np.einsum("oc,bct->bot", self.Wu, x[B:]).astype(F) - self.bias + tt[B:]], axis=0)
        return y.astype(F)

    def rows(self, x, t, nrep):
        """what the step kernels are given: channel-last rows [nrep B][T][C]"""
        B = SHAPE[0]
        tt = np.full((nrep * B,), t)
        return self.unet(np.concatenate([x] * nrep, 0), tt, None, None, None, False).transpose(0, 2, 1)


def _cond(B):
    return {"cross_attn_cond": np.zeros((B, 1, 4), dtype=F), "cross_attn_masks": None, "global_cond": None, "input_concat_cond": None}


def _gd(S_, objective, eta, scale, scale_cfg, steps=1000):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    betas, alphas = get_beta_schedule("linear", steps)
    return GaussianDiffusion(steps=steps, betas=betas, alphas=alphas, objective=objective, loss_type="l2", device="cpu",
                             cfg_dropout_proba=0.0, embedding_scale=scale, batch_cfg=True, scale_cfg=scale_cfg, sampling_timesteps=S_,
                             ddim_sampling_eta=eta)


def _chain(net, rows, times, init, noises, hist, blends, nrep, scale, scale_cfg, objective, clip):
    """the float64 model step after step; between two steps the latents (and the history) are stored in float32, as the kernels store them"""
    B, C, T = SHAPE
    x = np.asarray(init, dtype=F)
    for i, row in enumerate(rows):
        st = S.step_model(net.rows(x, times[i], nrep), x, None if noises is None else noises[i], hist, row, None if blends is None else blends[i],
                          B, C, nrep, scale, scale_cfg, 0.7, objective, clip)
        x = st.val["x_next"].astype(F)
        if hist is not None:
            hist = st.val["hist"].astype(F)
    return x


def _blend_ops(rng, kb):
    B, C, T = SHAPE
    known, eps_k = (rng.standard_normal(SHAPE) * 0.5).astype(F), rng.standard_normal(SHAPE).astype(F)
    keep = S.keep_mask(B, T, rng)
    levels = [(float(p), float(q)) for p, q in kb.tolist()]
    return [(known, eps_k, keep, p, q) for p, q in levels], blend_edits(levels, known, keep[:, None, :], eps_k)


@pytest.mark.parametrize("blend", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("cfg", [(1, 1.0, False), (2, 0.8, False), (2, 0.8, True)], ids=["nocfg", "cfg", "cfg-rescale"])
@pytest.mark.parametrize("objective", S.OBJECTIVES)
def test_model_matches_oracle_ddim(objective, cfg, blend):
    """kinds 0 and 1: rows of ddim_coeff_table (eta = 1: every step draws noise), kb of blend_table"""
    nrep, scale, scale_cfg = cfg
    rng = np.random.default_rng(31)
    net = _Net(SHAPE[1], rng)
    n = 5
    gd = _gd(n, objective, 1.0, scale, scale_cfg)
    rows, times = gd.ddim_coeff_table()
    rows, times = rows.numpy(), times.tolist()
    assert rows[:-1, 5].tolist() == [0.0] * (n - 1) and rows[-1, 5] == 1.0 and (rows[:-1, 4] != 0).all()
    og = O.OracleGaussianDiffusion(steps=1000, betas=O.get_beta_schedule("linear", 1000), objective=objective, cfg_dropout_proba=0.0,
                                   embedding_scale=scale, batch_cfg=True, scale_cfg=scale_cfg, sampling_timesteps=n, ddim_sampling_eta=1.0)
    init = rng.standard_normal(SHAPE).astype(F)
    noises = [rng.standard_normal(SHAPE).astype(F) for _ in range(n)]
    blends, edits = _blend_ops(rng, gd.blend_table("ddim")[0]) if blend else (None, None)
    ref = oracle_loop("ddim", og, net, SHAPE, [_cond(SHAPE[0])] * n, init, noises, edits=edits)
    got = _chain(net, rows, times, init, noises, None, blends, nrep, scale, scale_cfg, objective, 1)
    e = rel_err(got, ref)
    print(f"ddim {objective} nrep={nrep} rescale={scale_cfg} blend={blend}: rel_err {e:.2e}")
    assert e < ANCHOR_TOL


@pytest.mark.parametrize("blend", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("objective", S.OBJECTIVES)
def test_model_matches_oracle_ddpm(objective, blend):
    """kind 2: rows of ddpm_coeff_table, the row of t = 0 with sd = 0 included"""
    rng = np.random.default_rng(32)
    net = _Net(SHAPE[1], rng)
    n = 50
    gd = _gd(None, objective, 1.0, 0.8, True, steps=n)
    rows, times = gd.ddpm_coeff_table()
    rows, times = rows.numpy(), times.tolist()
    assert (rows[:, 5] == 2.0).all() and rows[-1, 4] == 0.0 and (rows[:-1, 4] != 0).all()
    og = O.OracleGaussianDiffusion(steps=n, betas=O.get_beta_schedule("linear", n), objective=objective, cfg_dropout_proba=0.0,
                                   embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    init = rng.standard_normal(SHAPE).astype(F)
    noises = [rng.random(SHAPE).astype(F) for _ in range(n)]
    blends, edits = _blend_ops(rng, gd.blend_table("ddpm")[0]) if blend else (None, None)
    ref = oracle_loop("ddpm", og, net, SHAPE, [_cond(SHAPE[0])] * n, init, noises, edits=edits)
    got = _chain(net, rows, times, init, noises, None, blends, 2, 0.8, 1, objective, 1)
    e = rel_err(got, ref)
    print(f"ddpm {objective} blend={blend}: rel_err {e:.2e}")
    assert e < ANCHOR_TOL


@pytest.mark.parametrize("blend", [False, True], ids=["plain", "blend"])
def test_model_matches_oracle_vdm(blend):
    """kind 3: rows of VDM.coeff_table, kb of VDM.blend_table; clip off, no noise"""
    from jen1_amd.vdm import VDM
    rng = np.random.default_rng(33)
    net = _Net(SHAPE[1], rng)
    n = 6
    vd = VDM(loss_type="l2", device="cpu", cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    rows, times = vd.coeff_table(n)
    rows, times = rows.numpy(), times.tolist()
    assert (rows[:, 5] == 3.0).all()
    ov = O.OracleVDM(cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    init = rng.standard_normal(SHAPE).astype(F)
    blends, edits = _blend_ops(rng, vd.blend_table(n)[0]) if blend else (None, None)
    ref = oracle_loop("vdm", ov, net, SHAPE, [_cond(SHAPE[0])] * n, init, [None] * n, edits=edits)
    got = _chain(net, rows, times, init, None, None, blends, 2, 0.8, 1, "v", 0)
    e = rel_err(got, ref)
    print(f"vdm blend={blend}: rel_err {e:.2e}")
    assert e < ANCHOR_TOL


@pytest.mark.parametrize("blend", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("objective", S.OBJECTIVES)
def test_model_matches_dpm_loop(objective, order, blend):
    """kind 4 (b1 == 0 in row 0 and at order 1, != 0 elsewhere at order 2) and its closing kind-1 row: rows of dpm_coeff_table; the
    history is the clipped, unblended x0"""
    rng = np.random.default_rng(34)
    net = _Net(SHAPE[1], rng)
    n = 6
    gd = _gd(n, objective, 1.0, 0.8, True)
    rows, times = gd.dpm_coeff_table(order)
    rows, times = rows.numpy(), times.tolist()
    assert (rows[:-1, 5] == 4.0).all() and rows[-1, 5] == 1.0 and rows[0, 4] == 0.0 and ((rows[1:-1, 4] != 0).all() == (order == 2))
    og = O.OracleGaussianDiffusion(steps=1000, betas=O.get_beta_schedule("linear", 1000), objective=objective, cfg_dropout_proba=0.0,
                                   embedding_scale=0.8, batch_cfg=True, scale_cfg=True, sampling_timesteps=n)
    init = rng.standard_normal(SHAPE).astype(F)
    blends, edits = _blend_ops(rng, gd.blend_table("ddim")[0]) if blend else (None, None)
    ref = np_dpm_loop(og, net, SHAPE, [_cond(SHAPE[0])] * n, init, order=order, edits=edits)
    hist = np.full(SHAPE, np.nan, dtype=F)                # row 0 has b1 == 0 and must not read it
    got = _chain(net, rows, times, init, None, hist, blends, 2, 0.8, 1, objective, 1)
    e = rel_err(got, ref)
    print(f"dpm {objective} order={order} blend={blend}: rel_err {e:.2e}")
    assert np.isfinite(got).all() and e < ANCHOR_TOL


def test_blend_is_np_blend():
    """the float32 restatement's blend is known_blend_common.np_blend bit for bit, and an exact select where keep is 0 or 1"""
    c = next(c for c in S.PACK_CASES if c.entry == "cfg_ddim_step_pack_blend" and c.row == "k0" and c.shape[2] > 32)
    d = S.case_inputs(c)
    args, kw = S.model_args(c, d)
    plain = S.step_f32(*(args[:5] + (None,) + args[6:]), **kw).val["x_next"]
    got = S.step_f32(*args, **kw).val["x_next"]
    p, q = S.blend_level()
    keep = d["keep"][:, None, :]
    assert np.array_equal(got.view(np.uint32), np_blend(plain, d["known"], keep, d["eps_k"], p, q).view(np.uint32))
    kn = (p * d["known"]).astype(F) + (q * d["eps_k"]).astype(F)
    k3 = np.broadcast_to(keep, got.shape)
    assert (k3 == 1).any() and (k3 == 0).any() and ((k3 > 0) & (k3 < 1)).any()
    assert np.array_equal(got[k3 == 1], kn[k3 == 1]) and np.array_equal(got[k3 == 0], plain[k3 == 0])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the bounds
# ---------------------------------------------------------------------------------------------------------------------
def _worst_ratio(c, bf16):
    d = S.case_inputs(c, bf16=bf16)
    args, kw = S.model_args(c, d, bf16=bf16)
    m = S.step_model(*args, **kw)
    names = ("o",) if c.entry == "cfg_combine" else tuple(m.val)
    worst = {}
    for sums in ("seq", "pairwise"):
        f = S.step_f32(*args, sums=sums, **kw)
        for k in names:
            diff = np.abs(f.val[k].astype(np.float64) - m.val[k])
            err = np.broadcast_to(m.err[k], diff.shape)
            assert np.isfinite(diff).all() and np.isfinite(err).all(), (S.case_id(c), k)
            assert (diff[err == 0] == 0).all(), (S.case_id(c), k)
            r = float((diff[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0
            if k == "rows" and kw["rows_bf16"]:
                # the 2^-8 |value| of a bf16 row IS round-to-nearest's own worst case, not arithmetic that a summation order could share:
                # the stored row stays inside the whole bound, and what it is rounded from (x_next, below) inside half of its own
                assert r <= 1.0, (S.case_id(c), r)
                continue
            worst[k] = max(worst.get(k, 0.0), r)
    return worst


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_float32_restatement_uses_at_most_half_of_every_bound(bf16):
    worst = {}
    for c in S.ALL_CASES:
        for k, r in _worst_ratio(c, bf16).items():
            if r > worst.get((c.entry, k), (0.0, None))[0]:
                worst[(c.entry, k)] = (r, S.case_id(c))
    for (entry, k), (r, cid) in sorted(worst.items()):
        print(f"{entry:26s} {k:7s} worst error / bound {r:.3f}   ({cid})")
    bad = {k: v for k, v in worst.items() if v[0] > 0.5}
    assert not bad, bad


def test_bound_notices_a_wrong_result():
    """without the std rescale the bounds are a few ulp wide: an x_next that is off by 2^-18 of its size is outside for most elements, and
    so are parts without their last column"""
    c = next(c for c in S.PACK_CASES if c.row == "k0" and not c.scale_cfg and S.shape_fields(c.shape)[2] % 32 not in (0, 1))
    d = S.case_inputs(c)
    args, kw = S.model_args(c, d)
    m = S.step_model(*args, **kw)
    xn = m.val["x_next"]
    assert (np.abs(xn * 2.0 ** -18) > m.err["x_next"]).mean() > 0.5
    T = xn.shape[2]
    short = xn[:, :, T - T % 32:T - 1].sum(-1)                         # the last time block without its last column
    assert (np.abs(short - m.val["parts"][:, -1, :, 0]) > m.err["parts"][:, -1, :, 0]).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------------
# 3. the case tables
# ---------------------------------------------------------------------------------------------------------------------
def test_case_tables_cover_what_every_entry_point_accepts():
    assert {c.entry for c in S.ALL_CASES} == set(S.ENTRY_POINTS)
    for table, shapes in ((S.SCALAR_CASES, S.SCALAR_SHAPES), (S.VEC_UNPACKED_CASES, S.VEC_SHAPES), (S.PACK_CASES, S.VEC_SHAPES),
                          (S.TAIL_CASES, S.VEC_SHAPES)):
        for entry in sorted({c.entry for c in table}):
            cs = [c for c in table if c.entry == entry]
            assert len(set(cs)) == len(cs), entry
            assert {c.shape[:-1] for c in cs} == {s[:-1] for s in shapes}, entry                  # every shape
            assert {c.scale_cfg for c in cs} == {0, 1} and {c.phi for c in cs} == set(S.PHIS), entry
            assert {(c.scale_cfg, c.phi) for c in cs if c.shape[-1] == 2} == {(a, b) for a in (0, 1) for b in S.PHIS}, entry
            if entry == "cfg_combine":
                assert all(c.shape[-1] == 2 for c in cs)
                continue
            rows = S.MS_ROWS if entry.endswith("_ms") else S.NOISE_ROWS
            assert {c.row for c in cs} == set(rows), entry                                        # every row kind the form takes
            assert {c.shape[-1] for c in cs} == {1, 2}, entry                                     # both nrep
            assert {c.objective for c in cs} == set(S.OBJECTIVES) and {c.clip for c in cs} == {0, 1}, entry
            assert {(c.objective, c.clip) for c in cs if c.row != "k3"} == {(o, k) for o in S.OBJECTIVES for k in (0, 1)}, entry
            assert all(c.clip == 0 for c in cs if c.row == "k3")
            assert any(c.scale_cfg and c.shape[-1] == 2 and c.row == r for c in cs for r in rows)
            if entry.endswith("_ms"):
                assert {c.blend for c in cs} == {False, True} and {c.blend for c in cs if c.row == "k4"} == {False, True}, entry
            else:
                assert all(c.blend == entry.endswith("_blend") for c in cs), entry
            if entry in ("cfg_ddim_step", "cfg_ddim_step_adv"):
                assert {c.outs for c in cs} == {False, True}, entry
            assert {c.indexed for c in cs} == ({False, True} if entry == "cfg_ddim_step" else {True}), entry
            assert any(S.bit_exact(c) for c in cs), entry
    rows_seen = {c.row for c in S.ALL_CASES if c.row}
    assert rows_seen == set(S.ROW_KINDS)
    assert {S.ROW_KIND_ID[r] for r in rows_seen} == {0, 1, 2, 3, 4}


def test_coefficient_rows_are_what_they_say():
    for v in (0, 1):
        for name in S.ROW_KINDS:
            r = S.coef_row(name, v)
            assert r.dtype == np.float32 and r.shape == (8,) and r[5] == S.ROW_KIND_ID[name]
            assert r[1] >= 0.05                                        # sqrt_recipm1 (sigma_t of a VDM row) as in the product's tables
        assert S.coef_row("k0", v)[4] != 0 and S.coef_row("k0_det", v)[4] == 0 and S.coef_row("k2", v)[4] != 0
        assert S.coef_row("k4_first", v)[4] == 0 and S.coef_row("k4", v)[4] != 0
        assert not np.array_equal(S.coef_row("k0", 0), S.coef_row("k0", 1))
    # a DDIM row at eta = 0 and the first-order multistep row are the same update in two forms: b0 = sqrt(an) - a sqrt(a) sigma-ratio
    k0, k4 = S.coef_row("k0_det").astype(np.float64), S.coef_row("k4_first").astype(np.float64)
    assert abs(k4[2] - (k0[2] - k0[6] * k4[3])) < 1e-6


def test_vector_cases_are_aligned_and_scalar_cases_are_not():
    for s in S.VEC_SHAPES:
        assert S.is_vector(s, 2) and S.is_vector(s, 4), s
    for s in S.SCALAR_SHAPES:
        assert not S.is_vector(s, 2) and not S.is_vector(s, 4), s
        B, C, T, ld, nrep = s
        assert 2 <= C <= 256 and ld >= C                                # and the general kernel takes them
    assert {s[2] % 32 for s in S.VEC_SHAPES} >= {0, 1, 31} and min(s[2] for s in S.VEC_SHAPES) < 32
    assert any(s[3] > s[1] for s in S.VEC_SHAPES) and any(s[4] > s[1] for s in S.VEC_SHAPES)
    for sizes, zero_bytes in S.TAIL_FILLS:
        assert all(b % 16 == 0 for b in sizes) and zero_bytes % 16 == 0
    assert {len(s) for s, _ in S.TAIL_FILLS} == {1, 3}
    assert {min(64, -(-z // (1 << 18))) for _, z in S.TAIL_FILLS} == {1, 2, 64} and max(z for _, z in S.TAIL_FILLS) > 64 << 18
