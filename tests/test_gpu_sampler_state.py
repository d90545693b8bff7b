"""-m gpu: the state that the fused sampler step carries from one step to the next (DDIMStepper, jen1_step_tail).

A replayed step ends in one launch that writes the DDIM / DDPM / VDM update of the latents, the next step's packed network input rows and
their GroupNorm partials, the next step's sentinels and the arena reset.  The host decides when that carried state may be trusted, and the
plans it lives in are shared by every stepper of the same shape.  Here:

  A  the fused tail against the separate launches (JEN1_STEP_PACK=0 JEN1_STEP_TAIL=0, eager) bit for bit over a matrix of cases on the full
     model, and after every fused step the carried network input against a fresh pack_input of the same latents;
  B  state coherence: schedules of different samplers on one plan, edits of the latents / concat context / conditioning between steps,
     the batch split over two plans (n_streams = 2), the step-index use of bench.py, two steppers interleaved on one plan -- against the
     numpy oracle (tiny model, float32) and bitwise against the unfused path (tiny and full bf16 model);
  C  a plan outside jen1_step_tail's preconditions falls back to the step-pack launch.

Every random draw is injected, so every comparison is deterministic.  Bitwise comparisons run on plans with fixed-order statistics: the
default plan has them everywhere when its long levels run as the sample-resident launch; any other plan is built with
Plan(deterministic=True).  So is the B = 1, T = 9000 CFG plan: its default form is not run-to-run reproducible (two runs of the separate
launches already differ), so bits of the fused tail cannot be compared there.
"""
import contextlib

import numpy as np
import pytest
import torch

from helpers import filled, rel_err
from jen1_amd import synth
from jen1_amd.config import UNetSpec, full_model_config, tiny_model_config

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3          # float32 against the oracle (BASELINE.json; test_gpu_model.py)
PATH_TOL = 2e-5         # float32 across execution paths (test_gpu_deep.py)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cond_dev(cond):
    return {k: dev(v) for k, v in cond.items()}


def _model(dtype, tiny=False):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.model import UNetCFG1d
    cfg = tiny_model_config() if tiny else full_model_config()
    return UNetCFG1d(**cfg, init_seed=1234, compute_dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def tiny_f32():
    return _model("f32", tiny=True)


@pytest.fixture(scope="module")
def oracle_tiny():
    from oracle import jen1_oracle as O
    cfg = tiny_model_config()
    return O.OracleUNetCFG1d(filled(UNetSpec(**cfg).param_shapes()), **cfg)


@pytest.fixture(scope="module")
def full_models():
    """built on first use: {"bf16", "f32", "fp8"} -> UNetCFG1d of the full configuration"""
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = _model(dtype)
        return made[dtype]
    return get


@contextlib.contextmanager
def fixed_order(m, on):
    old = m.deterministic
    m.deterministic = bool(on)
    try:
        yield
    finally:
        m.deterministic = old


def needs_fixed_order(m, B, T, nrep, causal, S):
    """True when the default sampler plan of this shape keeps float-atomic statistics somewhere (launch-per-layer levels), i.e. is
    not bit-reproducible by itself"""
    with fixed_order(m, False):
        plan = m.engine().plan(B, T, nrep, causal, slot=0, n_t=S)
    return not (plan.use_long and plan.deep_level is not None)


@contextlib.contextmanager
def step_flags(monkeypatch, fused):
    with monkeypatch.context() as mp:
        mp.setenv("JEN1_STEP_PACK", "1" if fused else "0")
        mp.setenv("JEN1_STEP_TAIL", "1" if fused else "0")
        yield


def gdm(S, scale=0.8, objective="noise", eta=1.0, steps=1000, betas=None):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    if betas is None:
        betas, _ = get_beta_schedule("linear", steps)
    return GaussianDiffusion(steps=steps, betas=betas, objective=objective, loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                             embedding_scale=scale, batch_cfg=True, scale_cfg=True, sampling_timesteps=S, ddim_sampling_eta=eta)


def vdm(S, scale=0.8):
    from jen1_amd.vdm import VDM
    v = VDM(loss_type="l2", device="cuda", cfg_dropout_proba=0.0, embedding_scale=scale, batch_cfg=True, scale_cfg=True)
    v._steps = S                    # (the schedule length DDIMStepper reads: VDM.p_sample_loop sets it the same way)
    return v


def stepper(sampler, m, shape, cond, monkeypatch, fused, use_graph, mode="ddim", causal=False, n_streams=1, plan_slot=0):
    from jen1_amd.diffusion import DDIMStepper
    with step_flags(monkeypatch, fused):
        st = DDIMStepper(sampler, m, shape, cond, causal=causal, use_graph=use_graph, n_streams=n_streams, plan_slot=plan_slot, mode=mode)
    assert st.fused_pack == fused
    return st


def packed_input(plan):
    """the plan's network input activation (all nrep * B rows, the concat-context channels included) and its GroupNorm statistics"""
    X0 = next(a for a in plan.acts if a.t.data_ptr() == plan.pack_rows[0])
    return X0.t, X0.gn


def trajectory(st, init, noises, after=None, check_pack=False):
    """reset at ``init``, step through the schedule with injected noise; ``after(i, st)`` runs after step i (edits).  Returns the latents
    after step 0 and after the last step.  check_pack: after every step the carried network input must equal a pack of the same
    latents / context, rows and statistics bit for bit."""
    st.reset(init, fresh_noise=False)
    first = None
    for i in range(st.num_steps):
        st.step(i, noise=noises[i] if noises is not None else None)
        if check_pack:
            for _, plan, _, _ in st.parts:
                rows, gn = packed_input(plan)
                keep_rows, keep_gn = rows.clone(), gn.clone()
                plan.run_pack()
                assert torch.equal(rows, keep_rows), f"step {i}: the rows the step kernel carried differ from pack_input's"
                assert torch.equal(gn, keep_gn), f"step {i}: the statistics the step kernel carried differ from pack_input's"
        if i == 0:
            first = st.x.clone()
        if after is not None:
            after(i, st)
    st.check()
    torch.cuda.synchronize()
    return first, st.x.clone()


# ================================================================== A. fused tail == separate launches, full model
A_CASES = {
    # id: (dtype, B, T, S, sampler, scale, objective, eta, task, causal, fixed-order statistics: None = when the default plan needs them)
    "bf16-B8-nocfg-noise": ("bf16", 8, 1500, 3, "ddim", 1.0, "noise", 1.0, "text_guided", False, None),
    "bf16-B3-T1499-cfg3-x0": ("bf16", 3, 1499, 3, "ddim", 3.0, "x0", 1.0, "text_guided", False, None),
    "bf16-B2-inpaint-cfg": ("bf16", 2, 1500, 3, "ddim", 0.8, "v", 0.0, "music_inpaint", False, None),
    "bf16-B2-cont-causal": ("bf16", 2, 1500, 3, "ddim", 1.0, "noise", 1.0, "music_cont", True, None),
    "bf16-B2-ddpm": ("bf16", 2, 1500, 4, "ddpm", 0.8, "noise", 1.0, "music_inpaint", False, None),
    "bf16-B2-vdm": ("bf16", 2, 1500, 3, "vdm", 0.8, "v", 1.0, "music_cont", False, None),
    "f32-B2-inpaint": ("f32", 2, 1500, 3, "ddim", 0.8, "noise", 1.0, "music_inpaint", False, None),
    "fp8-B1-T9000-cfg-cont-causal": ("fp8", 1, 9000, 3, "ddim", 0.8, "noise", 1.0, "music_cont", True, True),
}


def make_sampler(kind, S, scale, objective, eta):
    from jen1_amd.diffusion import get_beta_schedule
    if kind == "ddim":
        return gdm(S, scale, objective, eta), "ddim"
    if kind == "ddpm":
        betas, _ = get_beta_schedule("cosine", S)
        return gdm(S, scale, objective, steps=S, betas=betas), "ddpm"
    return vdm(S, scale), "vdm"


@pytest.mark.parametrize("case", list(A_CASES), ids=list(A_CASES))
def test_fused_tail_matches_separate_launches(full_models, monkeypatch, case):
    dtype, B, T, S, kind, scale, objective, eta, task, causal, fixed = A_CASES[case]
    m = full_models(dtype)
    sampler, mode = make_sampler(kind, S, scale, objective, eta)
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, task))
    init = dev(synth.noise_list(1, shape, seed=41)[0])
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=43, uniform=(mode == "ddpm"))]
    det = needs_fixed_order(m, B, T, 2 if scale != 1.0 else 1, causal, S) if fixed is None else fixed
    with fixed_order(m, det):
        ref = stepper(sampler, m, shape, cond, monkeypatch, False, False, mode, causal)
        want = trajectory(ref, init, noises)
        st = stepper(sampler, m, shape, cond, monkeypatch, True, True, mode, causal)
        assert st.fused_tail, "the default stepper of this case should end its step in jen1_step_tail"
        assert st.plan is ref.plan
        got = trajectory(st, init, noises, check_pack=True)
    assert torch.isfinite(want[1]).all()
    assert torch.equal(got[0], want[0]), f"{case}: step 0 differs from the separate launches ({rel_err(got[0].cpu(), want[0].cpu()):.3e})"
    assert torch.equal(got[1], want[1]), f"{case}: the last step differs from the separate launches ({rel_err(got[1].cpu(), want[1].cpu()):.3e})"


# ================================================================== B. state coherence
def oracle_loop(kind, sampler_o, onet, shape, conds, init, noises, edits=None, causal=False):
    """the oracle's sampling loop one step at a time (OracleGaussianDiffusion.ddim_sample / p_sample_loop, OracleVDM.sample):
    conds[i] conditions step i, edits[i](x) -> x is applied after step i"""
    from oracle import jen1_oracle as O
    f = np.float32
    B = shape[0]
    x = np.asarray(init, dtype=f).reshape(shape)
    edits = edits or {}
    if kind == "ddim":
        sched = sampler_o.ddim_times()
    elif kind == "ddpm":
        sched = [(t, None) for t in reversed(range(sampler_o.num_timesteps))]
    else:
        steps = O.linspace_f32(1.0, 0.0, len(noises) + 1)
        al, sg = np.cos(steps * f(np.pi / 2)).astype(f), np.sin(steps * f(np.pi / 2)).astype(f)
        sched = list(range(len(noises)))
    for i, t in enumerate(sched):
        if kind == "ddim":
            t, tn = t
            eps, x0 = sampler_o.model_predictions(x, np.full((B,), t, np.int64), onet, conds[i], clip_x_start=True, causal=causal)
            if tn < 0:
                x = x0
            else:
                sa, c, sigma = sampler_o.ddim_coeffs(t, tn)
                x = (x0 * sa + c * eps + sigma * np.asarray(noises[i], dtype=f)).astype(f)
        elif kind == "ddpm":
            t = t[0]
            tt = np.full((B,), t, np.int64)
            _, x0 = sampler_o.model_predictions(x, tt, onet, conds[i], clip_x_start=False, causal=False)
            x0 = np.clip(x0, -1.0, 1.0)
            ex = lambda a: sampler_o._ex(a, tt, 3)
            mean = ex(sampler_o.posterior_mean_coef1) * x0 + ex(sampler_o.posterior_mean_coef2) * x
            noise = np.asarray(noises[i], dtype=f) if t > 0 else 0.0
            x = (mean + np.exp(0.5 * ex(sampler_o.posterior_log_variance_clipped)) * noise).astype(f)
        else:
            v = sampler_o._model_call(onet, x, np.full((B,), steps[i], dtype=f), conds[i], causal, None)
            x_pred = al[i] * x - sg[i] * v
            noise_pred = sg[i] * x + al[i] * v
            x = (al[i + 1] * x_pred + sg[i + 1] * noise_pred).astype(f)
        if i in edits:
            x = edits[i](x)
    return x


def oracle_gd(S, scale=0.8, steps=1000, betas=None):
    from oracle import jen1_oracle as O
    if betas is None:
        betas = O.get_beta_schedule("linear", steps)
    return O.OracleGaussianDiffusion(steps=steps, betas=np.asarray(betas, dtype=np.float32), objective="noise", cfg_dropout_proba=0.0,
                                     embedding_scale=scale, batch_cfg=True, scale_cfg=True, sampling_timesteps=S, ddim_sampling_eta=1.0)


def schedule_set(S):
    """four samplers whose steppers share one plan (same B, T, nrep and S): DDIM over 1000 and over 500 training steps, DDPM with S
    training steps, VDM with S steps"""
    from jen1_amd.diffusion import get_beta_schedule
    from jen1_amd.vdm import VDM
    b500, _ = get_beta_schedule("linear", 500)
    bp, _ = get_beta_schedule("cosine", S)
    return {
        "a": gdm(S),
        "vdm": VDM(loss_type="l2", device="cuda", cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True),
        "b": gdm(S, steps=500, betas=b500),
        "ddpm": gdm(S, steps=S, betas=bp),
    }, {"b": b500.numpy(), "ddpm": bp.numpy()}


def _sample(samplers, name, m, shape, cond, init, noises, unoises, S):
    s = samplers[name]
    if name == "vdm":
        y = s.sample(m, shape, cond, step=S, init_noise=init)
    else:
        y = s.sample(m, shape, cond, init_noise=init, step_noises=unoises if name == "ddpm" else noises)
    torch.cuda.synchronize()
    return y.clone()


ORDER = ("a", "vdm", "b", "ddpm", "a", "vdm")


def test_schedules_sharing_a_plan_tiny_vs_oracle(tiny_f32, oracle_tiny):
    """B.1: DDIM (1000 and 500 training steps), VDM and DDPM of the same length share one plan (Engine.plan's key has no schedule in
    it); each sampler's cached stepper must bring its own schedule tables back when it runs again after another one"""
    from oracle import jen1_oracle as O
    m, S, B, T = tiny_f32, 6, 2, 300
    shape = (B, 128, T)
    c_np = synth.conditioning(B, T, "music_inpaint")
    cond = cond_dev(c_np)
    init_np = synth.noise_list(1, shape, seed=51)[0]
    n_np = synth.noise_list(S, shape, seed=52)
    u_np = synth.noise_list(S, shape, seed=53, uniform=True)
    init, noises, unoises = dev(init_np), [dev(n) for n in n_np], [dev(n) for n in u_np]
    samplers, betas = schedule_set(S)
    with fixed_order(m, True):
        outs = [(name, _sample(samplers, name, m, shape, cond, init, noises, unoises, S)) for name in ORDER]
        plans = {id(st.plan) for s in samplers.values() for st in s._steppers.values()}
    assert len(plans) == 1, "the four samplers were meant to share one plan"
    first = {}
    for name, y in outs:
        if name in first:
            assert torch.equal(y, first[name]), f"{name} after the others: {rel_err(y.cpu(), first[name].cpu()):.3e} from its first call"
        else:
            first[name] = y
    conds = [c_np] * S
    ov = O.OracleVDM(cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    refs = {"a": oracle_loop("ddim", oracle_gd(S), oracle_tiny, shape, conds, init_np, n_np),
            "b": oracle_loop("ddim", oracle_gd(S, steps=500, betas=betas["b"]), oracle_tiny, shape, conds, init_np, n_np),
            "ddpm": oracle_loop("ddpm", oracle_gd(S, steps=S, betas=betas["ddpm"]), oracle_tiny, shape, conds, init_np, u_np),
            "vdm": oracle_loop("vdm", ov, oracle_tiny, shape, conds, init_np, [None] * S)}
    for name, y in first.items():
        e = rel_err(y.cpu().numpy(), refs[name])
        assert e < F32_TOL, (name, e)


def test_schedules_sharing_a_plan_full_bf16(full_models):
    """B.1 on the full model in bf16 (the plan carries the tail launch): every repeated call bit-identical to its first call"""
    m, S, B, T = full_models("bf16"), 6, 2, 1500
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, "music_inpaint"))
    init = dev(synth.noise_list(1, shape, seed=51)[0])
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=52)]
    unoises = [dev(n) for n in synth.noise_list(S, shape, seed=53, uniform=True)]
    samplers, _ = schedule_set(S)
    with fixed_order(m, needs_fixed_order(m, B, T, 2, False, S)):
        outs = [(name, _sample(samplers, name, m, shape, cond, init, noises, unoises, S)) for name in ORDER]
    sts = [st for s in samplers.values() for st in s._steppers.values()]
    assert len({id(st.plan) for st in sts}) == 1 and all(st.fused_tail for st in sts)
    first = {}
    for name, y in outs:
        assert torch.isfinite(y).all()
        if name in first:
            assert torch.equal(y, first[name]), f"{name} after the others: {rel_err(y.cpu(), first[name].cpu()):.3e} from its first call"
        else:
            first[name] = y
    assert not torch.equal(first["a"], first["b"])


def repaint(ogd, B, T, S, span):
    """after step i < S-1: the latents on ``span`` replaced by a fixed clip q_sample'd to the step's next timestep with an injected
    noise (the repaint / inpainting edit), as numpy arrays {i: known [B, 128, T]}"""
    clip = synth.latents(B, T, key="repaint")
    en = synth.noise_list(S, (B, 128, T), seed=61)
    times = ogd.ddim_times()
    return {i: ogd.q_sample(clip, np.full((B,), times[i][1], np.int64), en[i]).astype(np.float32) for i in range(S - 1)}


def edit_run(st, init, noises, known, span, ctx_at=None, ctx_new=None, rebind_at=None, cond_new=None, via_setter=False):
    a, b = span
    known_d = {i: dev(k) for i, k in known.items()}

    def after(i, st):
        if i in known_d:
            if via_setter:
                x = st.x.clone()
                x[..., a:b] = known_d[i][..., a:b]
                st.set_x(x)
            else:
                st.x[..., a:b] = known_d[i][..., a:b]         # in place, into the plan's own buffer
        if i == ctx_at:
            st.plan.ctx_in.copy_(ctx_new)                       # the concat context, in place
        if i == rebind_at:
            st.rebind(cond_new)
    return trajectory(st, init, noises, after)


def oracle_edits(known, span):
    a, b = span

    def mk(k):
        def f(x):
            x = x.copy()
            x[..., a:b] = k[..., a:b]
            return x
        return f
    return {i: mk(k) for i, k in known.items()}


@pytest.mark.parametrize("what", ["latents", "context", "rebind"])
def test_edits_between_steps_tiny_vs_oracle(tiny_f32, oracle_tiny, monkeypatch, what):
    """B.2: a repaint-style write into st.x after every step, an in-place write of the plan's concat context, rebind() to another
    task's conditioning mid-trajectory: the fused pack must take them up exactly as the unfused path does, and both must follow the
    oracle loop that applies the same edits"""
    m, S, B, T = tiny_f32, 6, 2, 300
    shape, span = (B, 128, T), (90, 210)
    c0, c1 = synth.conditioning(B, T, "music_inpaint"), synth.conditioning(B, T, "music_cont")
    init_np, n_np = synth.noise_list(1, shape, seed=71)[0], synth.noise_list(S, shape, seed=72)
    init, noises = dev(init_np), [dev(n) for n in n_np]
    ogd = oracle_gd(S)
    known = repaint(ogd, B, T, S, span) if what == "latents" else {}
    at = 2
    kw = {}
    conds = [c0] * S
    if what == "context":
        kw = dict(ctx_at=at, ctx_new=dev(c1["input_concat_cond"]))
        conds = [c0] * (at + 1) + [dict(c0, input_concat_cond=c1["input_concat_cond"])] * (S - at - 1)
    elif what == "rebind":
        kw = dict(rebind_at=at, cond_new=cond_dev(c1))
        conds = [c0] * (at + 1) + [c1] * (S - at - 1)
    gd = gdm(S)
    outs = []
    with fixed_order(m, True):
        for fused, ug in ((False, False), (True, False), (True, True)):
            st = stepper(gd, m, shape, cond_dev(c0), monkeypatch, fused, ug)
            outs.append(edit_run(st, init, noises, known, span, **kw))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1]), \
            f"{what}: the fused pack differs from the unfused path ({rel_err(o[1].cpu(), outs[0][1].cpu()):.3e})"
    ref = oracle_loop("ddim", ogd, oracle_tiny, shape, conds, init_np, n_np, edits=oracle_edits(known, span))
    e = rel_err(outs[0][1].cpu().numpy(), ref)
    assert e < F32_TOL, (what, e)


def test_edits_between_steps_full_bf16(full_models, monkeypatch):
    """B.2 on the full model (tail launch): latents, concat context and rebind in one trajectory, bit for bit against the unfused path"""
    m, S, B, T = full_models("bf16"), 4, 2, 1500
    shape, span = (B, 128, T), (450, 1050)
    c0, c1 = synth.conditioning(B, T, "music_inpaint"), synth.conditioning(B, T, "text_guided")
    init = dev(synth.noise_list(1, shape, seed=71)[0])
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=72)]
    known = repaint(oracle_gd(S), B, T, S, span)
    gd = gdm(S)
    outs = []
    with fixed_order(m, needs_fixed_order(m, B, T, 2, False, S)):
        for fused, ug in ((False, False), (True, True)):
            st = stepper(gd, m, shape, cond_dev(c0), monkeypatch, fused, ug)
            assert st.fused_tail == fused
            outs.append(edit_run(st, init, noises, known, span, ctx_at=0, ctx_new=dev(synth.concat_cond(B, T, "music_cont")),
                                 rebind_at=1, cond_new=cond_dev(c1)))
    assert torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1]), \
        f"the tail path differs from the unfused path with edits ({rel_err(outs[1][1].cpu(), outs[0][1].cpu()):.3e})"


@pytest.mark.parametrize("B", [8, 3])
def test_two_streams_tiny_vs_oracle(tiny_f32, oracle_tiny, monkeypatch, B):
    """B.3: the batch split over two plans (n_streams = 2: 4 + 4 on slots 0 and 1, 2 + 1 on two slot-0 plans), eagerly and as replayed
    graphs: bit for bit its own unfused path, one step within PATH_TOL of one stream (sub-batches of another size sum in another order;
    four steps from t = 999 amplify that to ~1e-4), the trajectory within F32_TOL of the oracle; repaint edits through set_x"""
    m, S, T = tiny_f32, 4, 300
    shape, span = (B, 128, T), (30, 150)
    c_np = synth.conditioning(B, T, "music_inpaint")
    init_np, n_np = synth.noise_list(1, shape, seed=81)[0], synth.noise_list(S, shape, seed=82)
    init, noises = dev(init_np), [dev(n) for n in n_np]
    ogd = oracle_gd(S)
    known = repaint(ogd, B, T, S, span)
    gd = gdm(S)
    res = {}
    with fixed_order(m, True):
        for ns, fused, ug in ((1, False, False), (2, False, False), (2, True, False), (2, True, True), (1, True, True)):
            st = stepper(gd, m, shape, cond_dev(c_np), monkeypatch, fused, ug, n_streams=ns)
            assert len(st.parts) == ns
            res[(ns, fused, ug)] = (trajectory(st, init, noises), edit_run(st, init, noises, known, span, via_setter=True))
    ref = res[(2, False, False)]
    for k in ((2, True, False), (2, True, True)):
        for a, b in zip(res[k], ref):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"n_streams=2 fused={k[1]} graph={k[2]}: differs from its unfused path"
    for one in ((1, False, False), (1, True, True)):
        for a, b in zip(res[one], ref):
            e = rel_err(a[0].cpu().numpy(), b[0].cpu().numpy())
            assert e < PATH_TOL, (one, e)
    conds = [c_np] * S
    plain = oracle_loop("ddim", ogd, oracle_tiny, shape, conds, init_np, n_np)
    edited = oracle_loop("ddim", ogd, oracle_tiny, shape, conds, init_np, n_np, edits=oracle_edits(known, span))
    assert rel_err(ref[0][1].cpu().numpy(), plain) < F32_TOL
    assert rel_err(ref[1][1].cpu().numpy(), edited) < F32_TOL


def test_two_streams_full_bf16(full_models, monkeypatch):
    """B.3 on the full model: B = 3 as 2 + 1, both parts with the tail launch, bit for bit against the unfused split, with set_x edits"""
    m, S, B, T = full_models("bf16"), 4, 3, 1500
    shape, span = (B, 128, T), (450, 1050)
    cond = cond_dev(synth.conditioning(B, T, "music_inpaint"))
    init = dev(synth.noise_list(1, shape, seed=81)[0])
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=82)]
    known = repaint(oracle_gd(S), B, T, S, span)
    gd = gdm(S)
    det = needs_fixed_order(m, 2, T, 2, False, S) or needs_fixed_order(m, 1, T, 2, False, S)
    outs = []
    with fixed_order(m, det):
        for fused, ug in ((False, False), (True, True)):
            st = stepper(gd, m, shape, cond, monkeypatch, fused, ug, n_streams=2)
            assert len(st.parts) == 2 and st.fused_tail == fused
            outs.append((trajectory(st, init, noises), edit_run(st, init, noises, known, span, via_setter=True)))
    for a, b in zip(outs[1], outs[0]):
        assert torch.isfinite(b[1]).all()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "n_streams=2 with the tail launch differs from its unfused path"


def _bench_sequence(st, init, noises):
    """bench.py's timed_steps: the step index wraps without a reset; and one index stepped twice"""
    S = st.num_steps
    st.reset(init, fresh_noise=False)
    seq = list(range(S)) + [0, 1, 1] + list(range(2, S))
    out = []
    for i in seq:
        st.step(i, noise=noises[i])
        out.append(st.x.clone())
    st.check()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_step_index_wrap_and_repeat(tiny_f32, full_models, monkeypatch, which):
    """B.4: step(0) after step(S-1) without reset() (bench.py wraps like this), and step(i) twice: bit for bit the unfused path"""
    m = tiny_f32 if which == "tiny" else full_models("bf16")
    S, B, T = 4, 2, (300 if which == "tiny" else 1500)
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, "music_cont"))
    init = dev(synth.noise_list(1, shape, seed=91)[0])
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=92)]
    gd = gdm(S, scale=1.0)
    det = True if which == "tiny" else needs_fixed_order(m, B, T, 1, False, S)
    with fixed_order(m, det):
        outs = [_bench_sequence(stepper(gd, m, shape, cond, monkeypatch, fused, ug), init, noises)
                for fused, ug in ((False, False), (True, True))]
    for k, (a, b) in enumerate(zip(outs[1], outs[0])):
        assert torch.isfinite(b).all()
        assert torch.equal(a, b), f"call {k} of the wrapped / repeated sequence differs from the unfused path"


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_interleaved_steppers_on_one_plan_raise(tiny_f32, full_models, monkeypatch, which):
    """B.5: two steppers of the same shape and plan_slot share one plan; stepping the first after the second has taken the plan over
    raises (naming plan_slot) instead of running on the other's latents, and a reset() brings back its own tables and conditioning"""
    m = tiny_f32 if which == "tiny" else full_models("bf16")
    S, B, T = 4, 2, (300 if which == "tiny" else 1500)
    shape = (B, 128, T)
    c1, c2 = cond_dev(synth.conditioning(B, T, "music_inpaint")), cond_dev(synth.conditioning(B, T, "music_cont"))
    x1, x2 = (dev(n) for n in synth.noise_list(2, shape, seed=101))
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=102)]
    det = True if which == "tiny" else needs_fixed_order(m, B, T, 2, False, S)
    with fixed_order(m, det):
        st1 = stepper(gdm(S), m, shape, c1, monkeypatch, True, True)
        want = trajectory(st1, x1, noises)
        st2 = stepper(vdm(S), m, shape, c2, monkeypatch, True, True, mode="vdm")
        assert st2.plan is st1.plan
        st1.reset(x1, fresh_noise=False)
        st1.step(0, noise=noises[0])
        st2.reset(x2, fresh_noise=False)
        st2.step(0)
        with pytest.raises(RuntimeError, match="plan_slot"):
            st1.step(1, noise=noises[1])
        got = trajectory(st1, x1, noises)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "after reset() the first stepper does not repeat its own trajectory"


# ================================================================== C. tail eligibility
@pytest.mark.parametrize("how", ["rows", "limit", "arena"])
def test_ineligible_tail_falls_back_to_step_pack(full_models, monkeypatch, how):
    """C: jen1_step_tail rejects a sentinel table outside [1, 60000] rows and an arena that is not 16-byte aligned and sized; the stepper
    checks the same preconditions and keeps the step-pack launch for such a plan (same bits as the tail path) instead of failing"""
    from jen1_amd import diffusion as D
    m, S, B, T = full_models("bf16"), 3, 2, 1500
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, "music_inpaint"))
    init = dev(synth.noise_list(1, shape, seed=111)[0])
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=112)]
    gd = gdm(S)
    with fixed_order(m, needs_fixed_order(m, B, T, 2, False, S)):
        st = stepper(gd, m, shape, cond, monkeypatch, True, True)
        assert st.fused_tail
        want = trajectory(st, init, noises)
        plan = st.plan
        tab, n_rows, sync, zp, zb = plan.poison_args
        with monkeypatch.context() as mp:
            if how == "rows":
                mp.setattr(plan, "poison_args", (tab, 60001, sync, zp, zb))
            elif how == "limit":
                mp.setattr(D, "_TAIL_MAX_ROWS", n_rows - 1)
            else:
                mp.setattr(plan, "poison_args", (tab, n_rows, sync, zp, zb - 4))
            fb = stepper(gd, m, shape, cond, monkeypatch, True, True)
        assert fb.fused_pack and not fb.fused_tail
        assert fb.launches_per_step == st.launches_per_step + 1      # (the sentinel / arena node back at the head of the step)
        got = trajectory(fb, init, noises)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "the step-pack fallback differs from the tail path"
