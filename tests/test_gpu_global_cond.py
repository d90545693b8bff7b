"""-m gpu: global conditioning (``context_features`` / ``features=``) against what the reference computed with it
(tests/golden/global_cond.npz, make_global_cond_golden.py): the tiny configuration + ``context_features = 24``, B = 3 (odd: the CFG pair
makes 6 rows), T = 96, a distinct timestep and distinct features per row.

The mapping, the FiLM GEMM and the selection launch are float32 in both compute modes, so the float32 cases are the discriminating ones
(``helpers.F32_TOL``) and the bf16 cases cover the casts (``helpers.BF16_TOL``).  The fixture's ``y.effect`` (what reversing the feature
rows does to the output, >= 10 x F32_TOL by construction) keeps a parity test from passing while the features are ignored.
Steppers that are compared bit for bit or to 1e-5 run on plans with fixed-order statistics (``model.deterministic``), as the other
sampler tests do on the tiny configuration: float atomics alone move a 4-step trajectory by more than that.
"""
import contextlib
import json

import numpy as np
import pytest
import torch

from helpers import BF16_TOL, F32_TOL, bf16_gate, golden, record_parity, rel_err
from jen1_amd import synth
from jen1_amd.config import full_model_config, tiny_model_config
from jen1_amd.init_fill import fill_normal, fill_uniform

pytestmark = pytest.mark.gpu

F_CTX, B, T, S = 24, 3, 96, 4
TIMES = [999, 499, 7]
SHAPE = (B, 128, T)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def g():
    return golden("global_cond")


def features(g):
    """the fixture's features: its stored scale times the written-down normal draw (make_global_cond_golden.features)"""
    return dev((float(g["feature_scale"]) * fill_normal("synth.features", (B, F_CTX), 5)).astype(np.float32))


def _model(dtype, featured=True, **kw):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.model import UNetCFG1d
    cfg = dict(tiny_model_config(), context_features=F_CTX) if featured else tiny_model_config()
    return UNetCFG1d(**cfg, init_seed=1234, compute_dtype=dtype, device="cuda", **kw)


@pytest.fixture(scope="module")
def models():
    return {"f32": _model("f32"), "bf16": _model("bf16")}


@pytest.fixture(scope="module")
def inputs(g):
    cond = {k: dev(v) for k, v in synth.conditioning(B, T).items()}
    f = features(g)
    return dict(x=dev(synth.latents(B, T)), t=torch.tensor(TIMES, device="cuda"), cond=cond, f=f,
                init=dev(synth.noise_list(1, SHAPE, seed=7)[0]), noises=[dev(n) for n in synth.noise_list(S, SHAPE, seed=11)])


def with_features(cond, f):
    return dict(cond, global_cond=f)


@contextlib.contextmanager
def fixed_order(*ms):
    old = [m.deterministic for m in ms]
    for m in ms:
        m.deterministic = True
    try:
        yield
    finally:
        for m, o in zip(ms, old):
            m.deterministic = o


def gdm(steps=S, **kw):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    betas, _ = get_beta_schedule("linear", 1000)
    args = dict(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0, embedding_scale=0.8,
                batch_cfg=True, scale_cfg=True, sampling_timesteps=steps)
    args.update(kw)
    return GaussianDiffusion(**args)


def forward(m, inp, f, **kw):
    c = inp["cond"]
    y = m(inp["x"], inp["t"], embedding=c["cross_attn_cond"], embedding_mask=c["cross_attn_masks"], embedding_mask_proba=0.0,
          channels_list=[c["input_concat_cond"]], features=f, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


CASES = {"y.nocfg.causal": dict(embedding_scale=1.0, causal=True),
         "y.cfg": dict(embedding_scale=0.8, batch_cfg=True, scale_cfg=True, causal=False),
         "y.cfg.twopass": dict(embedding_scale=0.8, batch_cfg=False, scale_cfg=False, causal=False)}


# ------------------------------------------------------------------ 1. the mapping table
def test_mapping_table_after_run_time(models, inputs, g):
    """rows s B + b of a per-sample plan's mapping table hold mapping(t_s, features_b): the diagonal (s = b) against the reference's
    ``get_mapping`` (three small float32 GEMVs: 1e-5 relative); the general forward's B-row mapping against the same"""
    m = models["f32"]
    eng = m.engine()
    plan = eng.plan(B, T, 2, False, n_t=len(TIMES), per_sample=True, slot=7)
    assert plan.per_sample and tuple(plan.mapping.shape) == (len(TIMES) * B, m.spec.mapping_features)
    assert tuple(plan.film.shape) == (B, eng.W.film_ld) and tuple(plan.film_tab.shape) == (len(TIMES) * B, eng.W.film_ld)
    assert tuple(plan.kvx.t.shape)[1] == len(TIMES)                 # the time-token K/V table does not depend on features
    plan.set_features(inputs["f"])
    plan.set_times(inputs["t"])
    plan.run_time()
    torch.cuda.synchronize()
    tab = plan.mapping.cpu().numpy().reshape(len(TIMES), B, -1)
    diag = np.stack([tab[i, i] for i in range(B)])
    e = rel_err(diag, g["mapping"])
    print(f"mapping table diagonal against get_mapping: {e:.3e}")
    assert e < 1e-5, e
    for s in range(len(TIMES)):          # every row depends on its batch element's features and on its schedule entry
        for b in range(B):
            if s != b:
                assert rel_err(tab[s, b], tab[b, b]) > 1e-3 and rel_err(tab[s, b], tab[s, s]) > 1e-3, (s, b)
    forward(m, inputs, inputs["f"], **CASES["y.cfg"])
    e = rel_err(eng.plan(B, T, 2, False).mapping.cpu().numpy(), g["mapping"])
    print(f"general forward's mapping against get_mapping: {e:.3e}")
    assert e < 1e-5, e


# ------------------------------------------------------------------ 2. the general forward
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_forward_vs_reference(models, inputs, g, mode):
    m, tol = models[mode], (F32_TOL if mode == "f32" else BF16_TOL)
    for name, kw in CASES.items():
        y = forward(m, inputs, inputs["f"], **kw)
        e = rel_err(y[:, :, ::2], g[name])
        print(f"{name} {mode}: {e:.3e}")
        assert e < tol, (name, e)
    if mode == "f32":
        y = forward(m, inputs, inputs["f"], **CASES["y.cfg"])
        y_rev = forward(m, inputs, inputs["f"].flip(0).contiguous(), **CASES["y.cfg"])
        eff = rel_err(y_rev[:, :, ::2], g["y.cfg"])
        print(f"reversed feature rows against y.cfg: {eff:.3e} (fixture {float(g['y.effect']):.3e})")
        assert eff >= 0.5 * float(g["y.effect"]), eff
        assert rel_err(y_rev, y) >= 0.5 * float(g["y.effect"])
    with pytest.raises(AssertionError, match="context_features exists but no features provided"):
        forward(m, inputs, None, **CASES["y.cfg"])
    with pytest.raises(ValueError, match="features of shape"):
        forward(m, inputs, inputs["f"][:2], **CASES["y.cfg"])


# ------------------------------------------------------------------ 3. fused DDIM, three ways
def ddim(gd, m, inp, f, **kw):
    """(stacked trajectory, final latents): the stack holds the input of every step (gdm.py:205), so the result of the last step --
    what a caller gets -- comes from a second run without the stack, as in the fixture"""
    args = dict(init_noise=inp["init"], step_noises=inp["noises"], **kw)
    traj = gd.sample(m, SHAPE, with_features(inp["cond"], f), return_all_timesteps=True, **args)
    final = gd.sample(m, SHAPE, with_features(inp["cond"], f), **args)
    torch.cuda.synchronize()
    assert tuple(traj.shape) == (B, S + 1, 128, T) and tuple(final.shape) == SHAPE
    return traj.cpu().numpy(), final.cpu().numpy()


def check_ddim(run, g, tag, tol, what):
    traj, final = run
    e = rel_err(final, g[f"ddim4{tag}.final"])
    et = rel_err(traj[:, :, :, ::8], g[f"ddim4{tag}.traj"])
    print(f"ddim4{tag} {what}: final latents {e:.3e}, trajectory {et:.3e}")
    assert e < tol and et < tol, (what, e, et)


def test_fused_ddim_three_ways(models, inputs, g):
    """4-step DDIM (eta = 1, injected noise, CFG pair batched) as a graph replay, as the eager stepper and as the literal loop
    (``fused=False``): the stacked trajectory and the final latents of each against the reference's, float32; the replayed and the
    eager stepper agree to the bit"""
    m = models["f32"]
    gd = gdm()
    with fixed_order(m):
        replay = ddim(gd, m, inputs, inputs["f"], use_graph=True)
        eager = ddim(gd, m, inputs, inputs["f"], use_graph=False)
    assert any(st.per_sample and st.use_graph for st in gd._steppers.values())
    n = len(gd._steppers)
    literal = ddim(gd, m, inputs, inputs["f"], fused=False)
    assert len(gd._steppers) == n
    check_ddim(replay, g, "", F32_TOL, "graph replay")
    check_ddim(eager, g, "", F32_TOL, "eager stepper")
    check_ddim(literal, g, "", F32_TOL, "literal loop")
    assert np.array_equal(replay[0], eager[0]) and np.array_equal(replay[1], eager[1]), "the replayed and the eager stepper differ"
    rev = ddim(gd, m, inputs, inputs["f"].flip(0).contiguous())
    check_ddim(rev, g, ".rev", F32_TOL, "graph replay, reversed feature rows")


def test_fused_ddim_bf16_replay_equals_eager(models, inputs):
    """bf16: the casts of the per-sample stepper -- the replayed and the eager stepper agree to the bit (the 4-step trajectory itself is
    not compared with the float32 reference in bf16: it starts at t = 999, where x0 = 157 (...) is clamped, and amplifies bf16 rounding
    beyond any bound that could be derived for it; the bf16 forward is gated in test_forward_vs_reference)"""
    m = models["bf16"]
    gd = gdm()
    with fixed_order(m):
        replay = ddim(gd, m, inputs, inputs["f"], use_graph=True)
        eager = ddim(gd, m, inputs, inputs["f"], use_graph=False)
    assert any(st.per_sample and st.use_graph for st in gd._steppers.values())
    assert np.isfinite(replay[1]).all() and float(np.abs(replay[1]).max()) <= 1.0 + 1e-6
    assert np.array_equal(replay[0], eager[0]) and np.array_equal(replay[1], eager[1])


# ------------------------------------------------------------------ 4. stale tables
def run_stepper(st, inp):
    """a whole trajectory on the stepper itself; returns its final latents"""
    st.reset(inp["init"])
    for i in range(st.num_steps):
        st.step(i, noise=inp["noises"][i])
    st.check()
    torch.cuda.synchronize()
    return st.x.cpu().numpy().copy()


def test_rebind_refills_the_tables_and_steppers_share_a_plan(models, inputs, g):
    """one stepper: trajectory A, ``rebind`` with the reversed features, trajectory B with the same noise -- B is the reversed-rows
    fixture, not A again; a second stepper of the same shape on the same plan (another GaussianDiffusion object), interleaved with the
    first, gets its own features back every time"""
    m = models["f32"]
    f, f_rev = inputs["f"], inputs["f"].flip(0).contiguous()
    c, c_rev = with_features(inputs["cond"], f), with_features(inputs["cond"], f_rev)
    with fixed_order(m):
        gd1, gd2 = gdm(), gdm()
        st1 = gd1.stepper(m, SHAPE, c)
        a = run_stepper(st1, inputs)
        assert rel_err(a, g["ddim4.final"]) < F32_TOL
        assert gd1.stepper(m, SHAPE, c_rev) is st1            # (rebinds)
        b = run_stepper(st1, inputs)
        e = rel_err(b, g["ddim4.rev.final"])
        print(f"after rebind with reversed features: {e:.3e} against the reversed fixture, {rel_err(b, g['ddim4.final']):.3e} against the first")
        assert e < F32_TOL, e
        assert rel_err(b, a) > 5 * F32_TOL
        st2 = gd2.stepper(m, SHAPE, c)
        assert st2 is not st1 and st2.plan is st1.plan
        for k in range(2):
            a2 = run_stepper(st2, inputs)
            assert rel_err(a2, g["ddim4.final"]) < F32_TOL, k
            b1 = run_stepper(st1, inputs)
            assert rel_err(b1, g["ddim4.rev.final"]) < F32_TOL, k
            assert np.array_equal(b1, b) and np.array_equal(a2, a)
        # a features tensor edited in place between two sampling runs is taken up as well
        c["global_cond"] = f.clone()
        st2.rebind(c)
        c["global_cond"].copy_(f_rev)
        st2.rebind(c)
        assert np.array_equal(run_stepper(st2, inputs), b)


# ------------------------------------------------------------------ 5. the other modes against the literal loop
def test_dpmpp_and_vdm_fused_vs_literal_loop(models, inputs):
    from jen1_amd.vdm import VDM
    m = models["f32"]
    c = with_features(inputs["cond"], inputs["f"])
    c_rev = with_features(inputs["cond"], inputs["f"].flip(0).contiguous())
    gd = gdm(3)
    fused = gd.dpm_sample(m, SHAPE, c, init_noise=inputs["init"])
    fused_rev = gd.dpm_sample(m, SHAPE, c_rev, init_noise=inputs["init"])
    assert any(st.mode == "dpmpp" and st.per_sample for st in gd._steppers.values())
    literal = gd._dpm_generic(m, SHAPE, c, init_noise=inputs["init"])
    torch.cuda.synchronize()
    e = rel_err(fused.cpu().numpy(), literal.cpu().numpy())
    print(f"dpmpp 3 steps, fused against the literal loop: {e:.3e}")
    assert e < F32_TOL, e
    assert rel_err(fused_rev.cpu().numpy(), literal.cpu().numpy()) > 5 * F32_TOL
    vd = VDM(loss_type="l2", device="cuda", cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    fused = vd.sample(m, SHAPE, c, step=3, init_noise=inputs["init"])
    assert any(st.mode == "vdm" and st.per_sample for st in vd._steppers.values())
    literal = vd.sample(m, SHAPE, c, step=3, init_noise=inputs["init"], fused=False)
    torch.cuda.synchronize()
    e = rel_err(fused.cpu().numpy(), literal.cpu().numpy())
    print(f"vdm 3 steps, fused against the literal loop: {e:.3e}")
    assert e < F32_TOL, e


# ------------------------------------------------------------------ 6. zero to_features == no features
def test_zero_to_features_is_the_featureless_model(inputs):
    """to_features weight and bias zero: the added term is exactly GELU(0) = 0.  General forward: bit for bit; fused stepper: 1e-5
    relative (the per-sample FiLM form may split the persistent launch's work differently)"""
    plain, feat = _model("f32", featured=False), _model("f32")
    with torch.no_grad():
        feat.to_features._modules["0"].weight.zero_()
        feat.to_features._modules["0"].bias.zero_()
    sd_p, sd_f = plain.state_dict(), feat.state_dict()
    assert all(torch.equal(sd_p[k], sd_f[k]) for k in sd_p)
    with fixed_order(plain, feat):
        for name, kw in CASES.items():
            y0 = forward(plain, inputs, None, **kw)
            y1 = forward(feat, inputs, inputs["f"], **kw)
            assert np.array_equal(y0, y1), (name, rel_err(y1, y0))
        gd = gdm()
        s0 = ddim(gd, plain, inputs, None)
        s1 = ddim(gd, feat, inputs, inputs["f"])
    e, et = rel_err(s1[1], s0[1]), rel_err(s1[0], s0[0])
    print(f"fused DDIM, zero to_features against the featureless model: final latents {e:.3e}, trajectory {et:.3e}")
    assert e < 1e-5 and et < 1e-5, (e, et)


# ------------------------------------------------------------------ 7. launches per step
def test_launches_per_step_five_and_six():
    """the full configuration, B = 2, T = 1500, CFG pair: three persistent launches + jen1_step_tail + the partials' sum = 5; with
    features the selection launch makes 6.  Nothing of the network runs (zero weights, no graph capture): the count is the plan's"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.model import UNetCFG1d
    Bf, Tf = 2, 1500
    cond = {k: dev(v) for k, v in synth.conditioning(Bf, Tf).items()}
    gd = gdm(2)
    plain = UNetCFG1d(**full_model_config(), init_seed=None, compute_dtype="bf16", device="cuda")
    st = gd.stepper(plain, (Bf, 128, Tf), cond, use_graph=False)
    assert st.fused_tail and not st.per_sample and st.launches_per_step == 5
    assert not any(getattr(op, "kind", "") == "film_select" for op in st.plan.ops)
    del st, plain
    gd._steppers.clear()
    feat = UNetCFG1d(**dict(full_model_config(), context_features=64), init_seed=None, compute_dtype="bf16", device="cuda")
    st = gd.stepper(feat, (Bf, 128, Tf), dict(cond, global_cond=torch.zeros((Bf, 64), device="cuda")), use_graph=False)
    assert st.fused_tail and st.per_sample and st.launches_per_step == 6
    assert [getattr(op, "kind", "") for op in st.plan.ops].count("film_select") == 1


# ------------------------------------------------------------------ 8. training
@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_training_loss_and_gradients(g, inputs, mode, graphed, monkeypatch):
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.train import GraphedLossStep
    m = _model(mode)
    m.train()
    opt = FusedAdamW(m.parameters(), lr=0.0, max_norm=None)
    graph = m.train_graph(mode)
    graph.attach_optimizer(opt)
    gd = gdm(1000)
    x0 = dev(synth.latents(B, T, key="clip"))
    noise = dev(fill_uniform("synth.trainnoise.global_cond", SHAPE, 3, 0.0, 1.0))
    t = torch.tensor([17, 801, 300], dtype=torch.long, device="cuda")
    cond = with_features(inputs["cond"], inputs["f"])
    opt.zero_grad()
    if graphed:
        monkeypatch.setattr(torch, "rand_like", lambda x, **kw: noise.clone())       # (the captured pass draws its own noise)
        step = GraphedLossStep(graph, gd, scale=1.0)
        step(x0, t, cond, False)               # capture
        # the replay reads the features from its static buffer: refreshed from what this call passes
        opt.zero_grad()
        loss = step(x0, t, with_features(inputs["cond"], inputs["f"].clone()), False)
    else:
        loss = gd.training_loosses(m, x0, t, cond, noise=noise, causal=False)
        loss.backward()
    torch.cuda.synchronize()
    names = json.loads(str(g["train.grad_names"]))
    params = dict(m.named_parameters())
    le = abs(float(loss.detach()) - float(g["train.loss"])) / abs(float(g["train.loss"]))
    ref = g["train.gradnorm"]
    ne = max(abs(float(params[n].grad.norm()) - ref[i]) / ref[i] for i, n in enumerate(names))
    be = rel_err(params["to_features.0.bias"].grad.cpu().numpy(), g["train.grad.to_features.0.bias"])
    what = "graphed" if graphed else "eager"
    print(f"training {mode} {what}: loss {le:.3e}, worst gradient norm {ne:.3e}, to_features.0.bias gradient {be:.3e}")
    record_parity("global_cond_train", what, mode, loss=le, norm=ne, bias_grad=be)
    assert float(params["to_features.0.weight"].grad.abs().max()) > 0
    if mode == "f32":
        assert le < 1e-3 and ne < 1e-3 and be < 1e-3, (le, ne, be)
    else:
        assert le < bf16_gate("configs3_micro_batch", "bf16", "loss"), le
        assert ne < bf16_gate("configs3_micro_batch", "bf16", "norm"), ne
    if graphed:                                # a replay with other features gives another loss: the static buffer is refreshed
        other = float(step(x0, t, with_features(inputs["cond"], inputs["f"].flip(0).contiguous()), False))
        assert abs(other - float(loss)) > 1e-4 * abs(float(loss)), (other, float(loss))


def test_trainer_runs_with_global_cond_ids(inputs):
    """``UnifiedMultiTaskTrainer.train`` with ``global_cond_ids``: the conditioner's global entries reach the pass, gradients arrive at
    ``to_features``"""
    import random
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    gd = gdm(1000)
    emb, msk, f = inputs["cond"]["cross_attn_cond"], inputs["cond"]["cross_attn_masks"], inputs["f"]

    def conditioner(md, device):
        i = torch.tensor(md, device=device)
        return {"prompt": (emb[i], msk[i]), "seconds": [f[i][:, None, :8], None], "key": [f[i][:, None, 8:], None]}

    for use_graph in (False, True):
        m = _model("f32")
        opt = FusedAdamW(m.parameters(), lr=1e-3)
        tr = UnifiedMultiTaskTrainer.build(m, gd, conditioner, opt, None, grad_accum_every=2, rng=random.Random(5), use_graph=use_graph,
                                           global_cond_ids=("seconds", "key"))
        opt.zero_grad()
        loss, per_task = tr.train(dev(synth.latents(B, T, key="clip")), list(range(B)))
        if not use_graph:
            loss.backward()
        torch.cuda.synchronize()
        assert np.isfinite(float(loss)) and set(per_task) == {"text_guided", "music_inpaint", "music_cont"}
        grads = dict(m.named_parameters())
        assert float(grads["to_features.0.weight"].grad.abs().max()) > 0, use_graph


# ------------------------------------------------------------------ 9. the conditioners
def cond_weights():
    return {"seconds.embedder.embedding.0.weights": fill_normal("cond.seconds.freq", (128,), 21),
            "seconds.embedder.embedding.1.weight": fill_uniform("cond.seconds.weight", (8, 257), 21, -1 / 16, 1 / 16),
            "seconds.embedder.embedding.1.bias": fill_uniform("cond.seconds.bias", (8,), 21, -1 / 16, 1 / 16),
            "key.int_embedder.weight": fill_normal("cond.key.table", (9, 16), 21)}


def test_int_number_multi_conditioners_vs_reference(g):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.conditioners import IntConditionerHIP, MultiConditionerHIP, NumberConditionerHIP
    from jen1_amd.tasks import get_conditioning
    w = cond_weights()
    num, itc = NumberConditionerHIP(8, 0, 30), IntConditionerHIP(16, 0, 8)
    num.load_state_dict({k[len("seconds."):]: v for k, v in w.items() if k.startswith("seconds.")})
    itc.load_state_dict({k[len("key."):]: v for k, v in w.items() if k.startswith("key.")})
    numbers, ints = [-5, 0, 12.5, 30, 99], [-3, 0, 5, 8, 20]
    e, mask = num(numbers, "cuda")
    assert tuple(e.shape) == (5, 1, 8) and tuple(mask.shape) == (5, 1) and bool((mask == 1).all()) and e.is_cuda
    err = rel_err(e.cpu().numpy(), g["cond.number"])
    print(f"NumberConditionerHIP: {err:.3e}")
    assert err < 1e-5, err
    e, mask = itc(ints, "cuda")
    assert tuple(e.shape) == (5, 1, 16) and tuple(mask.shape) == (5, 1)
    assert np.array_equal(e.cpu().numpy(), g["cond.int"])                      # a gather: exact
    assert np.array_equal(e.cpu().numpy()[:, 0], w["key.int_embedder.weight"][[0, 0, 5, 8, 8]])
    multi = MultiConditionerHIP({"seconds": num, "key": itc})
    out = multi([{"seconds": a, "key": [b]} for a, b in zip(numbers, ints)], "cuda")
    gc = get_conditioning(out, cross_attn_cond_ids=(), global_cond_ids=("seconds", "key"), input_concat_ids=())["global_cond"]
    assert tuple(gc.shape) == (5, F_CTX)
    err = rel_err(gc.cpu().numpy(), g["cond.global_cond"])
    assert err < 1e-5, err


# ------------------------------------------------------------------ 10. the table budget
def test_table_budget_falls_back_to_the_literal_loop(models, inputs, g, monkeypatch):
    from jen1_amd import diffusion as D
    m = models["f32"]
    c = with_features(inputs["cond"], inputs["f"])
    film_ld = m.engine().W.film_ld
    assert D.film_table_bytes(m, B, S) == 2 * S * B * film_ld * 4
    assert D.FILM_TABLE_BUDGET == 1 << 30
    assert D.film_tables_fit(m, c, B, S) and D.film_tables_fit(m, inputs["cond"], B, 10 ** 9)
    monkeypatch.setenv("JEN1_FILM_TABLE_BUDGET", str(D.film_table_bytes(m, B, S) - 1))
    assert not D.film_tables_fit(m, c, B, S) and D.film_tables_fit(m, c, B, S - 1)
    gd = gdm()
    run = ddim(gd, m, inputs, inputs["f"])
    assert not gd.__dict__.get("_steppers"), "over the budget no fused stepper is built"
    check_ddim(run, g, "", F32_TOL, "literal loop (over the table budget)")
    monkeypatch.delenv("JEN1_FILM_TABLE_BUDGET")
    ddim(gd, m, inputs, inputs["f"])
    assert len(gd._steppers) == 1
