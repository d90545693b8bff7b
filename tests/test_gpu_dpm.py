"""-m gpu: the DPM-Solver++(2M) row of the fused sampler step (DDIMStepper(mode="dpmpp"), jen1_step_tail_ms / jen1_cfg_ddim_step_pack_ms).

  A  the bits of one step from what the stepper exposes: x_after == (b0 h + a x_before) + b1 h_prev in torch float32 with the row's three
     float32 values, h the history the step left (its clipped x0); with the known-region blend on top; tiny f32 and full bf16;
  B  one trajectory through every launch form: the tail launch, the step + pack launch, eager and as a replayed graph, the batch split
     over two plans; bit for bit;
  C  the trajectory against the numpy restatement around the oracle network (tests/dpm_common.py) and against the literal torch loop on
     the same HIP model, three objectives, with and without the CFG pair, with inpaint masks;
  D  no stale state: reset(), another stepper on the shared plan in between, a zero mask, Jen1.generate(sampler="dpmpp2m").

Nothing here draws noise after the start, so every comparison is deterministic.  Bitwise comparisons run on plans with fixed-order
statistics (see test_gpu_sampler_state.py).
"""
import contextlib

import numpy as np
import pytest
import torch

from dpm_common import np_dpm_loop
from helpers import filled, rel_err
from jen1_amd import synth
from jen1_amd.config import GDMConfig, UNetSpec, full_model_config, tiny_model_config
from known_blend_common import blend_edits, masks, np_blend, np_levels

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


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
    """after the module: what its models, plans and graphs held goes back to the device"""
    yield
    import gc
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tiny_f32():
    return _model("f32", tiny=True)


@pytest.fixture(scope="module")
def oracle_tiny():
    from oracle import jen1_oracle as O
    cfg = tiny_model_config()
    return O.OracleUNetCFG1d(filled(UNetSpec(**cfg).param_shapes()), **cfg)


@contextlib.contextmanager
def fixed_order(m, on):
    old = m.deterministic
    m.deterministic = bool(on)
    try:
        yield
    finally:
        m.deterministic = old


def needs_fixed_order(m, B, T, nrep, causal, S):
    """True when the default sampler plan of this shape keeps float-atomic statistics somewhere, i.e. is not bit-reproducible by itself"""
    with fixed_order(m, False):
        plan = m.engine().plan(B, T, nrep, causal, slot=0, n_t=S)
    return not (plan.use_long and plan.deep_level is not None)


def gdm(S, scale=0.8, objective="noise", eta=1.0):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    betas, _ = get_beta_schedule("linear", 1000)
    return GaussianDiffusion(steps=1000, betas=betas, objective=objective, loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                             embedding_scale=scale, batch_cfg=True, scale_cfg=True, sampling_timesteps=S, ddim_sampling_eta=eta)


def stepper(gd, m, shape, cond, monkeypatch, tail=True, use_graph=True, n_streams=1, blend=False, order=2, mode="dpmpp"):
    from jen1_amd.diffusion import DDIMStepper
    with monkeypatch.context() as mp:
        mp.setenv("JEN1_STEP_PACK", "1")
        mp.setenv("JEN1_STEP_TAIL", "1" if tail else "0")
        st = DDIMStepper(gd, m, shape, cond, use_graph=use_graph, n_streams=n_streams, mode=mode, blend=blend, order=order)
    assert st.fused_pack
    return st


@pytest.fixture(scope="module")
def full_bf16_lazy():
    """built on first use"""
    made = []

    def get():
        if not made:
            made.append(_model("bf16"))
        return made[0]
    return get


def which_model(which, tiny_f32, full_bf16_lazy):
    """(model, T): the tiny float32 model at T = 300, or the full bf16 model at T = 1500 (whose plans carry the tail launch)"""
    return (tiny_f32, 300) if which == "tiny" else (full_bf16_lazy(), 1500)


def trajectory(st, init):
    st.reset(init)
    first = None
    for i in range(st.num_steps):
        st.step(i)
        if i == 0:
            first = st.x.clone()
    st.check()
    torch.cuda.synchronize()
    return first, st.x.clone()


def known_draws(shape, mask="inpaint"):
    B, _, T = shape
    known = (synth.latents(B, T, key="known") * 0.5).astype(np.float32)
    eps_k = synth.noise_list(1, shape, seed=33)[0]
    return known, masks(B, T, mask), eps_k


# ================================================================== A. the bits of one step
@pytest.mark.parametrize("blend", [False, True], ids=["plain", "blend"])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_one_step_bits_from_what_the_stepper_exposes(tiny_f32, full_bf16_lazy, monkeypatch, which, blend):
    from jen1_amd.diffusion import blend_known
    m, T = which_model(which, tiny_f32, full_bf16_lazy)
    S, B = 5, 2
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, "music_inpaint"))
    init = dev(synth.noise_list(1, shape, seed=31)[0])
    gd = gdm(S, objective="noise" if which == "tiny" else "v")
    det = True if which == "tiny" else needs_fixed_order(m, B, T, 2, False, S)
    with fixed_order(m, det):
        st = stepper(gd, m, shape, cond, monkeypatch, blend=blend)
        if which == "full":
            assert st.fused_tail and st.launches_per_step == 5
        assert st.noise_all.numel() == 1 and len(st.hist) == 1 and tuple(st.hist[0].shape) == shape
        if blend:
            known, keep, eps_k = (dev(a) for a in known_draws(shape))
            st.set_known(known, keep, noise=eps_k)
        st.reset(init)
        assert not st.hist[0].any(), "reset() leaves an empty history"
        rows = st.coef.tolist()
        assert [r[5] for r in rows] == [4.0] * (S - 1) + [1.0] and rows[0][4] == 0.0 and all(r[4] != 0.0 for r in rows[1:-1])
        for i in range(S):
            x_before, h_prev = st.x.clone(), st.hist[0].clone()
            st.step(i)
            torch.cuda.synchronize()
            x_after, h = st.x.clone(), st.hist[0].clone()
            assert torch.isfinite(h).all() and float(h.abs().max()) <= 1.0, f"step {i}: the history is the clipped x0"
            assert not torch.equal(h, h_prev), f"step {i}: the history was not rewritten"
            if i not in (0, 1, S - 1):
                continue
            b0, a, b1 = rows[i][2:5]
            want = h if i == S - 1 else (b0 * h + a * x_before) + b1 * h_prev
            if blend:
                want = blend_known(want, known, keep, eps_k, *st._kb_host[i])
            assert torch.equal(x_after, want), f"step {i}: {rel_err(x_after.cpu(), want.cpu()):.3e} from the formula"
        st.check()
        if blend:
            sel = (keep == 1).expand(shape)
            assert torch.equal(st.x[sel], known[sel])


# ================================================================== B. one trajectory, every path
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_every_launch_form_gives_the_same_bits(tiny_f32, full_bf16_lazy, monkeypatch, which):
    """the tail launch as a replayed graph against the step + pack launch (JEN1_STEP_TAIL=0), against eager launches, and the same with
    the blend; the batch of 3 split 2 + 1 over two plans: tail graph against step + pack eager.  (Two streams against one: sub-batches
    of another size sum their statistics in another order, so that pair is compared on step 0 within PATH_TOL in float32, as
    test_two_streams_tiny_vs_oracle does.)"""
    m, T = which_model(which, tiny_f32, full_bf16_lazy)
    S, B = 4, 3
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, "music_inpaint"))
    init = dev(synth.noise_list(1, shape, seed=41)[0])
    gd = gdm(S)
    det = True if which == "tiny" else any(needs_fixed_order(m, b, T, 2, False, S) for b in (3, 2, 1))
    with fixed_order(m, det):
        ref_st = stepper(gd, m, shape, cond, monkeypatch, tail=True, use_graph=True)
        if which == "full":
            assert ref_st.fused_tail
        ref = trajectory(ref_st, init)
        assert torch.isfinite(ref[1]).all() and not torch.equal(ref[0], ref[1])
        for tail, ug in ((False, True), (True, False), (False, False)):
            st = stepper(gd, m, shape, cond, monkeypatch, tail=tail, use_graph=ug)
            assert not (st.fused_tail and not tail)
            got = trajectory(st, init)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), f"tail={tail} graph={ug}: differs from the tail graph"
        known, keep, eps_k = (dev(a) for a in known_draws(shape))
        outs = []
        for tail, ug in ((True, True), (False, False)):
            st = stepper(gd, m, shape, cond, monkeypatch, tail=tail, use_graph=ug, blend=True)
            st.set_known(known, keep, noise=eps_k)
            outs.append(trajectory(st, init))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "blend: tail graph differs from pack eager"
        assert not torch.equal(outs[0][1], ref[1])
        two = []
        for tail, ug in ((True, True), (False, False)):
            st = stepper(gd, m, shape, cond, monkeypatch, tail=tail, use_graph=ug, n_streams=2)
            assert len(st.parts) == 2 and len(st.hist) == 2
            two.append(trajectory(st, init))
        assert torch.equal(two[0][0], two[1][0]) and torch.equal(two[0][1], two[1][1]), "two streams: tail graph differs from pack eager"
        if which == "tiny":
            e = rel_err(two[0][0].cpu().numpy(), ref[0].cpu().numpy())
            assert e < PATH_TOL, e


# ================================================================== C. against the oracle
def oracle_gd(S, scale, objective):
    from oracle import jen1_oracle as O
    return O.OracleGaussianDiffusion(steps=1000, betas=O.get_beta_schedule("linear", 1000), objective=objective, cfg_dropout_proba=0.0,
                                     embedding_scale=scale, batch_cfg=True, scale_cfg=True, sampling_timesteps=S)


@pytest.mark.parametrize("scale", [0.8, 1.0], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("objective", ["noise", "x0", "v"])
def test_trajectory_tiny_vs_oracle_and_literal_loop(tiny_f32, oracle_tiny, objective, scale):
    m, S, B, T = tiny_f32, 10, 2, 300
    shape = (B, 128, T)
    c_np = synth.conditioning(B, T, "music_inpaint")
    cond = cond_dev(c_np)
    init_np = synth.noise_list(1, shape, seed=51)[0]
    gd = gdm(S, scale, objective)
    with fixed_order(m, True):
        got = gd.dpm_sample(m, shape, cond, init_noise=dev(init_np))
        st = next(iter(gd._steppers.values()))
        assert st.mode == "dpmpp" and st.order == 2
        lit = gd._dpm_generic(m, shape, cond, init_noise=dev(init_np))
        via = gd.sample(m, shape, cond, init_noise=dev(init_np), sampler="dpmpp2m")
        first = gd.dpm_sample(m, shape, cond, init_noise=dev(init_np), order=1)
    assert torch.equal(via, got) and len(gd._steppers) == 2, "order is part of the stepper cache key"
    assert not torch.equal(first, got)
    ref = np_dpm_loop(oracle_gd(S, scale, objective), oracle_tiny, shape, [c_np] * S, init_np)
    e, p = rel_err(got.cpu().numpy(), ref), rel_err(got.cpu().numpy(), lit.cpu().numpy())
    print(f"{objective} scale {scale}: vs oracle {e:.3e}, vs the literal loop {p:.3e}")
    assert e < F32_TOL
    assert p < PATH_TOL


@pytest.mark.parametrize("mask", ["inpaint", "per-sample"])
def test_masked_trajectory_tiny_vs_oracle_and_literal_loop(tiny_f32, oracle_tiny, mask):
    m, S, B, T = tiny_f32, 10, 2, 300
    shape = (B, 128, T)
    c_np = synth.conditioning(B, T, "music_inpaint")
    cond = cond_dev(c_np)
    init_np = synth.noise_list(1, shape, seed=52)[0]
    known, keep, eps_k = known_draws(shape, mask)
    gd = gdm(S)
    kw = dict(init_noise=dev(init_np), known=dev(known), keep_mask=dev(keep), known_noise=dev(eps_k))
    with fixed_order(m, True):
        got = gd.dpm_sample(m, shape, cond, **kw)
        lit = gd._dpm_generic(m, shape, cond, init_noise=kw["init_noise"], known=kw["known"], keep=kw["keep_mask"],
                              known_noise=kw["known_noise"])
    og = oracle_gd(S, 0.8, "noise")
    start, levels = np_levels("ddim", og.alphas_cumprod, pairs=og.ddim_times())
    ref = np_dpm_loop(og, oracle_tiny, shape, [c_np] * S, np_blend(init_np, known, keep, eps_k, *start),
                      edits=blend_edits(levels, known, keep, eps_k))
    e, p = rel_err(got.cpu().numpy(), ref), rel_err(got.cpu().numpy(), lit.cpu().numpy())
    print(f"{mask}: vs oracle {e:.3e}, vs the literal loop {p:.3e}")
    assert e < F32_TOL
    assert p < PATH_TOL
    sel = np.broadcast_to(keep == 1, shape)
    assert np.array_equal(got.cpu().numpy()[sel], known[sel])


def test_without_the_vector_pack_kernel_the_literal_loop_runs(tiny_f32, monkeypatch):
    from jen1_amd.diffusion import DDIMStepper
    m, S, B, T = tiny_f32, 4, 2, 300
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, "text_guided"))
    init = dev(synth.noise_list(1, shape, seed=53)[0])
    gd = gdm(S)
    with fixed_order(m, True):
        want = gd._dpm_generic(m, shape, cond, init_noise=init)
        for name, value in (("JEN1_STEP_PACK", "0"), ("JEN1_CFG_STEP_SCALAR", "1")):
            with monkeypatch.context() as mp:
                mp.setenv(name, value)
                got = gd.dpm_sample(m, shape, cond, init_noise=init)
                assert not getattr(gd, "_steppers", {}), "no stepper without the multistep row"
                with pytest.raises(RuntimeError, match="multistep row"):
                    DDIMStepper(gd, m, shape, cond, mode="dpmpp")
            assert torch.equal(got, want), name


# ================================================================== D. no stale state
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_no_stale_state(tiny_f32, full_bf16_lazy, monkeypatch, which):
    m, T = which_model(which, tiny_f32, full_bf16_lazy)
    S, B = 4, 2
    shape = (B, 128, T)
    cond = cond_dev(synth.conditioning(B, T, "music_cont"))
    init, other = (dev(n) for n in synth.noise_list(2, shape, seed=61))
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=62)]
    gd = gdm(S)
    det = True if which == "tiny" else needs_fixed_order(m, B, T, 2, False, S)
    with fixed_order(m, det):
        st = stepper(gd, m, shape, cond, monkeypatch)
        want = trajectory(st, init)
        trajectory(st, other)                          # (leaves another trajectory's x0 in the history)
        got = trajectory(st, init)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "reset() + the same trajectory again: other bits"
        ddim = stepper(gd, m, shape, cond, monkeypatch, mode="ddim")
        assert ddim.plan is st.plan
        ddim.reset(other, fresh_noise=False)
        for i in range(S):
            ddim.step(i, noise=noises[i])
        with pytest.raises(RuntimeError, match="plan_slot"):
            st.step(1)
        got = trajectory(st, init)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "after a DDIM stepper on the shared plan: other bits"
        bl = stepper(gd, m, shape, cond, monkeypatch, blend=True)
        got = trajectory(bl, init)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "blend stepper before set_known: not the plain bits"
        known, _, eps_k = (dev(a) for a in known_draws(shape))
        bl.set_known(known, dev(masks(B, T, "zeros")), noise=eps_k)
        got = trajectory(bl, init)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "keep == 0: not the plain bits"


HOP = 320          # Encodec 48 kHz: one latent frame per 320 samples


class _Quantizer:
    def __init__(self, n_q=4, bins=64, dim=128):
        g = torch.Generator().manual_seed(11)
        self.tables = torch.randn((n_q, bins, dim), generator=g) * 0.3

    def decode(self, codes):                      # [n_q, B, T] -> [B, dim, T]: the sum of the codebook vectors
        out = 0
        for q in range(codes.shape[0]):
            out = out + self.tables.to(codes.device)[q][codes[q]]
        return out.transpose(1, 2)


class StubAudioEncoder:
    """the slice of ``encodec.EncodecModel`` generation.py touches (test_gpu_generation.py's); the decoder keeps what it was handed"""
    channels = 2
    sample_rate = 48000

    def __init__(self):
        self.quantizer = _Quantizer()
        self.handed = None

    def encode(self, audio):                      # -> [(codes [B, n_q, T], scale)]
        B, _, n = audio.shape
        frames = audio[:, :, : n // HOP * HOP].reshape(B, 2, n // HOP, HOP).mean(dim=(1, 3))
        base = (frames * 1000).round().long().abs() % 64
        codes = torch.stack([(base + 7 * q) % 64 for q in range(4)], dim=1)
        return [(codes, None)]

    def decoder(self, emb):                       # [B, 128, T] -> [B, 2, HOP * T]
        assert emb.device.type == "cpu"
        self.handed = emb.clone()
        return torch.tanh(emb[:, :2].repeat_interleave(HOP, dim=2))


@pytest.fixture(scope="module")
def jen1():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.generation import Jen1
    cond = synth.conditioning(8, 300, "text_guided")
    emb = torch.from_numpy(cond["cross_attn_cond"]).cuda()
    msk = torch.from_numpy(cond["cross_attn_masks"]).cuda()

    def conditioner(batch_metadata, device):
        n = len(batch_metadata)
        return {"prompt": (emb[:n].to(device), msk[:n].to(device))}

    return Jen1(None, device="cuda", audio_encoder=StubAudioEncoder(), conditioner=conditioner, model_config=tiny_model_config(),
                diffusion_config=GDMConfig(), compute_dtype="f32")


def test_generate_with_the_multistep_sampler(jen1):
    B, seconds, steps = 2, 2, 20
    n = seconds * 48000
    _, model = jen1.get_model_and_diffusion(steps, True)
    with fixed_order(model, True):
        a = jen1.generate("a calm piano piece", seed=3, steps=steps, batch_size=B, seconds=seconds, use_gdm=True, sampler="dpmpp2m")
        za = jen1.audio_encoder.handed
        b = jen1.generate("a calm piano piece", seed=3, steps=steps, batch_size=B, seconds=seconds, use_gdm=True, sampler="dpmpp2m")
        c = jen1.generate("a calm piano piece", seed=4, steps=steps, batch_size=B, seconds=seconds, use_gdm=True, sampler="dpmpp2m")
        d = jen1.generate("a calm piano piece", seed=3, steps=steps, batch_size=B, seconds=seconds, use_gdm=True)
        assert a.shape == (B, 2, n) and torch.isfinite(a).all() and torch.isfinite(za).all()
        assert torch.equal(a, b), "a fixed seed must reproduce the audio"
        assert not torch.equal(a, c) and not torch.equal(a, d)
        audio = torch.randn((B, 2, n), generator=torch.Generator().manual_seed(5)) * 0.1
        jen1.generate("x", seed=9, steps=steps, batch_size=B, seconds=seconds, use_gdm=True, sampler="dpmpp2m", preserve_known=True,
                      task="music_inpaint", init_audio=audio, init_audio_sr=48000, inpainting_scope=(0.5, 1.5))
        z = jen1.audio_encoder.handed
    known = jen1.get_emb(audio.cuda())
    keep = torch.nn.functional.interpolate(jen1.get_mask(n, 0.5, 1.5, B).cuda(), size=known.shape[2])
    sel = (keep == 1).expand(known.shape).cpu()
    assert torch.isfinite(z).all() and torch.equal(z[sel], known.cpu()[sel]) and not torch.equal(z[~sel], known.cpu()[~sel])
    with pytest.raises(ValueError, match="use_gdm"):
        jen1.generate("x", seed=9, steps=steps, batch_size=B, seconds=seconds, use_gdm=False, sampler="dpmpp2m")
