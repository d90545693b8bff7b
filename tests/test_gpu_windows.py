"""-m gpu: long-form sampling on overlapping windows merged on a shared canvas (jen1_amd/windows.py, csrc/windows.hip;
GaussianDiffusion.sample_windows, VDM.sample_windows, Jen1.generate(window_seconds=...)).

  1  jen1_window_merge against the float64 restatement of windows_common.py, element by element
  2  jen1_window_gather bit for bit
  3  fused sample_windows (tiny model, float32) against the numpy oracle's loop with the numpy merge as its per-step edits
  4  fused against the package's literal loops (the merge as their ``edit``), dpmpp2m and its merged history included
  5  a plan of one window gives the bits of sample / dpm_sample
  6  after a run every window is a crop of the returned canvas; the per-step noise agrees where windows share a frame
  7  known audio on the canvas, an inpaint span across the window seams: the kept frames come back exactly
  8  Jen1.generate(window_seconds=...)
  9  full model, bf16, eight windows of 1500 frames: the shape long-form generation runs at

Every random draw is injected unless the test is about the draws.  Bitwise comparisons run on plans with fixed-order statistics.
"""
import contextlib

import numpy as np
import pytest
import torch

from helpers import filled, record_parity, rel_err
from jen1_amd import synth
from jen1_amd.config import GDMConfig, UNetSpec, full_model_config, tiny_model_config
from windows_common import merge_edits, np_cover, np_gather, np_merge, np_offsets, oracle_loop

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3          # float32 against the oracle (BASELINE.json; test_gpu_model.py)
PATH_TOL = 2e-5         # float32 across execution paths (test_gpu_deep.py)
S_ORACLE = 6            # the schedule length of test_gpu_known_blend.py's oracle trajectories
C, T, L, HOP_F = 128, 300, 560, 100          # the tiny model's window on a canvas of four windows: offsets (0, 100, 200, 260)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cond_dev(cond):
    return {k: dev(v) for k, v in cond.items()}


def make_plan(*a, **kw):
    from jen1_amd.windows import WindowPlan
    return WindowPlan(*a, **kw)


def _model(dtype, tiny=False):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.model import UNetCFG1d
    cfg = tiny_model_config() if tiny else full_model_config()
    return UNetCFG1d(**cfg, init_seed=1234, compute_dtype=dtype, device="cuda")


@pytest.fixture(scope="module", autouse=True)
def release_device_memory():
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
def full_bf16():
    return _model("bf16")


@pytest.fixture(scope="module")
def oracle_tiny():
    from oracle import jen1_oracle as O
    cfg = tiny_model_config()
    return O.OracleUNetCFG1d(filled(UNetSpec(**cfg).param_shapes()), **cfg)


@contextlib.contextmanager
def fixed_order(m, on=True):
    old = m.deterministic
    m.deterministic = bool(on)
    try:
        yield
    finally:
        m.deterministic = old


def gdm(S, scale=0.8, objective="noise", eta=1.0, steps=1000, betas=None):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    if betas is None:
        betas, _ = get_beta_schedule("linear", steps)
    return GaussianDiffusion(steps=steps, betas=betas, objective=objective, loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                             embedding_scale=scale, batch_cfg=True, scale_cfg=True, sampling_timesteps=S, ddim_sampling_eta=eta)


def vdm(scale=0.8):
    from jen1_amd.vdm import VDM
    return VDM(loss_type="l2", device="cuda", cfg_dropout_proba=0.0, embedding_scale=scale, batch_cfg=True, scale_cfg=True)


def make_sampler(kind, S):
    """(sampler, keywords of sample_windows that select the kind)"""
    from jen1_amd.diffusion import get_beta_schedule
    if kind == "ddim":
        return gdm(S), {}
    if kind == "dpmpp2m":
        return gdm(S), {"sampler": "dpmpp2m"}
    if kind == "ddpm":
        betas, _ = get_beta_schedule("cosine", S)
        return gdm(S, steps=S, betas=betas), {}
    return vdm(), {"step": S}


def canvas_draws(n, S, kind, length=L, seed=61):
    """start noise and per-step noise ON THE CANVAS (numpy); the per-step keyword only for the samplers that draw"""
    shape = (n, C, length)
    init = synth.noise_list(1, shape, seed=seed)[0]
    noises = synth.noise_list(S, shape, seed=seed + 1, uniform=(kind == "ddpm"))
    return init, noises


def run_windows(sampler, kw, m, plan, n, cond, init, noises, kind, **more):
    if kind in ("ddim", "ddpm"):
        more = dict(more, step_noises=[dev(a) for a in noises])
    return sampler.sample_windows(m, plan, n, cond, init_noise=dev(init), **kw, **more)


# ================================================================== 1. the merge kernel
MERGE_CASES = {
    # id: (n, C, T, L, hop, ramp)
    "odd-ramp26": (2, 5, 37, 70, 11, 26),                  # T, L no multiples of four, offsets (0, 11, 22, 33)
    "odd-ramp1": (2, 5, 37, 70, 11, 1),
    "tiny-window": (2, 128, 300, 560, 100, None),          # offsets (0, 100, 200, 260), ramp 200: up to four windows on a frame
    "odd-offsets": (2, 3, 300, 564, 101, None),            # windows at 101, 202 and 264
    "odd-canvas": (2, 3, 300, 562, 100, None),             # canvas rows that are not 16-byte aligned, the last window pulled in to 262
    "long-form": (1, 2, 1500, 6750, 750, None),            # the geometry of eight 10 s windows (L = 6750 is no multiple of four)
    "more-than-a-block": (1, 2, 8, 2052, 4, 3),            # W = 512 windows; > 256 work items per channel
}


@pytest.mark.parametrize("case", list(MERGE_CASES), ids=list(MERGE_CASES))
def test_merge_kernel_against_float64(case):
    n, Cc, Tt, Ll, hop, ramp = MERGE_CASES[case]
    plan = make_plan(Ll, Tt, hop, ramp)
    offs = np_offsets(Ll, Tt, hop)
    assert plan.offsets == offs
    if case.startswith("odd-ramp"):
        assert offs == [0, 11, 22, 33]
    rng = np.random.default_rng(7)
    rows_np = rng.standard_normal((n * plan.W, Cc, Tt)).astype(np.float32)
    rows = dev(rows_np)
    version = rows._version
    canvas = torch.full((n, Cc, Ll), float("nan"), device="cuda")
    assert plan.merge_(rows, canvas) is canvas
    torch.cuda.synchronize()
    assert rows._version > version, "merge_ leaves the version counter bumped"
    want, big = np_merge(rows_np, Ll, offs, plan.ramp)
    cover = np_cover(Ll, Tt, offs)
    got = canvas.cpu().numpy()
    # c fused multiply-adds (each rounds a partial sum no larger than sum k max|x|) and one division: (c + 2) 2^-24 max|x|
    bound = (cover + 2)[None, None, :] * 2.0 ** -24 * big
    err = np.abs(got.astype(np.float64) - want)
    print(f"{case}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), (case, float((err / np.maximum(bound, 1e-300)).max()))
    out = rows.cpu().numpy()
    assert np.array_equal(out, np_gather(got, Tt, offs)), "every covering row holds the canvas' bits: the canvas is the gather inverted"
    single = np_gather(np.broadcast_to(cover == 1, got.shape), Tt, offs)
    assert single.any() and np.array_equal(out[single], rows_np[single]), "singly covered elements keep their input bits"
    assert not np.array_equal(out[~single], rows_np[~single])
    # without a canvas: the same rows
    again = dev(rows_np)
    assert plan.merge_(again) is None
    assert torch.equal(again, rows)


# ================================================================== 2. the gather kernel
@pytest.mark.parametrize("lead", [1, 3])
@pytest.mark.parametrize("shape", [(2, 5, 37, 70, 11), (1, 128, 300, 560, 100), (2, 3, 300, 564, 101), (2, 3, 300, 562, 100),
                                   (1, 1, 300, 560, 100), (1, 2, 1500, 6750, 750)])
def test_gather_kernel_is_bit_exact(shape, lead):
    n, Cc, Tt, Ll, hop = shape
    plan = make_plan(Ll, Tt, hop)
    rng = np.random.default_rng(9)
    canvas = rng.standard_normal(((lead,) if lead > 1 else ()) + (n, Cc, Ll)).astype(np.float32)
    got = plan.gather(dev(canvas))
    want = np_gather(canvas, Tt, plan.offsets)
    assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want)
    out = torch.zeros_like(got)
    assert plan.gather(dev(canvas), out=out) is out and torch.equal(out, got)


# ================================================================== 3. fused sample_windows against the oracle
def oracle_sampler(kind, S):
    from jen1_amd.diffusion import get_beta_schedule
    from oracle import jen1_oracle as O
    kw = dict(objective="noise", cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    if kind == "ddim":
        return O.OracleGaussianDiffusion(steps=1000, betas=O.get_beta_schedule("linear", 1000), sampling_timesteps=S, ddim_sampling_eta=1.0, **kw)
    if kind == "ddpm":
        betas, _ = get_beta_schedule("cosine", S)
        return O.OracleGaussianDiffusion(steps=S, betas=betas.numpy().astype(np.float32), **kw)
    return O.OracleVDM(cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)


@pytest.mark.parametrize("kind", ["ddim", "ddpm", "vdm"])
def test_fused_windows_tiny_vs_oracle(tiny_f32, oracle_tiny, kind):
    """one piece of four windows: the oracle denoises the four rows, the numpy merge is applied after every step"""
    m, S, n = tiny_f32, S_ORACLE, 1
    plan = make_plan(L, T, HOP_F)
    assert plan.offsets == [0, 100, 200, 260] and plan.W == 4
    shape = (n * plan.W, C, T)
    c_np = synth.conditioning(shape[0], T, "music_inpaint")
    init, noises = canvas_draws(n, S, kind)
    ref = oracle_loop(kind, oracle_sampler(kind, S), oracle_tiny, shape, [c_np] * S, np_gather(init, T, plan.offsets),
                      [np_gather(a, T, plan.offsets) for a in noises], edits=merge_edits(S, L, plan.offsets, plan.ramp))
    sampler, kw = make_sampler(kind, S)
    with fixed_order(m):
        got = run_windows(sampler, kw, m, plan, n, cond_dev(c_np), init, noises, kind)
    assert tuple(got.shape) == (n, C, L)
    e = rel_err(np_gather(got.cpu().numpy(), T, plan.offsets), ref)
    print(f"{kind}: windowed trajectory vs the oracle {e:.3e}")
    assert e < F32_TOL, (kind, e)


# ================================================================== 4. fused against the literal loops
@pytest.mark.parametrize("kind", ["ddim", "ddpm", "vdm", "dpmpp2m"])
def test_fused_windows_match_the_literal_loop(tiny_f32, kind):
    m, S, n = tiny_f32, 4, 1
    plan = make_plan(L, T, HOP_F)
    cond = cond_dev(synth.conditioning(n * plan.W, T, "music_inpaint"))
    init, noises = canvas_draws(n, S, kind, seed=71)
    sampler, kw = make_sampler(kind, S)
    with fixed_order(m):
        fused = run_windows(sampler, kw, m, plan, n, cond, init, noises, kind)
        literal = run_windows(sampler, kw, m, plan, n, cond, init, noises, kind, fused=False)
    assert torch.isfinite(literal).all()
    e = rel_err(fused.cpu().numpy(), literal.cpu().numpy())
    print(f"{kind}: fused vs literal windowed loop {e:.3e}")
    assert e < PATH_TOL, (kind, e)


# ================================================================== 5. one window
@pytest.mark.parametrize("kind", ["ddim", "ddpm", "vdm", "dpmpp2m"])
def test_one_window_gives_the_bits_of_sample(tiny_f32, kind):
    m, S, n = tiny_f32, 3, 2
    plan = make_plan(T, T, 150)
    assert plan.W == 1
    shape = (n, C, T)
    cond = cond_dev(synth.conditioning(n, T, "music_inpaint"))
    init, noises = canvas_draws(n, S, kind, length=T, seed=81)
    sampler, kw = make_sampler(kind, S)
    more = {"step_noises": [dev(a) for a in noises]} if kind in ("ddim", "ddpm") else {}
    with fixed_order(m):
        want = sampler.sample(m, shape, cond, init_noise=dev(init), **kw, **more)
        got = sampler.sample_windows(m, plan, n, cond, init_noise=dev(init), **kw, **more)
    assert torch.equal(got, want), f"{kind}: W == 1 differs from sample ({rel_err(got.cpu(), want.cpu()):.3e})"


# ================================================================== 6. the windows agree
def test_windows_are_crops_of_the_canvas_and_share_their_noise(tiny_f32):
    m, S, n = tiny_f32, 3, 1
    plan = make_plan(L, T, HOP_F)
    shape = (n * plan.W, C, T)
    cond = cond_dev(synth.conditioning(shape[0], T, "music_inpaint"))
    gd = gdm(S, eta=1.0)
    torch.manual_seed(3)
    with fixed_order(m):
        canvas = gd.sample_windows(m, plan, n, cond)                          # the draws are the sampler's own, made on the canvas
        st = gd.stepper(m, shape, cond, n_streams=1)
    assert len(st.parts) == 1 and torch.isfinite(canvas).all()
    assert torch.equal(plan.gather(canvas), st.x), "after the last merge every window is a crop of the returned canvas"
    table = st.noise_all
    assert tuple(table.shape) == (S,) + shape and float(table.abs().max()) > 0
    for j in range(plan.W - 1):
        d = plan.offsets[j + 1] - plan.offsets[j]
        assert torch.equal(table[:, j, :, d:], table[:, j + 1, :, :T - d]), f"windows {j} and {j + 1} draw different noise at shared frames"
    assert not torch.equal(table[:, 0, :, :100], table[:, 1, :, :100])


# ================================================================== 7. known audio across the seams
@pytest.mark.parametrize("kind", ["ddim", "vdm"])
def test_known_audio_on_the_canvas_is_kept_exactly(tiny_f32, kind):
    m, S, n = tiny_f32, 3, 1
    plan = make_plan(L, T, HOP_F)
    cond = cond_dev(synth.conditioning(n * plan.W, T, "music_inpaint"))
    init, noises = canvas_draws(n, S, kind, seed=91)
    known = (synth.latents(n, L, key="known") * np.float32(0.5)).astype(np.float32)
    keep = np.ones((n, 1, L), dtype=np.float32)
    keep[:, :, 80:330] = 0.0                     # generated: crosses the starts of windows 1 .. 3 and the end of window 0
    sampler, kw = make_sampler(kind, S)
    with fixed_order(m):
        out = run_windows(sampler, kw, m, plan, n, cond, init, noises, kind, known=dev(known), keep_mask=dev(keep))
        free = run_windows(sampler, kw, m, plan, n, cond, init, noises, kind)
    sel = torch.from_numpy(np.broadcast_to(keep == 1, known.shape).copy()).cuda()
    assert torch.isfinite(out).all()
    assert torch.equal(out[sel], dev(known)[sel]), "the kept frames are the known latents, bit for bit"
    assert not torch.equal(out[~sel], dev(known)[~sel]) and not torch.equal(free[sel], dev(known)[sel])
    with pytest.raises(ValueError):
        run_windows(sampler, kw, m, plan, n, cond, init, noises, kind, known=dev(known))


# ================================================================== 8. Jen1.generate
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
    """the slice of ``encodec.EncodecModel`` generation.py touches (test_gpu_known_blend.py's, restated), with a ``decode_latents`` that
    returns ``length`` samples; the decoders keep what they were handed"""
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

    def decode_latents(self, emb, seg_frames, scales=None, length=None):
        assert sum(seg_frames) == emb.shape[2]
        return self.decoder(emb)[:, :, :length]


@pytest.fixture(scope="module")
def jen1():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.generation import Jen1
    cond = synth.conditioning(8, 300, "text_guided")
    emb = torch.from_numpy(cond["cross_attn_cond"]).cuda()
    msk = torch.from_numpy(cond["cross_attn_masks"]).cuda()
    seen = []

    def conditioner(batch_metadata, device):
        """a prompt "p<i>" selects row i of the bank; anything else row 0"""
        seen.append([dict(r) for r in batch_metadata])
        idx = [int(r["prompt"][1:]) if r["prompt"][:1] == "p" and r["prompt"][1:].isdigit() else 0 for r in batch_metadata]
        return {"prompt": (emb[idx].to(device), msk[idx].to(device))}

    j = Jen1(None, device="cuda", audio_encoder=StubAudioEncoder(), conditioner=conditioner, model_config=tiny_model_config(),
             diffusion_config=GDMConfig(), compute_dtype="f32")
    j.seen = seen
    return j


@pytest.mark.parametrize("use_gdm,sampler", [(True, None), (True, "dpmpp2m"), (False, None)])
def test_generate_long_form(jen1, use_gdm, sampler):
    """3.5 s as windows of 2 s (300 frames, hop 150: offsets 0, 150, 225 on a canvas of 525 frames), one batch of three rows per piece"""
    seconds, steps = 3.5, 3
    _, model = jen1.get_model_and_diffusion(steps, use_gdm)
    del jen1.seen[:]
    with fixed_order(model):
        out = jen1.generate(["p1", "p2", "p3"], seed=9, steps=steps, batch_size=1, seconds=seconds, use_gdm=use_gdm, sampler=sampler,
                            window_seconds=2, window_overlap=0.5, decode="segments")
    assert tuple(out.shape) == (1, 2, int(seconds * 48000)) and torch.isfinite(out).all()
    z = jen1.audio_encoder.handed
    assert tuple(z.shape) == (1, 128, 525), "the decoder receives the canvas latents"
    assert [r["prompt"] for r in jen1.seen[-1]] == ["p1", "p2", "p3"], "W prompts reach the conditioner as W distinct rows"
    with fixed_order(model):
        same = jen1.generate("p1", seed=9, steps=steps, batch_size=1, seconds=seconds, use_gdm=use_gdm, sampler=sampler,
                             window_seconds=2, decode="segments")
    assert len(jen1.seen[-1]) == 3 and not torch.equal(same, out), "per-window prompts change the piece"
    with pytest.raises(ValueError, match="W = 3"):
        jen1.generate(["p1", "p2"], seed=9, steps=steps, seconds=seconds, use_gdm=use_gdm, sampler=sampler, window_seconds=2)


def test_generate_inpaint_across_windows_keeps_the_known_frames(jen1):
    seconds, steps, n = 3.5, 3, int(3.5 * 48000)
    audio = torch.randn((1, 2, n), generator=torch.Generator().manual_seed(5)) * 0.1
    _, model = jen1.get_model_and_diffusion(steps, True)
    known = jen1.get_emb(audio.cuda())
    keep = torch.nn.functional.interpolate(jen1.get_mask(n, 0.8, 2.6, 1).cuda(), size=known.shape[2])
    sel = (keep == 1).expand(known.shape).cpu()
    with fixed_order(model):
        jen1.generate("p1", seed=9, steps=steps, batch_size=1, seconds=seconds, use_gdm=True, task="music_inpaint", init_audio=audio,
                      init_audio_sr=48000, inpainting_scope=(0.8, 2.6), preserve_known=True, window_seconds=2)
    z = jen1.audio_encoder.handed
    assert 0 < int(sel.sum()) < sel.numel() and torch.isfinite(z).all()
    assert torch.equal(z[sel], known.cpu()[sel]) and not torch.equal(z[~sel], known.cpu()[~sel])


@pytest.mark.parametrize("use_gdm", [True, False])
def test_generate_short_piece_is_the_call_without_the_keywords(jen1, use_gdm):
    steps = 3
    _, model = jen1.get_model_and_diffusion(steps, use_gdm)
    with fixed_order(model):
        want = jen1.generate("p1", seed=9, steps=steps, batch_size=2, seconds=2, use_gdm=use_gdm)
        z_want = jen1.audio_encoder.handed
        got = jen1.generate("p1", seed=9, steps=steps, batch_size=2, seconds=2, use_gdm=use_gdm, window_seconds=2, window_overlap=0.25)
        z_got = jen1.audio_encoder.handed
    assert torch.equal(z_got, z_want) and torch.equal(got, want)


# ================================================================== 9. the full model at the shape long-form generation runs at
def test_full_model_eight_windows(full_bf16):
    m, S, n = full_bf16, 2, 1
    plan = make_plan(6750, 1500, 750)
    assert plan.W == 8 and plan.ramp == 750
    shape = (n * plan.W, C, 1500)
    cond = cond_dev(synth.conditioning(shape[0], 1500, "text_guided"))
    gd = gdm(S, scale=1.0)
    init, noises = canvas_draws(n, S, "ddim", length=6750, seed=101)
    plain = gd.stepper(m, shape, cond)
    out = gd.sample_windows(m, plan, n, cond, init_noise=dev(init), step_noises=[dev(a) for a in noises])
    st = gd.stepper(m, shape, cond, n_streams=1)
    assert tuple(out.shape) == (n, C, 6750) and torch.isfinite(out).all()
    assert torch.equal(plan.gather(out), st.x), "the windows agree at the seams: each is a crop of the canvas"
    assert st.launches_per_step == plain.launches_per_step, "the replayed step is the plain stepper's"
    extra = 1 + (1 if st.parts[0].fused else 0) + (1 if st.parts[0].tail else 0)          # merge + re-pack + sentinels / arena
    record_parity("windows_full", "W8.T1500.L6750", "bf16", launches_per_step=st.launches_per_step, extra_launches_per_merged_step=extra)
