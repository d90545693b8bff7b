"""-m gpu: the EMA of the weights (jen1_amd/ema.py) -- the fused AdamW + EMA kernel against a float64 oracle and against the plain AdamW
kernel, the trainer, ``swap`` / ``copy_to`` for sampling, checkpoint resume, ``Jen1(weights="ema")`` and two data-parallel ranks."""
import numpy as np
import pytest
import torch

from jen1_amd import synth
from jen1_amd.config import tiny_model_config
from test_ema import _schedule_np

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _oracle_ema(e_prev, p_new, t, s):
    """float64 restatement of the EMA of step t applied to the kernel's previous EMA and new parameters -> (expected, tolerance)"""
    mode, decay = _schedule_np(np.array([t]), s["beta"], s["update_after_step"], s["update_every"], s["warmup"], s["inv_gamma"],
                               s["power"], s["min_decay"])
    e = e_prev.astype(np.float64)
    p = p_new.astype(np.float64)
    if mode[0] == 0:
        return e, np.zeros_like(e)
    if mode[0] == 1:
        return p, np.zeros_like(e)
    want = e + (1.0 - decay[0]) * (p - e)
    return want, 4 * ULP * np.maximum(np.abs(e), np.abs(p))


class _Flat:
    """p, m, v (and an EMA) over one flat float32 buffer of n elements, driven through the C entries directly"""

    def __init__(self, p0, with_ema):
        n = p0.numel()
        self.n = n
        self.p = p0.clone()
        self.m = torch.zeros(n, device="cuda")
        self.v = torch.zeros(n, device="cuda")
        self.ema = p0.clone() if with_ema else None
        self.steps = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.gn = torch.zeros(1, device="cuda")
        from jen1_amd import lib as L
        self.L = L
        self.lib = L.load()
        self.scratch = torch.zeros(int(self.lib.jen1_grad_sqnorm_scratch_bytes()) // 4, device="cuda")

    def step(self, g, hp, sched=None, skip_nonfinite=1):
        L, lib, s = self.L, self.lib, _stream()
        self.gn.zero_()
        L.check(lib.jen1_grad_sqnorm_ws(g.data_ptr(), self.n, self.gn.data_ptr(), self.scratch.data_ptr(), s), "sqnorm")
        args = [self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, hp["lr"], hp["b1"], hp["b2"], hp["eps"],
                hp["wd"], self.steps.data_ptr(), self.gn.data_ptr(), hp["max_norm"], skip_nonfinite]
        if sched is None:
            L.check(lib.jen1_adamw_step_counted(*args, s), "plain")
        else:
            L.check(lib.jen1_adamw_ema_step_counted(*args, self.ema.data_ptr(), sched["beta"], sched["update_after_step"],
                                                    sched["update_every"], int(sched["warmup"]), sched["inv_gamma"], sched["power"],
                                                    sched["min_decay"], s), "fused")


HP = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, max_norm=0.5)
SCHEDULES = [
    dict(beta=0.999, update_after_step=5, update_every=3, warmup=True, inv_gamma=1.0, power=2.0 / 3.0, min_decay=0.0),
    dict(beta=0.9, update_after_step=0, update_every=1, warmup=True, inv_gamma=1.0, power=0.75, min_decay=0.5),
    dict(beta=0.99, update_after_step=1, update_every=1, warmup=False, inv_gamma=1.0, power=2.0 / 3.0, min_decay=0.0),
    dict(beta=0.9999, update_after_step=100, update_every=10, warmup=True, inv_gamma=1.0, power=2.0 / 3.0, min_decay=0.0),
    dict(beta=0.95, update_after_step=12, update_every=2, warmup=True, inv_gamma=4.0, power=0.5, min_decay=0.1),
]


@pytest.mark.parametrize("si", range(len(SCHEDULES)))
def test_fused_kernel_vs_float64_oracle_and_plain_step(si):
    """multi-tensor flat buffer with an n % 4 = 3 tail and clipping on, 40 steps: p / m / v bit-identical to jen1_adamw_step_counted,
    the EMA within a few float32 ulps of the float64 oracle applied to the kernel's own new parameters"""
    sched = SCHEDULES[si]
    gen = torch.Generator().manual_seed(100 + si)
    n = 3 * 1024 + 517 + 4 * 333 + 2            # several "tensors" back to back, odd total (tail of 3 handled by block 0)
    assert n % 4 == 3
    p0 = (torch.randn(n, generator=gen) * 0.2).cuda()
    plain, fused = _Flat(p0, False), _Flat(p0, True)
    clipped = 0
    for step in range(1, 41):
        g = (torch.randn(n, generator=gen) * (0.01 + 0.05 * (step % 5))).cuda()
        e_prev = fused.ema.cpu().numpy()
        plain.step(g, HP)
        fused.step(g, HP, sched)
        torch.cuda.synchronize()
        clipped += int(float(fused.gn.sqrt()) > HP["max_norm"])
        assert torch.equal(plain.p, fused.p) and torch.equal(plain.m, fused.m) and torch.equal(plain.v, fused.v), step
        assert int(fused.steps) == step == int(plain.steps)
        want, tol = _oracle_ema(e_prev, fused.p.cpu().numpy(), step, sched)
        got = fused.ema.cpu().numpy().astype(np.float64)
        err = np.abs(got - want) - tol
        assert (err <= 0).all(), (step, float(err.max()), int(err.argmax()))
    assert clipped > 0
    assert not torch.equal(fused.ema, p0) or sched["update_after_step"] >= 40


def test_skip_nonfinite_leaves_the_ema_and_its_step_alone():
    sched = SCHEDULES[1]
    gen = torch.Generator().manual_seed(7)
    n = 4 * 257 + 2
    p0 = (torch.randn(n, generator=gen) * 0.2).cuda()
    grads = [(torch.randn(n, generator=gen) * 0.05).cuda() for _ in range(4)]
    a, b = _Flat(p0, True), _Flat(p0, True)
    for i, g in enumerate(grads):
        a.step(g, HP, sched)
        if i == 2:                                  # b sees one more step in between, with an inf gradient
            before = (b.p.clone(), b.m.clone(), b.v.clone(), b.ema.clone(), int(b.steps))
            bad = g.clone()
            bad[n // 3] = float("inf")
            b.step(bad, HP, sched)
            torch.cuda.synchronize()
            assert torch.equal(b.p, before[0]) and torch.equal(b.m, before[1]) and torch.equal(b.v, before[2])
            assert torch.equal(b.ema, before[3]) and int(b.steps) == before[4]
        b.step(g, HP, sched)
    torch.cuda.synchronize()
    assert int(a.steps) == int(b.steps) == 4
    assert torch.equal(a.p, b.p) and torch.equal(a.ema, b.ema)


def test_constant_decay_matches_torch_averaged_model():
    """warmup=False, update_after_step=1, update_every=1: torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(beta) driven by
    torch.optim.AdamW + clip_grad_norm_ on the same gradients"""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from jen1_amd.ema import ParamEMA
    from jen1_amd.optim import FusedAdamW
    beta = 0.9
    gen = torch.Generator().manual_seed(3)
    shapes = [(16, 8, 3), (16,), (5, 7), (3,), (33,)]
    init = [torch.randn(s, generator=gen) * 0.3 for s in shapes]
    grads = [[torch.randn(s, generator=gen) * 0.1 for s in shapes] for _ in range(12)]
    ref = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in init])
    avg = AveragedModel(ref, multi_avg_fn=get_ema_multi_avg_fn(beta))
    topt = torch.optim.AdamW(ref.parameters(), lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
    mine = torch.nn.ParameterList([torch.nn.Parameter(t.clone().cuda()) for t in init])
    opt = FusedAdamW(mine.parameters(), lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1, max_norm=0.3)
    ema = ParamEMA(opt, beta=beta, update_after_step=1, update_every=1, warmup=False, model=mine)
    for gs in grads:
        for p, g in zip(ref.parameters(), gs):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.3)
        topt.step()
        avg.update_parameters(ref)
        for p, g in zip(mine.parameters(), gs):
            p.grad.copy_(g)
        opt.step()
    torch.cuda.synchronize()
    got = ema.state_dict()
    for i, p in enumerate(avg.module.parameters()):
        want = p.detach()
        assert torch.allclose(got[str(i)], want, rtol=1e-4, atol=1e-6), (i, float((got[str(i)] - want).abs().max()))
    assert float((got["0"] - init[0]).abs().max()) > 1e-3


# ------------------------------------------------------------------ the trainer
def _tiny_trainer(use_graph, use_ema, ema_kwargs=None, lr=1e-3, compute_dtype="bf16", grad_accum_every=2):
    import random
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype=compute_dtype, device="cuda")
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.2, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    opt = FusedAdamW(model.parameters(), lr=lr)
    B, T = 6, 300
    emb = dev(synth.conditioning(B, T, "text_guided")["cross_attn_cond"])
    msk = dev(synth.conditioning(B, T, "text_guided")["cross_attn_masks"])

    def conditioner(metadata, device):
        idx = torch.tensor(metadata, device=device)
        return {"prompt": (emb[idx], msk[idx])}

    tr = UnifiedMultiTaskTrainer.build(model, gd, conditioner, opt, None, grad_accum_every=grad_accum_every, rng=random.Random(0),
                                       use_graph=use_graph, use_ema=use_ema, ema_kwargs=ema_kwargs)
    audio = dev(synth.latents(B, T, key="clip"))
    return tr, model, gd, opt, audio, list(range(B))


TRAIN_EMA = dict(beta=0.95, update_after_step=1, update_every=2, warmup=True, inv_gamma=1.0, power=0.75, min_decay=0.0)


@pytest.mark.parametrize("use_graph", [False, True])
def test_trainer_ema_does_not_perturb_training(use_graph):
    """grad_accum_every=2, 4 optimiser steps.  The backward pass is not run-to-run bit-reproducible (float atomics), so each optimiser
    step of the EMA run is replayed through the plain AdamW entry from the same state and gradient: bit-identical parameters and moments.
    The EMA changes only at optimiser steps and follows the float64 oracle applied to the recorded parameters.  A trainer without EMA
    keeps the plain path; its losses before the first optimiser step agree to the run-to-run spread of the backward pass"""
    from jen1_amd import lib as L
    tr, model, gd, opt, audio, md = _tiny_trainer(use_graph, True, TRAIN_EMA)
    assert tr.ema is not None and opt.ema is tr.ema
    lib = L.load()
    orig_step = opt.step
    replays = []

    def checked_step(lr=None):
        state = [t.clone() for t in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt._steps)]
        e_prev = tr.ema.ema.cpu().numpy()
        orig_step(lr)
        torch.cuda.synchronize()
        p, m, v, c = state
        s = _stream()
        L.check(lib.jen1_adamw_step_counted(p.data_ptr(), opt.flat_grad.data_ptr(), m.data_ptr(), v.data_ptr(), opt.numel,
                                            float(opt.lr if lr is None else lr), float(opt.betas[0]), float(opt.betas[1]), float(opt.eps),
                                            float(opt.weight_decay), c.data_ptr(), opt._gnorm_sq.data_ptr(), float(opt.max_norm or 0.0),
                                            1 if opt.skip_nonfinite else 0, s), "plain replay")
        torch.cuda.synchronize()
        replays.append((torch.equal(p, opt.flat_param) and torch.equal(m, opt.exp_avg) and torch.equal(v, opt.exp_avg_sq)
                        and torch.equal(c, opt._steps), e_prev, opt.flat_param.cpu().numpy(), tr.ema.ema.cpu().numpy()))

    opt.step = checked_step
    torch.manual_seed(0)
    losses, emas = [], [tr.ema.ema.clone()]
    for it in range(8):
        loss, _, stepped = tr.train_step(audio, md)
        torch.cuda.synchronize()
        losses.append(float(loss))
        emas.append(tr.ema.ema.clone())
        assert stepped == (it % 2 == 1)
        if not stepped:
            assert torch.equal(emas[-1], emas[-2]), it
    assert opt.step_count == 4 and len(replays) == 4
    for t, (same, e_prev, p_new, e_new) in enumerate(replays, start=1):
        assert same, f"optimiser step {t}: the EMA launch changed p / m / v"
        want, tol = _oracle_ema(e_prev, p_new, t, TRAIN_EMA)
        assert (np.abs(e_new.astype(np.float64) - want) <= tol).all(), t
    # t = 1 leaves the EMA at the initial weights, t = 2 and 4 update it
    assert torch.equal(emas[2], emas[0]) and not torch.equal(emas[4], emas[2]) and not torch.equal(emas[8], emas[6])
    tr0, *_ = _tiny_trainer(use_graph, False)
    assert tr0.ema is None and tr0.optimizer.ema is None
    torch.manual_seed(0)
    losses0 = [float(tr0.train_step(audio, md)[0]) for _ in range(2)]
    np.testing.assert_allclose(losses[:2], losses0, rtol=1e-3)


def _train_loss(model, gd, x0, t, cond, noise):
    """the training forward (TrainGraph, the training compute copies) of one batch, no backward; the model is left in eval mode"""
    model.train()
    torch.manual_seed(5)                        # the CFG dropout draw
    loss = float(gd.training_loosses(model, x0, t, cond, noise=noise, causal=False).detach())
    model.eval()
    return loss


def test_swap_samples_from_the_ema_and_restores_training():
    """``with ema.swap(model)``: diffusion.sample on the EMA weights == sampling from a fresh model written by ``copy_to``, bit for bit;
    after the block the parameters are the optimiser's buffer again and the training and sampling copies are the trained weights"""
    from jen1_amd.init_fill import fill_uniform
    from jen1_amd.model import UNetCFG1d
    tr, model, gd, opt, audio, md = _tiny_trainer(False, True, dict(beta=0.5, update_after_step=0, update_every=1, warmup=False),
                                                  lr=1e-2, compute_dtype="f32", grad_accum_every=1)
    torch.manual_seed(0)
    for _ in range(3):
        tr.train_step(audio, md)
    torch.cuda.synchronize()
    ema = tr.ema
    assert float((ema.ema - opt.flat_param).abs().max()) > 1e-3
    model.eval()
    model.deterministic = True
    B, T, S = 2, 300, 4
    cond = {k: dev(v) for k, v in synth.conditioning(B, T).items()}
    shape = (B, 128, T)
    init = dev(synth.noise_list(1, shape, seed=7)[0])
    noises = [dev(n) for n in synth.noise_list(S, shape, seed=11)]
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    betas, _ = get_beta_schedule("linear", 1000)
    sd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                           embedding_scale=0.8, batch_cfg=True, scale_cfg=True, sampling_timesteps=S)
    x = dev(synth.latents(B, T))
    t = torch.tensor([999, 499], device="cuda")
    kw = dict(embedding=cond["cross_attn_cond"], embedding_mask=cond["cross_attn_masks"], channels_list=[cond["input_concat_cond"]],
              embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    y_before = model(x, t, **kw).clone()
    x0 = dev(synth.latents(B, T, key="clip"))
    tt = torch.tensor([17, 801], dtype=torch.long, device="cuda")
    tcond = {k: dev(v) for k, v in synth.conditioning(B, T, "text_guided").items()}
    tnoise = dev(fill_uniform("synth.trainnoise.text_guided", (B, 128, T), 3, 0.0, 1.0))
    loss_before = _train_loss(model, gd, x0, tt, tcond, tnoise)
    flat_before = opt.flat_param.clone()
    with ema.swap(model):
        for p, o in zip(opt.params, opt.offsets):
            assert p.data_ptr() == ema.ema[o:].data_ptr()
        y_swap = sd.sample(model, shape, cond, init_noise=init, step_noises=noises)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError):
            opt.step()
    fresh = UNetCFG1d(**tiny_model_config(), init_seed=None, compute_dtype="f32", device="cuda")
    ema.copy_to(fresh)
    fresh.eval()
    fresh.deterministic = True
    y_fresh = sd.sample(fresh, shape, cond, init_noise=init, step_noises=noises)
    torch.cuda.synchronize()
    assert torch.equal(y_swap, y_fresh)
    # back on the trained weights: pointers, values, the sampling engine and the training compute copies
    for p, o in zip(opt.params, opt.offsets):
        assert p.data_ptr() == opt.flat_param[o:].data_ptr()
    assert torch.equal(opt.flat_param, flat_before)
    y_after = model(x, t, **kw)
    assert torch.equal(y_after, y_before)
    y_plain = sd.sample(model, shape, cond, init_noise=init, step_noises=noises)
    assert not torch.equal(y_plain, y_swap)
    loss_after = _train_loss(model, gd, x0, tt, tcond, tnoise)
    assert abs(loss_after - loss_before) <= 1e-5 * abs(loss_before), (loss_before, loss_after)
    loss, _, stepped = tr.train_step(audio, md)
    assert stepped and np.isfinite(float(loss)) and opt.step_count == 4


# ------------------------------------------------------------------ resume, generation, data parallel
def _synthetic_run(model, opt, ema, steps, first):
    """optimiser steps on fixed synthetic gradients (a function of the step number only)"""
    for k in range(first, first + steps):
        g = torch.Generator().manual_seed(1000 + k)
        opt.flat_grad.copy_((torch.randn(opt.numel, generator=g) * 0.05).cuda())
        opt.step()
    torch.cuda.synchronize()


def _ema_setup(seed=1234):
    from jen1_amd.ema import ParamEMA
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    model = UNetCFG1d(**tiny_model_config(), init_seed=seed, compute_dtype="f32", device="cuda")
    opt = FusedAdamW(model.parameters(), lr=1e-2)
    ema = ParamEMA(opt, beta=0.9, update_after_step=2, update_every=1, warmup=True, model=model)
    return model, opt, ema


def test_resume_is_bit_identical(tmp_path):
    from jen1_amd.checkpoint import load_checkpoint, save_checkpoint
    N, M = 3, 4
    m1, o1, e1 = _ema_setup()
    _synthetic_run(m1, o1, e1, N + M, 0)
    m2, o2, e2 = _ema_setup()
    _synthetic_run(m2, o2, e2, N, 0)
    path = str(tmp_path / "mid.pth")
    save_checkpoint(m2, o2, 1e-2, N, path, ema=e2)
    m3, o3, e3 = _ema_setup(seed=99)
    load_checkpoint(path, m3, optimizer=o3, ema=e3)
    assert o3.step_count == N
    _synthetic_run(m3, o3, e3, M, N)
    a, b = e1.state_dict(), e3.state_dict()
    pa, pb = m1.state_dict(), m3.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(pa[k], pb[k]), k
    assert any(not torch.equal(a[k], pa[k].cpu()) for k in a)


def test_jen1_samples_from_the_checkpoint_ema(tmp_path):
    from jen1_amd.checkpoint import save_checkpoint
    from jen1_amd.config import GDMConfig
    from jen1_amd.generation import Jen1
    from test_gpu_generation import StubAudioEncoder
    m, o, e = _ema_setup()
    _synthetic_run(m, o, e, 4, 0)
    path = str(tmp_path / "ema.pth")
    save_checkpoint(m, o, 1e-2, 4, path, ema=e)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    cond = synth.conditioning(2, 300, "text_guided")
    emb = torch.from_numpy(cond["cross_attn_cond"]).cuda()
    msk = torch.from_numpy(cond["cross_attn_masks"]).cuda()

    def conditioner(batch_metadata, device):
        n = len(batch_metadata)
        return {"prompt": (emb[:n].to(device), msk[:n].to(device))}

    kw = dict(device="cuda", audio_encoder=StubAudioEncoder(), conditioner=conditioner, model_config=tiny_model_config(),
              diffusion_config=GDMConfig(), compute_dtype="f32")
    j_ema = Jen1(path, weights="ema", **kw)
    j_ref = Jen1(None, **kw)
    with pytest.raises(ValueError):
        Jen1(path, weights="nope", **kw)
    _, me = j_ema.get_model_and_diffusion(3, True)
    _, mr = j_ref.get_model_and_diffusion(3, True)
    mr.load_state_dict(ck["ema"])
    for k, v in me.state_dict().items():
        assert torch.equal(v.cpu(), ck["ema"][k]), k
    me.deterministic = mr.deterministic = True
    a = j_ema.generate("p", seed=5, steps=3, batch_size=2, seconds=2, use_gdm=True)
    b = j_ref.generate("p", seed=5, steps=3, batch_size=2, seconds=2, use_gdm=True)
    assert torch.equal(a, b)


def _ema_ddp_worker(rank, world, port, q):
    try:
        import os
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        from jen1_amd.optim import allreduce_gradients
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            torch.cuda.set_device(0)
            m, opt, ema = _ema_setup()
            for k in range(5):
                g = torch.Generator().manual_seed(100 * rank + k)          # every rank its own gradients
                opt.flat_grad.copy_((torch.randn(opt.numel, generator=g) * 0.05).cuda())
                allreduce_gradients(opt.flat_grad, bucket_bytes=64 << 10)
                opt.step()
            torch.cuda.synchronize()
            mine = ema.ema.cpu()
            gathered = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(gathered, mine)
            q.put((rank, {"same": all(torch.equal(gathered[0], x) for x in gathered),
                          "moved": bool(float((mine - opt.flat_param.cpu()).abs().max()) > 0)}))
        finally:
            dist.destroy_process_group()
    except BaseException:
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise


def test_ema_two_ranks_gloo_stay_identical():
    import torch.multiprocessing as mp
    from test_gpu_train import _collect, _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ema_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(_collect(q, procs, 2, 300))
    for r in res.values():
        assert "error" not in r, r["error"]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0]["same"] and res[1]["same"] and res[0]["moved"]
