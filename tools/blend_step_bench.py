"""Time one replayed sampler step with and without the known-region blend at the bench workload (configs[1]: full model, B = 8,
128 x 1500, bf16, no CFG pair, 100-step DDIM schedule, graph replay), and print one JSON line.

Variants, timed in alternation (round robin, ``--rounds`` regions of ``--steps`` steps each per variant, after a warm-up; a region is
bracketed by device synchronisation on both sides; median and spread per variant):
  plain        the plain stepper (jen1_step_tail)
  blend        the blend stepper with an inpaint mask (jen1_step_tail_blend): the blend inside the tail launch
  torch_blend  the plain stepper, the same blend written in torch between the steps through ``set_x`` -- every step then re-packs the
               network input and resets the sentinels from the host (what the sampler offered before the blend steppers)
Gate: median(blend) - median(plain) <= spread(plain) + 1 % of median(plain), spread = max - min over the plain regions; and
blend < torch_blend.  Run it under a kernel trace to read the duration of the two tail kernels side by side.

    python tools/blend_step_bench.py [--steps 20] [--rounds 12] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1500)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "blend_step_bench needs a GPU"
    from jen1_amd import synth
    from jen1_amd.config import full_model_config
    from jen1_amd.diffusion import GaussianDiffusion, blend_known, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    B, T = args.batch, args.frames
    shape = (B, 128, T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    model = UNetCFG1d(**full_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                           embedding_scale=1.0, batch_cfg=True, scale_cfg=True, sampling_timesteps=100)
    cond = {k: (None if v is None else dev(v)) for k, v in synth.conditioning(B, T).items()}
    x0 = dev(synth.latents(B, T))
    known = dev(synth.latents(B, T, key="known") * np.float32(0.5))
    eps_k = dev(synth.noise_list(1, shape, seed=47)[0])
    keep = torch.ones((B, 1, T), device="cuda")
    keep[:, :, (3 * T) // 10:(7 * T) // 10] = 0.0                          # inpaint the middle 40 %
    # (both steppers on the plan of the bench: a region starts with a reset, which hands the plan over, and two untimed steps)
    plain = gd.stepper(model, shape, cond)
    blend = gd.stepper(model, shape, cond, blend=True)
    assert plain.fused_tail and blend.fused_tail and plain.launches_per_step == blend.launches_per_step
    blend.set_known(known, keep, eps_k)
    plain.reset(x0)                                                         # (draws the per-step noise tables once)
    blend.reset(x0)
    kb = blend.kb.tolist()
    S = plain.num_steps

    def run(name, k0, n):
        for i in range(k0, k0 + n):
            j = i % S
            if name == "blend":
                blend.step(j)
            else:
                plain.step(j)
                if name == "torch_blend":
                    plain.set_x(blend_known(plain.x, known, keep, eps_k, *kb[j]))

    def start(name):
        (blend if name == "blend" else plain).reset(x0, fresh_noise=False)
        run(name, 0, 2)

    names = ("plain", "blend", "torch_blend")
    for name in names:
        start(name)
        run(name, 2, args.warmup)
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    k = 2
    for _ in range(args.rounds):
        for name in names:
            start(name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, k, args.steps)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        k += args.steps
    plain.check()
    blend.check()
    out = {"what": f"one replayed DDIM step, full model bf16, B={B}, T={T}, no CFG pair, 100-step schedule: plain / blend in the tail launch / "
                   "blend in torch between steps", "steps_per_region": args.steps, "regions": args.rounds,
           "launches_per_step": plain.launches_per_step}
    for name in names:
        v = times[name]
        out[name] = {"ms_per_step_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "spread_ms": round(max(v) - min(v), 4)}
    a, b, c = (out[n]["ms_per_step_median"] for n in names)
    out["blend_minus_plain_ms"] = round(b - a, 4)
    out["blend_minus_plain_pct"] = round(100.0 * (b - a) / a, 3)
    out["gate_ms"] = round(out["plain"]["spread_ms"] + 0.01 * a, 4)
    out["blend_within_gate"] = bool(b - a <= out["plain"]["spread_ms"] + 0.01 * a)
    out["torch_blend_over_blend"] = round(c / b, 3)
    out["blend_faster_than_torch_blend"] = bool(b < c)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
