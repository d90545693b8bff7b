"""Time one replayed sampler step with the plain DDIM row and with the DPM-Solver++(2M) row at the bench workload (configs[1]: full
model, B = 8, 128 x 1500, bf16, no CFG pair, 100-step schedule, graph replay), and print one JSON line.

Variants, timed in alternation (round robin, ``--rounds`` regions of ``--steps`` steps each per variant, after a warm-up; a region is
bracketed by device synchronisation on both sides; median and spread per variant):
  plain   the plain stepper (jen1_step_tail; eta = 1, so every step reads its 6 MB slice of the noise table)
  dpmpp   the multistep stepper (jen1_step_tail_ms: no noise read, one 6 MB history read and one 6 MB history write)
Gate: median(dpmpp) - median(plain) <= spread(plain) + 1 % of median(plain), spread = max - min over the plain regions.  The multistep
step is measured against the plain stepper of the same run, never against itself.

    python tools/dpm_step_bench.py [--steps 20] [--rounds 12] [--warmup 10]
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
    assert torch.cuda.is_available(), "dpm_step_bench needs a GPU"
    from jen1_amd import synth
    from jen1_amd.config import full_model_config
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
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
    # (both steppers on the plan of the bench: a region starts with a reset, which hands the plan over, and two untimed steps)
    steppers = {"plain": gd.stepper(model, shape, cond), "dpmpp": gd.stepper(model, shape, cond, mode="dpmpp", order=2)}
    plain, ms = steppers["plain"], steppers["dpmpp"]
    assert plain.fused_tail and ms.fused_tail and plain.launches_per_step == ms.launches_per_step
    plain.reset(x0)                                                         # (draws the per-step noise table once)
    ms.reset(x0)
    S = plain.num_steps

    def run(name, k0, n):
        st = steppers[name]
        for i in range(k0, k0 + n):
            st.step(i % S)

    def start(name):
        steppers[name].reset(x0, fresh_noise=False)
        run(name, 0, 2)

    names = ("plain", "dpmpp")
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
    ms.check()
    out = {"what": f"one replayed sampler step, full model bf16, B={B}, T={T}, no CFG pair, 100-step schedule: DDIM row (eta = 1) / "
                   "DPM-Solver++(2M) row", "steps_per_region": args.steps, "regions": args.rounds,
           "launches_per_step": ms.launches_per_step}
    for name in names:
        v = times[name]
        out[name] = {"ms_per_step_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "spread_ms": round(max(v) - min(v), 4)}
    a, b = (out[n]["ms_per_step_median"] for n in names)
    out["dpmpp_minus_plain_ms"] = round(b - a, 4)
    out["dpmpp_minus_plain_pct"] = round(100.0 * (b - a) / a, 3)
    out["gate_ms"] = round(out["plain"]["spread_ms"] + 0.01 * a, 4)
    out["dpmpp_within_gate"] = bool(b - a <= out["plain"]["spread_ms"] + 0.01 * a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
