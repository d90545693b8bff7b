"""Time one replayed sampler step with and without global conditioning at the bench workload (configs[1]: full model, B = 8, 128 x 1500,
bf16, no CFG pair, 100-step DDIM schedule, graph replay), and print one JSON line.

Variants, timed in alternation (round robin, ``--rounds`` regions of ``--steps`` steps each per variant, after a warm-up; a region is
bracketed by device synchronisation on both sides; median and spread per variant):
  plain      the model without ``context_features``: FiLM rows shared by the batch (``film_step``), 5 launches per step
  featured   the same model + ``context_features = 64``: per-sample FiLM form of the persistent launches on the current tables,
             ``jen1_film_select`` at the head of the step, 6 launches per step
plus the selection launch alone (``--select-reps`` launches back to back, eager).

    python tools/global_cond_bench.py [--steps 20] [--rounds 12] [--warmup 10]
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
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--select-reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "global_cond_bench needs a GPU"
    from jen1_amd import synth
    from jen1_amd.config import full_model_config
    from jen1_amd.diffusion import GaussianDiffusion, film_table_bytes, get_beta_schedule
    from jen1_amd.init_fill import fill_normal
    from jen1_amd.model import UNetCFG1d
    B, T, F = args.batch, args.frames, args.features
    shape = (B, 128, T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                           embedding_scale=1.0, batch_cfg=True, scale_cfg=True, sampling_timesteps=100)
    cond = {k: (None if v is None else dev(v)) for k, v in synth.conditioning(B, T).items()}
    x0 = dev(synth.latents(B, T))
    models = {"plain": UNetCFG1d(**full_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda"),
              "featured": UNetCFG1d(**dict(full_model_config(), context_features=F), init_seed=1234, compute_dtype="bf16", device="cuda")}
    conds = {"plain": cond, "featured": dict(cond, global_cond=dev(fill_normal("synth.features", (B, F), 5)))}
    steppers = {k: gd.stepper(models[k], shape, conds[k]) for k in models}
    assert steppers["plain"].fused_tail and steppers["featured"].fused_tail
    assert steppers["plain"].launches_per_step + 1 == steppers["featured"].launches_per_step
    for st in steppers.values():
        st.reset(x0)
    S = steppers["plain"].num_steps

    def run(name, k0, n):
        st = steppers[name]
        for i in range(k0, k0 + n):
            st.step(i % S)

    def start(name):
        steppers[name].reset(x0, fresh_noise=False)
        run(name, 0, 2)

    names = ("plain", "featured")
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
    for st in steppers.values():
        st.check()
    plan = steppers["featured"].plan
    out = {"what": f"one replayed sampler step, full model bf16, B={B}, T={T}, no CFG pair, 100-step DDIM schedule: without / with "
                   f"context_features={F}", "steps_per_region": args.steps, "regions": args.rounds,
           "launches_per_step": {n: steppers[n].launches_per_step for n in names},
           "film_ld": int(models["featured"].engine().W.film_ld), "film_table_MiB": round(film_table_bytes(models["featured"], B, S) / 2 ** 20, 1)}
    for name in names:
        v = times[name]
        med = statistics.median(v)
        out[name] = {"ms_per_step_median": round(med, 4), "steps_per_s": round(1e3 / med, 1), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "spread_ms": round(max(v) - min(v), 4)}
    a, b = (out[n]["ms_per_step_median"] for n in names)
    out["featured_minus_plain_ms"] = round(b - a, 4)
    out["featured_minus_plain_pct"] = round(100.0 * (b - a) / a, 3)
    # the selection launch alone, back to back (launch-bound: an upper bound on what it adds inside a graph)
    sel = next(op for op in plan.ops if getattr(op, "kind", "") == "film_select")
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(10):
        sel(s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.select_reps):
        sel(s)
    e1.record()
    torch.cuda.synchronize()
    out["film_select_us_back_to_back"] = round(e0.elapsed_time(e1) * 1e3 / args.select_reps, 2)
    out["film_select_bytes"] = int(sel.bytes)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
