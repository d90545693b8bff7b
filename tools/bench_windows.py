"""What a merged step costs: one replayed sampler step of the windowed long-form sampler against the plain stepper at the same shape --
full model, bf16, one piece of W = 8 windows of T = 1500 frames on a canvas of 6750 (hop 750), i.e. B = 8 batch rows, 100-step DDIM
schedule, graph replay -- without the CFG pair and with it.  Prints one JSON line.

Variants, on ONE stepper (the plain path is untouched code), timed in alternation: ``--rounds`` rounds, each one region of ``--steps``
steps per variant after a warm-up; a region starts with reset() + 2 untimed steps and is bracketed by device synchronisation; median and
spread per variant:
  plain     st.step(i)
  windows   st.step(i); plan.merge_(st.x)      -- the merge launch, and through the version counter the re-pack of the network input
                                                 (pack_input_parts + the statistics' sum) and the sentinel / arena reset before the next step
The three extra launches are also timed by themselves: ``--launches`` back-to-back launches of each between two synchronisations (the
in-stream cost per launch; run the tool under a kernel trace for the kernels' own durations).

    python tools/bench_windows.py [--steps 100] [--rounds 5] [--warmup 20] [--launches 200]
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


def measure(model, plan, scale, args):
    from jen1_amd import synth
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    B, T = plan.W, plan.window
    shape = (B, 128, T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                           embedding_scale=scale, batch_cfg=True, scale_cfg=True, sampling_timesteps=100)
    cond = {k: (None if v is None else dev(v)) for k, v in synth.conditioning(B, T).items()}
    st = gd.stepper(model, shape, cond, n_streams=1)
    assert len(st.parts) == 1 and st.fused_tail
    x0 = plan.gather(dev(synth.noise_list(1, (1, 128, plan.length), seed=5)[0]))
    st.reset(x0)                                                            # (draws the per-step noise table once)
    S = st.num_steps

    def run(name, k0, n):
        for i in range(k0, k0 + n):
            st.step(i % S)
            if name == "windows":
                plan.merge_(st.x)

    def start(name):
        st.reset(x0, fresh_noise=False)
        run(name, 0, 2)

    names = ("plain", "windows")
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
    st.check()
    assert torch.isfinite(st.x).all()
    # the three extra launches by themselves, back to back
    s = torch.cuda.current_stream().cuda_stream
    eng_plan = st.parts[0].plan
    singles = {"merge": lambda: plan.merge_(st.x), "pack": lambda: eng_plan.run_pack(s), "poison": lambda: eng_plan.run_poison(s)}
    per_launch = {}
    for name, fn in singles.items():
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.launches):
            fn()
        torch.cuda.synchronize()
        per_launch[name + "_us"] = round((time.perf_counter() - t0) / args.launches * 1e6, 2)
    st.reset(x0, fresh_noise=False)                                         # (the raw launches left the plan mid-protocol: start over)
    out = {"launches_per_step": st.launches_per_step, "extra_launches_per_merged_step": 3, "back_to_back": per_launch}
    for name in names:
        v = times[name]
        out[name] = {"ms_per_step_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                     "steps_per_s": round(1e3 / statistics.median(v), 1)}
    a, b = (out[n]["ms_per_step_median"] for n in names)
    out["windows_minus_plain_ms"] = round(b - a, 4)
    out["windows_minus_plain_pct"] = round(100.0 * (b - a) / a, 2)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    assert args.steps >= 1 and args.rounds >= 1
    assert torch.cuda.is_available(), "bench_windows needs a GPU"
    from jen1_amd.config import full_model_config
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.windows import WindowPlan
    plan = WindowPlan(6750, 1500, 750)
    model = UNetCFG1d(**full_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    out = {"what": f"one replayed DDIM step, full model bf16, n=1 x W={plan.W} windows of T={plan.window} on a canvas of {plan.length} "
                   "(B=8 rows), 100-step schedule: plain stepper / step + window merge (+ re-pack + sentinel reset)",
           "steps_per_region": args.steps, "regions": args.rounds,
           # bytes the merge moves: every doubly covered row element read and written once (float32), the rest untouched
           "merge_bytes": int(2 * 4 * 128 * sum(max(0, a + plan.window - b) for a, b in zip(plan.offsets, plan.offsets[1:])) * 2)}
    out["nocfg"] = measure(model, plan, 1.0, args)
    out["cfg_pair"] = measure(model, plan, 0.8, args)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
