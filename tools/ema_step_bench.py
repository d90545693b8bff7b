"""Time ``FusedAdamW.step()`` (clip_grad_norm_ + AdamW) with and without an attached ``ParamEMA`` over the full
model's parameter count, and print one JSON line.

Variants, timed in alternation (round robin, ``--rounds`` rounds of ``--reps`` steps each, median per variant):
  plain       no EMA attached: jen1_grad_sqnorm + jen1_adamw_step_counted                       32 B/param (norm 4 + update 28)
  ema_update  EMA attached, every step an update step (update_every=1, update_after_step=0):
              jen1_grad_sqnorm + jen1_adamw_ema_step_counted                                    40 B/param (+ EMA read and write)
  ema_skip    EMA attached, a step the schedule leaves out (t % update_every != 0)               32 B/param
Achieved GB/s = algorithmic bytes / device-event time.  Target: ema_update's achieved GB/s (at 40 B/param) within 10 % of plain's.

    python tools/ema_step_bench.py [--params 296543106] [--reps 10] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

FULL_PARAMS = 296_543_106          # configs[3] full JEN-1 1D-UNet (BENCH extra.optimizer_step)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=FULL_PARAMS)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ema_step_bench needs a GPU"
    from jen1_amd.ema import ParamEMA
    from jen1_amd.optim import FusedAdamW
    n = args.params
    p = torch.nn.Parameter(torch.randn(n, device="cuda") * 0.02)
    opt = FusedAdamW([p], lr=3e-5, betas=(0.9, 0.95), weight_decay=0.1, max_norm=0.7)
    p.grad.normal_(0, 1e-3)
    ema = ParamEMA(opt, beta=0.9999, update_after_step=0, update_every=1, warmup=True)
    never = 1 << 30                    # update_every far beyond the steps taken: every step is one the schedule leaves out

    def setup(name):
        if name == "plain":
            opt.ema = None
        else:
            opt.ema = ema
            ema.update_every = 1 if name == "ema_update" else never

    names = ("plain", "ema_update", "ema_skip")
    for name in names:                 # warm-up: every variant's kernels loaded and run
        setup(name)
        for _ in range(2):
            opt.step()
    torch.cuda.synchronize()
    times = {k: [] for k in names}
    for _ in range(args.rounds):
        for name in names:
            setup(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                opt.step()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
    bytes_per = {"plain": 32, "ema_update": 40, "ema_skip": 32}
    out = {"what": f"FusedAdamW.step (clip 0.7 + AdamW) over {n} float32 parameters, with and without an attached ParamEMA",
           "n_params": n, "reps": args.reps, "rounds": args.rounds}
    for name in names:
        ms = statistics.median(times[name])
        r = {"ms": round(ms, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
             "bytes_per_param": bytes_per[name], "achieved_GBps": round(bytes_per[name] * n / (ms * 1e-3) / 1e9, 1)}
        if name == "ema_update":
            r["achieved_GBps_at_32B"] = round(32 * n / (ms * 1e-3) / 1e9, 1)
        out[name] = r
    ratio = out["ema_update"]["achieved_GBps"] / out["plain"]["achieved_GBps"]
    out["ema_update_vs_plain_GBps"] = round(ratio, 4)
    out["target_within_10pct"] = bool(ratio >= 0.9)
    out["ema_update_extra_ms"] = round(out["ema_update"]["ms"] - out["plain"]["ms"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
