"""Time the true-peak meter and the look-ahead limiter (csrc/limiter.hip) at the two shapes a user runs, next to the "clip" path of
``normalize_audio`` they replace and the stage all of it follows -- ``EncodecHIP.decode_latents`` of the same length, bf16 SEANet,
synthetic weights -- print one JSON line and write the table of profiles/limiter_bench.txt.

  peak             jen1_true_peak without the envelope (two launches: tiles, rows): ``audio.true_peak``
  envelope         jen1_true_peak with the envelope, as the limiter needs it
  limiter          jen1_limit_true_peak on that envelope (four launches: hold, carry, release, apply)
  limit_true_peak  envelope + limiter: ``audio.limit_true_peak`` without its allocations
  clip             loudness meter + jen1_gain_apply(limit "clip"): ``normalize_audio(limit="clip")`` without its allocations
  truepeak         loudness meter + jen1_gain_apply(limit "none") + envelope + limiter: ``normalize_audio(limit="truepeak")``
  decode           ``decode_latents(z, segment_frames, length)``: the yardstick
Shapes: [8, 2, 480 000] (10 s, B = 8) and [1, 2, 3 600 000] (75 s) at 48 kHz (F = 4), uniform noise in +-2 so that the limiter works on
every sample; ceiling -1 dBTP, look-ahead 1.5 ms (72 samples), release 100 ms.  Every variant is warmed up, then timed with device events
over ``--reps`` calls per region and ``--rounds`` regions (median, min, max of the per-call time).

    python tools/limiter_bench.py [--reps 50] [--rounds 7] [--warmup 5] [--no-decode] [--out profiles/limiter_bench.txt]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((8, 2, 480000), (1, 2, 3600000))
SR = 48000
ORDER = ("peak", "envelope", "limiter", "limit_true_peak", "clip", "truepeak", "decode")


def timed(fn, reps, rounds):
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return {"ms_median": round(statistics.median(out), 4), "ms_min": round(min(out), 4), "ms_max": round(max(out), 4)}


def table(out) -> str:
    lines = ["True-peak meter and look-ahead limiter (csrc/limiter.hip) next to the clip path and the decode in front of them (MI355X, one session,",
             "one machine)", "",
             f"python tools/limiter_bench.py (warm-up, then {out['regions']} regions of {out['reps_per_region']} calls per variant, device events; decode: a tenth of",
             f"the calls; 48 kHz, F = 4, tile {out['tile_samples']} samples, ceiling -1 dBTP, look-ahead {out['lookahead_samples']} samples, release 100 ms):", ""]
    for shape, res in out["shapes"].items():
        lines.append(f"   shape [{shape.replace('x', ', ')}]   true peak in {res['dbtp_in']} dBTP, out {res['dbtp_out']} dBTP")
        for name in ORDER:
            if name in res:
                t = res[name]
                lines.append(f"     {name:<16} {t['ms_median']:8.4f} ms  (regions {t['ms_min']:.4f} - {t['ms_max']:.4f})")
        if "decode" in res:
            lines.append(f"     clip / decode {100 * res['clip']['ms_median'] / res['decode']['ms_median']:.2f} %, truepeak / decode "
                         f"{100 * res['truepeak']['ms_median'] / res['decode']['ms_median']:.2f} %")
    return "\n".join(lines + ["", "raw:", json.dumps(out), ""])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limiter_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "limiter_bench needs a GPU"
    from jen1_amd import audio, lib as L
    from jen1_amd.init_fill import fill_normal
    lib = L.load()
    hop = audio.hop_samples(SR)
    sos = audio.k_weighting(SR)
    coef = (ctypes.c_double * 10)(*sos[0, [0, 1, 2, 4, 5]], *sos[1, [0, 1, 2, 4, 5]])
    F, taps = audio.true_peak_filter(SR)
    tp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    c, A, rho = audio.limiter_plan(SR, -1.0, 1.5, 100.0)
    window = torch.from_numpy(audio.attack_window(A)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    model = None
    if not args.no_decode:
        from encodec_common import dec_params                              # the synthetic weights of the test suite
        from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP
        dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in dec_params().items()}, compute_dtype="bf16")
        tables = np.stack([fill_normal(f"encodec.quantizer.layers.{i}.codebook.embed", (1024, 128), 1234) for i in range(16)])
        model = EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(tables)))
    out = {"what": "BS.1770 true-peak meter (4x polyphase, float64) and look-ahead limiter (hold, release scan, attack window) at 48 kHz; clip = "
                   "loudness meter + gain + clip; decode = EncodecHIP.decode_latents of the same length (bf16, synthetic weights)",
           "reps_per_region": args.reps, "regions": args.rounds, "tile_samples": int(lib.jen1_true_peak_tile()), "lookahead_samples": A, "shapes": {}}
    for rows, C, n in SHAPES:
        x = ((torch.rand((rows, C, n), generator=torch.Generator().manual_seed(3)) - 0.5) * 4.0).cuda()
        y = torch.empty_like(x)
        H = n // hop
        kw_bytes = int(lib.jen1_kweight_energy_workspace_bytes(rows, C, n, hop))
        tp_bytes = int(lib.jen1_true_peak_workspace_bytes(rows, C, n))
        lim_bytes = int(lib.jen1_limiter_workspace_bytes(rows, n, A))
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")
        kw_work, tp_work, lim_work = f64(kw_bytes // 8), f64(tp_bytes // 8), f64(lim_bytes // 8)
        e, stats, lufs, env, peak = f64(rows, C, H), f64(rows, 2), f64(rows), f64(rows, n), f64(rows)
        gain = torch.empty((rows,), dtype=torch.float32, device="cuda")
        target = torch.full((rows,), -14.0, dtype=torch.float64, device="cuda")

        def meter(src, with_env):
            L.check(lib.jen1_true_peak(src.data_ptr(), env.data_ptr() if with_env else None, n, peak.data_ptr(), tp, F, rows, C, n, tp_work.data_ptr(),
                                       tp_bytes, stream))

        def limiter(src):
            L.check(lib.jen1_limit_true_peak(src.data_ptr(), y.data_ptr(), C * n, None, 0, env.data_ptr(), n, window.data_ptr(), rows, C, n, A, c, rho,
                                             lim_work.data_ptr(), lim_bytes, stream))

        def gain_apply(limit):
            L.check(lib.jen1_kweight_energy(x.data_ptr(), e.data_ptr(), stats.data_ptr(), coef, rows, C, n, hop, kw_work.data_ptr(), kw_bytes, stream))
            L.check(lib.jen1_loudness_gate(e.data_ptr(), lufs.data_ptr(), rows, C, H, hop, stream))
            L.check(lib.jen1_gain_apply(x.data_ptr(), y.data_ptr(), gain.data_ptr(), lufs.data_ptr(), stats.data_ptr(), target.data_ptr(), rows, C, n,
                                        L.GAIN_LOUDNESS, limit, 0.0, 2e-3, stream))

        def truepeak():
            gain_apply(L.LIMIT_NONE)
            meter(y, True)
            limiter(y)

        variants = {"peak": lambda: meter(x, False), "envelope": lambda: meter(x, True), "limiter": lambda: limiter(x),
                    "limit_true_peak": lambda: (meter(x, True), limiter(x)), "clip": lambda: gain_apply(L.LIMIT_CLIP), "truepeak": truepeak}
        if model is not None:
            counts = model.segment_frames(n)
            z = torch.from_numpy(fill_normal("loudness_bench.emb", (rows, 128, sum(counts)), 4)).cuda()
            variants["decode"] = lambda: model.decode_latents(z, counts, length=n)
        res = {"workspace_bytes": {"true_peak": tp_bytes, "limiter": lim_bytes}}
        meter(x, True)
        res["dbtp_in"] = round(float(20.0 * torch.log10(peak.max())), 4)
        limiter(x)
        meter(y, False)
        res["dbtp_out"] = round(float(20.0 * torch.log10(peak.max())), 4)
        assert res["dbtp_out"] <= -1.0 + 0.01 and math.isfinite(res["dbtp_in"])
        meter(x, True)
        for name, fn in variants.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            res[name] = timed(fn, max(1, args.reps // 10) if name == "decode" else args.reps, args.rounds)
        out["shapes"][f"{rows}x{C}x{n}"] = res
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(table(out))


if __name__ == "__main__":
    main()
