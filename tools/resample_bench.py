"""Time the resampler / channel converter kernel (csrc/audio.hip: jen1_resample, through jen1_amd.audio.convert_audio) against what it
replaces, torch's dense formulation of the same filter on the same GPU in the same process, and print one JSON line per case.

Cases (``--batch`` 8 clips of ``--seconds`` 30 s each, float32, already on the device):
  stereo 44100 -> 48000      stereo 96000 -> 48000      mono 24000 -> stereo 48000
Variants, timed in alternation (round robin, ``--rounds`` regions of ``--calls`` calls each per variant, after a warm-up; a region is
bracketed by device synchronisation on both sides; median and spread per variant):
  hip     jen1_resample: one launch, the compact [n, W] table, channel rule while staging
  dense   the channel rule of encodec.utils.convert_audio, then F.pad + F.conv1d(stride = o) with the dense [n, 1, K] table + transpose /
          reshape / slice -- the operations torchaudio.functional.resample executes
Reported per case: microseconds per call, and for ``hip`` the fraction of 8.0 TB/s the ALGORITHMIC bytes (input read once + output written
once) reach.  Gate: median(hip) <= median(dense) + spread(hip), spread = max - min over the hip regions.  Before timing, the two outputs
are compared (max abs difference), so a faster-but-different kernel cannot pass unnoticed.

    python tools/resample_bench.py [--batch 8] [--seconds 30] [--calls 10] [--rounds 8] [--warmup 3]
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

HBM_BYTES_PER_S = 8.0e12


def dense_table(audio, sr, target):
    """the dense [n, K] float32 table, scattered back from the compact one (tests/test_audio_host.py checks that this is exact)"""
    o, n, w, taps, first = audio.resample_table(sr, target)
    h = np.zeros((n, 2 * w + o), np.float32)
    for p in range(n):
        h[p, first[p]:first[p] + taps.shape[1]] = taps[p]
    return o, n, w, torch.from_numpy(h).cuda()


def dense_convert(x, c_out, o, n, w, h):
    """encodec.utils.convert_audio + torchaudio.functional.resample in torch ops"""
    B, c_in, L = x.shape
    if c_out == 1 and c_in == 2:
        x = x.mean(dim=1, keepdim=True)
    elif c_out == 2 and c_in == 1:
        x = x.expand(B, 2, L)
    n_out = -(-n * L // o)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x.reshape(B * c_out, 1, L), (w, w + o)), h[:, None, :], stride=o)
    return y.transpose(1, 2).reshape(B, c_out, -1)[..., :n_out]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resample_bench needs a GPU"
    from jen1_amd import audio
    g = torch.Generator().manual_seed(0)
    for sr, target, c_in, c_out in ((44100, 48000, 2, 2), (96000, 48000, 2, 2), (24000, 48000, 1, 2)):
        L = int(args.seconds * sr)
        x = (torch.rand((args.batch, c_in, L), generator=g) * 2 - 1).cuda()
        o, n, w, h = dense_table(audio, sr, target)
        variants = {"hip": lambda: audio.convert_audio(x, sr, target, c_out), "dense": lambda: dense_convert(x, c_out, o, n, w, h)}
        a, b = variants["hip"](), variants["dense"]()
        assert a.shape == b.shape, (a.shape, b.shape)
        diff = float((a - b).abs().max())
        bytes_alg = 4 * (x.numel() + a.numel())
        del a, b
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.calls * 1e6)
        out = {"what": f"convert_audio, B={args.batch}, {args.seconds:g} s, {c_in} -> {c_out} channels, {sr} -> {target} Hz (o={o}, n={n}, w={w}, "
                       f"W={audio.resample_table(sr, target)[3].shape[1]}, K={2 * w + o})",
               "calls_per_region": args.calls, "regions": args.rounds, "algorithmic_bytes": bytes_alg, "max_abs_diff_hip_vs_dense": diff}
        for name, v in times.items():
            out[name] = {"us_per_call_median": round(statistics.median(v), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                         "spread_us": round(max(v) - min(v), 1)}
        med = out["hip"]["us_per_call_median"]
        out["hip"]["fraction_of_8TBps_algorithmic"] = round(bytes_alg / (med * 1e-6) / HBM_BYTES_PER_S, 4)
        out["dense_over_hip"] = round(out["dense"]["us_per_call_median"] / med, 2)
        out["hip_not_slower"] = bool(med <= out["dense"]["us_per_call_median"] + out["hip"]["spread_us"])
        print(json.dumps(out), flush=True)
        del x


if __name__ == "__main__":
    main()
