#!/usr/bin/env python
"""Time ``jen1_amd.analysis.analyze`` (four launches: onset flux + chromagram, autocorrelation, tempo, key) next to a float32 torch chain on the same GPU
(``torch.stft``, two matmuls, the flux, an FFT autocorrelation and the key correlations) for 8 x 10 s and 1 x 300 s of 48 kHz mono.

    python tools/analysis_bench.py [--reps 30] [--warmup 3] [--out profiles/analysis_bench.txt]

Per-call device-event times; the verdicts of both chains are printed next to each other."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

SR, N_FFT, HOP, N_MELS = 48000, 2048, 512, 128


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4)}


def torch_chain(x, mel_w, chroma_w, profiles, lo, hi):
    win = torch.hann_window(N_FFT, device=x.device)
    S = torch.stft(x, N_FFT, HOP, window=win, center=True, pad_mode="reflect", return_complex=True).abs()
    Y = torch.log1p(mel_w @ S)
    onset = torch.zeros((x.shape[0], S.shape[2]), device=x.device)
    onset[:, 1:] = torch.clamp(Y[:, :, 1:] - Y[:, :, :-1], min=0).mean(dim=1)
    prof = (chroma_w @ (S * S)).sum(dim=2)
    u = onset - onset.mean(dim=1, keepdim=True)
    F = u.shape[1]
    acf = torch.fft.irfft(torch.fft.rfft(u, 2 * F).abs() ** 2, 2 * F)[:, :F]
    lags = torch.arange(lo, hi + 1, device=x.device)
    s = acf[:, lo:hi + 1] * torch.exp(-0.5 * torch.log2(60.0 * (SR / HOP) / lags / 120.0) ** 2)
    tempo = 60.0 * (SR / HOP) / lags[s.argmax(dim=1)]
    p = prof - prof.mean(dim=1, keepdim=True)
    q = profiles - profiles.mean(dim=1, keepdim=True)
    corr = (p @ q.T) / (p.norm(dim=1, keepdim=True) * q.norm(dim=1)[None, :])
    return tempo, corr.argmax(dim=1)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analysis_bench.txt"))
    args = ap.parse_args(argv)
    import analysis_common as A
    from jen1_amd import analysis, spectral
    dev = torch.device("cuda")
    mel_w = torch.from_numpy(spectral.mel_filterbank(SR, N_FFT, N_MELS).astype(np.float32)).to(dev)
    chroma_w = torch.from_numpy(analysis.chroma_filterbank(SR, N_FFT).astype(np.float32)).to(dev)
    profiles = torch.from_numpy(analysis.key_profiles().astype(np.float32)).to(dev)
    lo, hi = A.lag_range(SR / HOP)
    click, scale = A.click_track(120, 10.0), A.passage("C", 10.0)
    mix = (0.5 * click + scale).astype(np.float32)
    result = {"what": "analysis.analyze (hip: four launches) against a float32 torch chain on the same GPU (torch.stft, two matmuls, flux, FFT "
                      "autocorrelation, key correlations); 48 kHz mono; per-call device-event times", "reps": args.reps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "shapes": {}}
    for rows, seconds in ((8, 10), (1, 300)):
        x = torch.from_numpy(np.tile(mix, (rows, seconds // 10))).to(dev).contiguous()
        hip = timed(lambda: analysis.analyze(x, SR, device=dev), args.reps, args.warmup)
        tch = timed(lambda: torch_chain(x, mel_w, chroma_w, profiles, lo, hi), args.reps, args.warmup)
        got = analysis.analyze(x, SR, device=dev)
        t_tempo, t_key = torch_chain(x, mel_w, chroma_w, profiles, lo, hi)
        result["shapes"][f"{rows}x{seconds}s"] = {
            "hip": hip, "torch": tch, "hip_over_torch": round(hip["ms_median"] / tch["ms_median"], 4),
            "tempo_hip": [round(float(v), 3) for v in got["tempo"].cpu()], "tempo_torch": [round(float(v), 3) for v in t_tempo.cpu()],
            "key_hip": [int(v) for v in got["key"].cpu()], "key_torch": [int(v) for v in t_key.cpu()]}
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
