#!/usr/bin/env python
"""Time the four steps of ``jen1_amd.effects.stretch_and_shift`` (``spectral.stft``, ``spectral.phase_vocoder``, ``spectral.istft``,
``audio.resample``) and the whole call for a training batch of 8 x 2 x 10 s at 48 kHz, next to ``encode_latents`` of the same batch -- the
step the augmentation sits in front of (a synthetic-weight float32 codec, as the dataset tests build it).

    python tools/vocoder_bench.py [--reps 20] [--warmup 3] [--out profiles/vocoder_bench.txt]

Per-call device-event times.  Nothing is gated on them."""
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

SR, N_FFT, HOP, BATCH, CHANNELS, SECONDS = 48000, 2048, 512, 8, 2, 10


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


def codec():
    import encodec_common as EC
    import rvq_encode_common as RC
    from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in EC.dec_params().items()}, compute_dtype="f32")
    enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in EC.enc_params().items()}, compute_dtype="f32")
    return EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(RC.golden_tables(16))), encoder=enc)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_bench.txt"))
    args = ap.parse_args(argv)
    import analysis_common as A
    from jen1_amd import audio, effects, spectral
    dev = torch.device("cuda")
    mix = (0.5 * A.click_track(120, float(SECONDS)) + A.passage("C", float(SECONDS))).astype(np.float32)
    x = torch.from_numpy(np.tile(mix, (BATCH, CHANNELS, 1))).to(dev).contiguous()
    n = int(x.shape[-1])
    rate, semitones = 1.1, 2
    f = effects.semitone_ratio(semitones)
    step = rate * f.denominator / f.numerator
    spec = spectral.stft(x, N_FFT, HOP, device=dev)
    moved = spectral.phase_vocoder(spec, step, HOP, device=dev)
    y = spectral.istft(moved, N_FFT, HOP, length=int(round(n / step)), device=dev)
    result = {"what": f"stretch_and_shift(rate {rate}, {semitones:+d} semitones = {f}) of {BATCH} x {CHANNELS} x {SECONDS} s at {SR} Hz, n_fft {N_FFT}, hop {HOP}: "
                      "its four steps and the whole call, next to encode_latents of the same batch (synthetic float32 codec); per-call device-event times",
              "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "frames_in": int(spec.shape[-1]), "frames_out": int(moved.shape[-1]), "samples_before_resample": int(y.shape[-1]),
              "stft": timed(lambda: spectral.stft(x, N_FFT, HOP, device=dev), args.reps, args.warmup),
              "phase_vocoder": timed(lambda: spectral.phase_vocoder(spec, step, HOP, device=dev), args.reps, args.warmup),
              "istft": timed(lambda: spectral.istft(moved, N_FFT, HOP, length=int(round(n / step)), device=dev), args.reps, args.warmup),
              "resample": timed(lambda: audio.resample(y, f.numerator, f.denominator, device=dev), args.reps, args.warmup),
              "stretch_and_shift": timed(lambda: effects.stretch_and_shift(x, SR, rate=rate, semitones=semitones, device=dev), args.reps, args.warmup)}
    ae = codec()
    result["encode_latents"] = timed(lambda: ae.encode_latents(x), max(3, args.reps // 4), 1)
    result["stretch_and_shift_over_encode_latents"] = round(result["stretch_and_shift"]["ms_median"] / result["encode_latents"]["ms_median"], 4)
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
