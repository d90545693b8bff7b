"""Time the codec's two ways out of and into the latents at the bench workload (B = 8 clips of 10 s at 48 kHz, bf16 SEANet, synthetic
weights), and print one JSON line.

Two pairs of variants, each pair timed in alternation in one process (round robin, ``--rounds`` regions of ``--calls`` calls per variant
after a warm-up; a region is bracketed by device synchronisation on both sides; median and spread per variant):
  decode_whole     ``audio_encoder.decoder(z)`` on the 8 x 128 x 1515 latents in one piece (what generation.py:130 does): 484 800 samples
  decode_segments  ``decode_latents(z, segment_frames, length=480000)``: 11 segments per clip as batch rows, LSTM over 150 steps instead of
                   1515, linear overlap-add: 480 000 samples
  encode_loop      ``EncodecHIP.encode`` with one encoder pass per segment (JEN1_ENCODE_BATCHED=0)
  encode_batched   the same with equal-length segments as batch rows of one pass, scales and cut by the segment kernels
``encode_batched_faster`` is true when median(loop) - median(batched) exceeds the spread (max - min) of the loop regions.

    python tools/segment_codec_bench.py [--calls 3] [--rounds 8] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "segment_codec_bench needs a GPU"
    from encodec_common import dec_params, enc_params                     # the synthetic weights of the test suite
    from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    from jen1_amd.init_fill import fill_normal
    B, n = args.batch, args.seconds * 48000
    dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in dec_params().items()}, compute_dtype="bf16")
    enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in enc_params().items()}, compute_dtype="bf16")
    tables = np.stack([fill_normal(f"encodec.quantizer.layers.{i}.codebook.embed", (1024, 128), 1234) for i in range(16)])
    model = EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(tables)), encoder=enc)
    counts = model.segment_frames(n)
    z = torch.from_numpy(fill_normal("segment_codec_bench.emb", (B, 128, sum(counts)), 4)).cuda()
    audio = (torch.from_numpy(fill_normal("segment_codec_bench.audio", (B, 2, n), 5)) * 0.2).cuda()

    def encode(batched):
        model.encode_batched = batched
        return model.encode(audio)

    variants = {
        "decode_whole": lambda: model.decoder(z),
        "decode_segments": lambda: model.decode_latents(z, counts, length=n),
        "encode_loop": lambda: encode(False),
        "encode_batched": lambda: encode(True),
    }
    shapes = {}
    for name, fn in variants.items():
        for _ in range(args.warmup):
            out = fn()
        shapes[name] = list(out.shape) if isinstance(out, torch.Tensor) else [len(out), sum(int(c.shape[-1]) for c, _ in out)]
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for pair in (("decode_whole", "decode_segments"), ("encode_loop", "encode_batched")):
        for _ in range(args.rounds):
            for name in pair:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    variants[name]()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.calls * 1e3)
    # same codes either way (the A/B computes the same thing): agreement rate of the batched form with the loop
    a, b = encode(False), encode(True)
    agree = float(np.mean([float((ca == cb).float().mean()) for (ca, _), (cb, _) in zip(a, b)]))
    out = {"what": f"Encodec 48 kHz SEANet bf16, synthetic weights, B={B} x {args.seconds} s: decoder on all {sum(counts)} frames at once / per segment "
                   f"with overlap-add; encode as a loop over {len(counts)} segments / segment-batched", "calls_per_region": args.calls,
           "regions": args.rounds, "segment_frames": counts, "shapes": shapes, "encode_code_agreement": round(agree, 5)}
    for name, v in times.items():
        out[name] = {"ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3),
                     "spread_ms": round(max(v) - min(v), 3)}
    out["decode_segments_over_whole"] = round(out["decode_segments"]["ms_median"] / out["decode_whole"]["ms_median"], 3)
    out["encode_batched_over_loop"] = round(out["encode_batched"]["ms_median"] / out["encode_loop"]["ms_median"], 3)
    out["encode_batched_faster"] = bool(out["encode_loop"]["ms_median"] - out["encode_batched"]["ms_median"] > out["encode_loop"]["spread_ms"])
    out["decode_segments_faster"] = bool(out["decode_whole"]["ms_median"] - out["decode_segments"]["ms_median"] > out["decode_whole"]["spread_ms"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
