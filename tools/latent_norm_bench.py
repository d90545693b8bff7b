"""Time the two kernels of the latent whitening (csrc/latent_norm.hip) at the shapes a user runs, next to the torch chain each replaces
and to the stage in front of them, and print one JSON line per shape.

  moments        jen1_latent_moments (products on the f64 matrix instruction, one partial per 128 frames; the fixed-order reduce)
  moments_torch  ``x = z.double(); n, x.sum((0, 2)), einsum("bct,bdt->cd", x, x)`` added to a state
  affine         jen1_latent_affine, forward (A = W, pre = mean), out of place
  affine_torch   ``torch.matmul(W, z - mean[:, None])`` (float32)
  encode         ``EncodecHIP.encode_latents`` of the audio those latents come from (bf16 SEANet, synthetic weights): the yardstick
Shapes: 8 x 128 x 1515 (10 s clips, B = 8) and 1 x 128 x F, F the frames of the 75 s canvas.  Every variant is warmed up, then timed with
device events over ``--reps`` calls per region and ``--rounds`` regions (median, min, max of the per-call time); the variants of a shape
alternate region by region.  ``bytes`` and ``flop`` are counted from the shapes.  The script is its own process:

    python tools/latent_norm_bench.py [--reps 50] [--rounds 7] [--warmup 5] [--no-encode]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

C = 128
SR = 48000
CLIPS = ((8, 10.0), (1, 75.0))          # (rows, seconds)


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(variants, reps, rounds, warmup):
    for fn, _ in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, div) in variants.items():
            times[k].append(region(fn, max(1, reps // div)))
    return {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in times.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-encode", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "latent_norm_bench needs a GPU"
    from jen1_amd import lib as L
    from jen1_amd.encodec import segment_frame_counts
    from jen1_amd.init_fill import fill_normal
    from jen1_amd.normalizer import Normalizer, state_words
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    model = None
    if not args.no_encode:
        from encodec_common import dec_params, enc_params                     # the synthetic weights of the test suite
        from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
        tables = np.stack([fill_normal(f"encodec.quantizer.layers.{i}.codebook.embed", (1024, 128), 1234) for i in range(16)])
        dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in dec_params().items()}, compute_dtype="bf16")
        enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in enc_params().items()}, compute_dtype="bf16")
        model = EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(tables)), encoder=enc)
    for rows, seconds in CLIPS:
        n = int(seconds * SR)
        T = sum(segment_frame_counts(n, SR, SR - SR // 100))
        g = torch.Generator().manual_seed(3)
        z = (torch.randn((rows, C, T), generator=g) + torch.randn((1, C, 1), generator=g)).cuda()
        norm = Normalizer(C).update(z).finalize("zca")
        W, mean = norm.weight, norm.mean
        state = torch.zeros(state_words(C), dtype=torch.float64, device="cuda")
        tstate = torch.zeros_like(state)
        nbytes = int(lib.jen1_latent_moments_workspace(rows, C, T))
        work = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
        y = torch.empty_like(z)

        def moments():
            L.check(lib.jen1_latent_moments(z.data_ptr(), None, state.data_ptr(), work.data_ptr(), nbytes, rows, C, T, stream))

        def moments_torch():
            x = z.double()
            tstate[0] += x.shape[0] * x.shape[2]
            tstate[1:1 + C] += x.sum(dim=(0, 2))
            tstate[1 + C:] += torch.einsum("bct,bdt->cd", x, x).reshape(-1)

        def affine():
            L.check(lib.jen1_latent_affine(z.data_ptr(), y.data_ptr(), W.data_ptr(), mean.data_ptr(), None, rows, C, T, stream))

        def affine_torch():
            return torch.matmul(W, z - mean[:, None])

        variants = {"moments": (moments, 1), "moments_torch": (moments_torch, 1), "affine": (affine, 1), "affine_torch": (affine_torch, 1)}
        if model is not None:
            audio = (torch.randn((rows, 2, n), generator=g) * 0.2).cuda()
            variants["encode"] = (lambda: model.encode_latents(audio), 10)
        res = alternate(variants, args.reps, args.rounds, args.warmup)
        agree = float((affine_torch() - y).abs().max() / y.abs().max())
        out = {"what": f"latent whitening, {rows} x {C} x {T} frames ({rows} clips of {seconds:g} s)", "reps_per_region": args.reps,
               "regions": args.rounds, **res,
               "flop": {"moments": 2 * C * C * rows * T, "affine": 2 * C * C * rows * T},
               "bytes": {"moments": 4 * rows * C * T + 2 * nbytes, "affine": 8 * rows * C * T + 4 * C * C}, "workspace_bytes": nbytes,
               "moments_over_torch": round(res["moments"]["ms_median"] / res["moments_torch"]["ms_median"], 4),
               "affine_over_torch": round(res["affine"]["ms_median"] / res["affine_torch"]["ms_median"], 4),
               "affine_vs_torch_max_rel_diff": agree}
        if model is not None:
            out["moments_over_encode"] = round(res["moments"]["ms_median"] / res["encode"]["ms_median"], 5)
            out["affine_over_encode"] = round(res["affine"]["ms_median"] / res["encode"]["ms_median"], 5)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
