"""Time the loudness meter and the gain behind it (csrc/loudness.hip) at the two shapes a user runs, next to the stage they follow --
``EncodecHIP.decode_latents`` of the same length, bf16 SEANet, synthetic weights -- and print one JSON line.

  meter        jen1_kweight_energy (four launches: chunk end states, carry, chunk energies, hop sums) + jen1_loudness_gate
  meter_apply  the same + jen1_gain_apply (strategy "loudness", limit "clip"), i.e. ``normalize_audio`` without its allocations
  decode       ``decode_latents(z, segment_frames, length)``: the yardstick
Shapes: [8, 2, 480 000] (10 s, B = 8) and [1, 2, 3 600 000] (75 s).  Every variant is warmed up, then timed with device events over
``--reps`` calls per region and ``--rounds`` regions (median, min, max of the per-call time).  ``bytes`` is what the passes read and write,
counted from the shapes.  Per-launch times come from a kernel trace of this script in a run of its own (``--no-decode`` keeps the trace
to the loudness kernels):

    python tools/loudness_bench.py [--reps 50] [--rounds 7] [--warmup 5] [--no-decode]
"""
import argparse
import ctypes
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

SHAPES = ((8, 2, 480000), (1, 2, 3600000))
SR = 48000


def pass_bytes(lib, rows, C, n, hop):
    """bytes each launch reads + writes, from the shapes (float32 samples, float64 everything else)"""
    N = lib.jen1_kweight_chunk(hop)
    nch, lines, H = -(-n // N), rows * C, n // hop
    x = 4 * lines * n
    return {"chunk_states": x + 8 * lines * nch * 6, "carry": 8 * lines * nch * (4 + 4 + 2 + 4), "chunk_energies": x + 8 * lines * nch * 5,
            "hop_sums": 8 * lines * (nch + H), "gate": 8 * lines * H * 2, "gain_apply": 2 * x}


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loudness_bench needs a GPU"
    from jen1_amd import audio, lib as L
    from jen1_amd.init_fill import fill_normal
    lib = L.load()
    hop = audio.hop_samples(SR)
    sos = audio.k_weighting(SR)
    coef = (ctypes.c_double * 10)(*sos[0, [0, 1, 2, 4, 5]], *sos[1, [0, 1, 2, 4, 5]])
    stream = torch.cuda.current_stream().cuda_stream
    model = None
    if not args.no_decode:
        from encodec_common import dec_params                              # the synthetic weights of the test suite
        from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP
        dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in dec_params().items()}, compute_dtype="bf16")
        tables = np.stack([fill_normal(f"encodec.quantizer.layers.{i}.codebook.embed", (1024, 128), 1234) for i in range(16)])
        model = EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(tables)))
    out = {"what": "BS.1770 meter (K-weighted hop energies in float64, state carry; gate) and gain + clip limiter at 48 kHz; decode = "
                   "EncodecHIP.decode_latents of the same length (bf16, synthetic weights)", "reps_per_region": args.reps, "regions": args.rounds,
           "chunk_samples": int(lib.jen1_kweight_chunk(hop)), "shapes": {}}
    for rows, C, n in SHAPES:
        x = (torch.rand((rows, C, n), generator=torch.Generator().manual_seed(3)) - 0.5).cuda()
        y = torch.empty_like(x)
        H = n // hop
        nbytes = int(lib.jen1_kweight_energy_workspace_bytes(rows, C, n, hop))
        work = torch.empty((nbytes // 8,), dtype=torch.float64, device="cuda")
        e = torch.empty((rows, C, H), dtype=torch.float64, device="cuda")
        stats = torch.empty((rows, 2), dtype=torch.float64, device="cuda")
        lufs = torch.empty((rows,), dtype=torch.float64, device="cuda")
        gain = torch.empty((rows,), dtype=torch.float32, device="cuda")
        target = torch.full((rows,), -14.0, dtype=torch.float64, device="cuda")

        def meter():
            L.check(lib.jen1_kweight_energy(x.data_ptr(), e.data_ptr(), stats.data_ptr(), coef, rows, C, n, hop, work.data_ptr(), nbytes, stream))
            L.check(lib.jen1_loudness_gate(e.data_ptr(), lufs.data_ptr(), rows, C, H, hop, stream))

        def meter_apply():
            meter()
            L.check(lib.jen1_gain_apply(x.data_ptr(), y.data_ptr(), gain.data_ptr(), lufs.data_ptr(), stats.data_ptr(), target.data_ptr(), rows, C, n,
                                        L.GAIN_LOUDNESS, L.LIMIT_CLIP, 0.0, 2e-3, stream))

        variants = {"meter": meter, "meter_apply": meter_apply}
        if model is not None:
            counts = model.segment_frames(n)
            z = torch.from_numpy(fill_normal("loudness_bench.emb", (rows, 128, sum(counts)), 4)).cuda()
            variants["decode"] = lambda: model.decode_latents(z, counts, length=n)
        res = {"workspace_bytes": nbytes, "bytes": pass_bytes(lib, rows, C, n, hop)}
        for name, fn in variants.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            heavy = name == "decode"
            res[name] = timed(fn, max(1, args.reps // 10) if heavy else args.reps, args.rounds)
        res["lufs"] = [round(float(v), 4) for v in lufs.cpu()]
        if model is not None:
            res["meter_over_decode"] = round(res["meter"]["ms_median"] / res["decode"]["ms_median"], 5)
            res["meter_apply_over_decode"] = round(res["meter_apply"]["ms_median"] / res["decode"]["ms_median"], 5)
        out["shapes"][f"{rows}x{C}x{n}"] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
