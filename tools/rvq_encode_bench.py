"""Time the fused residual search against the path it replaces, and print one JSON line per shape.

  quantize   ``ResidualVectorQuantizerHIP.quantize`` (codes + latents): one jen1_rvq_encode launch
  parts      ``quantizer.encode`` then ``quantizer.decode``: per codebook a float32 GEMM, torch.argmax, a gather and a subtract, then
             jen1_rvq_decode
at 1 x 150, 1 x 1515 and 8 x 1515 frames (n_q = 16, bins = 1024), and ``EncodecHIP.encode_latents`` against ``Jen1.get_emb_segments`` for
8 clips of 10 s (bf16 SEANet encoder, synthetic weights).

Method: both variants warmed, then timed in alternation in one process; a region is ``calls`` calls between two device events, with
``calls`` chosen so that a region is at least ``--region-ms`` of device time, ``--rounds`` regions per variant; median and (min, max) per
variant.  ``fused_faster`` is true when median(parts) - median(quantize) exceeds the spread (max - min) of both.  The kernel's share of
the f32 matrix peak is 2 frames bins D n_q FLOP over the fused call's time over 157.3 TFLOP/s (an upper bound of the kernel's own time:
take that from a separate ``rocprofv3 --kernel-trace --stats`` run of this tool with ``--rounds 1``).

    python tools/rvq_encode_bench.py [--rounds 7] [--region-ms 80] [--no-codec]
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

F32_MATRIX_PEAK = 157.3e12


def region_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(variants, rounds, target_ms):
    """{name: fn} -> {name: {ms_median, ms_min, ms_max, calls}}: warm-up, calls per region from a first estimate, round robin"""
    calls = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(1, int(np.ceil(target_ms / max(region_ms(fn, 3), 1e-3))))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(region_ms(fn, calls[name]))
    return {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "calls_per_region": calls[k]}
            for k, v in times.items()}


def verdict(res, new, old):
    spread = max(res[new]["ms_max"] - res[new]["ms_min"], res[old]["ms_max"] - res[old]["ms_min"])
    return {"speedup": round(res[old]["ms_median"] / res[new]["ms_median"], 3),
            "fused_faster": bool(res[old]["ms_median"] - res[new]["ms_median"] > spread)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--region-ms", type=float, default=80.0)
    ap.add_argument("--no-codec", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rvq_encode_bench needs a GPU"
    from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    from jen1_amd.init_fill import fill_normal
    tables = np.stack([fill_normal(f"encodec.quantizer.layers.{i}.codebook.embed", (1024, 128), 1234) for i in range(16)])
    quant = ResidualVectorQuantizerHIP(torch.from_numpy(tables))
    for B, T in ((1, 150), (1, 1515), (8, 1515)):
        emb = torch.from_numpy(fill_normal(f"rvq_encode_bench.emb.{B}x{T}", (B, 128, T), 3)).cuda()
        res = alternate({"quantize": lambda: quant.quantize(emb), "parts": lambda: quant.decode(quant.encode(emb))}, args.rounds, args.region_ms)
        codes, z = quant.quantize(emb)
        agree = float((codes == quant.encode(emb)).all(dim=0).float().mean())
        flop = 2.0 * B * T * 1024 * 128 * 16
        out = {"what": f"RVQ search + decode, n_q=16 bins=1024 D=128, {B} x {T} frames", **res, **verdict(res, "quantize", "parts"),
               "frames_with_equal_codes": round(agree, 5), "gflop": round(flop / 1e9, 3),
               "quantize_share_of_f32_matrix_peak": round(flop / (res["quantize"]["ms_median"] * 1e-3) / F32_MATRIX_PEAK, 4)}
        print(json.dumps(out), flush=True)
    if args.no_codec:
        return
    from encodec_common import dec_params, enc_params                     # the synthetic weights of the test suite
    from jen1_amd.generation import Jen1
    dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in dec_params().items()}, compute_dtype="bf16")
    enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in enc_params().items()}, compute_dtype="bf16")
    model = EncodecHIP(dec, quant, encoder=enc)
    j = Jen1(None, device="cuda", audio_encoder=model, conditioner=lambda md, device: None)
    audio = (torch.from_numpy(fill_normal("rvq_encode_bench.audio", (8, 2, 480000), 5)) * 0.2).cuda()
    res = alternate({"encode_latents": lambda: model.encode_latents(audio), "get_emb_segments": lambda: j.get_emb_segments(audio)},
                    args.rounds, args.region_ms)
    print(json.dumps({"what": "waveform -> latents, 8 clips of 10 s at 48 kHz, bf16 SEANet encoder, synthetic weights", **res,
                      **verdict(res, "encode_latents", "get_emb_segments")}), flush=True)


if __name__ == "__main__":
    main()
