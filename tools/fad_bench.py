"""Time the VGGish embedder of the Frechet Audio Distance (jen1_amd/fad.py, csrc/vggish.hip) at full width with synthetic weights, part
by part, next to the same network as a float32 ``torch`` chain on the same GPU, and write profiles/fad_bench.txt.

  front      convert_audio to 16 kHz mono + jen1_mel (linear mel of every frame)
  convs      jen1_vggish_conv1 (reads the mel buffer, applies the log) + the five jen1_conv3x3 launches
  linears    three jen1_train_gemm launches + two jen1_vggish_relu
  embed      VGGishHIP.embed: all of the above, in passes of fad.CHUNK examples
  torch      ``conv2d`` / ``relu`` / ``max_pool2d`` / ``linear`` in float32 (NCHW) on the examples ``vggish_examples`` gives: the yardstick
             for convs + linears (there is no earlier path in this package to compare against); torch_convs is its ``features`` half
Workloads: 8 and 64 clips of 10 s of 48 kHz stereo (80 and 640 examples).  Every variant is warmed up, then timed with device events
over ``--reps`` calls per region and ``--rounds`` regions (median, min, max of the per-call time), the variants alternating region by
region.  FLOP are counted from the shapes (2 per multiply-add of the five matrix-core convolutions and the linears) and set against the
157 TFLOP/s float32 matrix peak of the MI355X.  The script is its own process:

    python tools/fad_bench.py [--reps 5] [--rounds 5] [--warmup 2] [--out profiles/fad_bench.txt]
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

import torch  # noqa: E402

PEAK_F32_MATRIX = 157e12
SR = 48000
WORKLOADS = ((8, 10.0), (64, 10.0))


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(variants, reps, rounds, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(region(fn, reps))
    return {k: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)} for k, v in times.items()}


def matrix_flop(net) -> dict:
    """per example: the five matrix-core convolutions and the three linears"""
    from jen1_amd import fad as F
    conv = sum(2 * 9 * net.channels[i - 1] * net.channels[i] * F.GRID[i][0] * F.GRID[i][1] for i in range(1, 6))
    lin = sum(2 * int(w.shape[0]) * int(w.shape[1]) for w in net.lin_w)
    return {"convs": conv, "linears": lin}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fad_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fad_bench needs a GPU"
    import fad_common as O                          # the torch.nn model of the test suite: synthetic weights
    from jen1_amd import fad as F
    from jen1_amd import lib as L
    model = O.VGGishModel(**O.FULL, seed=0)
    net = F.VGGishHIP.from_module(model)
    tmodel = model.cuda().float()
    rt = net._runtime()
    flop = matrix_flop(net)
    lines = []
    for rows, seconds in WORKLOADS:
        g = torch.Generator().manual_seed(5)
        wav = (0.2 * torch.randn((rows, 2, int(seconds * SR)), generator=g)).cuda()
        mel, counts, frames = F._mel(wav, SR, None, "fad_bench")
        N = sum(counts)
        host = (L.c_int * len(counts))(*counts)
        n = min(N, F.CHUNK)                         # convs / linears / torch are timed on one pass and scaled to N
        ex, _ = F.vggish_examples(wav, SR)
        out_t = torch.empty((net.dim, n), dtype=torch.float32, device="cuda")

        def first(y):
            L.check(rt.lib.jen1_vggish_conv1(mel.data_ptr(), host, len(counts), frames, 0, 0, n, net.conv_w[0].data_ptr(),
                                             net.conv_b[0].data_ptr(), y.data_ptr(), net.channels[0], rt.stream()), "jen1_vggish_conv1")

        flat = net._convs(first, n)

        def torch_convs():
            with torch.no_grad():
                return tmodel.features(ex[:n, None])

        def torch_chain():
            with torch.no_grad():
                return tmodel(ex[:n])

        variants = {"front": lambda: F._mel(wav, SR, None, "fad_bench"),
                    "convs": lambda: net._convs(first, n),
                    "linears": lambda: net._linears(flat, out_t, 0),
                    "embed": lambda: net.embed(wav, SR),
                    "torch_convs": torch_convs, "torch": torch_chain}
        res = alternate(variants, args.reps, args.rounds, args.warmup)
        got = net.forward(ex[:n])
        agree = float((got - torch_chain()).abs().max() / got.abs().max())
        scale = N / n
        tf = lambda name, f: round(f * n / (res[name]["ms_median"] * 1e-3) / 1e12, 2)
        out = {"what": f"VGGish embedder, full width, {rows} clips of {seconds:g} s of 48 kHz stereo = {N} examples", "examples": N,
               "examples_timed_per_pass": n, "reps_per_region": args.reps, "regions": args.rounds, **res,
               "matrix_flop_per_example": flop,
               "tflops": {"convs": tf("convs", flop["convs"]), "linears": tf("linears", flop["linears"]),
                          "torch_convs": tf("torch_convs", flop["convs"]), "torch": tf("torch", flop["convs"] + flop["linears"])},
               "share_of_f32_matrix_peak": {"convs": round(tf("convs", flop["convs"]) * 1e12 / PEAK_F32_MATRIX, 4),
                                            "linears": round(tf("linears", flop["linears"]) * 1e12 / PEAK_F32_MATRIX, 4)},
               "network_over_torch": round((res["convs"]["ms_median"] + res["linears"]["ms_median"]) / res["torch"]["ms_median"], 4),
               "convs_over_torch_convs": round(res["convs"]["ms_median"] / res["torch_convs"]["ms_median"], 4),
               "passes_in_embed": round(scale, 3), "forward_vs_torch_max_rel_diff": agree}
        print(json.dumps(out), flush=True)
        lines.append(json.dumps(out))
    props = torch.cuda.get_device_properties(0)
    head = (f"VGGish embedder of the Frechet Audio Distance (csrc/vggish.hip, jen1_amd/fad.py) next to a float32 torch chain on the same GPU\n"
            f"python tools/fad_bench.py --reps {args.reps} --rounds {args.rounds} --warmup {args.warmup}: {props.name}, torch {torch.__version__}, "
            f"{time.strftime('%Y-%m-%d')}; device events, medians over regions, variants alternating; the tool's output, verbatim:\n\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
