"""Time the spectral metrics (csrc/spectral.hip through jen1_amd/spectral.py) at the two shapes a user runs -- 8 x 10 s and 1 x 75 s of
stereo at 48 kHz -- and, beside every figure, the ``torch.stft``-based chain that does the same work on the same GPU.

  stft             ``spectral.stft`` at (2048, 512, 2048) and (4096, 480, 2400)        | ``torch.stft`` (reflect, one-sided, complex)
  mel_spectrogram  128 htk bands, power, natural log, at (2048, 512, 2048)             | ``torch.stft`` -> |.|^2 -> dense filterbank matmul -> clamp -> log
  mrstft_distance  RESOLUTIONS_48K, floor 1e-5                                         | per resolution two ``torch.stft``, |.|, the two reductions

Every variant is warmed up, then every call is timed on its own with device events (``--reps`` calls, at least 20): median and min.
``bytes`` is what the algorithm has to move, counted from the shapes (the waveform in, the result out; the distance reads two waveforms
per resolution and writes a few doubles); ``of_peak`` is bytes / median time as a fraction of 8.0 TB/s.  The result is one JSON document,
printed and written to ``--out`` (profiles/spectral_bench.txt).

    python tools/spectral_bench.py [--reps 30] [--warmup 3] [--out profiles/spectral_bench.txt]
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

SHAPES = ((8, 2, 480000), (1, 2, 3600000))
SR = 48000
HBM_BYTES_PER_S = 8.0e12
STFT_RESOLUTIONS = ((2048, 512, 2048), (4096, 480, 2400))
MEL = dict(n_fft=2048, hop=512, n_mels=128, floor=1e-10)
FLOOR = 1e-5


def frames_of(n, hop):
    return 1 + n // hop


def torch_stft(x, n_fft, hop, win, window):
    return torch.stft(x.reshape(-1, x.shape[-1]), n_fft, hop_length=hop, win_length=win, window=window, center=True, pad_mode="reflect",
                      return_complex=True)


def torch_mel(x, fb, window, n_fft, hop, floor):
    return torch.log(torch.clamp(torch.matmul(fb, torch_stft(x, n_fft, hop, n_fft, window).abs() ** 2), min=floor))


def torch_mrstft(x, y, resolutions, windows, floor):
    sc, lm = [], []
    for (n_fft, hop, win), w in zip(resolutions, windows):
        ax, ay = torch_stft(x, n_fft, hop, win, w).abs(), torch_stft(y, n_fft, hop, win, w).abs()
        sc.append(torch.sqrt(((ax - ay) ** 2).sum(dim=(1, 2)) / (ay ** 2).sum(dim=(1, 2))))
        lm.append((torch.log(torch.clamp(ax, min=floor)) - torch.log(torch.clamp(ay, min=floor))).abs().mean(dim=(1, 2)))
    return torch.stack(sc, dim=-1), torch.stack(lm, dim=-1)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms_median": round(statistics.median(out), 4), "ms_min": round(min(out), 4)}


def both(ours, theirs, nbytes, reps, warmup):
    res = {"bytes": int(nbytes), "hip": timed(ours, reps, warmup)}
    try:
        res["torch"] = timed(theirs, reps, warmup)
        res["hip_over_torch"] = round(res["hip"]["ms_median"] / res["torch"]["ms_median"], 4)
    except Exception as e:                                  # a torch build without an FFT library: say so, keep our column
        res["torch"] = {"unavailable": f"{type(e).__name__}: {e}"[:200]}
    res["hip"]["of_peak"] = round(nbytes / (res["hip"]["ms_median"] * 1e-3) / HBM_BYTES_PER_S, 5)
    if "ms_median" in res["torch"]:
        res["torch"]["of_peak"] = round(nbytes / (res["torch"]["ms_median"] * 1e-3) / HBM_BYTES_PER_S, 5)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.txt"))
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 timed repeats"
    assert torch.cuda.is_available(), "spectral_bench needs a GPU"
    from jen1_amd import spectral as S
    out = {"what": "spectral metrics at 48 kHz stereo: hip = csrc/spectral.hip through jen1_amd.spectral, torch = the torch.stft-based chain on the "
                   "same GPU; per-call device-event times; bytes = waveform in + result out, of_peak = bytes / median / 8.0 TB/s",
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "shapes": {}}
    fb = torch.from_numpy(S.mel_filterbank(SR, MEL["n_fft"], MEL["n_mels"])).float().cuda()
    for B, C, n in SHAPES:
        g = torch.Generator().manual_seed(3)
        x = ((torch.rand((B, C, n), generator=g) - 0.5) * 0.5).cuda()
        y = (x + 0.02 * (torch.rand((B, C, n), generator=g) - 0.5).cuda()).contiguous()
        rows = B * C
        res = {}
        for n_fft, hop, win in STFT_RESOLUTIONS:
            w = torch.hann_window(win, device="cuda")
            nbytes = 4 * rows * n + 8 * rows * (n_fft // 2 + 1) * frames_of(n, hop)
            res[f"stft_{n_fft}_{hop}_{win}"] = both(lambda: S.stft(x, n_fft, hop, win), lambda: torch_stft(x, n_fft, hop, win, w), nbytes, args.reps,
                                                    args.warmup)
        w = torch.hann_window(MEL["n_fft"], device="cuda")
        nbytes = 4 * rows * n + 4 * rows * MEL["n_mels"] * frames_of(n, MEL["hop"])
        res["mel_spectrogram"] = both(lambda: S.mel_spectrogram(x, SR, MEL["n_fft"], MEL["hop"], n_mels=MEL["n_mels"], log="log", floor=MEL["floor"]),
                                      lambda: torch_mel(x, fb, w, MEL["n_fft"], MEL["hop"], MEL["floor"]), nbytes, args.reps, args.warmup)
        ws = [torch.hann_window(r[2], device="cuda") for r in S.RESOLUTIONS_48K]
        nbytes = len(S.RESOLUTIONS_48K) * 2 * 4 * rows * n + 3 * 8 * rows * len(S.RESOLUTIONS_48K)
        res["mrstft_distance"] = both(lambda: S.mrstft_distance(x, y, floor=FLOOR), lambda: torch_mrstft(x, y, S.RESOLUTIONS_48K, ws, FLOOR), nbytes,
                                      args.reps, args.warmup)
        d = S.mrstft_distance(x, y, floor=FLOOR)
        res["mrstft_total"] = [round(float(v), 6) for v in d["total"].cpu()]
        try:
            sc, lm = torch_mrstft(x, y, S.RESOLUTIONS_48K, ws, FLOOR)
            res["mrstft_total_torch"] = [round(float(v), 6) for v in (sc + lm).reshape(B, C, -1).mean(dim=(1, 2)).cpu()]
        except Exception:
            pass
        out["shapes"][f"{B}x{C}x{n}"] = res
        del x, y
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
