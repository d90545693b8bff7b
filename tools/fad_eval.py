"""Frechet Audio Distance between two folders of .wav files on the HIP kernels (jen1_amd/fad.py).

    python tools/fad_eval.py --test DIR --reference DIR_or_stats.pt --vggish WEIGHTS.pt [--save-stats OUT.pt] [--final-relu]

``--vggish``: a ``torch.save``d state dict with the keys of the common PyTorch port of VGGish (``features.{0,3,6,8,11,13}``,
``embeddings.{0,2,4}``; a ``{"state_dict": ...}`` wrapper is unwrapped).  ``--reference``: a folder, or the statistics an earlier run saved
with ``--save-stats`` (a reference set is embedded once and reused for every checkpoint).  Files are read with ``jen1_amd.wav`` (mono or
stereo, any sample rate) and embedded one by one; files shorter than one example (0.975 s) add nothing.  Prints one JSON line:
``{"fad": ..., "test_embeddings": ..., "reference_embeddings": ..., "test_files": ..., "reference_files": ...}``.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def wav_files(folder: str):
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith(".wav"))
    if not names:
        raise SystemExit(f"{folder}: no .wav files")
    return [os.path.join(folder, n) for n in names]


def folder_stats(fad, folder: str, device):
    from jen1_amd import wav

    def batches():
        for path in wav_files(folder):
            audio, sr = wav.load(path)
            if audio.shape[0] > 2:
                audio = audio[:2]
            yield torch.from_numpy(audio).to(device), sr
    return fad.stats(batches()), len(wav_files(folder))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--test", required=True)
    ap.add_argument("--reference", required=True)
    ap.add_argument("--vggish", required=True)
    ap.add_argument("--save-stats", default=None, help="where to save the reference statistics")
    ap.add_argument("--final-relu", action="store_true")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args()
    from jen1_amd import fad as F
    sd = torch.load(args.vggish, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    fad = F.FrechetAudioDistance(F.VGGishHIP.from_state_dict(sd, final_relu=args.final_relu, device=args.device))
    test, n_test = folder_stats(fad, args.test, args.device)
    if os.path.isdir(args.reference):
        ref, n_ref = folder_stats(fad, args.reference, args.device)
    else:
        ref, n_ref = F.FrechetStats.from_state_dict(torch.load(args.reference, map_location="cpu")), None
    if args.save_stats:
        torch.save(ref.state_dict(), args.save_stats)
    print(json.dumps({"fad": F.frechet_distance(test, ref), "test_embeddings": test.count, "reference_embeddings": ref.count,
                      "test_files": n_test, "reference_files": n_ref}))


if __name__ == "__main__":
    main()
