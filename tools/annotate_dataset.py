#!/usr/bin/env python
"""Measure the tempo and key of every file of a dataset folder and write them where ``MusicDataset`` reads them.

    python tools/annotate_dataset.py FOLDER [--overwrite]

Walks ``FOLDER/audios/*.wav`` (read with ``jen1_amd.wav``), converts each file to 48 kHz mono, analyses the whole file with
``jen1_amd.analysis.analyze`` and adds ``tempo``, ``key``, ``key_name``, ``tempo_strength`` and ``key_strength`` to
``FOLDER/metadata/<song>.json``, creating the file if there is none.  Entries that are already there stay unless ``--overwrite`` is
given; a value the analyser cannot decide (tempo 0, key -1) is not written."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "jen-1-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

RATE = 48000


def merge(old: dict, measured: dict, overwrite: bool) -> dict:
    """``old`` with the decided entries of ``measured``; what ``old`` has wins unless ``overwrite``"""
    out = dict(old)
    decided = dict(measured)
    if not decided.get("tempo", 0.0) > 0.0:
        decided.pop("tempo", None)
        decided.pop("tempo_strength", None)
    if decided.get("key", -1) < 0:
        for name in ("key", "key_name", "key_strength"):
            decided.pop(name, None)
    for name, value in decided.items():
        if overwrite or name not in out:
            out[name] = value
    return out


def measure(path: str, device: str) -> dict:
    import torch
    from jen1_amd import analysis, audio, wav
    data, sr = wav.load(path)
    x = torch.from_numpy(data[None].copy()).to(torch.float32)
    if x.shape[1] > 2:
        x = x.mean(dim=1, keepdim=True)
    x = audio.convert_audio(x.to(device), sr, RATE, 1, device=device)
    res = {k: v.cpu() for k, v in analysis.analyze(x, RATE, device=device).items()}
    key = int(res["key"][0])
    return {"tempo": float(res["tempo"][0]), "tempo_strength": float(res["tempo_strength"][0]), "key": key,
            "key_name": analysis.KEY_NAMES[key] if key >= 0 else None, "key_strength": float(res["key_strength"][0])}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("folder")
    ap.add_argument("--overwrite", action="store_true", help="replace tempo / key entries that are already in the JSON files")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    audios, metas = os.path.join(args.folder, "audios"), os.path.join(args.folder, "metadata")
    os.makedirs(metas, exist_ok=True)
    for name in sorted(n for n in os.listdir(audios) if n.endswith(".wav")):
        target = os.path.join(metas, os.path.splitext(name)[0] + ".json")
        old = {}
        if os.path.exists(target):
            with open(target, "r") as f:
                old = json.load(f)
        new = merge(old, measure(os.path.join(audios, name), args.device), args.overwrite)
        with open(target, "w") as f:
            json.dump(new, f, indent=1)
        print(f"{name}: tempo {new.get('tempo')}, key {new.get('key_name')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
