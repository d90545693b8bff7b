"""Writes tests/golden/dataset_index.npz: what the reference's ``MusicDataset.get_index_offset`` returns for every item of a small
dataset, with and without ``aug_shift``.  Results only: 7 durations, the sample duration, the seed, and per setting the (index, offset)
of every item.

The reference's ``dataset/dataloader.py`` imports ``torchaudio`` and ``encodec`` at module level and builds the codec in ``__init__``;
neither is needed for the index arithmetic, so both are stubbed in ``sys.modules`` and the instance is made with ``__new__``.

    JEN1_REFERENCE=/path/to/reference python tests/golden/make_dataset_golden.py
"""
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DURATIONS = [12.5, 30.0, 10.0, 47.25, 21.125, 10.5, 95.0]        # seconds; float32 holds every one and every partial sum exactly
SAMPLE_DURATION = 10
SEED = 20240


def main():
    for name in ("torchaudio", "encodec", "encodec.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["encodec"].EncodecModel = object
    sys.modules["encodec.utils"].convert_audio = None
    sys.path.insert(0, os.environ.get("JEN1_REFERENCE", "/root/reference"))
    from dataset.dataloader import MusicDataset

    out = {"durations": np.asarray(DURATIONS, dtype=np.float64), "sample_duration": np.int64(SAMPLE_DURATION), "seed": np.int64(SEED)}
    for aug in (False, True):
        ds = MusicDataset.__new__(MusicDataset)
        ds.sample_duration, ds.aug_shift = SAMPLE_DURATION, aug
        ds.cumsum = torch.cumsum(torch.tensor(DURATIONS), dim=0)
        n = int(ds.cumsum[-1] // SAMPLE_DURATION)
        random.seed(SEED)
        index, offset = [], []
        for item in range(n):
            i, off = ds.get_index_offset(item)
            index.append(int(i))
            offset.append(float(off))
        tag = "aug" if aug else "plain"
        out[f"{tag}.index"] = np.asarray(index, dtype=np.int64)
        out[f"{tag}.offset"] = np.asarray(offset, dtype=np.float64)
    np.savez(os.path.join(HERE, "dataset_index.npz"), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})


if __name__ == "__main__":
    main()
