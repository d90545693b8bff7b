"""The three-file dataset of tests/test_gpu_dataset.py and the ``MusicDataset`` subclass its loaders build; a module of its own so that
spawned DataLoader workers can import the class by name.  Nothing here imports the HIP library.

With ``sample_duration=1`` the half interval of ``get_index_offset`` is 0: a window that touches a file boundary cannot be pushed back
and fails the reference's own assertion (item 2 and item 5 below), so not every item number is a valid one.  ``TaggedDataset`` serves the
first valid window of each file -- items 0, 3 and 6 of three files of 2.5 s -- through the unchanged ``get_index_offset``.
"""
import json
import os
import struct
import sys

import numpy as np

from jen1_amd import wav
from jen1_amd.dataset import MusicDataset

SECONDS = 2.5
ITEMS = (0, 3, 6)                                        # -> (file 0, 0.0 s), (file 1, 0.5 s), (file 2, 1.0 s)
FILES = [("a_mono_44k", 1, 44100, "pcm16"), ("b_stereo_48k", 2, 48000, "float32"), ("c_stereo_48k", 2, 48000, "pcm24")]


def _audio(channels, frames, seed):
    t = np.arange(frames, dtype=np.float64)
    g = np.random.default_rng(seed)
    x = np.stack([0.3 * np.sin(2 * np.pi * (220.0 * (c + 1) + 30 * seed) * t / 44100.0) for c in range(channels)])
    return (x + 0.05 * g.standard_normal(x.shape)).astype(np.float32)


def _save_pcm24(path, x, sr):
    channels = x.shape[0]
    v = np.clip(np.rint(x.T.astype(np.float64) * 8388608.0), -8388608, 8388607).astype(np.int64).reshape(-1) & 0xFFFFFF
    body = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    fmt = struct.pack("<HHIIHH", 1, channels, sr, sr * channels * 3, channels * 3, 24)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(body) + (len(body) & 1)) + b"WAVEfmt " + struct.pack("<I", 16) + fmt)
        f.write(b"data" + struct.pack("<I", len(body)) + body + b"\0" * (len(body) & 1))


def make_dataset(root) -> str:
    os.makedirs(os.path.join(root, "audios"))
    os.makedirs(os.path.join(root, "metadata"))
    for i, (name, channels, sr, encoding) in enumerate(FILES):
        x = _audio(channels, int(sr * SECONDS), i)
        path = os.path.join(root, "audios", name + ".wav")
        if encoding == "pcm24":
            _save_pcm24(path, x, sr)
        else:
            wav.save(path, x, sr, encoding)
        with open(os.path.join(root, "metadata", name + ".json"), "w") as f:
            json.dump({"prompt": f"prompt of {name}"}, f)
    return str(root)


class TaggedDataset(MusicDataset):
    """the valid windows ``ITEMS``; every item's metadata says which process read it and whether that process had loaded the HIP library"""

    def __len__(self):
        return len(ITEMS)

    def __getitem__(self, i):
        chunk, sr, meta = super().__getitem__(ITEMS[i])
        lib = sys.modules.get("jen1_amd.lib")
        return chunk, sr, dict(meta, item=ITEMS[i], pid=os.getpid(), lib_loaded=lib is not None and getattr(lib, "_lib", None) is not None,
                               torch_cuda_initialized=_cuda_initialized())


def _cuda_initialized() -> bool:
    import torch
    return bool(torch.cuda.is_initialized())
