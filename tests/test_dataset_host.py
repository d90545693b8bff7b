"""jen1_amd/dataset.py on the host: the index arithmetic against what the reference's ``get_index_offset`` returned
(tests/golden/dataset_index.npz, made by tests/golden/make_dataset_golden.py), the listed deviations, and ``LatentCollate`` with a stub
encoder that records what it is given."""
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

from helpers import golden
from jen1_amd import wav
from jen1_amd.dataset import LatentCollate, LatentLoader, MusicDataset, collate, get_dataloaders


def _tone(channels, frames, seed):
    return (np.random.default_rng(seed).random((channels, frames)) * 0.5 - 0.25).astype(np.float32)


def _make_dir(root, files, with_json=True):
    """files: {name: (channels, sr, seconds, encoding)} -> dataset folder with audios/ and metadata/"""
    os.makedirs(root / "audios")
    os.makedirs(root / "metadata")
    for i, (name, (channels, sr, seconds, encoding)) in enumerate(files.items()):
        wav.save(root / "audios" / f"{name}.wav", _tone(channels, int(sr * seconds), i), sr, encoding)
        if with_json:
            (root / "metadata" / f"{name}.json").write_text(json.dumps({"prompt": f"song {name}"}))
    return str(root)


def _dataset(folder, **kw):
    args = dict(dataset_dir=folder, sr=48000, channels=2, min_duration=1.0, max_duration=20.0, sample_duration=1, aug_shift=False, device="cpu",
                durations_path=None, cumsum_path=None, audio_file_txt_path=None)
    args.update(kw)
    return MusicDataset(**args)


@pytest.mark.parametrize("aug", [False, True], ids=["plain", "aug_shift"])
def test_get_index_offset_vs_reference(aug):
    g = golden("dataset_index")
    ds = MusicDataset.__new__(MusicDataset)
    ds.sample_duration, ds.aug_shift = int(g["sample_duration"]), aug
    ds.cumsum = torch.cumsum(torch.tensor(g["durations"].tolist()), dim=0)
    tag = "aug" if aug else "plain"
    assert len(ds) == len(g[f"{tag}.index"]) == 22
    random.seed(int(g["seed"]))
    got = [ds.get_index_offset(item) for item in range(len(ds))]
    assert [int(i) for i, _ in got] == g[f"{tag}.index"].tolist()
    assert [float(o) for _, o in got] == g[f"{tag}.offset"].tolist()
    if aug:
        assert g["aug.offset"].tolist() != g["plain.offset"].tolist()


def test_filter_len_and_listing(tmp_path):
    folder = _make_dir(tmp_path / "d", {"b": (1, 8000, 2.5, "pcm16"), "a": (2, 8000, 3.0, "float32"), "short": (1, 8000, 0.5, "pcm16"),
                                        "long": (1, 8000, 20.0, "pcm16")})
    (tmp_path / "d" / "audios" / "c.mp3").write_bytes(b"not audio")
    (tmp_path / "d" / "audios" / "notes.txt").write_text("x")
    ds = _dataset(folder)
    # only .wav, in name order; min_duration <= d < max_duration (20.0 s is out, 0.5 s is out)
    assert [os.path.basename(f) for f in ds.audio_files] == ["a.wav", "b.wav"]
    assert ds.durations == [3.0, 2.5] and ds.cumsum.tolist() == [3.0, 5.5]
    assert len(ds) == 5                                            # int(5.5 // 1), not the number of files
    ds.filter(["x", "y", "z"], [1.0, 0.99, 19.99])
    assert ds.audio_files == ["x", "z"] and ds.durations == [1.0, 19.99]


def test_durations_and_cumsum_start_as_none_or_loaded(tmp_path):
    folder = _make_dir(tmp_path / "d", {"a": (1, 8000, 2.0, "pcm16")})
    torch.save([2.0], tmp_path / "dur.pt")
    torch.save(torch.tensor([2.0]), tmp_path / "cum.pt")
    listing = tmp_path / "files.txt"
    listing.write_text(f"{folder}/audios/a.wav\n")
    ds = _dataset(folder, durations_path=str(tmp_path / "dur.pt"), cumsum_path=str(tmp_path / "cum.pt"), audio_file_txt_path=str(listing))
    assert ds.durations == [2.0] and ds.cumsum.tolist() == [2.0] and ds.audio_files == [f"{folder}/audios/a.wav"] and len(ds) == 2
    bare = MusicDataset.__new__(MusicDataset)
    bare.audio_files_dir = f"{folder}/audios"
    bare.min_duration, bare.max_duration, bare.durations, bare.cumsum = 0.0, 10.0, None, None
    bare.init_dataset()
    assert bare.durations == [2.0]


def _lib_loaded() -> bool:
    lib = sys.modules.get("jen1_amd.lib")
    return lib is not None and lib._lib is not None


def test_getitem_reads_the_file_the_index_names(tmp_path):
    """item 2 lies in the second file: the chunk comes from THAT file (the reference indexes the file list with the item number, which
    here would run past the two files)"""
    loaded_before = _lib_loaded()                                  # (an earlier test of the same process may have loaded it)
    folder = _make_dir(tmp_path / "d", {"a": (2, 8000, 3.0, "float32"), "b": (1, 16000, 4.5, "pcm16")})
    ds = _dataset(folder, sample_duration=2)
    assert len(ds) == 3
    chunk, sr, meta = ds[2]
    index, offset = ds.get_index_offset(2)
    assert int(index) == 1 and float(offset) == 1.0 and sr == 16000 and meta == {"prompt": "song b"}
    assert chunk.dtype == torch.float32 and chunk.shape == (1, 32000)
    assert np.array_equal(chunk.numpy(), wav.load(f"{folder}/audios/b.wav")[0][:, 16000:48000])
    chunk, sr, meta = ds[1]                                        # a window over the boundary is pushed back into the first file
    assert sr == 8000 and chunk.shape == (2, 16000) and meta == {"prompt": "song a"}
    assert np.array_equal(chunk.numpy(), wav.load(f"{folder}/audios/a.wav")[0][:, 8000:24000])
    assert _lib_loaded() == loaded_before, "reading items loaded the HIP library"


def test_missing_metadata_names_the_file(tmp_path):
    folder = _make_dir(tmp_path / "d", {"a": (1, 8000, 2.0, "pcm16")}, with_json=False)
    with pytest.raises(FileNotFoundError, match="metadata/a.json"):
        _dataset(folder)[0]


class StubEncoder:
    sample_rate, channels = 48000, 2

    def __init__(self):
        self.audio = None

    def encode_latents(self, audio):
        self.audio = audio.clone()
        return audio[:, :1, ::320].repeat(1, 128, 1), [audio.shape[-1] // 320], None


def test_latent_collate_converts_once_per_rate_trims_and_pads():
    calls = []

    def convert(x, sr, target_sr, target_channels):
        calls.append((tuple(x.shape), sr, target_sr, target_channels))
        return x.repeat_interleave(target_sr // sr, dim=-1) if sr != target_sr else x

    enc = StubEncoder()
    fn = LatentCollate(enc, "cpu", 1, convert_audio=convert)
    a = torch.from_numpy(_tone(1, 24000, 1))           # mono, 24 kHz, exactly 1 s
    b = torch.from_numpy(_tone(2, 48000, 2))           # stereo, 48 kHz, exactly 1 s
    c = torch.from_numpy(_tone(2, 20000, 3))           # stereo, 24 kHz, short: padded
    d = torch.from_numpy(_tone(1, 50000, 4))           # mono, 48 kHz, long: trimmed
    emb, meta = fn([(a, 24000, "A"), (b, 48000, "B"), (c, 24000, "C"), (d, 48000, "D")])
    assert meta == ["A", "B", "C", "D"]
    assert sorted(calls) == [((2, 2, 24000), 24000, 48000, 2), ((2, 2, 50000), 48000, 48000, 2)]
    x = enc.audio
    assert x.shape == (4, 2, 48000) and x.dtype == torch.float32 and emb.shape == (4, 128, 150)
    assert torch.equal(x[0], a.expand(2, -1).repeat_interleave(2, dim=-1))
    assert torch.equal(x[1], b)
    assert torch.equal(x[2, :, :40000], c.repeat_interleave(2, dim=-1)) and float(x[2, :, 40000:].abs().max()) == 0.0
    assert torch.equal(x[3], d.expand(2, -1)[:, :48000])
    mono = LatentCollate(type("E", (StubEncoder,), {"channels": 1})(), "cpu", 1, convert_audio=convert)
    mono([(b, 48000, "B")])
    assert torch.equal(mono.audio_encoder.audio[0], b.mean(dim=0, keepdim=True))


def test_get_dataloaders_host(tmp_path):
    folder = _make_dir(tmp_path / "d", {"a": (2, 48000, 4.5, "pcm16"), "b": (1, 48000, 4.5, "pcm16")})
    enc = StubEncoder()
    kw = dict(sr=48000, channels=2, min_duration=1.0, max_duration=20.0, sample_duration=2, aug_shift=False, batch_size=2, shuffle=False, device="cpu")
    train, val = get_dataloaders(folder, split_ratio=0.5, audio_encoder=enc, **kw)
    assert isinstance(train, LatentLoader) and len(train) == 1 and len(val) == 1              # 2 + 2 items, batches of 2
    emb, meta = next(iter(train))
    assert emb.shape == (2, 128, 300) and len(meta) == 2 and all(set(m) == {"prompt"} for m in meta)
    assert enc.audio.shape == (2, 2, 96000)
    raw, _ = get_dataloaders((folder, folder), **kw)                                         # no encoder: the raw item lists
    batches = list(raw)
    assert len(raw) == len(batches) == 2 and [m["prompt"] for b in batches for _, _, m in b] == ["song a", "song a", "song b", "song b"]
    items = batches[1]
    assert items[0][1] == 48000 and items[0][0].shape == (1, 96000) and collate(items) == items
