"""From a folder of audio files to the trainer's batches: the reference's ``dataset/dataloader.py`` on this project's own parts.

``MusicDataset`` keeps the reference's constructor, ``filter`` and ``get_index_offset`` (the same arithmetic on the same float32 ``cumsum``
tensor: tests/golden/dataset_index.npz pins every item).  What differs:
  * the codec does NOT run in ``__getitem__``.  An item is ``(chunk float32 [C, n], sr, metadata)`` on the CPU, read with ``jen1_amd.wav``,
    so DataLoader workers never open the GPU; ``LatentCollate`` turns a list of items into ``(emb [B, 128, T'], [metadata ...])`` in the
    process that consumes the loader (one ``convert_audio`` per input rate, one ``encode_latents`` per batch);
  * ``get_song_chunk`` is given the file ``index`` that ``get_index_offset`` found, not the item number (reference dataloader.py:100);
  * ``durations`` and ``cumsum`` start as None (the reference leaves them unset when no path is given and then reads them);
  * ``__len__`` is ``int(cumsum[-1] // sample_duration)``, the item count ``get_index_offset`` was written for, not the number of files;
  * a missing ``metadata/<song>.json`` raises FileNotFoundError naming the file (the reference: UnboundLocalError);
  * only ``.wav`` files are listed (there is no mp3 decoder on this path).
"""
from __future__ import annotations

import json
import os
import random
from typing import Callable, List, Optional

import torch
from torch.utils.data import DataLoader, Dataset, random_split

from . import wav as wavio


class MusicDataset(Dataset):
    def __init__(self, dataset_dir, sr, channels, min_duration, max_duration, sample_duration, aug_shift, device="cpu", durations_path=None,
                 cumsum_path=None, audio_file_txt_path=None):
        super().__init__()
        self.dataset_dir, self.sr, self.channels = dataset_dir, sr, channels
        self.min_duration, self.max_duration, self.sample_duration = min_duration, max_duration, sample_duration
        self.aug_shift, self.device = aug_shift, device
        self.audio_files_dir = f"{dataset_dir}/audios"
        self.metadatas_dir = f"{dataset_dir}/metadata"
        self.durations = None if durations_path is None else torch.load(durations_path)
        self.cumsum = None if cumsum_path is None else torch.load(cumsum_path)
        self.audio_files: List[str] = []
        if audio_file_txt_path is not None:
            self.audio_file_txt_path = audio_file_txt_path
            with open(audio_file_txt_path, "r") as file:
                self.audio_files = [line.strip() for line in file]
        self.init_dataset()

    def get_duration_sec(self, file) -> float:
        frames, sr, _channels = wavio.info(file)
        return frames / sr

    def filter(self, audio_files, durations) -> None:
        """keeps the files with min_duration <= duration < max_duration; ``cumsum`` is the running total of their durations in seconds"""
        keep = [i for i in range(len(audio_files)) if self.min_duration <= durations[i] < self.max_duration]
        self.audio_files = [audio_files[i] for i in keep]
        self.durations = [durations[i] for i in keep]
        self.cumsum = torch.cumsum(torch.tensor(self.durations), dim=0)

    def init_dataset(self) -> None:
        if self.durations is None and self.cumsum is None:
            names = sorted(n for n in os.listdir(self.audio_files_dir) if n.endswith(".wav"))
            files = [f"{self.audio_files_dir}/{n}" for n in names]
            self.filter(audio_files=files, durations=[self.get_duration_sec(f) for f in files])

    def get_index_offset(self, item):
        """item -> (index of the file, offset in seconds into it): items tile the concatenation of all files in steps of
        ``sample_duration``; the window is shifted by up to half of it when ``aug_shift`` is set, the file is the one under the window's
        midpoint, and a window that crosses a file boundary is pushed back inside that file"""
        half = self.sample_duration // 2
        shift = random.randint(-half, half) if self.aug_shift else 0
        offset = item * self.sample_duration + shift
        mid = offset + half
        total = self.cumsum[-1]
        assert 0 <= mid < total, f"Midpoint {mid} of item beyond total length {total}"
        index = torch.searchsorted(self.cumsum, mid)
        start = self.cumsum[index - 1] if index > 0 else 0.0
        end = self.cumsum[index]
        assert start <= mid <= end, f"Midpoint {mid} not inside interval [{start}, {end}] for index {index}"
        last = end - self.sample_duration
        if offset > last:
            offset = max(start, offset - half)
        elif offset < start:
            offset = min(last, offset + half)
        assert start <= offset <= last, f"Offset {offset} not in [{start}, {end} for index {index}]"
        return index, offset - start

    def get_song_chunk(self, index, offset):
        data, sr = wavio.load(self.audio_files[int(index)])
        first = int(offset * sr)
        return torch.from_numpy(data[:, first:first + int(self.sample_duration * sr)].copy()), sr

    def get_metadata(self, index):
        song = os.path.splitext(os.path.basename(self.audio_files[int(index)]))[0]
        path = f"{self.metadatas_dir}/{song}.json"
        if not os.path.exists(path):
            raise FileNotFoundError(f"no metadata for {self.audio_files[int(index)]}: {path} is missing")
        with open(path, "r") as file:
            return json.load(file)

    def __len__(self) -> int:
        return int(self.cumsum[-1] // self.sample_duration)

    def __getitem__(self, item):
        index, offset = self.get_index_offset(item)
        chunk, sr = self.get_song_chunk(index, offset)
        return chunk, sr, self.get_metadata(index)


def collate(batch):
    """the worker-side collate: the items as a list (clips differ in rate, channels and length until ``LatentCollate`` has converted them)"""
    return list(batch)


class LatentCollate:
    """``[(chunk [C, n], sr, metadata), ...]`` -> ``(emb [B, 128, T'], [metadata, ...])``, what ``UnifiedMultiTaskTrainer.train_loop`` reads.
    Runs in the process that owns the GPU.  Clips of one input rate are converted together (one ``convert_audio`` call per distinct rate;
    the channel rule of ``encodec.utils.convert_audio`` -- mono repeated, stereo averaged -- is applied on the host first, so that clips of
    one rate stack), every clip is trimmed or zero-padded to exactly ``sample_duration * sample_rate`` samples, and the batch is encoded by
    one ``audio_encoder.encode_latents`` call.  ``normalize`` / ``target_lufs`` (not in the reference): a strategy of
    ``jen1_amd.audio.normalize_audio`` applied with ``limit="clip"`` to the padded, converted batch in front of the encoder, so that clips
    reach it at one level and not at whatever level their files have; None feeds them as they are.  ``normalizer`` (not in the reference
    beyond its empty stub): a fitted ``jen1_amd.normalizer.Normalizer``; the batch's latents go through its ``normalize`` behind
    ``encode_latents``, so the trainer sees whitened latents.  ``with_lengths`` (for FITTING one, ``Normalizer.fit``): the batch carries a
    third entry, the valid latent frames of every clip -- its own sample count behind the conversion, mapped to frames -- so that the
    zero padding of short clips stays out of the statistics.  ``analyze`` (not in the reference): a tuple from ("tempo", "key"); for every
    item whose metadata lacks a named entry the value is measured from the clip itself (``jen1_amd.analysis.analyze`` on the converted
    batch, in front of ``normalize`` and the encoder, with the clip's valid sample count) and put into a COPY of its metadata.  Values
    the JSON has win; a clip the analyser cannot decide (tempo 0, key -1) gets no entry, so the conditioner's own rule for a missing key
    applies.  The results come to the host in one copy per batch, behind the enqueued encode call.  ``analyzer``: a stand-in for
    ``analysis.analyze`` with its signature.  ``augment`` (not in the reference): a ``jen1_amd.effects.Augment``; every item gets one
    draw (rate, semitones), the items of one draw are stretched and shifted together on the converted batch (in front of the analyser,
    ``normalize`` and the encoder) and cropped or zero-padded back to the batch's length, a clip's valid sample count becomes
    ``min(n_out, round(valid / rate))``, and the ``tempo`` / ``key`` entries the JSON has are moved with the draw in a COPY of the
    metadata -- measured entries are measured on the augmented audio and need no such step.  None (the default) changes nothing.
    ``augmenter``: a stand-in for ``effects.stretch_and_shift`` called as ``augmenter(wav, sr, rate=, semitones=)``."""

    def __init__(self, audio_encoder, device="cuda", sample_duration=10, convert_audio: Optional[Callable] = None,
                 normalize: Optional[str] = None, target_lufs=-14.0, normalizer=None, with_lengths: bool = False, analyze=(),
                 analyzer: Optional[Callable] = None, augment=None, augmenter: Optional[Callable] = None):
        self.augment, self._augmenter = augment, augmenter
        self.analyze = tuple(analyze)
        bad = [a for a in self.analyze if a not in ("tempo", "key")]
        if bad:
            raise ValueError(f"unknown analyze entries {bad}: a tuple from ('tempo', 'key')")
        self._analyzer = analyzer
        self.audio_encoder, self.device, self.sample_duration = audio_encoder, device, sample_duration
        self._convert = convert_audio
        if normalize is not None:
            from . import audio
            if normalize not in audio.STRATEGIES:
                raise ValueError(f"unknown normalize {normalize!r}: None or one of {audio.STRATEGIES}")
        self.normalize, self.target_lufs = normalize, target_lufs
        self.normalizer, self.with_lengths = normalizer, bool(with_lengths)

    def valid_frames(self, n_valid: int, n_out: int, frames: int) -> int:
        """the latent frames that hold audio of a clip of ``n_valid`` samples padded to ``n_out``: the frames the encoder gives the clip
        alone (its segments start where the padded clip's do), or the clip's share of ``frames``, rounded up, without that query"""
        n_valid = max(0, min(int(n_valid), n_out))
        count = getattr(self.audio_encoder, "segment_frames", None)
        t = sum(count(n_valid)) if count is not None and n_valid > 0 else -(-n_valid * frames // n_out)
        return max(0, min(int(t), frames))

    def convert_audio(self, wav, sr, target_sr, target_channels):
        if self._convert is not None:
            return self._convert(wav, sr, target_sr, target_channels)
        from . import audio
        return audio.convert_audio(wav, sr, target_sr, target_channels, device=self.device)

    def analyze_batch(self, wav, rate, valid):
        if self._analyzer is not None:
            return self._analyzer(wav, rate, lengths=valid)
        from . import analysis
        return analysis.analyze(wav, rate, lengths=valid, device=self.device)

    def augment_batch(self, wav, rate, speed, semitones):
        if self._augmenter is not None:
            return self._augmenter(wav, rate, rate=speed, semitones=semitones)
        from . import effects
        return effects.stretch_and_shift(wav, rate, rate=speed, semitones=semitones, device=self.device)

    def apply_augment(self, out, rate, valid, meta):
        """one draw per item, the items of one draw as one batch: ``out`` changed in place, (valid, meta) of the augmented clips"""
        n_out = int(out.shape[-1])
        draws = [self.augment.draw() for _ in meta]
        groups = {}
        for i, d in enumerate(draws):
            groups.setdefault(d, []).append(i)
        valid, meta = list(valid), list(meta)
        for (speed, semis), idx in groups.items():
            if float(speed) == 1.0 and int(semis) == 0:
                continue
            y = self.augment_batch(out[idx], rate, speed, semis).to(self.device, torch.float32)
            n = min(n_out, int(y.shape[-1]))
            out[idx] = 0.0
            out[idx, :, :n] = y[:, :, :n]
            for i in idx:
                valid[i] = min(n_out, int(round(valid[i] / float(speed))))
                meta[i] = self.augment.transform_metadata(meta[i], speed, semis)
        return valid, meta

    def fill_metadata(self, meta, measured):
        """copies of ``meta`` with the entries of ``self.analyze`` they lack, from one device-to-host copy of the measured [tempo; key]"""
        host = torch.stack([torch.as_tensor(measured["tempo"]).to(torch.float64), torch.as_tensor(measured["key"]).to(torch.float64)]).cpu()
        out = []
        for i, md in enumerate(meta):
            md = dict(md)
            bpm, k = float(host[0, i]), int(host[1, i])
            if "tempo" in self.analyze and "tempo" not in md and bpm > 0.0:
                md["tempo"] = bpm
            if "key" in self.analyze and "key" not in md and k >= 0:
                md["key"] = k
            out.append(md)
        return out

    @staticmethod
    def _channels(chunk: torch.Tensor, target: int) -> torch.Tensor:
        c = chunk.shape[0]
        if c == target:
            return chunk
        if target == 1:
            return chunk.mean(dim=0, keepdim=True)
        if c == 1:
            return chunk.expand(target, -1)
        raise RuntimeError(f"impossible to convert from {c} to {target} channels")

    @torch.no_grad()
    def __call__(self, batch):
        ae = self.audio_encoder
        rate, channels = int(ae.sample_rate), int(ae.channels)
        n_out = int(self.sample_duration * rate)
        out = torch.zeros((len(batch), channels, n_out), dtype=torch.float32, device=self.device)
        by_rate = {}
        valid = [0] * len(batch)
        for i, (_chunk, sr, _meta) in enumerate(batch):
            by_rate.setdefault(int(sr), []).append(i)
        for sr, idx in by_rate.items():
            clips = [self._channels(torch.as_tensor(batch[i][0], dtype=torch.float32), channels) for i in idx]
            longest = max(c.shape[-1] for c in clips)
            group = torch.zeros((len(idx), channels, longest), dtype=torch.float32)
            for j, c in enumerate(clips):
                group[j, :, :c.shape[-1]] = c
            conv = self.convert_audio(group.to(self.device), sr, rate, channels)
            n = min(n_out, conv.shape[-1])
            out[idx, :, :n] = conv[:, :, :n].to(self.device, torch.float32)
            for i, c in zip(idx, clips):
                valid[i] = min(n, -(-c.shape[-1] * rate // sr))
        meta = [meta for _chunk, _sr, meta in batch]
        if self.augment is not None:
            valid, meta = self.apply_augment(out, rate, valid, meta)
        measured = None
        if self.analyze and any(name not in md for md in meta for name in self.analyze):
            measured = self.analyze_batch(out, rate, valid)                  # device tensors: nothing waits here
        if self.normalize is not None:             # the level of every clip, set in one call on the padded batch (not in the reference)
            from . import audio
            out = audio.normalize_audio(out, rate, strategy=self.normalize, target_lufs=self.target_lufs, limit="clip", device=self.device)
        emb = ae.encode_latents(out)[0]
        if measured is not None:
            meta = self.fill_metadata(meta, measured)
        lengths = [self.valid_frames(v, n_out, emb.shape[-1]) for v in valid] if self.with_lengths else None
        if self.normalizer is not None:
            emb = self.normalizer.normalize(emb)
        return (emb, meta) if lengths is None else (emb, meta, lengths)


class LatentLoader:
    """a DataLoader of raw items with ``LatentCollate`` applied as its batches are consumed (a DataLoader's own ``collate_fn`` would run
    inside the workers)"""

    def __init__(self, loader: DataLoader, collate_fn: Optional[LatentCollate]):
        self.loader, self.collate_fn = loader, collate_fn

    def __len__(self) -> int:
        return len(self.loader)

    def __iter__(self):
        for batch in self.loader:
            yield batch if self.collate_fn is None else self.collate_fn(batch)


def get_dataloaders(dataset_dir, sr, channels, min_duration, max_duration, sample_duration, aug_shift, batch_size: int = 50, shuffle: bool = True,
                    split_ratio=0.8, device="cpu", durations_path=None, cumsum_path=None, audio_file_txt_path=None, *, audio_encoder=None,
                    num_workers: int = 0, dataset_cls=None, normalize: Optional[str] = None, target_lufs=-14.0, normalizer=None,
                    with_lengths: bool = False, analyze=(), augment=None):
    """(train loader, validation loader) of ``(emb, metadata)`` batches.  ``dataset_dir``: one folder (split by ``split_ratio``) or a
    (train, validation) pair.  ``audio_encoder`` (an ``EncodecHIP``) installs ``LatentCollate`` on ``device``; without it the loaders yield
    the raw item lists.  ``num_workers`` > 0 reads the files in spawned worker processes, which never touch the GPU.  ``dataset_cls``: a
    ``MusicDataset`` subclass to build instead (one that selects or tags items; importable by name when workers are used).  ``normalize`` /
    ``target_lufs``, ``normalizer``, ``with_lengths`` and ``analyze`` are handed to ``LatentCollate``; ``augment`` (a
    ``jen1_amd.effects.Augment``) to the training loader's only."""
    cls = MusicDataset if dataset_cls is None else dataset_cls

    def make(folder):
        return cls(dataset_dir=folder, sr=sr, channels=channels, min_duration=min_duration, max_duration=max_duration,
                   sample_duration=sample_duration, aug_shift=aug_shift, device=device, durations_path=durations_path,
                   cumsum_path=cumsum_path, audio_file_txt_path=audio_file_txt_path)
    if not isinstance(dataset_dir, tuple):
        dataset = make(dataset_dir)
        train_size = int(split_ratio * len(dataset))
        train_dataset, val_dataset = random_split(dataset, [train_size, len(dataset) - train_size])
    else:
        train_dataset, val_dataset = make(dataset_dir[0]), make(dataset_dir[1])
    def collate_fn(aug):
        return None if audio_encoder is None else LatentCollate(audio_encoder, device, sample_duration, normalize=normalize, target_lufs=target_lufs,
                                                                   normalizer=normalizer, with_lengths=with_lengths, analyze=analyze, augment=aug)
    fn = collate_fn(None)
    train_fn = fn if augment is None else collate_fn(augment)
    kw = dict(batch_size=batch_size, collate_fn=collate, drop_last=True, num_workers=num_workers)
    if num_workers > 0:
        kw["multiprocessing_context"] = "spawn"        # never fork a process that has initialised the GPU
    return (LatentLoader(DataLoader(train_dataset, shuffle=shuffle, **kw), train_fn),
            LatentLoader(DataLoader(val_dataset, shuffle=False, **kw), fn))
