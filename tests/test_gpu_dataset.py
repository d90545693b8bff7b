"""-m gpu: from three WAV files to a training step.  ``get_dataloaders`` over a folder of a 44.1 kHz mono pcm16 file, a 48 kHz stereo float32
file and a 48 kHz stereo 24-bit file (tests/dataset_common.py), ``sample_duration=1``: the first batch against the same clips converted
and encoded by hand, with and without worker processes (which must never load the HIP library), and one micro-batch of
``UnifiedMultiTaskTrainer.train_loop`` over that loader.

What "equal to the by-hand result" can mean: two runs of the same encoder pass are not bit-identical (float atomics in its split-K
convolutions; measured on MI355X: 5e-6 apart in float32), so a second ``encode_latents`` run is no bit-exact yardstick for the first.  The
test therefore pins the batch bit for bit where that is defined -- the audio ``LatentCollate`` hands to ``encode_latents`` equals the
by-hand conversion, and ``emb`` is that call's result -- and compares ``emb`` with a by-hand ``encode_latents`` run of the float32 codec
frame by frame: fewer than 5 % of the frames may differ at all (the cap of tests/test_gpu_rvq_encode.py)."""
import os
import random

import numpy as np
import pytest
import torch

import dataset_common as DC
import encodec_common as EC
import rvq_encode_common as RC
from jen1_amd import wav

pytestmark = pytest.mark.gpu

KW = dict(sr=48000, channels=2, min_duration=1.0, max_duration=20.0, sample_duration=1, aug_shift=False, batch_size=3, shuffle=False, device="cuda")


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in EC.dec_params().items()}, compute_dtype="f32")
    enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in EC.enc_params().items()}, compute_dtype="f32")
    return EncodecHIP(dec, ResidualVectorQuantizerHIP(torch.from_numpy(RC.golden_tables(16))), encoder=enc)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return DC.make_dataset(tmp_path_factory.mktemp("dataset"))


@pytest.fixture(scope="module")
def by_hand(codec, folder):
    """the three clips read, converted and encoded without the dataset: item 0 / 3 / 6 start at 0.0 / 0.5 / 1.0 s of their files"""
    from jen1_amd import audio
    clips = []
    for (name, channels, sr, _), start in zip(DC.FILES, (0.0, 0.5, 1.0)):
        x, rate = wav.load(os.path.join(folder, "audios", name + ".wav"))
        assert rate == sr and x.shape == (channels, int(sr * DC.SECONDS))
        x = torch.from_numpy(x[:, int(start * sr):int(start * sr) + sr]).expand(2, -1)[None].contiguous().cuda()
        y = audio.convert_audio(x, sr, 48000, 2)
        assert y.shape == (1, 2, 48000)
        clips.append(y)
    audio = torch.cat(clips, dim=0)
    return audio, codec.encode_latents(audio)[0]


@pytest.mark.parametrize("workers", [0, 2])
def test_first_batch_vs_by_hand(codec, folder, by_hand, workers):
    from jen1_amd.dataset import get_dataloaders
    train, val = get_dataloaders((folder, folder), audio_encoder=codec, num_workers=workers, dataset_cls=DC.TaggedDataset, **KW)
    assert len(train) == 1 and len(val) == 1
    seen = []
    inner = codec.encode_latents
    codec.encode_latents = lambda a: (seen.append((a.clone(), inner(a))), seen[-1][1])[1]
    try:
        emb, meta = next(iter(train))
    finally:
        del codec.encode_latents
    want_audio, want_emb = by_hand
    # 1 s = 48 000 samples is TWO segments of the codec (length 48 000, stride 47 520: offsets 0 and 47 520), 150 + 2 frames, as
    # ``EncodecModel.encode`` cuts it and tests/test_gpu_codec_segments.py::test_encode_of_whole_seconds pins it
    assert codec.segment_frames(48000) == [150, 2]
    assert emb.shape == (3, 128, 152) and emb.dtype == torch.float32 and emb.device.type == "cuda"
    assert [m["prompt"] for m in meta] == [f"prompt of {name}" for name, *_ in DC.FILES] and [m["item"] for m in meta] == list(DC.ITEMS)
    assert len(seen) == 1 and torch.equal(seen[0][0].view(torch.int32), want_audio.view(torch.int32)), "the audio handed to the encoder differs"
    assert emb is seen[0][1][0] or torch.equal(emb.view(torch.int32), seen[0][1][0].view(torch.int32))
    differ = 1.0 - float((emb == want_emb).all(dim=1).float().mean())
    print(f"dataset first batch, {workers} workers: share of frames that differ from the by-hand run {differ:.5f}")
    assert differ < 0.05, differ
    if workers:
        assert all(m["pid"] != os.getpid() for m in meta), "the items were read in this process"
        assert not any(m["lib_loaded"] or m["torch_cuda_initialized"] for m in meta), "a DataLoader worker opened the GPU"
    else:
        assert all(m["pid"] == os.getpid() for m in meta)


def test_train_loop_over_the_loader(codec, folder):
    from jen1_amd import synth
    from jen1_amd.config import tiny_model_config
    from jen1_amd.dataset import get_dataloaders
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.2, embedding_scale=0.8,
                           batch_cfg=True, scale_cfg=True)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    cond = synth.conditioning(3, 152, "text_guided")
    emb, msk = torch.from_numpy(cond["cross_attn_cond"]).cuda(), torch.from_numpy(cond["cross_attn_masks"]).cuda()
    seen = []

    def conditioner(metadata, device):
        seen.extend(m["prompt"] for m in metadata)
        return {"prompt": (emb[:len(metadata)], msk[:len(metadata)])}

    loaders = get_dataloaders((folder, folder), audio_encoder=codec, dataset_cls=DC.TaggedDataset, **KW)
    tr = UnifiedMultiTaskTrainer.build(model, gd, conditioner, opt, None, grad_accum_every=1, rng=random.Random(0), use_graph=False, dls=(loaders[0], None))
    losses = []
    inner = tr.train_step
    tr.train_step = lambda a, m: (lambda out: (losses.append(out[0]), out)[1])(inner(a, m))
    p0 = opt.flat_param.clone()
    torch.manual_seed(0)
    tr.train_loop(max_steps=1)
    torch.cuda.synchronize()
    assert tr.global_step == 1 and opt.step_count == 1 and len(losses) == 1
    assert np.isfinite(float(losses[0])) and float(losses[0]) > 0
    assert sorted(seen) == sorted(f"prompt of {name}" for name, *_ in DC.FILES)
    assert float((opt.flat_param - p0).abs().max()) > 0
