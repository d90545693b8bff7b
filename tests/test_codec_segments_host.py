"""CPU: the float64 restatements of the codec's segment path (tests/codec_segments_common.py) against the Hugging Face port of Encodec,
the stored output of its ``decode`` (tests/golden/codec_segments.npz), the scale policy and the argument errors of
``Jen1.generate(decode=..., segment_scales=...)`` and the frame-count arithmetic of the segment layout.
"""
import numpy as np
import pytest
import torch

import codec_segments_common as CC
from helpers import golden, rel_err


# ------------------------------------------------------------------ restatements against the port
OLA_CASES = [
    # L_0, stride, lengths
    (48000, 47520, [48000, 4800]),
    (640, 608, [640, 640, 640]),
    (640, 320, [640, 640, 416, 96]),          # 1056 samples: the second-to-last frame is short too
]


@pytest.mark.parametrize("L0,stride,lengths", OLA_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_overlap_add_matches_the_port(L0, stride, lengths):
    tr = pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(L0 + stride + len(lengths))
    frames = [torch.randn((2, 2, n), generator=g) for n in lengths]
    want = tr.EncodecModel._linear_overlap_add(frames, stride).numpy()
    got = CC.overlap_add([f.numpy() for f in frames], stride)
    assert got.shape == want.shape == (2, 2, stride * (len(lengths) - 1) + lengths[-1])
    assert rel_err(got, want) < 2e-6                      # the float32 arithmetic of the port (its linspace, its sums)
    # the float32 restatement is the same formula: as close to float64 as the port is
    assert rel_err(CC.overlap_add([f.numpy() for f in frames], stride, dtype=np.float32), got) < 2e-6


@pytest.mark.parametrize("pads", [(3, 3), (1, 1), (4, 4 + 6)], ids=str)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_pad1d_matches_the_port(n, pads):
    pytest.importorskip("transformers")
    from transformers.models.encodec.modeling_encodec import EncodecConv1d
    x = torch.arange(1.0, 1.0 + 2 * 3 * n).reshape(2, 3, n)
    want = EncodecConv1d._pad1d(x, pads, mode="reflect").numpy()
    got = CC.pad1d(x.numpy(), *pads)
    assert got.shape == want.shape == (2, 3, n + sum(pads))
    assert np.array_equal(got, want)


def test_pad1d_small_input_rule_by_hand():
    """2 samples, padding (3, 3): zero-extend to x0 x1 0 0, reflect 3 either side, drop the last 2"""
    assert CC.pad1d(np.array([5.0, 7.0]), 3, 3).tolist() == [0.0, 0.0, 7.0, 5.0, 7.0, 0.0, 0.0, 0.0]
    # longer than the padding: numpy's reflect
    x = np.arange(1.0, 6.0)
    assert np.array_equal(CC.pad1d(x, 3, 4), np.pad(x, (3, 4), mode="reflect"))


def test_restated_blocks_equal_the_oracle_where_it_applies():
    from oracle import encodec_oracle as EO
    p = CC.dec_params()
    emb = CC.fill_normal("codec_segments.emb.check", (1, 128, 5), 3)
    assert np.array_equal(CC.seanet_decoder(p, emb), EO.seanet_decoder(p, emb))


# ------------------------------------------------------------------ golden
def test_oracle_decoder_and_overlap_add_match_the_ports_decode():
    from oracle import encodec_oracle as EO
    g = golden("codec_segments")
    codes, scales = CC.golden_codes_and_scales()
    p, tables = CC.dec_params(), CC.tables(CC.GOLDEN_NQ)
    frames = [EO.seanet_decoder(p, EO.rvq_decode(codes[s].transpose(1, 0, 2), tables)) for s in range(len(CC.GOLDEN_COUNTS))]
    y = CC.overlap_add(frames, CC.GOLDEN_STRIDE, scales[:, :, 0].T)
    assert y.shape == g["decode.y"].shape == (2, 2, 11442)
    assert rel_err(y, g["decode.y"]) < 1e-4


# ------------------------------------------------------------------ scale policy
def test_known_segment_scales_policy():
    from jen1_amd.generation import known_segment_scales
    from jen1_amd.tasks import get_mask
    L, stride, N = 100, 90, 400
    segs = [(off, min(L, N - off)) for off in range(0, N, stride)]             # offsets 0, 90, 180, 270, 360 (the last 40 long)
    scales = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0], [0.5, 0.25, 2.0, 1.0, 8.0]])
    keep = get_mask(N, 2.0, 4.0, 2, sample_rate=100)                           # generated: samples 200 .. 399
    got = known_segment_scales(scales, keep, segs)
    # segments 0 (0..100) and 1 (90..190) are wholly kept; 2 (180..280) straddles the border; 3 and 4 are generated
    fill = torch.sqrt((scales[:, :2] ** 2).mean(dim=1))
    want = scales.clone()
    want[:, 2:] = fill[:, None]
    assert torch.allclose(got, want, rtol=1e-6, atol=0)
    assert torch.equal(got[:, :2], scales[:, :2])
    assert np.allclose(CC.known_scales(scales.numpy(), keep[0, 0].numpy(), segs), got.numpy(), rtol=1e-6, atol=0)
    # inpainting the middle: the kept segments lie on both sides
    keep = get_mask(N, 1.0, 2.6, 2, sample_rate=100)                           # generated: 100 .. 259
    got = known_segment_scales(scales, keep[0, 0], segs)                       # (a plain [N] mask is accepted too)
    k = torch.tensor([True, False, False, True, True])                         # 0 .. 99 ends where the scope starts; 270 .. and 360 .. lie behind it
    fill = torch.sqrt((scales[:, k] ** 2).mean(dim=1))
    assert torch.equal(got[:, k], scales[:, k]) and torch.allclose(got[:, ~k], fill[:, None].expand(2, 2), rtol=1e-6, atol=0)
    # nothing wholly kept: unit scales
    assert torch.equal(known_segment_scales(scales, torch.zeros(N), segs), torch.ones_like(scales))
    assert np.array_equal(CC.known_scales(scales.numpy(), np.zeros(N), segs), np.ones((2, 5)))
    # everything kept: the encoder's own scales
    assert torch.equal(known_segment_scales(scales, torch.ones(N), segs), scales)
    with pytest.raises(ValueError, match="do not match"):
        known_segment_scales(scales[:, :4], keep, segs)


def test_generate_argument_errors_come_before_any_launch():
    from jen1_amd.generation import Jen1

    class Enc:                       # has no decode_latents
        channels = 2

    calls = []
    j = Jen1(None, device="cpu", audio_encoder=Enc(), conditioner=lambda meta, device: calls.append(1))
    with pytest.raises(ValueError, match="unknown decode"):
        j.generate("p", seed=1, steps=2, seconds=1, use_gdm=True, decode="frames")
    with pytest.raises(ValueError, match="unknown segment_scales"):
        j.generate("p", seed=1, steps=2, seconds=1, use_gdm=True, decode="segments", segment_scales="rms")
    with pytest.raises(ValueError, match="decode_latents"):
        j.generate("p", seed=1, steps=2, seconds=1, use_gdm=True, decode="segments")
    with pytest.raises(ValueError, match="needs decode='segments'"):
        j.generate("p", seed=1, steps=2, seconds=1, use_gdm=True, task="music_cont", segment_scales="known")

    class Enc2(Enc):
        def decode_latents(self, *a, **k):
            raise AssertionError("not reached")
    j = Jen1(None, device="cpu", audio_encoder=Enc2(), conditioner=lambda meta, device: calls.append(1))
    with pytest.raises(ValueError, match="needs known audio"):
        j.generate("p", seed=1, steps=2, seconds=1, use_gdm=True, task="text_guided", decode="segments", segment_scales="known")
    assert not calls


# ------------------------------------------------------------------ segment counts
def test_segment_frame_counts():
    from jen1_amd.encodec import segment_frame_counts, segment_lengths
    counts = segment_frame_counts(480000, 48000, 47520)
    assert len(counts) == 11 and sum(counts) == 1515 and counts == [150] * 10 + [15]
    assert segment_frame_counts(48000, 48000, 47520) == [150, 2]
    assert segment_frame_counts(96000, 48000, 47520) == [150, 150, 3]
    assert segment_frame_counts(95100, 48000, 47520) == [150, 149, 1]
    assert segment_lengths(95100, 48000, 47520) == CC.segment_lengths(95100, 48000, 47520) == [48000, 47580, 60]
    # the overlap-add of those segments covers the clip: stride (S - 1) + 320 T_last >= N
    for n in (480000, 48000, 96000, 95100, 47520, 47521):
        c = segment_frame_counts(n, 48000, 47520)
        assert 47520 * (len(c) - 1) + 320 * c[-1] >= n
