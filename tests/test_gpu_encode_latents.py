"""-m gpu: ``EncodecHIP.encode_latents`` / ``ResidualVectorQuantizerHIP.quantize`` (the fused residual search, jen1_rvq_encode) against
the path they shorten -- ``encode`` to codes, ``quantizer.decode`` of the concatenated codes -- on the synthetic codec of
tests/encodec_common.py, and ``Jen1(latents="fused")`` on top of them.

The two paths search with different float32 arithmetic (a GEMM's summation order against the fused kernel's), so a frame whose two best
entries score within rounding of each other may get different codes; tests/test_gpu_rvq_encode.py bounds how often the float64 reference
itself cannot tell (under 5 % of cells at 16 x 1024).  Here: segment frames and scales are equal, the latents are bit-equal on every frame
whose codes agree, and fewer than 5 % of the frames have codes that differ.

The comparison runs the float32 encoder.  Two runs of the same encoder pass are not bit-identical in either mode (its convolutions split K
over workgroups with float atomics): measured on MI355X, the 128-channel output of two runs differs by 5e-6 in float32, where no frame's
codes moved, and by 3e-2 in bf16, where 7 - 12 % of the frames got other codes -- that is the encoder twice, not the search, which gave
equal codes on 100 % of the frames of tools/rvq_encode_bench.py's shapes when both paths were handed the same tensor.
"""
import contextlib

import numpy as np
import pytest
import torch

import encodec_common as EC
import rvq_encode_common as RC
from helpers import record_parity
from jen1_amd.init_fill import fill_normal

pytestmark = pytest.mark.gpu

DIFFER_CAP = 0.05


def _codec(mode):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.encodec import EncodecHIP, ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    dec = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in EC.dec_params().items()}, compute_dtype=mode)
    enc = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in EC.enc_params().items()}, compute_dtype=mode)
    quant = ResidualVectorQuantizerHIP(torch.from_numpy(RC.golden_tables(16)))
    return EncodecHIP(dec, quant, encoder=enc)


@pytest.fixture(scope="module")
def codec():
    return _codec("bf16")


@pytest.fixture(scope="module")
def codec_f32():
    return _codec("f32")


def _jen1(codec, **kw):
    from jen1_amd import synth
    from jen1_amd.config import GDMConfig, tiny_model_config
    from jen1_amd.generation import Jen1
    cond = synth.conditioning(2, 300, "text_guided")
    emb, msk = torch.from_numpy(cond["cross_attn_cond"]).cuda(), torch.from_numpy(cond["cross_attn_masks"]).cuda()
    return Jen1(None, device="cuda", audio_encoder=codec, conditioner=lambda md, device: {"prompt": (emb[:len(md)], msk[:len(md)])},
                model_config=tiny_model_config(), diffusion_config=GDMConfig(), compute_dtype="bf16", **kw)


@contextlib.contextmanager
def recorded_searches(quant):
    """every ``quantize_into`` call of the block, as (emb, B_out, t0)"""
    calls = []
    inner = quant.quantize_into

    def spy(emb, n_q, codes, latents, B_out, t0):
        calls.append((emb.clone(), B_out, t0))
        return inner(emb, n_q, codes, latents, B_out, t0)

    quant.quantize_into = spy
    try:
        yield calls
    finally:
        del quant.quantize_into


@pytest.mark.parametrize("n,counts", [(48000, [150, 2]), (72000, [150, 77]), (118560, [150, 150, 74])], ids=["1.0s", "1.5s", "2.47s"])
def test_encode_latents_vs_get_emb_segments(codec_f32, n, counts):
    codec = codec_f32
    B = 2
    audio = torch.from_numpy(fill_normal(f"encode_latents.audio.{n}", (B, 2, n), 7) * np.array([0.2, 0.7], dtype=np.float32).reshape(2, 1, 1)).cuda()
    seen = {}
    inner = codec.encode
    codec.encode = lambda a: seen.setdefault("frames", inner(a))
    try:
        want, want_counts, want_scales = _jen1(codec).get_emb_segments(audio)
    finally:
        del codec.encode
    with recorded_searches(codec.quantizer) as calls:
        got, got_counts, got_scales = codec.encode_latents(audio)
    assert got_counts == want_counts == counts
    assert got.shape == want.shape == (B, 128, sum(counts)) and got.dtype == want.dtype and got.device == want.device
    assert got_scales.shape == want_scales.shape == (B, len(counts)) and torch.equal(got_scales, want_scales) and got_scales.device == want_scales.device
    # the codes behind the fused latents: the same search again, codes only, into the same time slots
    fused_codes = torch.full((16, B, sum(counts)), -1, dtype=torch.int64, device="cuda")
    for emb, B_out, t0 in calls:
        codec.quantizer.quantize_into(emb, None, fused_codes, None, B_out, t0)
    assert int(fused_codes.min()) >= 0
    assert torch.equal(codec.quantizer.decode(fused_codes), got), "the latents are not the decode of the fused search's own codes"
    plain_codes = torch.cat([c for c, _ in seen["frames"]], dim=-1).permute(1, 0, 2)                      # [n_q, B, T']
    same = (plain_codes == fused_codes).all(dim=0)                                                       # [B, T']
    differ = 1.0 - float(same.float().mean())
    record_parity("encode_latents", f"n{n}", "f32", frames_that_differ=differ)
    print(f"encode_latents n={n}: share of frames whose codes differ {differ:.5f}")
    sel = same[:, None, :].expand_as(got)
    assert torch.equal(got[sel].view(torch.int32), want[sel].view(torch.int32))
    assert differ < DIFFER_CAP, differ


def test_quantize_outputs(codec):
    q = codec.quantizer
    emb = torch.from_numpy(RC.frames(3, 37, key="encode_latents.quantize")).cuda()
    codes, z = q.quantize(emb)
    assert codes.shape == (16, 3, 37) and codes.dtype == torch.int64 and z.shape == (3, 128, 37) and codes.device == z.device and z.device.type == q.device.type
    assert torch.equal(q.decode(codes).view(torch.int32), z.view(torch.int32))
    c8, none = q.quantize(emb, 8, latents=False)
    assert none is None and torch.equal(c8, codes[:8])
    none, z8 = q.quantize(emb, 8, codes=False)
    assert none is None and torch.equal(z8.view(torch.int32), q.decode(c8).view(torch.int32))
    with pytest.raises(ValueError):
        q.quantize(emb, codes=False, latents=False)


def test_quantize_in_a_captured_graph(codec):
    from jen1_amd import graphs
    q = codec.quantizer
    first = torch.from_numpy(RC.frames(2, 45, key="encode_latents.graph.a")).cuda()
    second = torch.from_numpy(RC.frames(2, 45, key="encode_latents.graph.b")).cuda()
    want_first, want_second = q.quantize(first), q.quantize(second)           # (also the launch that sets the kernel's LDS attribute)
    torch.cuda.synchronize()
    static = first.clone()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with graphs.capture(g):
            codes, z = q.quantize(static)
    torch.cuda.current_stream().wait_stream(s)
    for data, want in ((first, want_first), (second, want_second), (first, want_first)):
        static.copy_(data)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(codes, want[0]) and torch.equal(z.view(torch.int32), want[1].view(torch.int32))


@contextlib.contextmanager
def fixed_order(m):
    """the sampler's bit-reproducible mode (no float-atomic statistics), as in tests/test_gpu_known_blend.py"""
    old = m.deterministic
    m.deterministic = True
    try:
        yield
    finally:
        m.deterministic = old


def test_generate_with_fused_latents(codec):
    """music_cont from 1.2 s of audio: ``latents="fused"`` asks ``encode_latents`` (and never ``encode``) for the known latents, and the
    sampler ends on the bits it ends on when the same instance, set back to ``"codes"``, is handed that ``encode_latents`` result by hand
    (compared where the sampler hands over to the decoder)"""
    prefix = torch.from_numpy(fill_normal("encode_latents.prefix", (2, 2, 57600), 5) * np.array([0.1, 0.6], dtype=np.float32).reshape(2, 1, 1))
    kw = dict(seed=3, steps=2, batch_size=2, seconds=2, use_gdm=True, task="music_cont", init_audio=prefix, preserve_known=True,
              decode="segments", segment_scales="known")
    with pytest.raises(ValueError):
        _jen1(codec, latents="other")
    assert _jen1(codec).latents == "codes"
    j = _jen1(codec, latents="fused")
    seen, sampled = [], []
    inner, inner_decode = codec.encode_latents, codec.decode_latents
    codec.encode_latents = lambda a: (seen.append(inner(a)), seen[-1])[1]
    codec.decode_latents = lambda z, counts, **k: (sampled.append(z.clone()), inner_decode(z, counts, **k))[1]

    def no_encode(a):
        raise AssertionError("latents='fused' went through encode")

    codec.encode = no_encode
    try:
        _, model = j.get_model_and_diffusion(2, True)
        with fixed_order(model):
            got = j.generate("strings", **kw)
            assert len(seen) == 1 and seen[0][1] == [150, 150, 3] and len(sampled) == 1
            assert tuple(got.shape) == (2, 2, 96000) and torch.isfinite(got).all() and float(got.abs().max()) > 0
            j.latents = "codes"
            j.get_emb_segments = lambda a: seen[0]
            want = j.generate("strings", **kw)
            del j.get_emb_segments
        assert len(seen) == 1 and len(sampled) == 2 and want.shape == got.shape
        assert torch.equal(sampled[0].view(torch.int32), sampled[1].view(torch.int32))
        # get_emb: the latents alone
        j.latents = "fused"
        audio = prefix[:, :, :30000].cuda()
        z = j.get_emb(audio)
        assert len(seen) == 2 and z is seen[1][0] and z.shape == (2, 128, 94) and z.device == audio.device
    finally:
        del codec.encode_latents, codec.decode_latents, codec.encode
