"""-m gpu: the codec's segment path -- the kernels jen1_codec_overlap_add / _segment_scales / _segment_cut / _pad1d of csrc/encodec.hip
through the C ABI, the small-input convolutions, ``EncodecHIP.encode`` / ``decode`` / ``decode_latents`` and
``Jen1.generate(decode="segments")`` -- against the float64 restatements of tests/codec_segments_common.py (pinned on the CPU by
tests/test_codec_segments_host.py) and the stored output of the Hugging Face port's ``decode`` (tests/golden/codec_segments.npz).

Overlap-add gate, per element: ``|out - ref| <= 8 e``, e = the largest error of a float32 numpy restatement of the same sums against the
float64 one on the same rows (bf16 rows: both read the bf16-rounded values; the output is float32, so there is no rounding term).
Every output buffer is pre-filled with a sentinel and carries a guard region that must come back untouched.
"""
import numpy as np
import pytest
import torch

import codec_segments_common as CC
from encodec_common import _p64, bf16_round
from helpers import BF16_TOL, F32_TOL, golden, record_parity, rel_err

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16"]
TOL = {"f32": F32_TOL, "bf16": BF16_TOL}
SENTINEL = -7.25                # exact in bf16
JUNK = 3.0e4                    # padding columns of the rows the overlap-add reads: finite, and no result may depend on them
GUARD = 64
MARGIN = 8.0                    # x the float32 restatement's own error


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import lib as L
    return L.load()


def _sync_check(rc, what):
    from jen1_amd import lib as L
    L.check(rc, what)
    torch.cuda.synchronize()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _is_sentinel(t: torch.Tensor) -> bool:
    return bool(torch.equal(_bits(t), _bits(torch.full_like(t, SENTINEL))))


def _tdt(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _dt(mode):
    from jen1_amd import lib as L
    return L.BF16 if mode == "bf16" else L.F32


# ---------------------------------------------------------------------------------------------------------------------
# overlap-add kernel
# ---------------------------------------------------------------------------------------------------------------------
OLA_CASES = {
    # name: (L_0, stride, frame lengths)
    "short_last": (640, 608, [640, 640, 96]),
    "three_overlap": (640, 200, [640] * 4),
    "no_overlap": (640, 640, [640, 640]),
    "one_frame": (640, 608, [640]),
    "last_inside_previous": (640, 608, [640, 640, 20]),           # 1216 .. 1236 lies inside frame 1 (608 .. 1248)
    "two_short": (640, 493, [640, 500, 7]),                       # 993 samples cut every 493: the second-to-last frame is short too
    "odd_stride": (640, 601, [640, 640, 640]),
}


def _ola_once(lib, segs_d, S, scale_d, B, C, n_out, stride, L0, L_last, mode):
    whole = torch.full((B * C * n_out + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    _sync_check(lib.jen1_codec_overlap_add(segs_d.data_ptr(), S, None if scale_d is None else scale_d.data_ptr(), whole.data_ptr(), B, C, 8,
                                           n_out, stride, L0, L_last, _dt(mode), _stream()), "jen1_codec_overlap_add")
    assert _is_sentinel(whole[B * C * n_out:]), "written past the end of out"
    return whole[:B * C * n_out].view(B, C, n_out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", list(OLA_CASES))
def test_overlap_add_kernel(lib, case, mode):
    from jen1_amd import lib as L
    L0, stride, lengths = OLA_CASES[case]
    S = len(lengths)
    total = stride * (S - 1) + lengths[-1]
    for C in (1, 2):
        for B in (1, 3):
            g = torch.Generator().manual_seed(1000 * C + 10 * B + S + stride)
            frames = [torch.randn((B, C, n), generator=g).numpy() for n in lengths]
            if mode == "bf16":
                frames = [bf16_round(f) for f in frames]                           # what the kernel reads
            scales = (torch.rand((B, S), generator=g) * 1.5 + 0.25).numpy()
            # rows as the decoder leaves them: frames of equal length share one tensor [n B][L][8], frame j of sample b is row j B + b
            by_len = {}
            for s, n in enumerate(lengths):
                by_len.setdefault(n, []).append(s)
            table, held = [None] * S, []
            for n, segs in by_len.items():
                rows = torch.full((len(segs) * B, n, 8), JUNK, dtype=_tdt(mode), device="cuda")
                for j, s in enumerate(segs):
                    rows[j * B:(j + 1) * B, :, :C] = torch.from_numpy(frames[s]).transpose(1, 2).to(_tdt(mode))
                    table[s] = (rows.data_ptr(), j * B, n)
                held.append(rows)
            segs_d = L.ola_seg_table(table, "cuda")
            for with_scale in (False, True):
                sc = scales if with_scale else None
                ref = CC.overlap_add(frames, stride, sc)
                emul_err = float(np.abs(CC.overlap_add(frames, stride, sc, dtype=np.float32) - ref).max())
                assert emul_err < 1e-5
                bound = MARGIN * emul_err
                scale_d = torch.from_numpy(scales).cuda() if with_scale else None
                out = _ola_once(lib, segs_d, S, scale_d, B, C, total, stride, L0, lengths[-1], mode)
                again = _ola_once(lib, segs_d, S, scale_d, B, C, total, stride, L0, lengths[-1], mode)
                assert torch.equal(_bits(out), _bits(again)), "two runs differ"
                got = out.cpu().numpy().astype(np.float64)
                assert np.isfinite(got).all()
                err = np.abs(got - ref)
                name = f"{case}.C{C}.B{B}.{'scaled' if with_scale else 'unit'}"
                record_parity("codec_overlap_add", name, mode, max_err=err.max(), emul_err=emul_err, bound=bound, max_ref=np.abs(ref).max())
                print(f"codec_overlap_add {name} {mode}: max|out-ref| {err.max():.3e} restatement {emul_err:.3e} bound {bound:.3e}")
                assert (err <= bound).all(), (name, mode, float(err.max()), bound)
                # the trim: fewer samples than the frames cover are the head of the same result
                n_out = max(1, total - 37)
                head = _ola_once(lib, segs_d, S, scale_d, B, C, n_out, stride, L0, lengths[-1], mode)
                assert torch.equal(_bits(head), _bits(out[:, :, :n_out])), "the trimmed output is not the head of the full one"


def test_overlap_add_rejects_bad_arguments(lib):
    from jen1_amd import lib as L
    rows = torch.zeros((1, 640, 8), device="cuda")
    segs = L.ola_seg_table([(rows.data_ptr(), 0, 640), (rows.data_ptr(), 0, 640)], "cuda")
    out = torch.full((2 * 1248 + GUARD,), SENTINEL, device="cuda")
    call = lambda **k: lib.jen1_codec_overlap_add(segs.data_ptr(), k.get("S", 2), None, out.data_ptr(), 1, k.get("C", 2), k.get("ld", 8),     # noqa: E731
                                                  k.get("n_out", 1248), k.get("stride", 608), 640, k.get("L_last", 640), k.get("dt", L.F32), _stream())
    assert call() == 0
    for bad in (dict(n_out=1249), dict(n_out=0), dict(C=9), dict(C=0), dict(ld=16), dict(stride=641), dict(stride=0), dict(L_last=641), dict(S=0),
                dict(dt=L.FP8)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert _is_sentinel(out[2 * 1248:])


# ---------------------------------------------------------------------------------------------------------------------
# segment scales and cut
# ---------------------------------------------------------------------------------------------------------------------
SEG_L, SEG_STRIDE, SEG_N = 640, 608, 640 * 2 + 37            # segments of 640, 640 and 101 samples


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_segment_scales_and_cut(lib, mode, C, normalize):
    B = 2
    lengths = CC.segment_lengths(SEG_N, SEG_L, SEG_STRIDE)
    assert lengths == [640, 640, 101]
    S = len(lengths)
    g = torch.Generator().manual_seed(50 + C)
    audio = (torch.randn((B, C, SEG_N), generator=g) * torch.tensor([0.3, 2.0]).view(B, 1, 1)).cuda()
    scale_buf = torch.full((B * S + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    _sync_check(lib.jen1_codec_segment_scales(audio.data_ptr(), scale_buf.data_ptr(), B, C, SEG_N, SEG_L, SEG_STRIDE, S, _stream()),
                "jen1_codec_segment_scales")
    assert _is_sentinel(scale_buf[B * S:])
    scale = scale_buf[:B * S].view(B, S)
    again = torch.full_like(scale_buf, SENTINEL)
    _sync_check(lib.jen1_codec_segment_scales(audio.data_ptr(), again.data_ptr(), B, C, SEG_N, SEG_L, SEG_STRIDE, S, _stream()), "jen1_codec_segment_scales")
    assert torch.equal(_bits(scale_buf), _bits(again)), "two runs differ"
    want = CC.segment_scales(audio.cpu().numpy(), SEG_L, SEG_STRIDE)
    rel = np.abs(scale.cpu().numpy().astype(np.float64) - want) / want
    record_parity("codec_segment_scales", f"C{C}", "f32", worst_rel=rel.max())
    assert (rel < 1e-6).all(), float(rel.max())
    tdt = _tdt(mode)
    for s0, n_sel in ((0, 2), (2, 1), (1, 1)):
        n = lengths[s0]
        rows_buf = torch.full((n_sel * B * n * 8 + GUARD,), SENTINEL, dtype=tdt, device="cuda")
        _sync_check(lib.jen1_codec_segment_cut(audio.data_ptr(), scale.data_ptr() if normalize else None, rows_buf.data_ptr(), B, C, SEG_N, n,
                                               SEG_STRIDE, S, s0, n_sel, _dt(mode), _stream()), "jen1_codec_segment_cut")
        assert _is_sentinel(rows_buf[n_sel * B * n * 8:]), "written past the end of the rows"
        rows = rows_buf[:n_sel * B * n * 8].view(n_sel, B, n, 8)
        assert float(rows[..., C:].float().abs().max()) == 0.0, "padding columns must be zero"
        for j in range(n_sel):
            off = (s0 + j) * SEG_STRIDE
            x = audio[:, :, off: off + n]
            if normalize:
                x = x / scale[:, s0 + j].view(B, 1, 1)                             # the torch expression of EncodecHIP.encode's loop
            expect = x.transpose(1, 2).to(tdt)
            assert torch.equal(_bits(rows[j, :, :, :C]), _bits(expect)), (s0, j)


def test_segment_kernels_reject_bad_arguments(lib):
    from jen1_amd import lib as L
    audio = torch.zeros((1, 2, SEG_N), device="cuda")
    scale = torch.zeros((1, 3), device="cuda")
    rows = torch.full((2 * 640 * 8 + GUARD,), SENTINEL, device="cuda")
    cut = lambda L_=640, s0=0, n=2, S=3, C=2, dt=L.F32: lib.jen1_codec_segment_cut(audio.data_ptr(), None, rows.data_ptr(), 1, C, SEG_N, L_,       # noqa: E731
                                                                                  SEG_STRIDE, S, s0, n, dt, _stream())
    assert cut() == 0
    assert cut(s0=1) != 0                 # segments 1 and 2: the second one is not 640 long
    assert cut(s0=2, n=1) != 0            # segment 2 has 101 samples
    assert cut(L_=101, s0=2, n=1) == 0
    assert cut(n=0) != 0 and cut(s0=-1) != 0 and cut(s0=3, n=1) != 0 and cut(C=9) != 0 and cut(dt=L.FP8) != 0 and cut(L_=0) != 0
    assert lib.jen1_codec_segment_scales(audio.data_ptr(), scale.data_ptr(), 1, 2, SEG_N, SEG_L, SEG_STRIDE, 4, _stream()) != 0   # segment 3 starts past the end
    assert lib.jen1_codec_segment_scales(audio.data_ptr(), scale.data_ptr(), 1, 2, SEG_N, SEG_L, 0, 3, _stream()) != 0
    x = torch.zeros((1, 2, 8), device="cuda")
    assert lib.jen1_codec_pad1d(x.data_ptr(), rows.data_ptr(), 1, 2, 8, 3, 3, L.F32, _stream()) == 0
    for bad in ((1, 2, 12, 3, 3), (1, 0, 8, 3, 3), (1, 2, 8, -1, 3), (0, 2, 8, 3, 3)):
        assert lib.jen1_codec_pad1d(x.data_ptr(), rows.data_ptr(), *bad, L.F32, _stream()) != 0, bad
    torch.cuda.synchronize()
    assert _is_sentinel(rows[2 * 640 * 8:])


# ---------------------------------------------------------------------------------------------------------------------
# pad1d and the small-input convolutions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pads", [(3, 3), (1, 1), (4, 10), (0, 2)], ids=str)
@pytest.mark.parametrize("n", [1, 2, 3, 9])
def test_pad1d_kernel(lib, mode, n, pads):
    rows, ld = 3, 16
    tdt = _tdt(mode)
    x = torch.arange(1.0, 1.0 + rows * n * ld).reshape(rows, n, ld).to(tdt).cuda()       # (integers up to 432: exact in bf16 up to 256, rounded above)
    n_p = n + sum(pads)
    buf = torch.full((rows * n_p * ld + GUARD,), SENTINEL, dtype=tdt, device="cuda")
    _sync_check(lib.jen1_codec_pad1d(x.data_ptr(), buf.data_ptr(), rows, n, ld, pads[0], pads[1], _dt(mode), _stream()), "jen1_codec_pad1d")
    assert _is_sentinel(buf[rows * n_p * ld:])
    got = buf[:rows * n_p * ld].view(rows, n_p, ld).float().cpu().numpy()
    want = CC.pad1d(x.float().cpu().numpy().transpose(0, 2, 1), *pads).transpose(0, 2, 1)
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def nets():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.encodec import ResidualVectorQuantizerHIP, SEANetDecoderHIP, SEANetEncoderHIP
    dp, ep = CC.dec_params(), CC.enc_params()
    out = {"dec_p": dp, "enc_p": ep, "tables": CC.tables(16)}
    for mode in MODES:
        out["dec", mode] = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in dp.items()}, compute_dtype=mode)
        out["enc", mode] = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in ep.items()}, compute_dtype=mode)
    out["quant"] = ResidualVectorQuantizerHIP(torch.from_numpy(out["tables"]))
    return out


def _model(nets, mode, **kw):
    from jen1_amd.encodec import EncodecHIP
    return EncodecHIP(nets["dec", mode], nets["quant"], encoder=nets["enc", mode], **kw)


# (which net, layer, stride): the k = 7 convolution in front of the decoder's LSTM, and the encoder's last down-sampling convolution
TINY_CONVS = [("dec", "layers.0", 1), ("enc", "layers.12", 8)]


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("which,name,stride", TINY_CONVS)
@pytest.mark.parametrize("mode", MODES)
def test_tiny_input_convolutions(nets, mode, which, name, stride, n):
    """``_conv(tiny=True)`` on fewer frames than the reflect padding: pad1d's small-input rule, against float64"""
    net, p = nets[which, mode], nets[which + "_p"]
    co, ci, k = p[f"{name}.conv.weight"].shape
    assert k == (7 if stride == 1 else 2 * stride)
    g = torch.Generator().manual_seed(700 + 10 * n + stride)
    x = net._to_rows(torch.randn((2, ci, n), generator=g).to(net.device))
    x64 = x[:, :, :ci].float().cpu().numpy().astype(np.float64).transpose(0, 2, 1)
    with pytest.raises(NotImplementedError):
        net._conv(x, name, stride=stride)                          # without tiny=True the guard of the index-map form stays
    y = net._conv(x, name, stride=stride, tiny=True)
    torch.cuda.synchronize()
    y = y.float().cpu().numpy().astype(np.float64)
    assert y.shape[-1] == co or float(np.abs(y[:, :, co:]).max()) == 0.0
    got = y[:, :, :co].transpose(0, 2, 1)
    ref = CC.sconv1d(x64, _p64(p, name, mode == "bf16"), name, stride)
    assert ref.dtype == np.float64 and got.shape == ref.shape == (2, co, -(-n // stride))
    e = rel_err(got, ref)
    record_parity("codec_tiny_conv", f"{which}.{name}.s{stride}.L{n}", mode, rel_err=e)
    assert np.isfinite(got).all() and e < TOL[mode], (which, name, n, mode, e)


@pytest.fixture(scope="module")
def clips(nets):
    """1 s and 2 s of audio, their encode by the float32 model and the restated encode, computed once"""
    out = {}
    model = _model(nets, "f32")
    for seconds in (1, 2):
        audio = CC.fill_normal(f"codec_segments.audio.{seconds}s", (1, 2, 48000 * seconds), 7) * 0.2
        out[seconds] = (audio, model.encode(torch.from_numpy(audio)), CC.encode_frames(nets["enc_p"], nets["tables"], audio, 48000, 47520))
    return out


@pytest.mark.parametrize("seconds,counts", [(1, [150, 2]), (2, [150, 150, 3])])
def test_encode_of_whole_seconds(nets, clips, seconds, counts):
    """a clip of exactly 1 s / 2 s ends in a segment of 480 / 960 samples = 2 / 3 frames, which the encoder's last convolution can only
    pad by the small-input rule.  The codes of a clip are compared the way tests/test_encodec.py does, as an agreement rate (pooled over
    the clip: the short segments hold 32 and 48 codes, where one flipped nearest-neighbour tie would already be 3 %); the latents of
    the short segment are compared directly."""
    audio, frames, want = clips[seconds]
    assert [int(c.shape[-1]) for c, _ in frames] == [int(c.shape[-1]) for c, _ in want] == counts
    for (c, s), (cw, sw) in zip(frames, want):
        assert tuple(c.shape) == cw.shape == (1, 16, cw.shape[-1]) and tuple(s.shape) == (1, 1)
        assert rel_err(s.numpy(), sw) < 1e-6
    agree = np.concatenate([(c.numpy() == cw).reshape(-1) for (c, _), (cw, _) in zip(frames, want)]).mean()
    record_parity("codec_encode_whole_seconds", f"{seconds}s", "f32", agreement=agree)
    print(f"codec_encode_whole_seconds {seconds}s: code agreement {agree:.5f}")
    assert agree > 0.995, agree
    off = 47520 * (len(counts) - 1)
    x = audio[:, :, off:] / want[-1][1].reshape(1, 1, 1).astype(np.float32)
    got = nets["enc", "f32"](torch.from_numpy(x)).numpy()
    ref = CC.seanet_encoder(nets["enc_p"], x)
    assert got.shape == ref.shape == (1, 128, counts[-1])
    assert rel_err(got, ref) < F32_TOL


# ---------------------------------------------------------------------------------------------------------------------
# EncodecHIP.decode / decode_latents / encode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_decode_vs_the_ports_decode(nets, mode):
    want = golden("codec_segments")["decode.y"]
    codes, scales = CC.golden_codes_and_scales()
    model = _model(nets, mode, segment=CC.GOLDEN_SEGMENT_S, overlap=CC.GOLDEN_OVERLAP)
    assert (model.segment_length, model.segment_stride) == (CC.GOLDEN_CHUNK, CC.GOLDEN_STRIDE)
    frames = [(torch.from_numpy(codes[s]), torch.from_numpy(scales[s])) for s in range(codes.shape[0])]
    y = model.decode(frames)
    assert y.device.type == "cpu" and y.dtype == torch.float32 and tuple(y.shape) == want.shape == (2, 2, 11442)
    e = rel_err(y.numpy(), want)
    record_parity("codec_decode_golden", "3x12", mode, rel_err=e)
    assert e < TOL[mode], (mode, e)
    # frames without scales decode at unit scale
    y1 = model.decode([(c, None) for c, _ in frames])
    ones = model.decode([(c, torch.ones_like(s)) for c, s in frames])
    assert rel_err(y1.numpy(), ones.numpy()) < TOL[mode]          # (two decoder passes: their split-K sums are not ordered)


# (overlap, frame counts, samples of the clip that cuts into them): with overlap 0.01 the stride is 3801 samples, more than 11 frames,
# so a short second-to-last segment needs a larger overlap (0.1: stride 3456)
RAGGED = [(0.01, (12, 12, 5), 3801 * 2 + 1500), (0.1, (12, 11, 1), 3456 * 2 + 38)]


@pytest.fixture(scope="module")
def ragged_refs(nets):
    out = {}
    for overlap, counts, n in RAGGED:
        stride = max(1, int((1 - overlap) * 3840))
        assert tuple(-(-m // 320) for m in CC.segment_lengths(n, 3840, stride)) == counts
        emb = CC.fill_normal(f"codec_segments.emb.{counts}", (2, 128, sum(counts)), 9)
        scales = CC.fill_uniform(f"codec_segments.scales.{counts}", (2, len(counts)), 9, 0.25, 1.75)
        ref, _ = CC.decode_latents(nets["dec_p"], emb, counts, stride, scales)
        out[counts] = (stride, emb, scales, ref)
    return out


@pytest.mark.parametrize("overlap,counts,n", RAGGED, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("mode", MODES)
def test_decode_latents_ragged(nets, ragged_refs, mode, overlap, counts, n):
    stride, emb, scales, ref = ragged_refs[counts]
    model = _model(nets, mode, segment=0.08, overlap=overlap)
    assert (model.segment_length, model.segment_stride) == (3840, stride) and model.segment_frames(n) == list(counts)
    total = stride * 2 + 320 * counts[-1]
    y = model.decode_latents(torch.from_numpy(emb).cuda(), counts, torch.from_numpy(scales))
    assert y.device.type == "cuda" and tuple(y.shape) == ref.shape == (2, 2, total)
    e = rel_err(y.cpu().numpy(), ref)
    record_parity("codec_decode_latents", "-".join(map(str, counts)), mode, rel_err=e)
    assert torch.isfinite(y).all() and e < TOL[mode], (mode, counts, e)
    cut = model.decode_latents(torch.from_numpy(emb).cuda(), counts, torch.from_numpy(scales), length=n)
    assert tuple(cut.shape) == (2, 2, n) and rel_err(cut.cpu().numpy(), ref[:, :, :n]) < TOL[mode]
    for bad in (dict(segment_frames=counts[:-1]), dict(segment_frames=counts, length=total + 1), dict(segment_frames=counts, length=0),
                dict(segment_frames=counts, scales=torch.ones((2, 2)))):
        with pytest.raises(ValueError):
            model.decode_latents(torch.from_numpy(emb).cuda(), **bad)
    if overlap == 0.1:               # the same counts under the 1 % overlap would leave samples 7321 .. 7601 uncovered
        with pytest.raises(ValueError, match="covers"):
            _model(nets, mode, segment=0.08).decode_latents(torch.from_numpy(emb).cuda(), counts)


def test_batched_encode_vs_the_loop(nets):
    """2.5 short segments, B = 2: one encoder pass per run of equal-length segments against one pass per segment.  Segments of 0.5 s
    (75, 75 and 38 frames: 2400 and 1216 codes each), the sizes tests/test_encodec.py compares codes at: the rate has to leave room for
    one flipped near-tie, which changes every later codebook of its frame (up to 15 codes), and 0.5 % of a 6-frame segment leaves none."""
    model = _model(nets, "f32", segment=0.5)
    assert (model.segment_length, model.segment_stride) == (24000, 23760)
    n = 23760 * 2 + 12000
    audio = torch.from_numpy(CC.fill_normal("codec_segments.audio.half", (2, 2, n), 7) * np.array([0.2, 0.7], dtype=np.float32).reshape(2, 1, 1))
    assert model.encode_batched
    batched = model.encode(audio)
    model.encode_batched = False
    loop = model.encode(audio)
    model.encode_batched = True
    assert len(batched) == len(loop) == 3 and [int(c.shape[-1]) for c, _ in batched] == [75, 75, 38]
    for (c, s), (cw, sw) in zip(batched, loop):
        assert c.shape == cw.shape and c.dtype == cw.dtype and c.device == cw.device and s.shape == sw.shape == (2, 1)
        assert rel_err(s.numpy(), sw.numpy()) < 1e-6
        rate = float((c == cw).float().mean())
        record_parity("codec_batched_encode", f"T{int(c.shape[-1])}", "f32", agreement=rate)
        print(f"codec_batched_encode T={int(c.shape[-1])}: code agreement {rate:.5f}")
        assert rate >= 0.995, rate
    plain = _model(nets, "f32", segment=0.5, normalize=False)
    a = plain.encode(audio)
    plain.encode_batched = False
    b = plain.encode(audio)
    assert all(s is None and sw is None and (c == cw).float().mean() >= 0.995 for (c, s), (cw, sw) in zip(a, b))


def test_decode_latents_at_the_workload_shape(nets):
    """8 x 10 s in bf16: 10 segments of 150 frames and one of 15 per sample.  The 80 + 8 sequences stay on the multi-workgroup LSTM (no
    barrier time-out), and a segment decoded on its own gives the rows it gets in the batched pass (row j B + b of the pass over the
    ten equal-length segments, built here the way ``decode_latents`` builds it)."""
    dec = nets["dec", "bf16"]
    model = _model(nets, "bf16")
    counts = model.segment_frames(480000)
    assert len(counts) == 11 and sum(counts) == 1515 and 80 <= dec.lstm_multi_rows()
    emb = torch.from_numpy(CC.fill_normal("codec_segments.emb.workload", (8, 128, 1515), 4)).cuda()
    y = model.decode_latents(emb, counts, length=480000)                          # (raises on a barrier time-out: _check_lstm)
    assert tuple(y.shape) == (8, 2, 480000) and torch.isfinite(y).all() and float(y.abs().max()) > 0
    assert dec.lstm_multi and int(dec.last_lstm_counters[:, 1].sum()) == 0
    offs = np.concatenate([[0], np.cumsum(counts)])
    full = dec.rows(torch.cat([emb[:, :, offs[s]:offs[s + 1]] for s in range(10)], dim=0))           # [80, 48000, 8]
    tail = dec.rows(emb[:, :, offs[10]:])                                                             # [8, 4800, 8]
    dec._check_lstm()
    for s in (0, 5, 10):
        alone = dec(emb[3:4, :, offs[s]:offs[s + 1]])                              # [1, 2, 320 T_s]
        batched = (full[s * 8 + 3] if s < 10 else tail[3])[:, :2].float().t()
        assert tuple(alone.shape[1:]) == tuple(batched.shape) == (2, 320 * counts[s])
        e = rel_err(batched.cpu().numpy(), alone[0].cpu().numpy())
        record_parity("codec_workload_rows", f"segment{s}", "bf16", rel_err=e)
        assert e < BF16_TOL, (s, e)


def test_bf16_batched_encoder_is_as_close_to_the_restatement_as_the_loop(nets):
    """the latents behind the codes, bf16: the segment-batched pass and the one-pass-per-segment loop against the restated encoder on the
    same normalised segments, both under the bf16 gate -- the two forms differ from each other by bf16 rounding, not by a bias"""
    model = _model(nets, "bf16", segment=0.08)
    enc = nets["enc", "bf16"]
    n = 3801 * 2 + 1920
    audio = CC.fill_normal("codec_segments.audio.short", (2, 2, n), 7) * np.array([0.2, 0.7], dtype=np.float32).reshape(2, 1, 1)
    x = torch.from_numpy(audio).cuda()
    scale = model.segment_scales(x)
    lengths = CC.segment_lengths(n, 3840, 3801)
    batched = {0: enc.from_rows(model.segment_rows(x, scale, 0, 2, 3840)), 2: enc.from_rows(model.segment_rows(x, scale, 2, 1, 1920))}
    enc._check_lstm()
    for s, m in enumerate(lengths):
        seg = audio[:, :, s * 3801: s * 3801 + m] / scale[:, s].cpu().numpy().reshape(2, 1, 1)
        ref = CC.seanet_encoder(nets["enc_p"], seg)
        loop = enc(torch.from_numpy(seg)).numpy()
        got = (batched[0][s * 2:(s + 1) * 2] if s < 2 else batched[2]).cpu().numpy()
        e_b, e_l = rel_err(got, ref), rel_err(loop, ref)
        record_parity("codec_bf16_encoder_forms", f"segment{s}", "bf16", batched=e_b, loop=e_l, between=rel_err(got, loop))
        print(f"codec_bf16_encoder_forms segment {s}: batched {e_b:.3e} loop {e_l:.3e} vs the restatement")
        assert got.shape == ref.shape and e_b < BF16_TOL and e_l < BF16_TOL, (s, e_b, e_l)


# ---------------------------------------------------------------------------------------------------------------------
# Jen1.generate
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_decodes_segment_by_segment(nets):
    from jen1_amd import synth
    from jen1_amd.config import GDMConfig, tiny_model_config
    from jen1_amd.generation import Jen1
    enc = _model(nets, "bf16")
    cond = synth.conditioning(2, 300, "text_guided")
    emb, msk = torch.from_numpy(cond["cross_attn_cond"]).cuda(), torch.from_numpy(cond["cross_attn_masks"]).cuda()
    j = Jen1(None, device="cuda", audio_encoder=enc, conditioner=lambda md, device: {"prompt": (emb[:len(md)], msk[:len(md)])},
             model_config=tiny_model_config(), diffusion_config=GDMConfig(), compute_dtype="bf16")
    whole = j.generate("strings", seed=2, steps=2, batch_size=2, seconds=1, use_gdm=True)
    assert tuple(whole.shape) == (2, 2, 152 * 320) == (2, 2, 48640)              # the two segments' frames side by side
    wav = j.generate("strings", seed=2, steps=2, batch_size=2, seconds=1, use_gdm=True, decode="segments")
    assert tuple(wav.shape) == (2, 2, 48000) and wav.device.type == "cuda"
    assert torch.isfinite(wav).all() and float(wav.abs().max()) > 0
    # music_cont over 1.99 s (95520 samples: 150 + 150 + 2 frames, an even count for the network's down-sampling) from a prefix of 1.2 s:
    # segment 0 (0 .. 1 s) is wholly kept, segments 1 and 2 are not
    seen = {}
    inner_encode, inner_decode = enc.encode, enc.decode_latents
    enc.encode = lambda a: seen.setdefault("frames", inner_encode(a))
    enc.decode_latents = lambda z, counts, **kw: (seen.update(counts=list(counts), kw=kw), inner_decode(z, counts, **kw))[1]
    try:
        prefix = torch.from_numpy(CC.fill_normal("codec_segments.audio.prefix", (2, 2, 57600), 5) * np.array([0.1, 0.6], dtype=np.float32).reshape(2, 1, 1))
        out = j.generate("strings", seed=3, steps=2, batch_size=2, seconds=1.99, use_gdm=True, task="music_cont", init_audio=prefix,
                         preserve_known=True, decode="segments", segment_scales="known")
    finally:
        enc.encode, enc.decode_latents = inner_encode, inner_decode
    assert tuple(out.shape) == (2, 2, 95520) and torch.isfinite(out).all()
    assert seen["counts"] == [150, 150, 2] and seen["kw"]["length"] == 95520
    enc_scales = np.concatenate([s.cpu().numpy().reshape(2, 1) for _, s in seen["frames"]], axis=1)
    keep = np.ones(95520)
    keep[57600:] = 0
    want = CC.known_scales(enc_scales, keep, [(0, 48000), (47520, 48000), (95040, 480)])
    assert np.array_equal(want[:, 0], enc_scales[:, 0].astype(np.float64)) and np.allclose(want[:, 1], want[:, 0]) and np.allclose(want[:, 2], want[:, 0])
    assert np.allclose(seen["kw"]["scales"].cpu().numpy(), want, rtol=1e-6, atol=0)
