"""-m gpu: the resampler / channel converter kernel (csrc/audio.hip: jen1_resample) against the dense float64 restatement of
tests/audio_common.py, and its place in ``Jen1.generate`` (the default ``convert_audio``, ``output_sr``)."""
import contextlib
import math

import numpy as np
import pytest
import torch

from audio_common import PAIRS_INTO_48K, dense_resample, dense_table, geometry, mix_channels

from jen1_amd import synth
from jen1_amd.config import GDMConfig, tiny_model_config

pytestmark = pytest.mark.gpu

HOP = 320
SENTINEL = -77.25


@pytest.fixture(scope="module")
def audio():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import audio as A
    return A


@pytest.fixture(scope="module")
def lib():
    from jen1_amd import lib as L
    L.build()
    return L.load()


def call_kernel(lib, A, x, sr, target, c_out, pad=37):
    """jen1_resample on x [rows, C, L] (CPU float32) with the output carved out of a larger buffer full of a sentinel; returns the
    output [rows, c_out, L_out] and the two guard bands"""
    rows, c_in, L = x.shape
    o, n, w, W, taps, first = A._tables(sr, target, torch.device("cuda", torch.cuda.current_device()))
    n_out = -(-n * L // o)
    buf = torch.full((pad + rows * c_out * n_out + pad,), SENTINEL, dtype=torch.float32, device="cuda")
    y = buf[pad:pad + rows * c_out * n_out]
    xd = x.cuda().contiguous()
    rc = lib.jen1_resample(xd.data_ptr(), y.data_ptr(), taps.data_ptr(), first.data_ptr(), rows, c_in, c_out, L, n_out, o, n, w, W,
                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.jen1_last_error()
    torch.cuda.synchronize()
    return y.view(rows, c_out, n_out).cpu(), buf[:pad].cpu(), buf[pad + rows * c_out * n_out:].cpu()


def table_bound(sr, target, W, xmax):
    """|kernel - float64 restatement| <= (W + 2) * 2^-24 * max_p sum_k |h[p][k]| * max|x|: W fused multiply-adds in float32, each rounding
    a partial sum that never exceeds sum|h| * max|x|, plus the rounding of the comparison itself"""
    h = dense_table(sr, target).astype(np.float64)
    return (W + 2) * 2.0 ** -24 * float(np.abs(h).sum(axis=1).max()) * xmax


# ------------------------------------------------------------------ 1. impulses, bit for bit
@pytest.mark.parametrize("sr,target", [(44100, 48000), (96000, 48000), (8000, 48000), (48000, 44100)])
def test_impulses_reproduce_the_table_bit_for_bit(audio, sr, target):
    """x = delta_i: every output is h[p][i + w - j o] where that index lies in [0, K), else 0 -- one product by 1.0 leaves no rounding
    freedom.  Pins phase, offset, first[] and the trim."""
    o, n, w, K = geometry(sr, target)
    h = dense_table(sr, target)
    L = 2 * o + 5
    where = sorted({0, 1, o - 1, o, L - 1})
    x = torch.zeros((len(where), L))
    for r, i in enumerate(where):
        x[r, i] = 1.0
    y = audio.resample(x, sr, target)
    n_out = -(-n * L // o)
    assert y.shape == (len(where), n_out) and y.device.type == "cpu"
    m = np.arange(n_out)
    j, p = m // n, m % n
    for r, i in enumerate(where):
        k = i + w - j * o
        want = np.where((k >= 0) & (k < K), h[p, np.clip(k, 0, K - 1)], np.float32(0))
        assert torch.equal(y[r], torch.from_numpy(want.astype(np.float32))), f"impulse at {i}: {int((y[r].numpy() != want).sum())} outputs differ"


# ------------------------------------------------------------------ 2. lengths at the frame edge, guard bands
def test_tile_rule(audio):
    """a tile is about 2 k outputs whatever n is, and its input window stays small when o >> n"""
    assert [audio.tile_frames(o, n) for o, n in ((147, 160), (2, 1), (1, 6), (6, 1), (1, 320), (5000, 5041))] == [12, 2048, 341, 682, 6, 1]


@pytest.mark.parametrize("rows", [1, 3])
def test_lengths_at_the_frame_and_tile_edges(audio, lib, rows):
    sr, target = 44100, 48000
    o, n, w, K = geometry(sr, target)
    tile_in = audio.tile_frames(o, n) * o                        # input samples behind one workgroup's tile
    lengths = [1, 146, 147, 148, 1000, 3 * tile_in + tile_in // 2 + 77]
    assert lengths[-1] % 2 == 1 and -(-n * lengths[-1] // o) > 3 * audio.tile_frames(o, n) * n
    g = torch.Generator().manual_seed(1)
    W = audio.resample_table(sr, target)[3].shape[1]
    for L in lengths:
        x = torch.rand((rows, 1, L), generator=g) * 2 - 1
        y, lo, hi = call_kernel(lib, audio, x, sr, target, 1)
        assert y.shape == (rows, 1, math.ceil(n * L / o))
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), f"L = {L}: the kernel wrote outside its output"
        assert audio.resample(x[:, 0], sr, target).shape == (rows, math.ceil(n * L / o))
        want = dense_resample(x.numpy(), sr, target, table=dense_table(sr, target))
        err = float(np.abs(y.numpy().astype(np.float64) - want).max())
        assert err <= table_bound(sr, target, W, 1.0), f"L = {L}: {err:.3e}"


# ------------------------------------------------------------------ 3. random input, every pair, every channel case
_X = {}


def random_input():
    if "x" not in _X:
        g = torch.Generator().manual_seed(20)
        _X["x"] = torch.rand((2, 2, 2000), generator=g) * 2 - 1
    return _X["x"]


@pytest.mark.parametrize("sr,target", PAIRS_INTO_48K + ((48000, 44100),))
def test_random_input_against_the_float64_restatement(audio, sr, target):
    x = random_input()
    xn = x.numpy()
    h = dense_table(sr, target)                                   # the same float32 table, dense
    W = audio.resample_table(sr, target)[3].shape[1]
    bound = table_bound(sr, target, W, float(np.abs(xn).max()))
    o, n, _, _ = geometry(sr, target)
    for c_in, c_out in ((1, 1), (2, 2), (2, 1), (1, 2)):
        src = x[:, :c_in]
        got = audio.convert_audio(src, sr, target, c_out)
        assert got.shape == (2, c_out, math.ceil(n * 2000 / o)) and got.dtype == torch.float32 and got.device.type == "cpu"
        want = dense_resample(mix_channels(xn[:, :c_in], c_out), sr, target, table=h)
        err = float(np.abs(got.numpy().astype(np.float64) - want).max())
        print(f"{sr} -> {target}, {c_in} -> {c_out} channels: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (c_in, c_out, err, bound)
        if (c_in, c_out) == (1, 2):
            assert torch.equal(got[:, 0], got[:, 1]), "mono -> stereo: the two channels must be the same bits"
        assert torch.equal(got, audio.convert_audio(src, sr, target, c_out)), "two runs of the same call differ"


def test_leading_axes_strides_and_channel_only_conversion(audio):
    x = random_input()
    ref = audio.convert_audio(x, 44100, 48000, 2)
    assert torch.equal(audio.convert_audio(x.reshape(1, 2, 1, 2, 2000), 44100, 48000, 2), ref.reshape(1, 2, 1, 2, -1))
    wide = torch.zeros((2, 2, 4000))
    wide[:, :, ::2] = x
    assert torch.equal(audio.convert_audio(wide[:, :, ::2], 44100, 48000, 2), ref)                  # non-contiguous input
    on_gpu = audio.convert_audio(x.cuda(), 44100, 48000, 2)
    assert on_gpu.device.type == "cuda" and torch.equal(on_gpu.cpu(), ref)
    assert torch.equal(audio.resample(x, 44100, 48000), ref)                                        # [..., L]: every row on its own
    # same rate, other channel count: the identity filter, only the channel rule
    assert torch.equal(audio.convert_audio(x, 48000, 48000, 1), (x[:, 0:1] + x[:, 1:2]) * 0.5)
    assert torch.equal(audio.convert_audio(x[:, :1], 48000, 48000, 2), torch.cat([x[:, :1], x[:, :1]], dim=1))


# ------------------------------------------------------------------ 4. argument errors (no launch)
def test_argument_errors(audio, lib):
    o, n, w, W, taps, first = audio._tables(44100, 48000, torch.device("cuda", torch.cuda.current_device()))
    x = torch.zeros((2, 147), device="cuda")
    y = torch.full((2, 160), SENTINEL, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    args = lambda **kw: [kw.get("x", x.data_ptr()), y.data_ptr(), taps.data_ptr(), first.data_ptr(), 1, kw.get("c_in", 1), kw.get("c_out", 1), 147,
                         kw.get("L_out", 160), o, n, w, kw.get("W", W), s]
    for bad, word in ((dict(L_out=161), "L_out"), (dict(c_out=3), "c_out"), (dict(c_in=0), "c_in"), (dict(W=0), "W"), (dict(x=None), "null")):
        assert lib.jen1_resample(*args(**bad)) != 0
        assert word in lib.jen1_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert lib.jen1_resample(*args()) == 0
    torch.cuda.synchronize()
    assert bool((y[0] == 0).all()) and bool((y[1] == SENTINEL).all())


# ------------------------------------------------------------------ 5. Jen1
class _Quantizer:
    def __init__(self, n_q=4, bins=64, dim=128):
        g = torch.Generator().manual_seed(11)
        self.tables = torch.randn((n_q, bins, dim), generator=g) * 0.3

    def decode(self, codes):
        out = 0
        for q in range(codes.shape[0]):
            out = out + self.tables.to(codes.device)[q][codes[q]]
        return out.transpose(1, 2)


class StubAudioEncoder:
    """the slice of ``encodec.EncodecModel`` generation.py touches (test_gpu_generation.py's)"""
    channels = 2
    sample_rate = 48000

    def __init__(self):
        self.quantizer = _Quantizer()

    def encode(self, audio):
        B, _, n = audio.shape
        frames = audio[:, :, : n // HOP * HOP].reshape(B, 2, n // HOP, HOP).mean(dim=(1, 3))
        base = (frames * 1000).round().long().abs() % 64
        return [(torch.stack([(base + 7 * q) % 64 for q in range(4)], dim=1), None)]

    def decoder(self, emb):
        assert emb.device.type == "cpu"
        return torch.tanh(emb[:, :2].repeat_interleave(HOP, dim=2))


@pytest.fixture(scope="module")
def jen1(audio):
    from jen1_amd.generation import Jen1
    cond = synth.conditioning(8, 300, "text_guided")
    emb = torch.from_numpy(cond["cross_attn_cond"]).cuda()
    msk = torch.from_numpy(cond["cross_attn_masks"]).cuda()

    def conditioner(batch_metadata, device):
        n = len(batch_metadata)
        return {"prompt": (emb[:n].to(device), msk[:n].to(device))}

    return Jen1(None, device="cuda", audio_encoder=StubAudioEncoder(), conditioner=conditioner, model_config=tiny_model_config(),
                diffusion_config=GDMConfig(), compute_dtype="f32")


@contextlib.contextmanager
def fixed_order(m, on):
    """the sampler's bit-reproducible mode (no float-atomic statistics), as in test_gpu_known_blend.py"""
    old = m.deterministic
    m.deterministic = bool(on)
    try:
        yield
    finally:
        m.deterministic = old


def test_generate_converts_init_audio_by_default(jen1, audio):
    """mono 24 kHz audio into the default ``convert_audio``: the bits of the call that is handed the converted audio at 48 kHz, and the
    continuation starts where the RESAMPLED prefix ends"""
    B, seconds, steps = 2, 2, 3
    L = 12000                                                            # 0.5 s at 24 kHz
    prefix = torch.rand((1, L), generator=torch.Generator().manual_seed(4)) * 0.2 - 0.1
    _, model = jen1.get_model_and_diffusion(steps, True)
    kw = dict(seed=3, steps=steps, batch_size=B, seconds=seconds, use_gdm=True, task="music_cont")
    with fixed_order(model, True):
        got = jen1.generate("y", init_audio=prefix, init_audio_sr=24000, **kw)
        converted = audio.convert_audio(prefix.unsqueeze(0).expand(B, -1, -1), 24000, 48000, 2)
        assert converted.shape == (B, 2, 2 * L)
        want = jen1.generate("y", init_audio=converted, init_audio_sr=48000, **kw)
    assert got.shape == (B, 2, seconds * 48000) and torch.equal(got, want)
    wav, placeholder, n_prefix = jen1._known_audio("music_cont", prefix, 24000, B, seconds * 48000)
    assert n_prefix == math.ceil(2 * L) and not placeholder and torch.equal(wav[:, :, :n_prefix], converted)
    start_s, end_s, causal = jen1._task_window("music_cont", seconds, None, n_prefix)
    keep = jen1.get_mask(seconds * 48000, start_s, end_s, B)
    assert causal and float(keep[:, :, :n_prefix].min()) == 1 and float(keep[:, :, n_prefix:].max()) == 0


def test_generate_output_sr(jen1, audio):
    steps = 3
    _, model = jen1.get_model_and_diffusion(steps, True)
    kw = dict(seed=3, steps=steps, batch_size=2, seconds=2, use_gdm=True)
    with fixed_order(model, True):
        plain = jen1.generate("y", **kw)
        same = jen1.generate("y", output_sr=48000, **kw)
        got = jen1.generate("y", output_sr=44100, **kw)
    N = plain.shape[2]
    assert N == 2 * 48000 and torch.equal(same, plain)
    assert got.shape == (2, 2, math.ceil(147 * N / 160)) and got.device == plain.device
    assert torch.equal(got, audio.resample(plain, 48000, 44100))
    with pytest.raises(ValueError, match="output_sr"):
        jen1.generate("y", output_sr=0, **kw)
