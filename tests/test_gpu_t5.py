"""-m gpu: the T5 encoder stack of the text conditioner on the HIP path (csrc/t5.hip, jen1_amd/t5.py): each kernel alone against the float64
restatement of tests/t5_common.py, the captured encoder against what transformers.T5EncoderModel computed (tests/golden/t5_encoder.npz),
and ``T5ConditionerHIP`` as the ``conditioner=`` of ``Jen1.generate``.

Gates.  float32: the suite's 1e-3 (helpers.rel_err: max-abs / max-ref); the kernels measure 1e-7 .. 1e-6, the encoder 1e-6 (printed by
every test, profiles/t5_parity.txt).  bf16, one kernel: the roundings the kernel makes, eps = 2^-8 being bf16's spacing relative to a value --
one rounding of the output for rmsnorm and gate (<= eps / 2 of the value, gated at eps of the largest), and for attention the rounding of P
plus that of the output (each <= eps / 2 of max |v|, because P sums to 1).  bf16, the whole encoder: 2x what was measured on MI355X
(T5_BF16_GATES below, profiles/t5_parity.txt), the rule profiles/r06_parity.txt set for every other bf16 gate of the suite.
"""
import numpy as np
import pytest
import torch

import t5_common as TC
from helpers import record_parity, rel_err
from jen1_amd.init_fill import fill_normal, fill_uniform

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3
BF16_EPS = 2.0 ** -8
MODES = ("f32", "bf16")
# (case): (relative L2, max-abs / max-ref) gates of the bf16 encoder against the fixture = 2x the values measured on MI355X
T5_BF16_GATES = {
    "tiny-gated": (8.4e-3, 8.9e-3),          # measured 4.20e-3, 4.47e-3
    "tiny-relu": (9.0e-3, 8.8e-3),           # measured 4.53e-3, 4.44e-3
    "wide": (9.6e-3, 1.29e-2),               # measured 4.81e-3, 6.45e-3
}


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import lib as L
    return L, L.load()


def tdt(mode):
    return torch.float32 if mode == "f32" else torch.bfloat16


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


# ---- the kernels one by one --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("with_add", (False, True))
@pytest.mark.parametrize("C", (64, 1000, 1024))
def test_rmsnorm(rt, C, with_add, mode):
    L, lib = rt
    rows = 5
    h0 = dev(1e4 * fill_normal(f"t5.rms.h.{C}", (rows, C), 1))            # flan-T5 magnitudes: the sum of squares is ~1e11
    add = dev(1e4 * fill_normal(f"t5.rms.add.{C}", (rows, C), 2)) if with_add else None
    w = dev(1.0 + 0.5 * fill_uniform(f"t5.rms.w.{C}", (C,), 3))
    h = h0.clone()
    y = torch.full((rows, C), float("nan"), dtype=tdt(mode), device="cuda")
    L.check(lib.jen1_t5_rmsnorm(h.data_ptr(), None if add is None else add.data_ptr(), w.data_ptr(), y.data_ptr(), rows, C, TC.EPS,
                                L.F32 if mode == "f32" else L.BF16, stream()), "jen1_t5_rmsnorm")
    torch.cuda.synchronize()
    hs = h0 + add if with_add else h0                                      # (one float32 addition: exact to compare)
    assert torch.equal(h, hs)
    ref = TC.rmsnorm(hs.double().cpu(), w.double().cpu())
    err = rel_err(y.float().cpu().numpy(), ref.numpy())
    print(f"rmsnorm C={C} add={with_add} {mode}: max-abs/max-ref {err:.3e}")
    assert torch.isfinite(y.float()).all()
    assert err < (F32_TOL if mode == "f32" else BF16_EPS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,d", ((24, 16), (128, 64), (100, 32)))
def test_attention(rt, N, d, mode):
    L, lib = rt
    B, H = 3, 2
    inner = H * d
    qkv = dev(fill_uniform(f"t5.att.qkv.{N}.{d}", (B, N, 3 * inner), 4), tdt(mode))
    tab = dev(10.0 * fill_uniform(f"t5.att.bias.{N}", (H, 2 * N - 1), 5))          # of order 10: a wrong j - i offset cannot hide
    mask = torch.zeros((B, N), dtype=torch.int32)
    mask[0, :] = 1                                                                 # every key
    mask[1, :1] = 1                                                                # one key
    mask[2, 1::3] = 1                                                              # not a prefix
    mask[2, N - 1] = 1
    o = torch.full((B, N, inner), float("nan"), dtype=tdt(mode), device="cuda")
    L.check(lib.jen1_t5_attention(qkv.data_ptr(), 3 * inner, o.data_ptr(), inner, tab.data_ptr(), mask.cuda().data_ptr(), B, H, N, d,
                                  L.F32 if mode == "f32" else L.BF16, stream()), "jen1_t5_attention")
    torch.cuda.synchronize()
    x = qkv.double().cpu().view(B, N, 3, H, d).permute(2, 0, 3, 1, 4)
    i, j = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
    bias = tab.double().cpu()[:, j - i + N - 1]                                    # [H, N, N]
    ref = TC.attention(x[0], x[1], x[2], bias, mask).transpose(1, 2).reshape(B, N, inner)
    got = o.float().cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[1].double(), x[2][1, :, :1].expand(H, N, d).transpose(0, 1).reshape(N, inner))      # one key: its value, exactly
    err = float((got.double() - ref).abs().max()) / float(x[2].abs().max())
    print(f"attention N={N} d={d} {mode}: max-abs / max |v| {err:.3e}, max-abs/max-ref {rel_err(got.numpy(), ref.numpy()):.3e}")
    assert err < (F32_TOL if mode == "f32" else BF16_EPS)
    if mode == "f32":
        assert rel_err(got.numpy(), ref.numpy()) < F32_TOL


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gated", (True, False))
@pytest.mark.parametrize("F", (96, 2816))
def test_gate(rt, F, gated, mode):
    L, lib = rt
    rows = 3
    x = dev(10.0 * fill_uniform(f"t5.gate.{F}.{gated}", (rows, (2 if gated else 1) * F), 6), tdt(mode))
    x[0, :4] = torch.tensor([-10.0, 10.0, 0.0, -0.5], device="cuda").to(x.dtype)
    y = torch.full((rows, F), float("nan"), dtype=tdt(mode), device="cuda")
    L.check(lib.jen1_t5_gate(x.data_ptr(), y.data_ptr(), rows, F, L.T5_ACT_GELU_NEW if gated else L.T5_ACT_RELU, L.F32 if mode == "f32" else L.BF16,
                             stream()), "jen1_t5_gate")
    torch.cuda.synchronize()
    ref = TC.gate(x.double().cpu(), gated)
    err = rel_err(y.float().cpu().numpy(), ref.numpy())
    print(f"gate F={F} gated={gated} {mode}: max-abs/max-ref {err:.3e}")
    assert err < (F32_TOL if mode == "f32" else BF16_EPS)
    if not gated:
        assert torch.equal(y, torch.relu(x))


def test_embed_and_out_of_range_ids(rt):
    L, lib = rt
    vocab, C = 50, 70
    table = dev(fill_normal("t5.embed.table", (vocab, C), 7))
    ids = torch.tensor([0, 49, 7, 7, 23], dtype=torch.int64, device="cuda")
    out = torch.full((5, C), float("nan"), device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.jen1_t5_embed(ids.data_ptr(), table.data_ptr(), out.data_ptr(), err.data_ptr(), 5, vocab, C, stream()), "jen1_t5_embed")
    assert int(err.item()) == 0 and torch.equal(out, table[ids])
    bad = torch.tensor([3, 50, -1, 1 << 40, 4], dtype=torch.int64, device="cuda")       # one past the table, negative, far outside
    L.check(lib.jen1_t5_embed(bad.data_ptr(), table.data_ptr(), out.data_ptr(), err.data_ptr(), 5, vocab, C, stream()), "jen1_t5_embed")
    assert int(err.item()) == 1
    assert torch.equal(out[[0, 4]], table[[3, 4]]) and float(out[1:4].abs().max()) == 0.0       # never used as an index: zero rows


# ---- the whole encoder -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return TC.load_fixture()


_REF2 = {}


def second_reference(case, sd):
    """the float64 restatement on the other ids / masks of the case's shape: computed once, shared by both modes"""
    if case not in _REF2:
        ids, mask = TC.case_inputs(case, 1)
        _REF2[case] = (ids, mask, TC.encoder(sd, ids, mask).numpy())
    return _REF2[case]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", TC.CASES)
def test_encoder_matches_hugging_face(rt, fixture, case, mode):
    from jen1_amd.t5 import T5EncoderHIP
    f = fixture[case]
    sd = TC.state_dict(f["schema"])
    enc = T5EncoderHIP.from_state_dict(sd, compute_dtype=mode)
    geo = TC.CASE_SPECS[case]["geo"]
    assert enc.geo.gated == geo["gated"] and enc.geo.d_kv == geo["d_kv"] and enc.geo.layers == geo["layers"]
    ids, mask = torch.from_numpy(f["input_ids"]), torch.from_numpy(f["attention_mask"])
    eager = enc(ids, mask, graph=False)
    assert enc.launches == 8 * geo["layers"] + 2
    replay = enc(ids.cuda(), mask.cuda())
    assert replay.shape == (*ids.shape, geo["d_model"]) and replay.dtype == torch.float32 and replay.device.type == "cuda"
    assert torch.equal(replay, eager)                                      # graph replay == eager run, bit for bit
    l2, mx = TC.metrics(replay.cpu().numpy()[:, :, ::f["step"]], f["out"])
    # other ids and masks of the same shape through the same buffers and graph: that input's result, then the first one's again
    ids2, mask2, ref2 = second_reference(case, sd)
    other = enc(torch.from_numpy(ids2), torch.from_numpy(mask2))
    l2b, mxb = TC.metrics(other.cpu().numpy(), ref2)
    print(f"encoder {case} {mode}: relative L2 {l2:.3e}, max-abs/max-ref {mx:.3e}; second input {l2b:.3e}, {mxb:.3e}")
    record_parity("t5_encoder", case, mode, l2=l2, maxabs=mx, l2_second=l2b, maxabs_second=mxb)
    gates = (F32_TOL, F32_TOL) if mode == "f32" else T5_BF16_GATES[case]
    assert l2 < gates[0] and mx < gates[1], (l2, mx)
    assert l2b < gates[0] and mxb < gates[1], (l2b, mxb)
    assert torch.equal(enc(ids, mask), replay)


def test_encoder_refuses_bad_input(rt, fixture):
    from jen1_amd import lib as L
    from jen1_amd.t5 import T5EncoderHIP
    f = fixture["tiny-gated"]
    enc = T5EncoderHIP.from_state_dict(TC.state_dict(f["schema"]))
    ids, mask = torch.from_numpy(f["input_ids"]).clone(), torch.from_numpy(f["attention_mask"]).clone()
    good = enc(ids, mask)
    bad = ids.clone()
    bad[1, 3] = 96                                                        # one past the table
    with pytest.raises(L.Jen1HipError, match="outside the table"):
        enc(bad, mask)
    assert torch.equal(enc(ids, mask), good)                               # the flag is cleared: the next call is served
    dark = mask.clone()
    dark[1] = 0
    with pytest.raises(ValueError, match="without a single token"):
        enc(ids, dark)
    with pytest.raises(ValueError):
        enc(torch.zeros((1, 129), dtype=torch.int64), torch.ones((1, 129), dtype=torch.int64))


# ---- as Jen1's conditioner -----------------------------------------------------------------------------------------------------------------
def test_conditioner_in_generate(rt, fixture):
    """``Jen1.generate`` with ``T5ConditionerHIP`` == ``generate`` with a hand-built conditioner that returns the same (emb, mask)"""
    from jen1_amd.config import GDMConfig, tiny_model_config
    from jen1_amd.generation import Jen1
    from jen1_amd.t5 import T5ConditionerHIP, T5EncoderHIP
    from test_gpu_generation import StubAudioEncoder
    sd = TC.state_dict(fixture["tiny-gated"]["schema"])
    enc = T5EncoderHIP.from_state_dict(sd)
    pw, pb = torch.from_numpy(TC.fill("t5.proj_out.weight", (1024, 64))), torch.from_numpy(TC.fill("t5.proj_out.bias", (1024,)))
    tok = TC.StubTokenizer()
    cond = T5ConditionerHIP(tok, enc, pw, pb, max_length=128)
    prompt = "a calm piano piece"
    emb, mask = cond.forward([prompt] * 2, "cuda")
    assert emb.shape == (2, 128, 1024) and emb.dtype == torch.float32 and mask.dtype == torch.bool and emb.device.type == "cuda"
    n = len(prompt) + 1
    assert mask[0].tolist() == [True] * n + [False] * (128 - n) and float(emb[:, n:].abs().max()) == 0.0
    # the projection of the encoder's output, against the float64 restatement of both
    e = tok([prompt] * 2)
    want = (TC.encoder(sd, e["input_ids"], e["attention_mask"]) @ pw.double().t() + pb.double()) * e["attention_mask"][..., None].double()
    assert rel_err(emb.cpu().numpy(), want.numpy()) < F32_TOL
    jen1 = Jen1(None, device="cuda", audio_encoder=StubAudioEncoder(), conditioner=cond, model_config=tiny_model_config(),
                diffusion_config=GDMConfig(), compute_dtype="f32")
    a = jen1.generate(prompt, seed=3, steps=3, batch_size=2, seconds=2, use_gdm=True)
    assert (cond.misses, tok.calls) == (1, 2) and cond.hits == 1           # generate() with the same prompt: no second pass
    jen1.conditioner = lambda meta, device: {"prompt": (emb[:len(meta)].to(device), mask[:len(meta)].to(device))}
    b = jen1.generate(prompt, seed=3, steps=3, batch_size=2, seconds=2, use_gdm=True)
    assert a.shape == (2, 2, 2 * 48000) and torch.isfinite(a).all()
    assert torch.allclose(a, b, atol=1e-4)                                 # (float atomics reorder sums at the 1e-7 level, test_gpu_generation.py)
