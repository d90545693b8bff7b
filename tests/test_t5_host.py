"""Host side of the T5 text conditioner (jen1_amd/t5.py), no GPU: the float64 restatement of tests/t5_common.py against what
transformers.T5EncoderModel computed (tests/golden/t5_encoder.npz), the bucket table, the geometry read from a state_dict's shapes, the
conditioner contract with a stub tokenizer and encoder, and the exported symbols of include/jen1_t5.h."""
import os
import re

import numpy as np
import pytest
import torch

import t5_common as TC
from helpers import ROOT
from jen1_amd import t5

# float32 Hugging Face outputs against a float64 restatement: a few float32 roundings through 2 blocks; 1e-5 is 40 ulp of max |y|
F64_VS_F32 = 1e-5


@pytest.fixture(scope="module")
def fixture():
    return TC.load_fixture()


@pytest.mark.parametrize("case", TC.CASES)
def test_restatement_matches_hugging_face(fixture, case):
    f = fixture[case]
    assert f["input_ids"].tolist() == TC.case_inputs(case)[0].tolist() and f["attention_mask"].tolist() == TC.case_inputs(case)[1].tolist()
    y = TC.encoder(TC.state_dict(f["schema"]), f["input_ids"], f["attention_mask"]).numpy()[:, :, ::f["step"]]
    l2, mx = TC.metrics(y, f["out"])
    print(f"{case}: relative L2 {l2:.3e}, max-abs/max-ref {mx:.3e}")
    assert y.shape == f["out"].shape and l2 < F64_VS_F32 and mx < F64_VS_F32


def test_bucket_table_equals_hugging_face_row(fixture):
    rel = torch.arange(-159, 160, dtype=torch.long)
    row = fixture["bucket_row"]
    assert t5.relative_position_bucket(rel).tolist() == row.tolist()
    assert TC.bucket(rel).tolist() == row.tolist()
    for dist in (16, 32, 64):               # exactly on a boundary of the logarithm
        assert row[159 + dist] != row[159 + dist - 1] and row[159 - dist] != row[159 - dist + 1]
    # the [heads, 2 N - 1] table the kernel reads: entry [h, (j - i) + N - 1]
    w = torch.from_numpy(TC.fill(TC.REL_BIAS, (32, 4)))
    for N in (1, 24, 128):
        tab = t5.bias_table(w, N)
        assert tab.shape == (4, 2 * N - 1) and tab.dtype == torch.float32
        want = TC.position_bias(w, N)
        i, j = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
        assert torch.equal(tab[:, j - i + N - 1], want)
        assert torch.equal(tab, w[torch.from_numpy(row[159 - (N - 1):159 + N])].t())


@pytest.mark.parametrize("case", TC.CASES)
def test_geometry_from_schema(fixture, case):
    g = t5.infer_geometry(dict(fixture[case]["schema"]))
    want = TC.CASE_SPECS[case]["geo"]
    assert g == t5.T5Geometry(want["vocab"], want["d_model"], want["heads"], want["d_kv"], want["d_ff"], want["layers"], 32, want["gated"])
    assert g.inner == want["heads"] * want["d_kv"]
    if case == "tiny-relu":
        assert g.inner != g.d_model


def test_geometry_rejects_other_state_dicts():
    with pytest.raises(KeyError):
        t5.infer_geometry({"shared.weight": (8, 8)})


class StubEncoder:
    def __init__(self, F=16):
        self.F, self.calls = F, 0

    def __call__(self, input_ids, attention_mask):
        self.calls += 1
        assert input_ids.dtype == torch.int64 and attention_mask.dtype == torch.bool
        B, N = input_ids.shape
        return (input_ids[..., None].float() * 0.01 + torch.arange(self.F, dtype=torch.float32) * 0.1 + 1.0)


class StubTail:
    """the arithmetic of TextConditionerTail on stock operators"""

    def __init__(self, w, b):
        self.w, self.b = w, b

    def __call__(self, hidden, mask):
        return (hidden @ self.w.t() + self.b) * mask[..., None].float(), mask


def make_conditioner(**kw):
    w = torch.from_numpy(TC.fill("t5.stub.proj.weight", (32, 16)))
    b = torch.from_numpy(TC.fill("t5.stub.proj.bias", (32,)))
    tok, enc = TC.StubTokenizer(), StubEncoder()
    return t5.T5ConditionerHIP(tok, enc, w, b, max_length=12, tail=StubTail(w, b), **kw), tok, enc, w, b


def test_conditioner_contract():
    cond, tok, enc, w, b = make_conditioner()
    texts = ["a piano", "drums and a very long prompt"]
    emb, mask = cond.forward(texts, "cpu")
    assert emb.shape == (2, 12, 32) and emb.dtype == torch.float32
    assert mask.shape == (2, 12) and mask.dtype == torch.bool
    assert mask[0].tolist() == [True] * 8 + [False] * 4 and mask[1].all()            # 7 characters + </s>; truncated to max_length
    enc_in = tok(texts, max_length=12)
    want = (enc(enc_in["input_ids"], enc_in["attention_mask"].bool()) @ w.t() + b) * mask[..., None].float()
    assert torch.equal(emb, want)
    assert float(emb[0, 8:].abs().max()) == 0.0 and float(emb[0, :8].abs().min()) > 0.0      # the mask multiply
    out = cond([{"prompt": t} for t in texts], "cpu")                                 # the MultiConditioner contract
    assert list(out) == ["prompt"] and torch.equal(out["prompt"][0], emb) and torch.equal(out["prompt"][1], mask)
    assert torch.equal(cond([{"prompt": [texts[0]]}, {"prompt": (texts[1],)}], "cpu")["prompt"][0], emb)      # collated lists are unwrapped
    with pytest.raises(ValueError):
        cond([{"text": "x"}], "cpu")


def test_conditioner_cache():
    cond, tok, enc, _, _ = make_conditioner(cache_size=2)
    meta = [{"prompt": "a piano"}, {"prompt": "a flute"}]
    first = cond(meta, "cpu")["prompt"]
    calls = (tok.calls, enc.calls)
    for _ in range(2):                      # the three identical calls of a trainer micro-batch cost one pass
        again = cond(meta, "cpu")["prompt"]
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    assert (tok.calls, enc.calls) == calls and (cond.hits, cond.misses) == (2, 1)
    again[0].zero_()                        # what a caller does to its copy does not reach the cache
    assert torch.equal(cond(meta, "cpu")["prompt"][0], first[0])
    cond([{"prompt": "b"}], "cpu")
    cond([{"prompt": "c"}], "cpu")          # two other prompt tuples push the first one out
    n = enc.calls
    cond(meta, "cpu")
    assert enc.calls == n + 1
    cond([{"prompt": "a flute"}, {"prompt": "a piano"}], "cpu")      # another order is another tuple
    assert enc.calls == n + 2


def test_all_false_mask_row_raises():
    cond, _, enc, _, _ = make_conditioner()
    with pytest.raises(ValueError, match="without a single token"):
        cond.forward(["a piano", ""], "cpu")                          # the stub tokenizer gives an empty prompt no token at all
    assert enc.calls == 0
    t5.check_mask(torch.tensor([[0, 1, 0], [1, 0, 0]]))
    with pytest.raises(ValueError):
        t5.check_mask(torch.tensor([[0, 1, 0], [0, 0, 0]]))


def test_header_symbols_are_exported():
    from jen1_amd import lib
    text = open(os.path.join(ROOT, "include", "jen1_t5.h")).read()
    names = re.findall(r"^int (jen1_t5_\w+)\(", text, flags=re.M)
    assert sorted(names) == ["jen1_t5_attention", "jen1_t5_embed", "jen1_t5_gate", "jen1_t5_rmsnorm"] == sorted(lib.T5_SYMBOLS)
    import ctypes
    so = ctypes.CDLL(lib.LIB_PATH) if os.path.exists(lib.LIB_PATH) else None
    assert so is not None, "the library has not been built"
    for n in names:
        assert n in lib.T5_SYMBOLS and hasattr(so, n), n
    for macro, value in (("JEN1_T5_MAX_TOKENS", lib.T5_MAX_TOKENS), ("JEN1_T5_ACT_GELU_NEW", lib.T5_ACT_GELU_NEW), ("JEN1_T5_ACT_RELU", lib.T5_ACT_RELU)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value
