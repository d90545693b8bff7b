"""Global conditioning (``context_features`` / ``features``), everything that needs no GPU: the parameter schema against the
reference's ``state_dict`` (tests/golden/global_cond.npz, make_global_cond_golden.py), the dispatcher op's schema and fake
implementation, the missing-features assert, ``MultiConditionerHIP``'s key rules, ``Jen1.generate(conditions=)`` and the checkpoint /
EMA round trips of the two new tensors."""
import json

import numpy as np
import pytest
import torch

from helpers import golden
from jen1_amd.config import UNetSpec, tiny_model_config

F_CTX = 24


def _cfg():
    return dict(tiny_model_config(), context_features=F_CTX)


def _model(seed=1234, **kw):
    from jen1_amd.model import UNetCFG1d
    return UNetCFG1d(**_cfg(), device="cpu", init_seed=seed, **kw)


def test_param_shapes_match_the_reference_state_dict():
    g = golden("global_cond")
    want = [(k, tuple(s)) for k, s in json.loads(str(g["schema"]))]
    got = UNetSpec(**_cfg()).param_shapes()
    assert got == want and len(got) == 237
    keys = [k for k, _ in got]
    i = keys.index("to_time.0.1.bias")
    mf = 4 * tiny_model_config()["channels"]
    assert got[i + 1] == ("to_features.0.weight", (mf, F_CTX)) and got[i + 2] == ("to_features.0.bias", (mf,))
    assert keys[i + 3].startswith("to_in.block.")
    # without context_features: exactly the list of tiny_unet.npz, whether the key is absent or None
    plain = [(k, tuple(s)) for k, s in json.loads(str(golden("tiny_unet")["schema"]))]
    assert UNetSpec(**tiny_model_config()).param_shapes() == plain
    assert UNetSpec(**tiny_model_config(), context_features=None).param_shapes() == plain
    assert [k for k in keys if "to_features" not in k] == [k for k, _ in plain]


def test_state_dict_and_every_init_form_carry_the_new_tensors():
    want = [k for k, _ in UNetSpec(**_cfg()).param_shapes()]
    for seed in ("torch", 1234, None):
        m = _model(seed)
        assert list(m.state_dict()) == want
        w, b = m.state_dict()["to_features.0.weight"], m.state_dict()["to_features.0.bias"]
        assert tuple(w.shape) == (256, F_CTX) and tuple(b.shape) == (256,)
        if seed is None:
            assert not w.any() and not b.any()
        else:
            assert w.abs().max() > 0 and b.abs().max() > 0
        if seed == "torch":          # nn.Linear's default: U(+-1 / sqrt(fan_in))
            assert float(w.abs().max()) <= F_CTX ** -0.5 and float(b.abs().max()) <= F_CTX ** -0.5


def test_fake_tensor_call_with_features_and_the_op_schema():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from jen1_amd import ops  # noqa: F401
    sch = str(torch.ops.jen1.unet_cfg_forward.default._schema)
    assert "Tensor x, Tensor time, Tensor embedding, Tensor? embedding_mask, Tensor? context" in sch and sch.endswith("-> Tensor")
    args = sch[sch.index("(") + 1: sch.rindex(") ->")]
    assert args.endswith("Tensor? dropout_rows, Tensor? features=None"), sch
    model = _model(None)
    plain = __import__("jen1_amd.model", fromlist=["UNetCFG1d"]).UNetCFG1d(**tiny_model_config(), device="cpu", init_seed=None)
    B, T = 3, 96
    with FakeTensorMode():
        sp = model.spec
        x = torch.empty((B, sp.in_channels, T))
        t = torch.empty((B,), dtype=torch.int64)
        kw = dict(embedding=torch.empty((B, sp.ctx_max_length, sp.ctx_features)), embedding_mask=torch.empty((B, sp.ctx_max_length)),
                  embedding_scale=0.8, batch_cfg=True, scale_cfg=True, channels_list=[torch.empty((B, sp.ctx_ch0, T))])
        y = model(x, t, features=torch.empty((B, F_CTX)), **kw)
        assert tuple(y.shape) == (B, sp.out_channels, T) and y.dtype == torch.float32
        with pytest.raises(AssertionError, match="context_features exists but no features provided"):
            model(x, t, **kw)
        with pytest.raises(AssertionError, match="features of shape"):
            model(x, t, features=torch.empty((B, F_CTX + 1)), **kw)
        # a model without context_features ignores them, as the reference does
        y = plain(x, t, features=torch.empty((B, 7)), **kw)
        assert tuple(y.shape) == (B, sp.out_channels, T)


def test_checkpoint_and_ema_round_trips_carry_the_new_tensors(tmp_path):
    from jen1_amd.checkpoint import load_checkpoint, save_checkpoint
    from jen1_amd.ema import ParamEMA
    from jen1_amd.optim import FusedAdamW
    m1 = _model(1)
    opt = FusedAdamW(m1.parameters())
    n = sum(int(np.prod(s)) for _, s in UNetSpec(**_cfg()).param_shapes())
    assert opt.flat_param.numel() >= n and any(p is m1.to_features._modules["0"].weight for p in m1.parameters())
    ema = ParamEMA(opt, model=m1)
    ema.ema.add_(torch.linspace(-1.0, 1.0, ema.ema.numel()))
    path = str(tmp_path / "gc.pth")
    save_checkpoint(m1, opt, 3e-5, 4, path, ema=ema)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    keys = [k for k, _ in UNetSpec(**_cfg()).param_shapes()]
    assert list(ck["model"]) == keys and set(ck["ema"]) == set(keys)
    for k in ("to_features.0.weight", "to_features.0.bias"):
        assert torch.equal(ck["model"][k], m1.state_dict()[k])
        assert not torch.equal(ck["ema"][k], ck["model"][k])
    m2 = _model(2)
    assert not torch.equal(m2.state_dict()["to_features.0.weight"], m1.state_dict()["to_features.0.weight"])
    load_checkpoint(path, m2)
    m3 = _model(3)
    load_checkpoint(path, m3, weights="ema")
    for k in ("to_features.0.weight", "to_features.0.bias"):
        assert torch.equal(m2.state_dict()[k], ck["model"][k]) and torch.equal(m3.state_dict()[k], ck["ema"][k])
    m4 = _model(4)
    opt4 = FusedAdamW(m4.parameters())
    ema4 = ParamEMA(opt4, model=m4)
    load_checkpoint(path, m4, optimizer=opt4, ema=ema4)
    got = ema4.state_dict()
    assert all(torch.equal(got[k], ck["ema"][k]) for k in keys)


# ------------------------------------------------------------------------------------------------------------------ conditioners
class _Stub:
    """records what MultiConditionerHIP hands a conditioner"""

    def __init__(self, width):
        self.width, self.seen = width, []

    def forward(self, values, device):
        self.seen.append(list(values))
        return [torch.full((len(values), 1, self.width), float(len(self.seen))), torch.ones((len(values), 1))]


def test_multi_conditioner_key_rules():
    from jen1_amd.conditioners import MultiConditionerHIP
    a, b = _Stub(8), _Stub(16)
    calls = []
    plain = lambda values, device: calls.append(list(values)) or (torch.zeros((len(values), 4, 2)), torch.ones((len(values), 4)))
    mc = MultiConditionerHIP({"seconds": a, "key": b, "prompt": plain}, default_keys={"key": "tonic"})
    rows = [{"seconds": [12.5, 99.0], "key": (5,), "prompt": "x"},          # a list of ANY length and a 1-tuple are unwrapped
            {"seconds": (1.0, 2.0), "tonic": 7, "key": 3, "prompt": ["y"]},   # a 2-tuple is passed as it is
            {"seconds": 3, "tonic": [8], "prompt": ("z",)}]                  # no "key": falls back to default_keys["key"]
    out = mc(rows, "cpu")
    assert list(out) == ["seconds", "key", "prompt"]
    assert a.seen == [[12.5, (1.0, 2.0), 3]]
    assert b.seen == [[5, 3, 8]]
    assert calls == [["x", "y", "z"]]
    assert tuple(out["seconds"][0].shape) == (3, 1, 8) and tuple(out["key"][0].shape) == (3, 1, 16)
    # as written in the reference the fallback key stays switched for the rows after it
    b.seen.clear()
    mc([{"seconds": 0, "tonic": 1, "prompt": "p"}, {"seconds": 0, "key": 2, "tonic": 4, "prompt": "p"}], "cpu")
    assert b.seen == [[1, 4]]
    with pytest.raises(ValueError, match="Conditioner key seconds not found in batch metadata"):
        mc([{"key": 1, "prompt": "p"}], "cpu")
    with pytest.raises(KeyError, match="tonic"):          # (as written: the fallback key itself is read without a check)
        mc([{"seconds": 1, "prompt": "p"}], "cpu")
    # the global_cond of the two through tasks.get_conditioning: [B, 8 + 16]
    from jen1_amd.tasks import get_conditioning
    gc = get_conditioning(out, cross_attn_cond_ids=(), global_cond_ids=("seconds", "key"), input_concat_ids=())["global_cond"]
    assert tuple(gc.shape) == (3, 24)


def test_int_and_number_conditioner_state_dicts_and_host_checks():
    from jen1_amd.conditioners import IntConditionerHIP, NumberConditionerHIP
    num = NumberConditionerHIP(8, 0, 30)
    assert list(num.state_dict()) == ["embedder.embedding.0.weights", "embedder.embedding.1.weight", "embedder.embedding.1.bias"]
    assert [tuple(v.shape) for v in num.state_dict().values()] == [(128,), (8, 257), (8,)]
    itc = IntConditionerHIP(16, 0, 8)
    assert list(itc.state_dict()) == ["int_embedder.weight"] and tuple(itc.weight.shape) == (9, 16)
    other = IntConditionerHIP(16, 0, 8)
    other.load_state_dict(itc.state_dict())
    assert torch.equal(other.weight, itc.weight)
    num2 = NumberConditionerHIP(8, 0, 30)
    num2.load_state_dict(num.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(num2.state_dict().values(), num.state_dict().values()))
    with pytest.raises(KeyError):
        itc.load_state_dict({"weight": itc.weight})
    with pytest.raises(ValueError):
        IntConditionerHIP(16, 0, 8, weight=torch.zeros((8, 16)))
    with pytest.raises(ValueError):
        NumberConditionerHIP(8, 3, 3)
    # the reference indexes with the clamped value itself: with min_val > 0 the top of the range is outside the table
    with pytest.raises(IndexError, match="does not subtract min_val"):
        IntConditionerHIP(4, 2, 5)([5], "cpu")

    # from_module of reference-shaped modules
    class RefInt(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.output_dim, self.min_val, self.max_val = 16, 0, 8
            self.int_embedder = torch.nn.Embedding(9, 16)

    ref = RefInt()
    got = IntConditionerHIP.from_module(ref)
    assert torch.equal(got.weight, ref.int_embedder.weight.detach()) and list(got.state_dict()) == list(ref.state_dict())


def _jen1(conditioner, global_ids=()):
    from jen1_amd.generation import Jen1
    return Jen1(None, device="cpu", audio_encoder=None, conditioner=conditioner, global_cond_ids=global_ids, model_config=_cfg())


def test_generate_merges_conditions_into_the_metadata_rows():
    from jen1_amd.generation import Jen1
    assert Jen1._metadata_rows("p", 2, None) is None                        # None keeps today's call exactly
    assert Jen1._metadata_rows("p", 2, {"seconds": 3}) == [{"prompt": "p", "seconds": 3}] * 2
    assert Jen1._metadata_rows("p", 2, [{"key": 1}, {"key": 2}]) == [{"prompt": "p", "key": 1}, {"prompt": "p", "key": 2}]
    with pytest.raises(ValueError):
        Jen1._metadata_rows("p", 3, [{"key": 1}])
    with pytest.raises(ValueError):
        Jen1._metadata_rows("p", 1, ["key"])

    seen = []

    class Done(Exception):
        pass

    def conditioner(rows, device):
        seen.append(rows)
        return {"prompt": (torch.zeros((len(rows), 128, 1024)), torch.ones((len(rows), 128), dtype=torch.bool))}

    class Enc:
        channels = 1

    j = _jen1(conditioner, global_ids=("seconds",))
    j.audio_encoder = Enc()
    j.get_emb = lambda wav: torch.zeros((wav.shape[0], 128, 8))
    j.get_model_and_diffusion = lambda steps, use_gdm: (None, None)
    j.device = "cpu"
    # the conditioner does not return the id that global_cond_ids names
    with pytest.raises(KeyError, match="seconds"):
        j.generate("p", seed=1, steps=2, batch_size=2, seconds=1, conditions={"seconds": 3})
    assert seen == [[{"prompt": "p", "seconds": 3}] * 2]
    seen.clear()
    with pytest.raises(KeyError, match="seconds"):
        j.generate("p", seed=1, steps=2, batch_size=2, seconds=1)
    assert seen == [[{"prompt": "p"}] * 2]
