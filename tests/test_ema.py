"""CPU tests of the EMA of the weights (jen1_amd/ema.py): the C entry point and its binding, the decay schedule against a float64
restatement, the config fields and the checkpoint's ``'ema'`` entry."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT
from jen1_amd import lib as L
from jen1_amd.checkpoint import load_checkpoint, save_checkpoint
from jen1_amd.config import TrainConfig, UNetSpec, tiny_model_config
from jen1_amd.ema import COPY, SKIP, UPDATE, ParamEMA, ema_schedule
from jen1_amd.optim import FusedAdamW


def test_library_exports_and_binds_the_fused_entry():
    hdr = open(os.path.join(ROOT, "include", "jen1_hip.h")).read()
    assert re.search(r"int jen1_adamw_ema_step_counted\(", hdr)
    assert "jen1_adamw_ema_step_counted" in L.SYMBOLS
    res, args = L.SYMBOLS["jen1_adamw_ema_step_counted"]
    # jen1_adamw_step_counted's arguments (without the stream), then ema, beta, update_after_step, update_every, warmup, inv_gamma,
    # power, min_decay, stream
    plain = L.SYMBOLS["jen1_adamw_step_counted"][1]
    assert args[:len(plain) - 1] == plain[:-1] and len(args) == len(plain) + 8
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("libjen1_hip.so not built")
    fn = getattr(L.load(), "jen1_adamw_ema_step_counted")
    assert fn.argtypes == args


def _schedule_np(t, beta, after, every, warmup, inv_gamma, power, min_decay):
    """float64 restatement over an array of steps: (mode, decay)"""
    t = np.asarray(t, dtype=np.int64)
    mode = np.where(t % every != 0, SKIP, np.where(t <= after, COPY, UPDATE))
    k = (t - after).astype(np.float64)
    if warmup:
        with np.errstate(invalid="ignore", divide="ignore"):
            d = 1.0 - np.power(1.0 + k / inv_gamma, -power)
        d = np.clip(d, min_decay, beta)
    else:
        d = np.full(t.shape, beta, dtype=np.float64)
    return mode, np.where(mode == UPDATE, d, 0.0)


@pytest.mark.parametrize("after,every,warmup,inv_gamma,power,min_decay,beta", [
    (100, 10, True, 1.0, 2.0 / 3.0, 0.0, 0.9999),          # the defaults
    (0, 1, True, 1.0, 0.75, 0.0, 0.999),
    (1, 1, False, 1.0, 2.0 / 3.0, 0.0, 0.995),
    (7, 3, True, 10.0, 0.5, 0.3, 0.99),
    (250, 25, False, 1.0, 2.0 / 3.0, 0.0, 0.9999),
])
def test_decay_schedule_matches_float64_restatement(after, every, warmup, inv_gamma, power, min_decay, beta):
    ts = np.arange(1, 100_001)
    want_mode, want_decay = _schedule_np(ts, beta, after, every, warmup, inv_gamma, power, min_decay)
    got = [ema_schedule(int(t), beta, after, every, warmup, inv_gamma, power, min_decay) for t in ts]
    got_mode = np.array([g[0] for g in got])
    got_decay = np.array([g[1] for g in got])
    np.testing.assert_array_equal(got_mode, want_mode)
    np.testing.assert_allclose(got_decay, want_decay, rtol=1e-15, atol=1e-15)
    upd = want_mode == UPDATE
    assert upd.any() and (got_decay[upd] <= beta).all() and (got_decay[upd] >= min_decay).all()


def test_config_fields_and_defaults():
    c = TrainConfig()
    assert c.use_ema is False
    assert c.ema_kwargs() == dict(beta=0.9999, update_after_step=100, update_every=10, warmup=True, inv_gamma=1.0, power=2.0 / 3.0,
                                  min_decay=0.0)


def _model(seed):
    from jen1_amd.model import UNetCFG1d
    return UNetCFG1d(**tiny_model_config(), device="cpu", init_seed=seed)


def test_ema_follows_the_optimiser_layout_and_validates():
    m = _model(1)
    opt = FusedAdamW(m.parameters())
    assert opt.ema is None
    ema = ParamEMA(opt, model=m)
    assert opt.ema is ema and ema.ema.shape == opt.flat_param.shape and torch.equal(ema.ema, opt.flat_param)
    ema.detach()
    assert opt.ema is None
    for bad in (dict(beta=1.0), dict(min_decay=0.5, beta=0.4), dict(update_every=0), dict(inv_gamma=0.0)):
        with pytest.raises(ValueError):
            ParamEMA(opt, **bad)


def test_checkpoint_ema_entry(tmp_path):
    m1 = _model(1)
    opt = FusedAdamW(m1.parameters())
    ema = ParamEMA(opt, model=m1)
    # EMA weights distinct from the model's: every entry moved by a deterministic offset
    ema.ema.add_(torch.linspace(-1.0, 1.0, ema.ema.numel()))
    path = str(tmp_path / "ema.pth")
    save_checkpoint(m1, opt, 3e-5, 4, path, ema=ema)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "epoch", "optimizer", "learning_rate", "ema"}
    # the existing keys are what a save without EMA writes
    path0 = str(tmp_path / "plain.pth")
    save_checkpoint(m1, opt, 3e-5, 4, path0)
    ck0 = torch.load(path0, map_location="cpu", weights_only=False)
    assert set(ck0) == {"model", "epoch", "optimizer", "learning_rate"}
    assert ck0["epoch"] == ck["epoch"] and ck0["learning_rate"] == ck["learning_rate"]
    assert list(ck0["model"]) == list(ck["model"]) and all(torch.equal(ck0["model"][k], ck["model"][k]) for k in ck0["model"])
    assert ck0["optimizer"]["param_groups"] == ck["optimizer"]["param_groups"]
    # 'ema': exactly the Appendix C key set and shapes, float32 CPU tensors, different from 'model'
    shapes = {k: tuple(s) for k, s in UNetSpec(**tiny_model_config()).param_shapes()}
    assert set(ck["ema"]) == set(shapes)
    for k, v in ck["ema"].items():
        assert tuple(v.shape) == shapes[k] and v.dtype == torch.float32 and v.device.type == "cpu", k
    assert any(not torch.equal(ck["ema"][k], ck["model"][k]) for k in shapes)
    # weights="ema" loads those tensors bit for bit
    m2 = _model(2)
    load_checkpoint(path, m2, weights="ema")
    sd = m2.state_dict()
    for k in shapes:
        assert torch.equal(sd[k], ck["ema"][k]), k
    # a file without 'ema' cannot give EMA weights ...
    with pytest.raises(KeyError):
        load_checkpoint(path0, _model(3), weights="ema")
    with pytest.raises(ValueError):
        load_checkpoint(path, _model(3), weights="nope")
    # ... but seeds a restored EMA from its model weights; a file with 'ema' restores the buffer
    m4 = _model(4)
    opt4 = FusedAdamW(m4.parameters())
    ema4 = ParamEMA(opt4, model=m4)
    load_checkpoint(path0, m4, optimizer=opt4, ema=ema4)
    assert torch.equal(ema4.ema, opt4.flat_param) and torch.equal(opt4.flat_param, opt.flat_param)
    load_checkpoint(path, m4, optimizer=opt4, ema=ema4)
    got = ema4.state_dict()
    assert all(torch.equal(got[k], ck["ema"][k]) for k in shapes)


def test_copy_to_writes_the_ema_weights():
    m1 = _model(1)
    opt = FusedAdamW(m1.parameters())
    ema = ParamEMA(opt, model=m1)
    ema.ema.mul_(0.5)
    m2 = _model(2)
    ema.copy_to(m2)
    want = ema.state_dict()
    for k, v in m2.state_dict().items():
        assert torch.equal(v, want[k]), k
