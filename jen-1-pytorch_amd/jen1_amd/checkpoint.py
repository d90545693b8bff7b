"""Checkpoint wire format of the reference.

Same file layout and loader tolerances as /root/reference/utils/script_util.py:79-148:
``torch.save({'model': state_dict, 'epoch', 'optimizer', 'learning_rate'})``; on load, keys missing from the file
keep the model's current value and a ``_orig_mod.`` prefix (torch.compile) is accepted.  The model's parameters use
the reference ``state_dict`` key schema, so files are interchangeable in both directions;
after loading, the HIP engine repacks its weights on next use.

With an EMA of the weights (jen1_amd/ema.py) the file carries one more key, ``'ema'``: the EMA weights under the same key schema.
The reference's loader reads only ``model`` / ``optimizer`` / ``epoch`` / ``learning_rate``, so such files still load there.
A latent ``Normalizer`` (jen1_amd/normalizer.py) is one more key of the same kind, ``'normalizer'``: its ``state_dict()``.
"""
from __future__ import annotations

import logging
import os
from typing import Optional

import torch


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def save_checkpoint(model, optimizer, lr, iteration, checkpoint_path, logger=None, ema=None, normalizer=None) -> None:
    """script_util.py:79-90 (without the old-checkpoint cleanup, which is run management, not format).  ``ema``: a ``ParamEMA`` over the
    model's parameters, saved under ``'ema'`` (its ``state_dict()``); ``normalizer``: the latent ``Normalizer`` the model was trained behind,
    saved under ``'normalizer'``; the other keys are unchanged."""
    if logger is not None:
        logger.info(f"Saving model and optimizer state at iteration {iteration} to {checkpoint_path}")
    ck = {"model": _unwrap(model).state_dict(), "epoch": iteration,
          "optimizer": optimizer.state_dict() if optimizer is not None else None, "learning_rate": lr}
    if ema is not None:
        ck["ema"] = ema.state_dict(_unwrap(model))
    if normalizer is not None:
        ck["normalizer"] = normalizer.state_dict()
    torch.save(ck, checkpoint_path)


def load_checkpoint(checkpoint_path, model, logger=None, optimizer=None, ema=None, weights: str = "model", normalizer=None):
    """script_util.py:93-124: returns (model, optimizer, learning_rate, epoch).

    ``ema``: a ``ParamEMA`` over the model's parameters, restored from the file's ``'ema'`` entry; a file without one (a checkpoint of the
    reference, or of a run without EMA) seeds it from the weights loaded into the model.  ``weights="ema"`` loads the file's EMA weights into
    the model instead of ``'model'`` (sampling from the EMA); the file must have them.  ``normalizer``: a ``Normalizer``, restored from the
    file's ``'normalizer'`` entry; a file without one leaves it untouched, which is logged."""
    if weights not in ("model", "ema"):
        raise ValueError(f"weights must be 'model' or 'ema', not {weights!r}")
    assert os.path.isfile(checkpoint_path)
    ck = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    epoch, learning_rate = ck["epoch"], ck["learning_rate"]
    if weights == "ema" and ck.get("ema") is None:
        raise KeyError(f"{checkpoint_path} holds no EMA weights ('ema'): it was saved without an EMA; load weights='model'")
    if optimizer is not None:
        optimizer.load_state_dict(ck["optimizer"])
    saved = ck[weights]
    m = _unwrap(model)
    new_state = {}
    for k, v in m.state_dict().items():
        if k in saved:
            new_state[k] = saved[k]
        elif f"_orig_mod.{k}" in saved:
            new_state[k] = saved[f"_orig_mod.{k}"]
        else:
            if logger is not None:
                logger.info("%s is not in the checkpoint" % k)
            new_state[k] = v
    m.load_state_dict(new_state)
    _repack(m)
    if ema is not None:
        if ck.get("ema") is not None:
            ema.load_state_dict(ck["ema"], model=m)
        else:
            ema.load_state_dict(m.state_dict(), model=m)
            (logger or logging.getLogger(__name__)).info(f"{checkpoint_path} has no EMA weights: the EMA starts from the loaded '{weights}' weights")
    if normalizer is not None:
        if ck.get("normalizer") is not None:
            normalizer.load_state_dict(ck["normalizer"])
        else:
            (logger or logging.getLogger(__name__)).info(f"{checkpoint_path} has no latent normalizer: the one passed in is left as it is")
    if logger is not None:
        logger.info(f"Loaded checkpoint '{checkpoint_path}' (epoch {epoch})")
    return model, optimizer, learning_rate, epoch


def load_normalizer(checkpoint_path):
    """the ``Normalizer`` saved in the file's ``'normalizer'`` entry, or None for a file without one (``Jen1`` builds its normalizer from
    this when none is passed in).  The file is mapped, not read: only the entry's own tensors are touched."""
    assert os.path.isfile(checkpoint_path)
    try:
        ck = torch.load(checkpoint_path, map_location="cpu", weights_only=False, mmap=True)
    except (RuntimeError, ValueError):             # (a file in the legacy, non-zip format cannot be mapped)
        ck = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    if ck.get("normalizer") is None:
        return None
    from .normalizer import Normalizer
    return Normalizer.from_state_dict(ck["normalizer"])


def load_model_diffsize(checkpoint_path, model):
    """script_util.py:127-148: copy every tensor whose key (with or without ``_orig_mod.``) and size match."""
    assert os.path.isfile(checkpoint_path)
    saved = torch.load(checkpoint_path, map_location="cpu", weights_only=False)["model"]
    m = _unwrap(model)
    state = m.state_dict()
    for k, v in saved.items():
        k2 = k.replace("_orig_mod.", "")
        if k in state and state[k].size() == v.size():
            state[k] = v
        elif k2 in state and state[k2].size() == v.size():
            state[k2] = v
        else:
            print("[WARNING] Parameter mismatch :", k)
    m.load_state_dict(state, strict=False)
    _repack(m)
    return model


def _repack(m) -> None:
    inv = getattr(m, "_invalidate", None)
    if callable(inv):
        inv()
