"""Exponential moving average (EMA) of the trained weights, updated inside the optimiser step.

The reference's training config has a ``use_ema`` switch (utils/config.py:90) with no code behind it; this is that code.  The
EMA is one more flat float32 buffer beside ``FusedAdamW.flat_param`` (same length, same per-tensor offsets), and while a
``ParamEMA`` is attached the optimiser launches ``jen1_adamw_ema_step_counted``: clip + AdamW + EMA in ONE pass over the flat
buffers, the EMA schedule decided on the device from the optimiser's step counter (no host synchronisation, capturable).

Schedule of optimiser step ``t`` (1-based; a step dropped by ``skip_nonfinite`` does not count), ``ema_schedule``:
  * ``t % update_every != 0``: the EMA is left alone;
  * ``t <= update_after_step``: the EMA is a copy of the new parameters;
  * otherwise, with ``k = t - update_after_step``: ``decay = clamp(1 - (1 + k / inv_gamma) ** -power, min_decay, beta)`` with
    ``warmup`` (``beta`` without), and ``ema += (1 - decay) * (p - ema)``.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Tuple

import torch

from . import lib as L
from .optim import FusedAdamW

SKIP, COPY, UPDATE = 0, 1, 2


def ema_schedule(t: int, beta: float = 0.9999, update_after_step: int = 100, update_every: int = 10, warmup: bool = True,
                 inv_gamma: float = 1.0, power: float = 2.0 / 3.0, min_decay: float = 0.0) -> Tuple[int, float]:
    """what the fused kernel does to the EMA at optimiser step ``t``: ``(SKIP | COPY | UPDATE, decay)`` (decay in double, as on the device;
    0.0 unless UPDATE)"""
    if t % update_every != 0:
        return SKIP, 0.0
    if t <= update_after_step:
        return COPY, 0.0
    if not warmup:
        return UPDATE, float(beta)
    k = float(t - update_after_step)
    decay = 1.0 - (1.0 + k / inv_gamma) ** (-power)
    return UPDATE, max(min(decay, float(beta)), float(min_decay))


class ParamEMA:
    """EMA of the parameters of ``optimizer`` (a ``FusedAdamW``), kept on the device and updated in the optimiser's own launch.

    Construction copies the current parameters into the EMA and attaches it: from then on ``optimizer.step()`` runs the fused entry.
    The EMA's step count is the optimiser's (``optimizer.step_count``), so it is saved and restored with the optimiser state.
    ``model`` (keyword-only): the module the parameters belong to; its parameter names key ``state_dict`` (the optimiser itself only
    holds the tensors).  Without it, ``state_dict`` / ``load_state_dict`` / ``copy_to`` take the model as an argument."""

    def __init__(self, optimizer: FusedAdamW, beta: float = 0.9999, update_after_step: int = 100, update_every: int = 10,
                 warmup: bool = True, inv_gamma: float = 1.0, power: float = 2.0 / 3.0, min_decay: float = 0.0, *, model=None):
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError(f"ParamEMA needs a FusedAdamW, got {type(optimizer).__name__}")
        if not (0.0 <= min_decay <= beta < 1.0):
            raise ValueError(f"need 0 <= min_decay <= beta < 1 (beta={beta}, min_decay={min_decay})")
        if int(update_every) < 1 or int(update_after_step) < 0 or inv_gamma <= 0.0 or power <= 0.0:
            raise ValueError("need update_every >= 1, update_after_step >= 0, inv_gamma > 0, power > 0")
        self.optimizer = optimizer
        self.beta, self.update_after_step, self.update_every = float(beta), int(update_after_step), int(update_every)
        self.warmup, self.inv_gamma, self.power, self.min_decay = bool(warmup), float(inv_gamma), float(power), float(min_decay)
        self.ema = optimizer.flat_param.detach().clone()
        self._swapped = False
        self._bound: Optional[Dict[int, str]] = self._names(model) if model is not None else None
        optimizer.ema = self

    # ------------------------------------------------------------------ schedule / launch
    def schedule(self, t: int) -> Tuple[int, float]:
        """``ema_schedule`` with this EMA's settings"""
        return ema_schedule(t, self.beta, self.update_after_step, self.update_every, self.warmup, self.inv_gamma, self.power, self.min_decay)

    def launch(self, lib, opt: FusedAdamW, lr: float, gn, stream) -> None:
        """``FusedAdamW.step``'s update launch when this EMA is attached (same arguments as ``jen1_adamw_step_counted`` + the EMA's)"""
        if self._swapped:
            raise RuntimeError("FusedAdamW.step inside ParamEMA.swap: the model holds the EMA weights")
        L.check(lib.jen1_adamw_ema_step_counted(opt.flat_param.data_ptr(), opt.flat_grad.data_ptr(), opt.exp_avg.data_ptr(),
                                                opt.exp_avg_sq.data_ptr(), opt.numel, float(lr), float(opt.betas[0]), float(opt.betas[1]),
                                                float(opt.eps), float(opt.weight_decay), opt._steps.data_ptr(), gn, float(opt.max_norm or 0.0),
                                                1 if opt.skip_nonfinite else 0, self.ema.data_ptr(), self.beta, self.update_after_step,
                                                self.update_every, 1 if self.warmup else 0, self.inv_gamma, self.power, self.min_decay, stream),
                "jen1_adamw_ema_step_counted")

    def detach(self) -> None:
        """stop updating: ``optimizer.step()`` launches the plain AdamW entry again"""
        if getattr(self.optimizer, "ema", None) is self:
            self.optimizer.ema = None

    # ------------------------------------------------------------------ weights
    def _views(self):
        for p, o in zip(self.optimizer.params, self.optimizer.offsets):
            yield p, self.ema[o:o + p.numel()].view_as(p)

    def _names(self, model) -> Dict[int, str]:
        names = {id(p): n for n, p in model.named_parameters()}
        missing = [i for i, p in enumerate(self.optimizer.params) if id(p) not in names]
        if missing:
            raise ValueError(f"{len(missing)} optimiser parameters are not parameters of the model")
        return names

    def state_dict(self, model=None) -> Dict[str, torch.Tensor]:
        """the EMA weights under the model's parameter names (the reference's ``state_dict`` key schema), float32 CPU tensors.
        ``model``: where the names come from (default: the model given at construction)"""
        names = self._names(model) if model is not None else self._bound_names()
        return {names[id(p)]: v.detach().to("cpu", copy=True).contiguous() for p, v in self._views()}

    def load_state_dict(self, sd: Dict[str, torch.Tensor], model=None) -> None:
        """restore the EMA weights from ``state_dict()``'s form (a ``_orig_mod.`` prefix is accepted, as for the model).  Every parameter
        must be present with its shape"""
        names = self._names(model) if model is not None else self._bound_names()
        for p, v in self._views():
            k = names[id(p)]
            src = sd[k] if k in sd else sd.get(f"_orig_mod.{k}")
            if src is None:
                raise KeyError(f"EMA weights lack {k!r}")
            if tuple(src.shape) != tuple(p.shape):
                raise ValueError(f"EMA weight {k!r} has shape {tuple(src.shape)}, the parameter {tuple(p.shape)}")
            v.copy_(src.to(torch.float32))

    def _bound_names(self) -> Dict[int, str]:
        if self._bound is None:
            raise ValueError("ParamEMA: pass the model (here or as ParamEMA(..., model=)) to name the EMA weights")
        return self._bound

    def copy_to(self, model, source=None) -> None:
        """write the EMA weights into ``model`` (any ``UNetCFG1d`` with the same key schema, on any device) and drop its packed copies.
        ``source``: the trained model, when none was given at construction (it names the weights)"""
        sd = self.state_dict(source)
        own = dict(model.named_parameters())
        missing = [k for k in sd if k not in own]
        if missing:
            raise KeyError(f"the model lacks EMA weights {missing[:4]}")
        with torch.no_grad():
            for k, v in sd.items():
                if tuple(own[k].shape) != tuple(v.shape):
                    raise ValueError(f"{k!r}: model shape {tuple(own[k].shape)}, EMA {tuple(v.shape)}")
                own[k].copy_(v)
        inv = getattr(model, "_invalidate", None)
        if callable(inv):
            inv()

    @contextlib.contextmanager
    def swap(self, model=None):
        """inside the block the optimiser's parameters (``model``'s) are views of the EMA buffer -- pointers exchanged, nothing copied --
        so ``model(...)`` / ``diffusion.sample(model, ...)`` run on the EMA weights.  The optimiser's ``post_step_hooks`` run on entry and
        on exit (the training compute copies and the sampling engine re-pack); ``model``, when given, is invalidated too.  Training after
        the block continues exactly as if it had not been entered.  No optimiser step inside the block."""
        if self._swapped:
            raise RuntimeError("ParamEMA.swap is not re-entrant")
        opt = self.optimizer
        if model is not None:
            names = self._names(model)           # the model's parameters are the optimiser's
            if self._bound is None:
                self._bound = names
        for p, v in self._views():
            p.data = v
        self._swapped = True
        try:
            self._repack(model)
            yield self
        finally:
            for p, o in zip(opt.params, opt.offsets):
                p.data = opt.flat_param[o:o + p.numel()].view_as(p)
            self._swapped = False
            self._repack(model)

    def _repack(self, model) -> None:
        for h in self.optimizer.post_step_hooks:
            h()
        inv = getattr(model, "_invalidate", None) if model is not None else None
        if callable(inv):
            inv()

