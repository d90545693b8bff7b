"""Producers of global conditioning: ``IntConditioner`` / ``NumberConditioner`` / ``MultiConditioner`` of
/root/reference/jen1/conditioners.py:118-208 on the HIP path.

``NumberConditionerHIP`` and ``IntConditionerHIP`` take a list of numbers (tempo, key, seconds_start, ...) and return the reference's
``[emb [B, 1, D], ones [B, 1]]``; the arithmetic is one ``jen1_cond_embed`` launch per call (csrc/global_cond.hip).
``MultiConditionerHIP`` is ``MultiConditioner.forward`` on the callable protocol ``Jen1`` and the trainer use:
``(batch_metadata, device) -> {key: (emb, mask)}``; ``tasks.get_conditioning`` concatenates the entries named by
``global_cond_ids`` into ``conditioning["global_cond"]``, which the denoiser takes as ``features=``.

The weights are explicit inputs (``from_module`` of a reference-shaped module, or tensors) and carry the reference's ``state_dict``
keys.  Nothing saves them into the model checkpoint and no optimiser sees them: the reference's trainer builds its optimiser from
the denoiser's parameters only, exactly as for the text conditioner's ``proj_out``.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Any, Callable, Dict, Mapping, Sequence

import torch

from . import lib as L

KIND_INT, KIND_NUMBER = 0, 1


def _embed(values: torch.Tensor, kind: int, table: torch.Tensor, freq, bias, D: int, rows_or_half: int, lo: float, hi: float) -> torch.Tensor:
    """one ``jen1_cond_embed`` launch: values [n] float32 on the device -> [n, D] float32"""
    if values.device.type != "cuda":
        raise L.Jen1HipError("the Int / Number conditioners run on a ROCm GPU only (no CPU path exists in this package)")
    n = int(values.numel())
    out = torch.empty((n, D), dtype=torch.float32, device=values.device)
    if n == 0:
        return out
    s = torch.cuda.current_stream(values.device).cuda_stream
    L.check(L.load().jen1_cond_embed(values.data_ptr(), kind, table.data_ptr(), None if freq is None else freq.data_ptr(),
                                     None if bias is None else bias.data_ptr(), out.data_ptr(), n, D, rows_or_half, float(lo), float(hi),
                                     float(hi) - float(lo), s),       # (the range in double, rounded once: as the reference's Python forms it)
            "jen1_cond_embed")
    return out


class _ConditionerBase:
    _keys: Sequence[str] = ()

    def _tensors(self) -> Dict[str, torch.Tensor]:
        raise NotImplementedError

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """the reference module's keys (conditioners.py:118-170)"""
        return OrderedDict((k, v.detach().clone()) for k, v in self._tensors().items())

    def load_state_dict(self, sd: Mapping[str, Any]) -> None:
        mine = self._tensors()
        missing, extra = [k for k in mine if k not in sd], [k for k in sd if k not in mine]
        if missing or extra:
            raise KeyError(f"{type(self).__name__}.load_state_dict: missing {missing}, unexpected {extra}")
        for k, t in mine.items():
            v = torch.as_tensor(sd[k])
            if tuple(v.shape) != tuple(t.shape):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {k} has shape {tuple(v.shape)}, expected {tuple(t.shape)}")
            t.copy_(v.to(torch.float32))

    def _on(self, device):
        """the weights on ``device`` (moved once, like the reference's ``.to(device)`` of its modules)"""
        for name, t in list(self.__dict__.items()):
            if torch.is_tensor(t):
                setattr(self, name, t.to(device))          # (the same tensor when it is there already)

    def __call__(self, values, device=None):
        return self.forward(values, device)


class IntConditionerHIP(_ConditionerBase):
    """``IntConditioner(output_dim, min_val, max_val)`` (conditioners.py:118-136): clamp to [min_val, max_val], then the row of the
    ``[max_val - min_val + 1, output_dim]`` table.  As written in the reference the table is indexed with the clamped value ITSELF,
    ``min_val`` is not subtracted: with ``min_val > 0`` the first ``min_val`` rows are never read and values above
    ``max_val - min_val`` raise ``IndexError`` (torch's embedding lookup does).  Reproduced here, raised on the host."""

    def __init__(self, output_dim: int, min_val: int = 0, max_val: int = 512, weight: torch.Tensor = None):
        self.output_dim, self.min_val, self.max_val = int(output_dim), int(min_val), int(max_val)
        rows = self.max_val - self.min_val + 1
        if weight is None:
            weight = torch.randn((rows, self.output_dim))            # nn.Embedding's default
        weight = torch.as_tensor(weight).detach().to(torch.float32).contiguous()
        if tuple(weight.shape) != (rows, self.output_dim):
            raise ValueError(f"IntConditionerHIP: weight of shape {tuple(weight.shape)}, expected {(rows, self.output_dim)}")
        self.weight = weight

    @classmethod
    def from_module(cls, module) -> "IntConditionerHIP":
        """from a reference-shaped ``IntConditioner`` (``output_dim``, ``min_val``, ``max_val``, ``int_embedder.weight``)"""
        return cls(module.output_dim, module.min_val, module.max_val, module.int_embedder.weight)

    def _tensors(self):
        return {"int_embedder.weight": self.weight}

    @torch.no_grad()
    def forward(self, ints: Sequence[int], device=None):
        device = self.weight.device if device is None else device
        self._on(device)
        vals = [int(v) for v in ints]
        rows = self.weight.shape[0]
        for v in vals:
            c = min(max(v, self.min_val), self.max_val)
            if not 0 <= c < rows:
                raise IndexError(f"IntConditionerHIP: value {v} clamps to {c}, outside the table's {rows} rows (the reference indexes "
                                 "with the clamped value itself and does not subtract min_val)")
        x = torch.tensor(vals, dtype=torch.float32).to(self.weight.device)
        emb = _embed(x, KIND_INT, self.weight, None, None, self.output_dim, rows, self.min_val, self.max_val)
        return [emb.unsqueeze(1), torch.ones((len(vals), 1), device=self.weight.device)]


class NumberConditionerHIP(_ConditionerBase):
    """``NumberConditioner(output_dim, min_val, max_val)`` (conditioners.py:139-170) around ``NumberEmbedder`` (utils/module.py:82-101):
    clamp, normalise to [0, 1], ``[x, sin(2 pi x w), cos(2 pi x w)]`` with ``dim = 256`` learned frequencies, ``Linear(257, output_dim)``,
    no activation."""

    def __init__(self, output_dim: int, min_val: float = 0, max_val: float = 1, weights: torch.Tensor = None, weight: torch.Tensor = None,
                 bias: torch.Tensor = None, dim: int = 256):
        self.output_dim, self.min_val, self.max_val = int(output_dim), float(min_val), float(max_val)
        if not self.max_val > self.min_val:
            raise ValueError("NumberConditionerHIP: max_val must be greater than min_val")
        assert dim % 2 == 0
        half = dim // 2
        if weights is None:                  # torch's defaults, as the reference's fresh modules hold them
            weights = torch.randn((half,))
        if weight is None or bias is None:
            lin = torch.nn.Linear(dim + 1, self.output_dim)
            weight = lin.weight if weight is None else weight
            bias = lin.bias if bias is None else bias
        f32 = lambda t: torch.as_tensor(t).detach().to(torch.float32).contiguous()
        self.weights, self.weight, self.bias = f32(weights), f32(weight), f32(bias)
        if tuple(self.weights.shape) != (half,) or tuple(self.weight.shape) != (self.output_dim, dim + 1) or tuple(self.bias.shape) != (self.output_dim,):
            raise ValueError(f"NumberConditionerHIP: shapes {tuple(self.weights.shape)}, {tuple(self.weight.shape)}, {tuple(self.bias.shape)}; "
                             f"expected {(half,)}, {(self.output_dim, dim + 1)}, {(self.output_dim,)}")
        self.half = half

    @classmethod
    def from_module(cls, module) -> "NumberConditionerHIP":
        """from a reference-shaped ``NumberConditioner`` (``embedder.embedding`` = [LearnedPositionalEmbedding, Linear])"""
        pos, lin = module.embedder.embedding[0], module.embedder.embedding[1]
        return cls(module.output_dim, module.min_val, module.max_val, pos.weights, lin.weight, lin.bias, dim=2 * pos.weights.numel())

    def _tensors(self):
        return {"embedder.embedding.0.weights": self.weights, "embedder.embedding.1.weight": self.weight,
                "embedder.embedding.1.bias": self.bias}

    @torch.no_grad()
    def forward(self, floats: Sequence[float], device=None):
        device = self.weight.device if device is None else device
        self._on(device)
        vals = [float(v) for v in floats]
        x = torch.tensor(vals, dtype=torch.float32).to(self.weight.device)
        emb = _embed(x, KIND_NUMBER, self.weight, self.weights, self.bias, self.output_dim, self.half, self.min_val, self.max_val)
        return [emb.unsqueeze(1), torch.ones((len(vals), 1), device=self.weight.device)]


class MultiConditionerHIP:
    """``MultiConditioner.forward`` (conditioners.py:173-208): every conditioner gets the list of its key's values over the batch.
    The reference's rules as written: a key missing from a row falls back to ``default_keys[key]`` (and, as written, STAYS switched for
    the rows after it), else ``ValueError``; a ``list`` value of any length, or a 1-tuple, is unwrapped to its first element.
    A conditioner is anything with ``forward(values, device)`` (``T5ConditionerHIP``, the two above) or a plain callable."""

    def __init__(self, conditioners: Dict[str, Callable], default_keys: Dict[str, str] = {}):
        self.conditioners = dict(conditioners)
        self.default_keys = dict(default_keys)

    def __call__(self, batch_metadata: Sequence[Dict[str, Any]], device) -> Dict[str, Any]:
        output = {}
        for key, conditioner in self.conditioners.items():
            condition_key = key
            inputs = []
            for x in batch_metadata:
                if condition_key not in x:
                    if condition_key in self.default_keys:
                        condition_key = self.default_keys[condition_key]
                    else:
                        raise ValueError(f"Conditioner key {condition_key} not found in batch metadata")
                v = x[condition_key]
                if isinstance(v, list) or isinstance(v, tuple) and len(v) == 1:       # conditioners.py:200-204, precedence included
                    inputs.append(v[0])
                else:
                    inputs.append(v)
            fwd = getattr(conditioner, "forward", conditioner)
            output[key] = fwd(inputs, device)
        return output

    forward = __call__
