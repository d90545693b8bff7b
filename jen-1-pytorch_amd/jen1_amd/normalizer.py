"""Whitening of the Encodec latents: the ``Normalizer`` the reference ships as an empty stub (jen1/normalizer.py: ``__init__(self, dim)``,
``forward(self, x): ...``, called by nothing), filled in as the JEN-1 paper describes it -- the latents are brought to zero mean per
channel and identity covariance before the diffusion sees them, the statistics gathered batch by batch over the data set.

  update     ``jen1_latent_moments`` adds a batch's frame count, ``sum z_c`` and ``sum z_c z_d`` to a float64 state ``[1 + C + C C]`` on
             the device (csrc/latent_norm.hip; float64 from the first product on, no host synchronisation).  States add: ``merge``, and a
             SUM all-reduce under DDP (``all_reduce``).
  finalize   on the host in float64: mean, covariance, ``torch.linalg.eigh``, eigenvalues floored at ``eps * lambda_max``, W and W^-1 both
             from the floored eigenvalues (``whitening``); rounded to float32 buffers.
  normalize / denormalize   ``jen1_latent_affine``: ``W (z - mean)`` and ``W^-1 z + mean`` on the exact-float32 matrix instructions.

There is no CPU path for ``update`` / ``normalize`` / ``denormalize``: they raise on tensors that are not on a GPU.  Not here: the
paper's PCA dimension REDUCTION (the denoiser's 128 input channels are fixed by the checkpoint schema).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import nn

from . import audio_host as H
from . import lib as L

KINDS = ("zca", "pca", "diag")


def state_words(dim: int) -> int:
    return 1 + dim + dim * dim


def latent_moments(z: torch.Tensor, host_lengths, state: torch.Tensor) -> torch.Tensor:
    """add the frame count, ``sum z_c`` and ``sum z_c z_d`` of ``z [B, C, T]`` (float32, contiguous, on a GPU) to ``state`` (float64
    ``[state_words(C)]``, moved to z's device first) and return it; ``host_lengths``: a ``c_int`` array of the valid frames per row, or None"""
    B, C, T = z.shape
    if state.device != z.device:
        state = state.to(z.device)
    nbytes = int(L.load().jen1_latent_moments_workspace(B, C, T))
    work = H.workspace(nbytes, z.device)
    H.launch(z.device, "jen1_latent_moments", z.data_ptr(), host_lengths, state.data_ptr(), work.data_ptr(), nbytes, B, C, T)
    return state


def whitening(state: torch.Tensor, kind: str = "zca", eps: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """moments ``[1 + C + C C]`` (n, S1, S2) -> (mean [C], W [C, C], W^-1 [C, C]), float64 on the CPU.
      "zca"   W = U L^-1/2 U^T      (the whitening closest to the identity: channels keep their meaning)
      "pca"   W = L^-1/2 U^T
      "diag"  W = diag(1 / std): per-channel scaling only, the latent-diffusion rule the paper contrasts itself with
    with cov = U L U^T and L floored at ``eps * lambda_max`` (the variances at ``eps`` times the largest one for "diag"); W^-1 is built
    from the same floored values, so W W^-1 = I by construction, whatever the rank of the data."""
    if kind not in KINDS:
        raise ValueError(f"unknown kind {kind!r}: one of {KINDS}")
    if not eps > 0.0:
        raise ValueError(f"eps must be positive, not {eps!r}")
    s = state.detach().to("cpu", torch.float64).reshape(-1)
    C = int(round((-1 + (1 + 4 * (s.numel() - 1)) ** 0.5) / 2))
    if state_words(C) != s.numel():
        raise ValueError(f"a state of {s.numel()} words is not 1 + C + C C for any C")
    n = float(s[0])
    if n < C + 1:
        raise ValueError(f"{int(n)} frames are too few to whiten {C} channels: at least C + 1 = {C + 1} are needed")
    mean = s[1:1 + C] / n
    # S2 / n - mean mean^T cancels: each entry carries an absolute error of about (mean^2 + var) 2^-53, i.e. a RELATIVE error of
    # (mean / std)^2 2^-53 on a variance.  A mean of 50 standard deviations costs 2500 x 1.1e-16 = 3e-13: float64 sums make the
    # one-pass form safe where float32 sums (2500 x 6e-8 = 1.5e-4) would not be.
    cov = s[1 + C:].reshape(C, C) / n - torch.outer(mean, mean)
    cov = 0.5 * (cov + cov.T)
    if kind == "diag":
        var = torch.diagonal(cov).clone()
        top = float(var.max())
        if not top > 0.0:
            raise ValueError("the latents are constant: there is no variance to normalise")
        std = var.clamp_min(eps * top).sqrt()
        return mean, torch.diag(1.0 / std), torch.diag(std)
    lam, U = torch.linalg.eigh(cov)
    top = float(lam.max())
    if not top > 0.0:
        raise ValueError("the latents are constant: there is no variance to normalise")
    root = lam.clamp_min(eps * top).sqrt()
    if kind == "zca":
        return mean, (U / root) @ U.T, (U * root) @ U.T
    return mean, U.T / root[:, None], U * root


class Normalizer(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        dim = int(dim)
        if dim < 16 or dim > 128 or dim % 16 != 0:
            raise ValueError(f"dim = {dim}: the kernels take a multiple of 16 in 16..128")
        self.dim = dim
        self.kind: Optional[str] = None            # None until finalize; "identity" for Normalizer.identity
        self.eps: Optional[float] = None
        self.register_buffer("state", torch.zeros(state_words(dim), dtype=torch.float64))
        self.register_buffer("mean", torch.zeros(dim, dtype=torch.float32))
        self.register_buffer("weight", torch.eye(dim, dtype=torch.float32))
        self.register_buffer("inverse", torch.eye(dim, dtype=torch.float32))

    @classmethod
    def identity(cls, dim: int) -> "Normalizer":
        """a normalizer that is ready without a fit and maps every latent to itself (W = W^-1 = I, no mean)"""
        self = cls(dim)
        self.kind = "identity"
        return self

    @property
    def fitted(self) -> bool:
        return self.kind is not None

    # ------------------------------------------------------------------ statistics
    def _check(self, z: torch.Tensor, what: str) -> torch.Tensor:
        if z.dim() != 3 or z.shape[1] != self.dim or z.shape[0] < 1 or z.shape[2] < 1:
            raise ValueError(f"{what}: latents must be [B, {self.dim}, T] with B, T >= 1, not {tuple(z.shape)}")
        if z.dtype != torch.float32:
            raise TypeError(f"{what}: latents must be float32, not {z.dtype}")
        H.gpu_device(z.device, what)
        return z.contiguous()

    @torch.no_grad()
    def update(self, z: torch.Tensor, lengths=None) -> "Normalizer":
        """add the frames of ``z [B, C, T]`` (float32, on a GPU) to the state; ``lengths`` (host integers, one per row, each in 0..T):
        the valid frames of every row -- frames at or beyond ``lengths[b]`` do not count.  No host synchronisation."""
        z = self._check(z, "Normalizer.update")
        host = None if lengths is None else H.c_ints(H.host_ints(lengths, int(z.shape[0]), "lengths"))
        self.state = latent_moments(z, host, self.state)
        return self

    @torch.no_grad()
    def merge(self, other: "Normalizer") -> "Normalizer":
        """add the statistics ``other`` has gathered: the states are sums, so the result is the fit over both data sets"""
        if other.dim != self.dim:
            raise ValueError(f"cannot merge a normalizer of {other.dim} channels into one of {self.dim}")
        self.state += other.state.to(self.state.device)
        return self

    def all_reduce(self, group=None) -> "Normalizer":
        """SUM all-reduce of the state over ``group``: every rank ends with the statistics of all ranks' batches"""
        import torch.distributed as dist
        dist.all_reduce(self.state, op=dist.ReduceOp.SUM, group=group)
        return self

    @torch.no_grad()
    def fit(self, loader, max_batches: Optional[int] = None, kind: str = "zca", eps: float = 1e-6) -> "Normalizer":
        """``update`` over the ``(emb, metadata)`` batches of ``loader`` (at most ``max_batches`` of them), then ``finalize``.  A batch may
        carry the valid frames of its rows as a third entry (``LatentCollate(with_lengths=True)``)."""
        for i, batch in enumerate(loader):
            if max_batches is not None and i >= max_batches:
                break
            self.update(batch[0], batch[2] if len(batch) > 2 else None)
        return self.finalize(kind, eps)

    @torch.no_grad()
    def finalize(self, kind: str = "zca", eps: float = 1e-6) -> "Normalizer":
        """the state -> ``mean``, ``weight`` (W) and ``inverse`` (W^-1), float32 buffers on the state's device (``whitening``); the state is
        kept, so the fit can be continued and finalized again.  Raises with fewer than C + 1 frames."""
        mean, W, Winv = whitening(self.state, kind, eps)
        dev = self.state.device
        self.mean = mean.to(dev, torch.float32)
        self.weight = W.to(dev, torch.float32).contiguous()
        self.inverse = Winv.to(dev, torch.float32).contiguous()
        self.kind, self.eps = kind, float(eps)
        return self

    # ------------------------------------------------------------------ the map
    def _affine(self, z: torch.Tensor, inverse: bool, what: str) -> torch.Tensor:
        if not self.fitted:
            raise RuntimeError(f"{what}: the normalizer has not been fitted (update + finalize, fit, load_state_dict or Normalizer.identity)")
        z = self._check(z, what)
        B, C, T = z.shape
        if self.weight.device != z.device:
            self.to(z.device)
        mean = None if self.kind == "identity" else self.mean.data_ptr()
        A, pre, post = (self.inverse, None, mean) if inverse else (self.weight, mean, None)
        y = torch.empty_like(z)
        H.launch(z.device, "jen1_latent_affine", z.data_ptr(), y.data_ptr(), A.data_ptr(), pre, post, B, C, T)
        return y

    @torch.no_grad()
    def normalize(self, z: torch.Tensor) -> torch.Tensor:
        """``W (z - mean)``: float32 ``[B, C, T]`` on z's device (the buffers follow the latents to their GPU)"""
        return self._affine(z, False, "Normalizer.normalize")

    @torch.no_grad()
    def denormalize(self, z: torch.Tensor) -> torch.Tensor:
        """``W^-1 z + mean``: the inverse of ``normalize``"""
        return self._affine(z, True, "Normalizer.denormalize")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.normalize(x)

    # ------------------------------------------------------------------ persistence
    def state_dict(self, *args, **kwargs):
        """the raw state (a loaded fit can be continued), the fitted ``mean`` / ``weight`` / ``inverse``, ``kind`` (None before a fit) and
        ``eps``; tensors on the CPU"""
        cpu = lambda t: t.detach().to("cpu").clone()
        return {"dim": self.dim, "state": cpu(self.state), "mean": cpu(self.mean), "weight": cpu(self.weight), "inverse": cpu(self.inverse),
                "kind": self.kind, "eps": self.eps}

    def load_state_dict(self, sd, *args, **kwargs):
        if int(sd["dim"]) != self.dim:
            raise ValueError(f"the saved normalizer has {sd['dim']} channels, this one {self.dim}")
        with torch.no_grad():
            for k in ("state", "mean", "weight", "inverse"):
                buf = getattr(self, k)
                if tuple(sd[k].shape) != tuple(buf.shape):
                    raise ValueError(f"{k}: shape {tuple(sd[k].shape)} in the file, {tuple(buf.shape)} here")
                buf.copy_(sd[k].to(buf.device, buf.dtype))
        self.kind, self.eps = sd["kind"], sd["eps"]
        return self

    @classmethod
    def from_state_dict(cls, sd) -> "Normalizer":
        return cls(int(sd["dim"])).load_state_dict(sd)
