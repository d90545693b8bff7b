"""Long-form sampling: overlapping sampler windows merged on a shared canvas (the MultiDiffusion scheme; not in the reference).

The latents of a piece live on one canvas ``[n, C, L]``.  At every sampler step each of the ``W`` windows of ``T`` frames is denoised as
an ordinary batch row (row ``s * W + j`` = window ``j`` of piece ``s``); after the update the windows are averaged where they overlap,
with the cross-fade weights ``k(p) = min(p + 1, T - p, ramp)``, and every window is set back to the merged values, so all windows are
crops of one canvas again before the next step.  Every sampler update here is linear in ``(x, eps / v / x0)``, so merging ``x`` after
the update (and the DPM-Solver++ history) is the whole algorithm: the denoiser, its plans and the captured graph of a stepper are
untouched.  The two kernels are ``jen1_window_merge`` and ``jen1_window_gather`` (csrc/windows.hip).

``WindowPlan`` is the host side: the offsets, the coverage check, and ``gather`` / ``merge_`` over the two entry points.
``sample_fused`` drives a ``DDIMStepper`` through its schedule with the merge between the steps (``GaussianDiffusion.sample_windows``
and ``VDM.sample_windows`` call it); ``literal_draws`` prepares the same trajectory for the literal loops' ``edit`` callback.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import lib as L


class WindowPlan:
    """``W = 1 + ceil((length - window) / hop)`` windows of ``window`` frames on a canvas of ``length`` frames, window ``j`` at
    ``min(j * hop, length - window)``: the last one is pulled in, so the overlaps may be uneven.  ``ramp`` is the length of the
    cross-fade at a window's edges (default ``window - hop``, at least 1): the weight numerator of window position ``p`` is the integer
    ``min(p + 1, window - p, ramp)``."""

    def __init__(self, length: int, window: int, hop: int, ramp: Optional[int] = None):
        length, window, hop = int(length), int(window), int(hop)
        if window < 1 or length < window:
            raise ValueError(f"WindowPlan: the canvas ({length} frames) is shorter than a window ({window} frames)")
        if hop < 1:
            raise ValueError(f"WindowPlan: hop = {hop}, must be at least 1")
        if hop > window:
            raise ValueError(f"WindowPlan: hop = {hop} exceeds the window ({window} frames): that would leave a gap")
        ramp = max(1, window - hop) if ramp is None else int(ramp)
        if not 1 <= ramp <= window:
            raise ValueError(f"WindowPlan: ramp = {ramp}, must be in [1, window = {window}]")
        self.length, self.window, self.hop, self.ramp = length, window, hop, ramp
        self.W = 1 + -(-(length - window) // hop)
        self.offsets: List[int] = [min(j * hop, length - window) for j in range(self.W)]
        self._check_coverage()
        self._dev: Dict[torch.device, torch.Tensor] = {}

    def _check_coverage(self) -> None:
        """ascending offsets inside the canvas that leave no frame uncovered (the kernels take the table as it is)"""
        o, T = self.offsets, self.window
        ok = o[0] == 0 and o[-1] == self.length - T and all(a < b <= a + T for a, b in zip(o, o[1:]))
        if not ok:
            raise ValueError(f"WindowPlan: the offsets {o} do not cover the canvas of {self.length} frames with windows of {T}")

    def __repr__(self) -> str:
        return f"WindowPlan(length={self.length}, window={self.window}, hop={self.hop}, ramp={self.ramp}: W={self.W})"

    def offsets_on(self, device) -> torch.Tensor:
        """the offsets as a device int32 [W] tensor, created once per device"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = torch.tensor(self.offsets, dtype=torch.int32, device=device)
        return t

    def weights(self, normalised: bool = False) -> torch.Tensor:
        """the cross-fade weights, float32 [W, window] (for tests and documents; the kernel works on the integers): ``k(p) / ramp``, in
        ``[1 / ramp, 1]`` and the same for every window; ``normalised=True``: ``k_j(p) / sum of k over the windows covering that canvas
        frame``, what the merge amounts to (the kernel divides the weighted sum by the integer sum once)"""
        T = self.window
        p = torch.arange(T)
        k = torch.minimum(torch.minimum(p + 1, T - p), torch.tensor(self.ramp)).to(torch.float64)
        if not normalised:
            return (k / self.ramp).to(torch.float32).expand(self.W, T).contiguous()
        total = torch.zeros(self.length, dtype=torch.float64)
        for off in self.offsets:
            total[off:off + T] += k
        return torch.stack([k / total[off:off + T] for off in self.offsets]).to(torch.float32)

    def starts_seconds(self, frames_per_second: float) -> List[float]:
        """where every window starts, in seconds (``seconds_start`` style conditioning per window)"""
        return [off / float(frames_per_second) for off in self.offsets]

    # ------------------------------------------------------------------ the two launches
    def _rows_shape(self, canvas_shape):
        if len(canvas_shape) not in (3, 4) or canvas_shape[-1] != self.length:
            raise ValueError(f"a canvas is [n, C, {self.length}] (or [lead, n, C, {self.length}]), not {tuple(canvas_shape)}")
        *lead, n, C, _ = canvas_shape
        return tuple(lead) + (n * self.W, C, self.window)

    def gather(self, canvas: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """canvas ``[n, C, L]`` (or ``[lead, n, C, L]``: a per-step table) -> the windows' rows ``[n W, C, T]`` (``[lead, n W, C, T]``), bit for
        bit, in one ``jen1_window_gather`` launch; ``out``: write into this tensor.  A plan of one window returns the canvas itself"""
        shape = self._rows_shape(tuple(canvas.shape))
        if canvas.dtype != torch.float32 or not canvas.is_cuda:
            raise ValueError("gather: a float32 tensor on the GPU")
        canvas = canvas.contiguous()
        if self.W == 1 and out is None:
            return canvas
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=canvas.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != canvas.device:
            raise ValueError(f"gather: out must be a contiguous float32 {shape} tensor on {canvas.device}")
        lead = shape[0] if len(shape) == 4 else 1
        n, C = canvas.shape[-3], canvas.shape[-2]
        s = torch.cuda.current_stream(canvas.device).cuda_stream
        L.check(L.load().jen1_window_gather(canvas.data_ptr(), out.data_ptr(), self.offsets_on(canvas.device).data_ptr(), lead, n, self.W, C,
                                            self.window, self.length, s), "jen1_window_gather")
        torch.autograd.graph.increment_version(out)
        return out

    def merge_(self, rows: torch.Tensor, canvas: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """merge the windows' rows ``[n W, C, T]`` in place (``jen1_window_merge``); ``canvas`` ``[n, C, L]``: also write the merged canvas
        there.  Returns ``canvas``.  The launch writes through the raw pointer, so the tensor's version counter is bumped here
        (``torch.autograd.graph.increment_version``, no launch): a stepper whose latents were merged notices it like any in-place torch
        write and re-packs its network input, no ``mark_dirty()`` at the call site.  A plan of one window launches nothing"""
        if rows.dim() != 3 or rows.shape[0] % self.W or rows.shape[2] != self.window:
            raise ValueError(f"merge_: rows are [n * {self.W}, C, {self.window}], not {tuple(rows.shape)}")
        if rows.dtype != torch.float32 or not rows.is_cuda or not rows.is_contiguous():
            raise ValueError("merge_: a contiguous float32 tensor on the GPU")
        n, C = rows.shape[0] // self.W, rows.shape[1]
        if canvas is not None and (tuple(canvas.shape) != (n, C, self.length) or canvas.dtype != torch.float32 or not canvas.is_contiguous()
                                   or canvas.device != rows.device):
            raise ValueError(f"merge_: canvas must be a contiguous float32 {(n, C, self.length)} tensor on {rows.device}")
        if self.W == 1:
            if canvas is not None:
                canvas.copy_(rows)
            return canvas
        s = torch.cuda.current_stream(rows.device).cuda_stream
        L.check(L.load().jen1_window_merge(rows.data_ptr(), self.offsets_on(rows.device).data_ptr(), n, self.W, C, self.window, self.length,
                                           self.ramp, None if canvas is None else canvas.data_ptr(), s), "jen1_window_merge")
        torch.autograd.graph.increment_version(rows)
        if canvas is not None:
            torch.autograd.graph.increment_version(canvas)
        return canvas


# ---------------------------------------------------------------------- the sampler loops
def check_canvas_args(plan: WindowPlan, n: int, C: int, conditioning, **canvas_tensors) -> None:
    """ValueError before anything is launched: the conditioning has one row per window, the injected tensors are canvases"""
    rows = n * plan.W
    emb = None if conditioning is None else conditioning.get("cross_attn_cond")
    if emb is not None and emb.shape[0] != rows:
        raise ValueError(f"sample_windows: the conditioning has {emb.shape[0]} rows, {n} pieces of {plan.W} windows need {rows}")
    for name, (t, ch) in canvas_tensors.items():
        if t is not None and tuple(t.shape) != (n, ch, plan.length):
            raise ValueError(f"sample_windows: {name} is given on the canvas, {(n, ch, plan.length)}, not {tuple(t.shape)}")


def _canvas(t, device):
    return None if t is None else t.detach().to(device, torch.float32).contiguous()


def _dropout(sampler, B: int, dropout_rows, i: int):
    """the CFG-dropout rows of step i as the samplers draw them (``GaussianDiffusion._fused_loop``)"""
    p = sampler.cfg_dropout_proba
    if p <= 0.0:
        return None
    if dropout_rows is not None:
        return torch.as_tensor(dropout_rows[i])
    if p >= 1.0:
        return torch.ones(B, dtype=torch.bool)
    return torch.bernoulli(torch.full((B,), float(p), device=sampler.device)).to(torch.bool)


def sample_fused(sampler, st, plan: WindowPlan, n: int, *, init_noise=None, step_noises: Optional[Sequence[torch.Tensor]] = None,
                 dropout_rows=None, known=None, keep_mask=None, known_noise=None) -> torch.Tensor:
    """one windowed trajectory on the fused stepper ``st`` (its batch rows are the ``n * plan.W`` windows): every draw is made on the
    canvas and gathered, so overlapping windows see identical noise and identical known audio at a shared frame; after every step the
    latents (and the multistep history) are merged.  Returns the canvas ``[n, C, L]``"""
    if len(st.parts) != 1:
        raise RuntimeError("sample_windows: the stepper splits its batch over several parts (n_streams > 1); the merge works on one "
                           "tensor holding every window, and merging per-part copies would not reach the sampler")
    dev = sampler.device
    B, C, T = st.shape
    assert B == n * plan.W and T == plan.window
    cshape = (n, C, plan.length)
    start = torch.randn(cshape, device=dev) if init_noise is None else _canvas(init_noise, dev).reshape(cshape)
    noisy = st.mode in ("ddim", "ddpm")
    if noisy and step_noises is None:                  # the whole per-step table, drawn on the canvas, into the stepper's in one launch
        table = torch.empty((st.num_steps,) + cshape, dtype=torch.float32, device=dev)
        table.normal_() if st.mode == "ddim" else table.uniform_()       # (p_sample draws rand_like, as written: gdm.py:161)
        plan.gather(table, out=st.noise_all)
        del table
    if known is not None:
        st.set_known(plan.gather(known), plan.gather(keep_mask), noise=plan.gather(start if known_noise is None else known_noise))
    st.reset(plan.gather(start), fresh_noise=False)
    S = st.num_steps
    out = None
    for i in range(S):
        noise = None
        if noisy and step_noises is not None and i < len(step_noises) and i < S - 1:
            noise = plan.gather(_canvas(step_noises[i], dev).reshape(cshape))
        st.step(i, noise=noise, drop_rows=_dropout(sampler, B, dropout_rows, i), set_rows=sampler.cfg_dropout_proba > 0.0)
        if plan.W > 1:
            if i == S - 1:
                out = plan.merge_(st.x, torch.empty(cshape, dtype=torch.float32, device=dev))
            else:
                plan.merge_(st.x)                      # (bumps the version of st.x: the next step re-packs the network input)
                for h in st.hist:                      # dpmpp: the history becomes the merged clipped x0
                    plan.merge_(h)
    if out is None:
        out = st.x.clone()
    st.check()
    return finish_known(out, known, keep_mask)


def finish_known(canvas: torch.Tensor, known, keep_mask) -> torch.Tensor:
    """the last step leaves the known latents in the kept frames of every window, and the merge of equal values may round
    (k1 x + k2 x) / (k1 + k2) one ulp off x: the kept frames of the returned canvas are set to the known latents once more (the
    blend at the level (1, 0) of the step that ends at x0, an exact select for a 0 / 1 mask)"""
    if known is None:
        return canvas
    from .diffusion import blend_known
    return blend_known(canvas, known, keep_mask, known, 1.0, 0.0)


def literal_draws(sampler, plan: WindowPlan, n: int, C: int, S: int, uniform: bool, noisy: bool, init_noise, step_noises, known, keep_mask,
                  known_noise):
    """the inputs of a literal sampling loop over the ``n * plan.W`` window rows: (start rows, per-step noise rows or None, known /
    keep / known-noise rows or None), every draw made on the canvas and gathered"""
    dev = sampler.device
    cshape = (n, C, plan.length)
    start = torch.randn(cshape, device=dev) if init_noise is None else _canvas(init_noise, dev).reshape(cshape)
    noises = None
    if noisy:
        draw = torch.rand if uniform else torch.randn
        noises = [plan.gather(draw(cshape, device=dev) if step_noises is None or i >= len(step_noises) else
                              _canvas(step_noises[i], dev).reshape(cshape)) for i in range(S)]
    kn = kp = ek = None
    if known is not None:
        kn, kp = plan.gather(known), plan.gather(keep_mask)
        ek = plan.gather(start if known_noise is None else known_noise)
    return plan.gather(start), noises, kn, kp, ek


def merge_edit(plan: WindowPlan):
    """the per-step ``edit`` of the literal loops: the merge, in place on a contiguous copy of what the loop hands over"""
    def edit(x: torch.Tensor, i: int) -> torch.Tensor:
        x = x.contiguous().clone()
        plan.merge_(x)
        return x
    return edit


def canvas_of(plan: WindowPlan, rows: torch.Tensor) -> torch.Tensor:
    """the canvas ``[n, C, L]`` of merged rows ``[n W, C, T]``: every window copied to its place (they agree where they overlap)"""
    n, C = rows.shape[0] // plan.W, rows.shape[1]
    r = rows.reshape(n, plan.W, C, plan.window)
    canvas = torch.empty((n, C, plan.length), dtype=rows.dtype, device=rows.device)
    for j, off in enumerate(plan.offsets):
        canvas[:, :, off:off + plan.window] = r[:, j]
    return canvas
