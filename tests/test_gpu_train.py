"""-m gpu: the training path (jen1_amd/train.py, include/jen1_train.h) -- forward + backward parity.

Per operator: the HIP forward / data gradient / parameter gradients against the same operator in plain PyTorch
float32 with torch.autograd on the CPU (the floating-point kernel reference this tier keeps).  Whole model: loss and
the gradient of every parameter of the tiny configuration against tests/golden/tiny_train.npz, which holds what the
reference's own ``training_loosses(...).backward()`` produced (tests/golden/make_golden.py).
Tolerances: float32 mode <= 1e-3 of the largest reference entry (BASELINE.json); bf16 mode 5e-2, stated per test.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import bf16_gate, golden, record_parity, rel_err
from jen1_amd import synth
from jen1_amd.config import tiny_model_config

pytestmark = pytest.mark.gpu

F32_TOL = 1e-3
BF16_TOL = 5e-2


@pytest.fixture(scope="module")
def rts():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.train import TrainRuntime
    return {"f32": TrainRuntime("f32"), "bf16": TrainRuntime("bf16")}


def _rows(x_bcl: torch.Tensor, dtype) -> torch.Tensor:
    """[B, C, L] float32 (CPU) -> channel-last [B, L, pad8(C)] on the GPU"""
    from jen1_amd.train import pad8
    B, C, Lx = x_bcl.shape
    out = torch.zeros((B, Lx, pad8(C)), dtype=dtype, device="cuda")
    out[:, :, :C] = x_bcl.transpose(1, 2).to("cuda")
    return out


def _back(y_rows: torch.Tensor, C: int) -> np.ndarray:
    return y_rows[:, :, :C].float().transpose(1, 2).cpu().numpy()


def _param(shape, gen, scale=1.0):
    return torch.nn.Parameter((torch.randn(shape, generator=gen) * scale))


def _tol(mode):
    return F32_TOL if mode == "f32" else BF16_TOL


CONV_CASES = [
    # kind, B, Ci, Co, L, k, stride, causal
    ("conv", 2, 16, 24, 37, 3, 1, False),
    ("conv", 2, 16, 24, 37, 3, 1, True),
    ("conv", 3, 13, 40, 50, 3, 1, False),      # C_in = 13: padded channel columns (the 257-channel to_in conv)
    ("conv", 2, 32, 64, 301, 9, 4, False),     # downsample f = 4
    ("conv", 2, 32, 64, 94, 5, 2, True),       # downsample f = 2, causal
    ("conv", 2, 64, 64, 1, 3, 1, False),       # bottom level, L = 1
    ("conv", 16, 128, 128, 6, 3, 1, False),    # split-K forward / data gradient
    ("conv1x1", 2, 48, 16, 29, 1, 1, False),
    ("zeropad", 2, 16, 16, 40, 3, 1, False),   # Upsample1d factor 1
    ("convT", 2, 24, 16, 19, 4, 2, False),     # Upsample1d factor 2
    ("convT", 2, 16, 8, 23, 8, 4, False),      # Upsample1d factor 4
]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_conv_family_forward_backward(rts, mode, case):
    from jen1_amd import train as TR
    rt = rts[mode]
    kind, B, Ci, Co, Lx, k, stride, causal = case
    gen = torch.Generator().manual_seed(sum(v for v in case if isinstance(v, int) and not isinstance(v, bool)))
    x = torch.randn((B, Ci, Lx), generator=gen).requires_grad_()
    if kind == "convT":
        w = _param((Ci, Co, k), gen, (Ci * k) ** -0.5)
    else:
        w = _param((Co, Ci, k), gen, (Ci * k) ** -0.5)
    b = _param((Co,), gen, 0.1)
    # reference: blocks.py:45-50 (pad then conv) / nn.ConvTranspose1d
    if kind == "convT":
        f = stride
        y_ref = F.conv_transpose1d(x, w, b, stride=f, padding=f // 2 + f % 2, output_padding=f % 2)
    elif kind == "zeropad":
        y_ref = F.conv1d(x, w, b, padding=1)
    else:
        pad = ((k - 1), 0) if causal else ((k - 1) // 2, (k - 1) - (k - 1) // 2)
        y_ref = F.conv1d(F.pad(x, pad), w, b, stride=stride)
    dy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(dy)
    ref = dict(y=y_ref.detach().numpy(), dx=x.grad.numpy(), dw=w.grad.numpy(), db=b.grad.numpy())

    wd = torch.nn.Parameter(w.detach().cuda())
    bd = torch.nn.Parameter(b.detach().cuda())
    xr = _rows(x.detach(), rt.tdtype).requires_grad_()
    if kind == "convT":
        y = TR.conv_transpose1d(rt, xr, wd, bd, stride, stride // 2 + stride % 2, stride % 2)
    elif kind == "zeropad":
        y = TR.conv1d_zero_pad(rt, xr, wd, bd, 1)
    else:
        y = TR.conv1d_same(rt, xr, wd, bd, stride, causal)
    assert y.shape[1] == y_ref.shape[2]
    y.backward(_rows(dy, rt.tdtype))
    torch.cuda.synchronize()
    tol = _tol(mode)
    assert rel_err(_back(y.detach(), Co), ref["y"]) < tol
    assert rel_err(_back(xr.grad, Ci), ref["dx"]) < tol
    assert float(xr.grad[:, :, Ci:].abs().max()) == 0.0 if xr.shape[-1] > Ci else True
    assert rel_err(wd.grad.cpu().numpy(), ref["dw"]) < tol
    assert rel_err(bd.grad.cpu().numpy(), ref["db"]) < tol
    # a second backward accumulates (gradient accumulation over micro-batches, trainer.py:139-143)
    y2 = TR.conv1d_same(rt, xr, wd, bd, stride, causal) if kind in ("conv", "conv1x1") else None
    if y2 is not None:
        y2.backward(_rows(dy, rt.tdtype))
        torch.cuda.synchronize()
        assert rel_err(wd.grad.cpu().numpy(), 2 * ref["dw"]) < tol


MANY_ROW_CASES = [
    # (kind, B, Ci, Co, L, k, stride, causal), launches of the big kernels, launches of jen1_train_gemm: the counts of a dry run of the host
    # code (tools/train_record.py) with the row thresholds at 64 and unpaired gradients
    (("conv", 2, 128, 128, 96, 3, 1, False), 3, 0),
    (("conv", 2, 128, 128, 96, 3, 1, True), 3, 0),
    (("conv", 3, 128, 128, 96, 3, 1, [1, 0, 1]), 3, 0),      # CausalRows: the padding per batch element in shift_b
    (("conv", 2, 128, 256, 97, 5, 2, True), 3, 0),           # strided: the data gradient divides in its row map
    (("conv", 2, 128, 128, 96, 1, 1, False), 3, 0),
    (("conv", 2, 257, 128, 96, 3, 1, False), 2, 1),          # Ci no multiple of 4: the data gradient stays on jen1_train_gemm
    (("convT", 2, 128, 128, 48, 4, 2, False), 3, 0),
    (("convT", 2, 128, 64, 48, 8, 4, False), 3, 0),
    (("linear", 1, 128, 128, 128, 1, 1, False), 3, 0),
]


@pytest.mark.parametrize("case,n_big,n_gemm", MANY_ROW_CASES, ids=lambda c: "-".join(str(v) for v in c) if isinstance(c, tuple) else None)
def test_conv_family_many_row_routes(case, n_big, n_gemm):
    """the host's argument mapping for the many-row routes (jen1_big_gemm_conv forward and data gradient -- pad' = k - 1 - pad, the tap
    reversal, the divisor, the shifted operand of ConvTranspose1d -- and jen1_big_gemm_tn_conv) through the autograd wrappers, bf16, with
    the row thresholds lowered so that small shapes take them; against torch float32 as test_conv_family_forward_backward does it"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import train as TR
    rt = TR.TrainRuntime("bf16")
    rt.big_conv_rows = rt.big_wgrad_rows = 64
    rt.pair_grads = False
    rt.stats = {}
    kind, B, Ci, Co, Lx, k, stride, causal = case
    gen = torch.Generator().manual_seed(sum(v for v in case if isinstance(v, int) and not isinstance(v, bool)))
    x = torch.randn((B, Ci, Lx), generator=gen).requires_grad_()
    w = _param((Ci, Co, k) if kind == "convT" else (Co, Ci, k), gen, (Ci * k) ** -0.5)
    b = _param((Co,), gen, 0.1)
    if kind == "convT":
        y_ref = F.conv_transpose1d(x, w, b, stride=stride, padding=stride // 2 + stride % 2, output_padding=stride % 2)
    else:
        # blocks.py:45-50 (pad then conv), per batch element where the causal flag is
        flags = causal if isinstance(causal, list) else [causal] * B
        pads = [((k - 1), 0) if f else ((k - 1) // 2, (k - 1) - (k - 1) // 2) for f in flags]
        y_ref = torch.cat([F.conv1d(F.pad(x[i:i + 1], p), w, b, stride=stride) for i, p in enumerate(pads)])
    dy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(dy)
    ref = dict(y=y_ref.detach().numpy(), dx=x.grad.numpy(), dw=w.grad.numpy(), db=b.grad.numpy())

    if kind == "linear":                       # (the reference's k = 1 convolution IS the linear: weight [Co, Ci])
        w, ref["dw"] = w.detach()[:, :, 0], ref["dw"][:, :, 0]
    wd = torch.nn.Parameter(w.detach().contiguous().cuda())
    bd = torch.nn.Parameter(b.detach().cuda())
    xr = _rows(x.detach(), rt.tdtype).requires_grad_()
    if kind == "convT":
        y = TR.conv_transpose1d(rt, xr, wd, bd, stride, stride // 2 + stride % 2, stride % 2)
    elif kind == "linear":
        y = TR.linear(rt, xr, wd, bd)
    else:
        y = TR.conv1d_same(rt, xr, wd, bd, stride, TR.CausalRows(torch.tensor(causal, device="cuda")) if isinstance(causal, list) else causal)
    assert y.shape[1] == y_ref.shape[2]
    y.backward(_rows(dy, rt.tdtype))
    torch.cuda.synchronize()
    assert rel_err(_back(y.detach(), Co), ref["y"]) < BF16_TOL
    assert rel_err(_back(xr.grad, Ci), ref["dx"]) < BF16_TOL
    assert float(xr.grad[:, :, Ci:].abs().max()) == 0.0 if xr.shape[-1] > Ci else True
    assert rel_err(wd.grad.cpu().numpy(), ref["dw"]) < BF16_TOL
    assert rel_err(bd.grad.cpu().numpy(), ref["db"]) < BF16_TOL
    assert rt.stats["big_gemm"][0] == n_big and rt.stats.get("train_gemm", [0])[0] == n_gemm, rt.stats


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("rows,ci,co,bias", [(2, 129, 512, True), (48, 512, 1024, True), (258, 1024, 256, False), (5, 64, 64, True)])
def test_linear_forward_backward(rts, mode, rows, ci, co, bias):
    from jen1_amd import train as TR
    rt = rts[mode]
    gen = torch.Generator().manual_seed(rows + ci)
    x = torch.randn((rows, ci), generator=gen).requires_grad_()
    w = _param((co, ci), gen, ci ** -0.5)
    b = _param((co,), gen, 0.1) if bias else None
    y_ref = F.linear(x, w, b)
    dy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(dy)
    wd = torch.nn.Parameter(w.detach().cuda())
    bd = torch.nn.Parameter(b.detach().cuda()) if bias else None
    xp = torch.zeros((rows, TR.pad8(ci)), dtype=rt.tdtype, device="cuda")
    xp[:, :ci] = x.detach().cuda()
    xp.requires_grad_()
    y = TR.linear(rt, xp, wd, bd)
    dyp = torch.zeros(y.shape, dtype=rt.tdtype, device="cuda")
    dyp[:, :co] = dy.cuda()
    y.backward(dyp)
    torch.cuda.synchronize()
    tol = _tol(mode)
    assert rel_err(y[:, :co].detach().float().cpu().numpy(), y_ref.detach().numpy()) < tol
    assert rel_err(xp.grad[:, :ci].float().cpu().numpy(), x.grad.numpy()) < tol
    assert rel_err(wd.grad.cpu().numpy(), w.grad.numpy()) < tol
    if bias:
        assert rel_err(bd.grad.cpu().numpy(), b.grad.numpy()) < tol


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,C,Lx,groups,film,silu,eps", [
    (2, 64, 75, 8, False, True, 1e-5), (2, 64, 75, 8, True, True, 1e-5), (3, 257, 40, 1, False, True, 1e-5),
    (2, 128, 24, 32, False, False, 1e-6), (16, 1024, 1, 8, True, True, 1e-5), (2, 128, 1500, 8, True, True, 1e-5)])
def test_group_norm_film_silu_forward_backward(rts, mode, B, C, Lx, groups, film, silu, eps):
    from jen1_amd import train as TR
    rt = rts[mode]
    gen = torch.Generator().manual_seed(C + Lx)
    x = (torch.randn((B, C, Lx), generator=gen) * 1.5 + 0.3).requires_grad_()
    ga, be = _param((C,), gen), _param((C,), gen, 0.2)
    fl = (torch.randn((B, 2 * C), generator=gen) * 0.5).requires_grad_() if film else None
    h = F.group_norm(x, groups, ga, be, eps)                          # blocks.py:137-143
    if film:
        h = h * (fl[:, :C, None] + 1) + fl[:, C:, None]
    y_ref = F.silu(h) if silu else h
    dy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(dy)
    gd, bd = torch.nn.Parameter(ga.detach().cuda()), torch.nn.Parameter(be.detach().cuda())
    xr = _rows(x.detach(), rt.tdtype).requires_grad_()
    fd = fl.detach().to("cuda", rt.tdtype).requires_grad_() if film else None
    y = TR.group_norm(rt, xr, gd, bd, C, groups, eps, fd, silu)
    y.backward(_rows(dy, rt.tdtype))
    torch.cuda.synchronize()
    tol = _tol(mode) * (4 if mode == "bf16" else 1)                   # bf16 storage of x: the group statistics see rounded inputs
    if Lx * C // groups == 1:
        return                                                         # degenerate group of one element: y == beta, nothing to compare
    assert rel_err(_back(y.detach(), C), y_ref.detach().numpy()) < tol
    assert rel_err(_back(xr.grad, C), x.grad.numpy()) < tol
    assert rel_err(gd.grad.cpu().numpy(), ga.grad.numpy()) < tol
    assert rel_err(bd.grad.cpu().numpy(), be.grad.numpy()) < tol
    if film:
        assert rel_err(fd.grad.float().cpu().numpy(), fl.grad.numpy()) < tol


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("rows,C", [(48, 512), (258, 1024), (7, 64), (600, 128)])
def test_layer_norm_forward_backward(rts, mode, rows, C):
    from jen1_amd import train as TR
    rt = rts[mode]
    gen = torch.Generator().manual_seed(rows)
    x = (torch.randn((2, rows, C), generator=gen) * 2 + 0.5).requires_grad_()
    ga, be = _param((C,), gen), _param((C,), gen, 0.2)
    y_ref = F.layer_norm(x, (C,), ga, be, 1e-5)
    dy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(dy)
    gd, bd = torch.nn.Parameter(ga.detach().cuda()), torch.nn.Parameter(be.detach().cuda())
    xd = x.detach().to("cuda", rt.tdtype).requires_grad_()
    y = TR.layer_norm(rt, xd, gd, bd)
    y.backward(dy.to("cuda", rt.tdtype))
    torch.cuda.synchronize()
    tol = _tol(mode)
    assert rel_err(y.detach().float().cpu().numpy(), y_ref.detach().numpy()) < tol
    assert rel_err(xd.grad.float().cpu().numpy(), x.grad.numpy()) < tol
    assert rel_err(gd.grad.cpu().numpy(), ga.grad.numpy()) < tol
    assert rel_err(bd.grad.cpu().numpy(), be.grad.numpy()) < tol


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("fn", ["gelu", "silu"])
def test_activation_forward_backward(rts, mode, fn):
    from jen1_amd import train as TR
    rt = rts[mode]
    gen = torch.Generator().manual_seed(3)
    x = (torch.randn((5, 1000), generator=gen) * 3).requires_grad_()
    y_ref = F.gelu(x) if fn == "gelu" else F.silu(x)
    dy = torch.randn(y_ref.shape, generator=gen)
    y_ref.backward(dy)
    xd = x.detach().to("cuda", rt.tdtype).requires_grad_()
    y = (TR.gelu if fn == "gelu" else TR.silu)(rt, xd)
    y.backward(dy.to("cuda", rt.tdtype))
    torch.cuda.synchronize()
    assert rel_err(y.detach().float().cpu().numpy(), y_ref.detach().numpy()) < _tol(mode)
    assert rel_err(xd.grad.float().cpu().numpy(), x.grad.numpy()) < _tol(mode)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("B,Nq,Nk,C,heads,causal,strided", [
    (2, 24, 24, 64, 8, False, True), (2, 24, 24, 64, 8, True, True), (3, 6, 129, 128, 8, False, False),
    (2, 1, 129, 512, 8, False, True), (2, 150, 150, 64, 8, True, True), (2, 75, 129, 128, 8, False, False),
    (2, 12, 130, 1024, 16, False, True), (1, 64, 64, 40, 8, True, False),
    # head widths 4, 12 and 20: in float32 the GEMM path's Q K^T and dO V^T have K = d with d % 8 == 4, the next head right behind
    (2, 24, 24, 32, 8, False, True), (2, 24, 40, 96, 8, True, False), (2, 30, 24, 160, 8, False, True)])
@pytest.mark.parametrize("small_attn", [True, False], ids=["one-launch", "gemm-path"])
def test_attention_core_forward_backward(rts, mode, B, Nq, Nk, C, heads, causal, strided, small_attn, monkeypatch):
    """AttentionBase.forward math path (blocks.py:355-380) incl. the causal mask of blocks.py:315-319; short sequences both through
    the one-launch kernels (jen1_attn_small_forward / _backward) and through the GEMM + softmax launches"""
    from jen1_amd import train as TR
    rt = rts[mode]
    monkeypatch.setattr(rt, "small_attn", small_attn)
    gen = torch.Generator().manual_seed(Nq * Nk)
    q = torch.randn((B, Nq, C), generator=gen).requires_grad_()
    kv = torch.randn((B, Nk, 2 * C), generator=gen).requires_grad_()
    d = C // heads

    def split(t, n):
        return t.reshape(B, n, heads, d).transpose(1, 2)

    k, v = kv[..., :C], kv[..., C:]
    # the padding mask of the context multiplies K and V (blocks.py:431-434); given for the non-causal (cross-attention) cases
    kv_mask = None if causal else (torch.rand((B, Nk), generator=gen) > 0.3).float()
    if kv_mask is not None:
        k, v = k * kv_mask[:, :, None], v * kv_mask[:, :, None]
    sim = torch.einsum("bhnd,bhmd->bhnm", split(q, Nq), split(k, Nk)) * d ** -0.5
    if causal:
        keep = ~torch.ones((Nq, Nk), dtype=torch.bool).triu(Nk - Nq + 1)
        sim = sim.masked_fill(~keep, -torch.finfo(sim.dtype).max)
    o_ref = torch.einsum("bhnm,bhmd->bhnd", sim.softmax(-1), split(v, Nk)).transpose(1, 2).reshape(B, Nq, C)
    do = torch.randn(o_ref.shape, generator=gen)
    o_ref.backward(do)
    qd = q.detach().to("cuda", rt.tdtype).requires_grad_()
    kvd = kv.detach().to("cuda", rt.tdtype).requires_grad_()
    # K | V travel as ONE tensor (to_kv's output); ``strided``: as it is / as the product of an elementwise op (the padding mask)
    o = TR.attention_core(rt, qd, kvd if strided else kvd * 1.0, heads, causal, None if kv_mask is None else kv_mask.cuda())
    o.backward(do.to("cuda", rt.tdtype))
    torch.cuda.synchronize()
    tol = _tol(mode)
    assert rel_err(o.detach().float().cpu().numpy(), o_ref.detach().numpy()) < tol
    assert rel_err(qd.grad.float().cpu().numpy(), q.grad.numpy()) < tol
    assert rel_err(kvd.grad.float().cpu().numpy(), kv.grad.numpy()) < tol


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_convert_clear_hands_over_and_zeroes(rts, mode):
    """jen1_convert_clear: the float32 split-K accumulator becomes the output (compute dtype) and is zero again"""
    from jen1_amd import lib as L
    rt = rts[mode]
    src = torch.randn(4096 + 8, device="cuda")
    want = src[:4096].to(rt.tdtype).clone()
    dst = torch.empty(4096, dtype=rt.tdtype, device="cuda")
    L.check(rt.lib.jen1_convert_clear(src.data_ptr(), dst.data_ptr(), 4096, rt.dt, rt.stream()), "jen1_convert_clear")
    torch.cuda.synchronize()
    assert torch.equal(dst, want)
    assert float(src[:4096].abs().max()) == 0.0 and float(src[4096:].abs().min()) > 0.0      # only n entries are touched


# ------------------------------------------------------------------ whole model against the reference's autograd
@pytest.fixture(scope="module")
def tiny_model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.model import UNetCFG1d
    return UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _loss_and_grads(model, mode, task, causal, objective):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    B, T = 2, 300
    betas, _ = get_beta_schedule("linear", 1000)
    t = torch.tensor([17, 801], dtype=torch.long, device="cuda")
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, task).items()}
    noise = dev(fill_uniform(f"synth.trainnoise.{task}", (B, 128, T), 3, 0.0, 1.0))
    gd = GaussianDiffusion(steps=1000, betas=betas, objective=objective, loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    model.train()
    for p in model.parameters():
        p.grad = None
    graph = model.train_graph(mode)
    loss = gd.training_loosses(graph, x0, t, cond, noise=noise, causal=causal)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("task,causal", [("text_guided", False), ("music_inpaint", False), ("music_cont", True)])
def test_tiny_training_gradients_vs_reference_autograd_f32(tiny_model, task, causal):
    """loss + the gradient of EVERY parameter (norm and a strided sample of entries) against the reference's
    ``training_loosses(...).backward()`` (gdm.py:245-272, trainer.py:141) on the same inputs and weights."""
    g = golden("tiny_train")
    names = json.loads(str(g["grad_names_all"]))
    loss, grads = _loss_and_grads(tiny_model, "f32", task, causal, "noise")
    ref_loss = float(g[f"loss.{task}.noise"])
    assert abs(loss - ref_loss) <= 1e-3 * abs(ref_loss)
    assert sorted(names) == sorted(grads.keys())
    ref_norm, ref_samp = g[f"gradnorm_all.{task}"], g[f"gradsample_all.{task}"]
    gmax = float(ref_norm.max())
    off = 0
    worst = 0.0
    for i, n in enumerate(names):
        gr = grads[n]
        assert gr is not None, f"no gradient for {n}"
        samp = gr.reshape(-1)[:: max(1, gr.numel() // 16)][:16].cpu().numpy()
        ref = ref_samp[off: off + samp.size]
        off += samp.size
        nrm = float(gr.norm())
        # every tensor's norm within 1e-3 (relative; tiny tensors against the largest norm of the model)
        assert abs(nrm - ref_norm[i]) <= 1e-3 * max(ref_norm[i], 1e-3 * gmax), (n, nrm, ref_norm[i])
        scale = max(float(np.abs(ref).max()), ref_norm[i] / np.sqrt(gr.numel()))
        err = float(np.abs(samp - ref).max() / max(scale, 1e-12))
        worst = max(worst, err)
        assert err < 5e-3, (n, err)
    assert off == ref_samp.size
    print(f"worst sampled-entry error {worst:.2e}")


@pytest.mark.parametrize("objective", ["x0", "v"])
def test_tiny_training_other_objectives_f32(tiny_model, objective):
    g = golden("tiny_train")
    names = json.loads(str(g["grad_names"]))
    loss, grads = _loss_and_grads(tiny_model, "f32", "music_inpaint", False, objective)
    ref_loss = float(g[f"loss.music_inpaint.{objective}"])
    assert abs(loss - ref_loss) <= 1e-3 * abs(ref_loss)
    ref = g[f"gradnorm.music_inpaint.{objective}"]
    for i, n in enumerate(names):
        assert abs(float(grads[n].norm()) - ref[i]) <= 1e-3 * max(ref[i], 1e-3 * float(ref.max())), (n, float(grads[n].norm()), ref[i])
    full = g["grad.to_time.0.0.weights"]
    assert full.shape == tuple(grads["to_time.0.0.weights"].shape)


def test_tiny_training_gradients_bf16(tiny_model):
    """bf16 storage / float32 accumulation: gradient norms within 5e-2 of the reference's float32 autograd"""
    g = golden("tiny_train")
    names = json.loads(str(g["grad_names_all"]))
    loss, grads = _loss_and_grads(tiny_model, "bf16", "text_guided", False, "noise")
    ref_loss = float(g["loss.text_guided.noise"])
    assert abs(loss - ref_loss) <= BF16_TOL * abs(ref_loss)
    ref_norm = g["gradnorm_all.text_guided"]
    gmax = float(ref_norm.max())
    bad = [(n, float(grads[n].norm()), float(ref_norm[i])) for i, n in enumerate(names)
           if abs(float(grads[n].norm()) - ref_norm[i]) > BF16_TOL * max(ref_norm[i], 1e-2 * gmax)]
    assert not bad, bad[:5]


def test_vdm_training_loss_and_gradients_vs_repaired_reference_f32(tiny_model):
    """``VDM.training_loosses`` (vdm.py:89-110 with the A-4 repair) through the differentiable HIP path: loss and every
    parameter's gradient norm against the reference's autograd on its own class with the same repair (tiny_vdm.npz)."""
    from jen1_amd.init_fill import fill_uniform
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.vdm import VDM
    g = golden("tiny_vdm")
    names = json.loads(str(g["grad_names_all"]))
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
    model.train()
    B, T = 2, 300
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T).items()}
    noise = dev(fill_uniform("synth.trainnoise.vdm", (B, 128, T), 3, 0.0, 1.0))
    vd = VDM(loss_type="l2", device="cuda", cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    loss = vd.training_loosses(model, x0, cond, noise=noise, causal=False, times=dev(g["times"]))
    loss.backward()
    torch.cuda.synchronize()
    ref = float(g["loss"])
    assert abs(float(loss.detach()) - ref) <= 1e-3 * abs(ref)
    grads = {n: p.grad for n, p in model.named_parameters()}
    ref_norm = g["gradnorm_all"]
    gmax = float(ref_norm.max())
    for i, n in enumerate(names):
        nrm = float(grads[n].norm())
        assert abs(nrm - ref_norm[i]) <= 1e-3 * max(ref_norm[i], 1e-3 * gmax), (n, nrm, ref_norm[i])


def test_training_step_updates_parameters_and_repacks(tiny_model):
    """one optimiser step through FusedAdamW changes the loss; the packed compute weights follow the parameters"""
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
    opt = FusedAdamW(model.parameters(), lr=1e-3, max_norm=0.7)
    graph = model.train_graph("f32")
    graph.attach_optimizer(opt)
    l0, _ = _loss_and_grads_keep(model, graph, opt)
    opt.step()
    l1, _ = _loss_and_grads_keep(model, graph, opt)
    assert l1 != l0 and np.isfinite(l1)
    assert float(opt.grad_norm()) > 0


def _loss_and_grads_keep(model, graph, opt):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    B, T = 2, 300
    betas, _ = get_beta_schedule("linear", 1000)
    t = torch.tensor([17, 801], dtype=torch.long, device="cuda")
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, "text_guided").items()}
    noise = dev(fill_uniform("synth.trainnoise.text_guided", (B, 128, T), 3, 0.0, 1.0))
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    opt.zero_grad()
    loss = gd.training_loosses(graph, x0, t, cond, noise=noise, causal=False)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), None


@pytest.mark.parametrize("use_graph", [False, True])
def test_unified_multitask_trainer_steps(tiny_model, use_graph):
    """trainer.py:126-213: three task sub-batches per micro-batch, gradient accumulation, clip + AdamW + LinearLR"""
    import random
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW, LinearLR
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.2, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    sched = LinearLR(1e-3)
    B, T = 6, 300
    emb = dev(synth.conditioning(B, T, "text_guided")["cross_attn_cond"])
    msk = dev(synth.conditioning(B, T, "text_guided")["cross_attn_masks"])

    def conditioner(metadata, device):
        idx = torch.tensor(metadata, device=device)
        return {"prompt": (emb[idx], msk[idx])}

    tr = UnifiedMultiTaskTrainer.build(model, gd, conditioner, opt, sched, grad_accum_every=2, rng=random.Random(0), use_graph=use_graph)
    audio = dev(synth.latents(B, T, key="clip"))
    p0 = opt.flat_param.clone()
    torch.manual_seed(0)
    losses, steps = [], 0
    for it in range(4):
        loss, per_task, stepped = tr.train_step(audio, list(range(B)))
        assert set(per_task) == {"text_guided", "music_inpaint", "music_cont"}
        assert abs(float(loss) - sum(float(v) for v in per_task.values())) < 1e-3 * abs(float(loss))
        losses.append(float(loss))
        steps += int(stepped)
        assert stepped == (it % 2 == 1)
    assert steps == 2 and opt.step_count == 2 and sched.last_epoch == 2
    assert all(np.isfinite(losses))
    assert float((opt.flat_param - p0).abs().max()) > 0
    assert tr.global_step == 4 and tr.grad_accum == 0


@pytest.mark.gpu
def test_train_loop_walks_the_loader_through_train_step(tiny_model):
    """train_loop (trainer.py:126-150, the call site of train.py:110-125): the micro-batches of ``dls[0]`` go through ``train_step``;
    ``max_steps`` bounds them; the accumulation window closes with an optimiser step"""
    import random
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.2, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    B, T = 6, 300
    emb = dev(synth.conditioning(B, T, "text_guided")["cross_attn_cond"])
    msk = dev(synth.conditioning(B, T, "text_guided")["cross_attn_masks"])

    def conditioner(metadata, device):
        idx = torch.tensor(metadata, device=device)
        return {"prompt": (emb[idx], msk[idx])}

    audio = torch.from_numpy(np.ascontiguousarray(synth.latents(B, T, key="clip")))
    loader = [(audio, list(range(B))) for _ in range(5)]
    tr = UnifiedMultiTaskTrainer.build(model, gd, conditioner, opt, None, grad_accum_every=2, rng=random.Random(0), use_graph=False,
                                       dls=(loader, None))
    p0 = opt.flat_param.clone()
    torch.manual_seed(0)
    tr.train_loop(max_steps=4)
    torch.cuda.synchronize()
    assert tr.global_step == 4 and opt.step_count == 2 and tr.grad_accum == 0
    assert float((opt.flat_param - p0).abs().max()) > 0


@pytest.mark.gpu
def test_train_loop_evaluates_and_writes_the_best_checkpoint(tmp_path):
    """train_loop runs ``eval_all_tasks`` every ``eval_interval`` micro-batches and once at the end (trainer.py:174-181);
    a new best validation loss writes a checkpoint in the reference's wire format (script_util.py:79-90) that ``load_checkpoint`` reads back"""
    import random
    from jen1_amd.checkpoint import load_checkpoint
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.2, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    B, T = 3, 300
    emb = dev(synth.conditioning(B, T, "text_guided")["cross_attn_cond"])
    msk = dev(synth.conditioning(B, T, "text_guided")["cross_attn_masks"])

    def conditioner(metadata, device):
        idx = torch.tensor(metadata, device=device)
        return {"prompt": (emb[idx], msk[idx])}

    audio = torch.from_numpy(np.ascontiguousarray(synth.latents(B, T, key="clip")))
    loader = [(audio, list(range(B))) for _ in range(3)]
    valid = [(audio, list(range(B)))]
    tr = UnifiedMultiTaskTrainer.build(model, gd, conditioner, opt, None, grad_accum_every=1, rng=random.Random(0), use_graph=False,
                                       dls=(loader, valid), save_dir=str(tmp_path / "ckpt"), eval_interval=2, num_epoch=0)
    torch.manual_seed(0)
    tr.train_loop()
    torch.cuda.synchronize()
    assert tr.global_step == 3 and opt.step_count == 3
    files = sorted((tmp_path / "ckpt").glob("Jen1_step_*_loss_*.pth"))
    assert files and np.isfinite(tr.best_avg_total_loss) and tr.best_avg_total_loss > 0
    assert str(files[-1]) == tr.last_checkpoint or tr.last_checkpoint in [str(f) for f in files]
    twin = UNetCFG1d(**tiny_model_config(), init_seed=99, compute_dtype="bf16", device="cuda")
    load_checkpoint(tr.last_checkpoint, twin)
    sd_a, sd_b = model.state_dict(), twin.state_dict()
    # (the checkpoint holds the weights at the time of the best evaluation: every key present, same shapes)
    assert sd_a.keys() == sd_b.keys() and all(sd_a[k].shape == sd_b[k].shape for k in sd_a)
    assert model.training


def test_graphed_step_matches_eager_gradients():
    """the captured forward + backward (train.GraphedLossStep) accumulates the same gradients as the eager path, replay
    after replay, also after the parameters moved (the weight packing is part of the graph)"""
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.train import GraphedLossStep
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    graph = model.train_graph("f32")
    graph.attach_optimizer(opt)
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    B, T = 2, 300
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, "music_cont").items()}
    t = torch.tensor([17, 801], dtype=torch.long, device="cuda")
    step = GraphedLossStep(graph, gd, scale=0.5)
    # eager pass BEFORE the capture, issued from the default stream: TrainGraph moves it to a private stream (a
    # backward pass on the null stream makes the later capture crash inside hipStreamEndCapture)
    gd.training_loosses(graph, x0, t, cond, causal=True).backward()
    step(x0, t, cond, True)                 # capture (its warm-up run draws noise of its own)
    for rnd in range(2):
        opt.zero_grad()
        torch.manual_seed(5 + rnd)
        le = gd.training_loosses(graph, x0, t, cond, causal=True)
        (le * 0.5).backward()
        torch.cuda.synchronize()
        ge = opt.flat_grad.clone()
        opt.zero_grad()
        torch.manual_seed(5 + rnd)
        lg = step(x0, t, cond, True)
        torch.cuda.synchronize()
        gg = opt.flat_grad.clone()
        le = le.detach()
        assert abs(float(lg) - float(le)) <= 1e-5 * abs(float(le)), (rnd, float(lg), float(le))
        assert float((gg - ge).abs().max()) <= 1e-4 * float(ge.abs().max()), rnd
        opt.step()      # parameters move; the next replay must re-pack


def test_full_model_training_gradients_vs_reference_autograd_f32():
    """BASELINE's full 296.5 M-parameter configuration, one clip x 128x1500 through the CFG pair, causal: loss and the
    gradient of every one of the 979 tensors against the reference's own autograd (tests/golden/full_train.npz)."""
    from jen1_amd.config import full_model_config
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    from jen1_amd.model import UNetCFG1d
    g = golden("full_train")
    names = json.loads(str(g["grad_names_all"]))
    model = UNetCFG1d(**full_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
    model.train()
    B, T = 1, 1500
    betas, _ = get_beta_schedule("linear", 1000)
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, "music_cont").items()}
    noise = dev(fill_uniform("synth.trainnoise.full", (B, 128, T), 3, 0.0, 1.0))
    t = torch.tensor([417], dtype=torch.long, device="cuda")
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    loss = gd.training_loosses(model, x0, t, cond, noise=noise, causal=True)       # picks model.train_graph() by itself
    loss.backward()
    torch.cuda.synchronize()
    ref_loss = float(g["loss"])
    assert abs(float(loss.detach()) - ref_loss) <= 1e-3 * abs(ref_loss)
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(names) == sorted(grads.keys()) and len(names) == 979
    ref_norm, ref_samp = g["gradnorm_all"], g["gradsample_all"]
    gmax = float(ref_norm.max())
    off, worst_n, worst_s = 0, 0.0, 0.0
    for i, n in enumerate(names):
        gr = grads[n]
        assert gr is not None, f"no gradient for {n}"
        samp = gr.reshape(-1)[:: max(1, gr.numel() // 16)][:16].cpu().numpy()
        ref = ref_samp[off: off + samp.size]
        off += samp.size
        nrm = float(gr.norm())
        en = abs(nrm - ref_norm[i]) / max(ref_norm[i], 1e-3 * gmax)
        scale = max(float(np.abs(ref).max()), ref_norm[i] / np.sqrt(gr.numel()))
        es = float(np.abs(samp - ref).max() / max(scale, 1e-12))
        worst_n, worst_s = max(worst_n, en), max(worst_s, es)
        assert en <= 1e-3, (n, nrm, ref_norm[i])
        assert es <= 5e-3, (n, es)
    assert off == ref_samp.size
    print(f"full model: worst norm error {worst_n:.2e}, worst sampled-entry error {worst_s:.2e}")


@pytest.mark.parametrize("mode,tol_loss,tol_norm,tol_samp", [("f32", 1e-3, 1e-3, 5e-3),
                                                             ("bf16", bf16_gate("configs3_micro_batch", "bf16", "loss"),
                                                              bf16_gate("configs3_micro_batch", "bf16", "norm"),
                                                              bf16_gate("configs3_micro_batch", "bf16", "samp"))])
def test_configs3_micro_batch_merged_passes_vs_reference_autograd(mode, tol_loss, tol_norm, tol_samp):
    """BASELINE configs[3] at its per-GPU shape: the full model, 8 clips as the 3 / 3 / 2 task sub-batches (text_guided,
    music_inpaint, music_cont with their masks) of one micro-batch.  The reference runs one pass per task and sums the three
    mean losses (trainer.py:183-213); the trainer here merges the sub-batches that share the causal flag into one pass with
    per-sample weights.  Per-task losses, the summed loss and the gradient of every one of the 979 tensors against the
    reference's own autograd (tests/golden/full_train8.npz, make_golden.py fulltrain8)."""
    from jen1_amd.config import full_model_config
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    g = golden("full_train8")
    names = json.loads(str(g["grad_names_all"]))
    model = UNetCFG1d(**full_model_config(), init_seed=1234, compute_dtype=mode, device="cuda")
    model.train()
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                           cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    opt = FusedAdamW(model.parameters(), lr=0.0, max_norm=None)
    tr = UnifiedMultiTaskTrainer.build(model, gd, None, opt, None, grad_accum_every=1, use_graph=False, allow_uneven_tasks=True,
                                       merge_tasks=True, compute_dtype=mode)
    parts, noises = [], {}
    for task, x0, t, cond, noise, causal in synth.train8_inputs():
        parts.append((task, dev(x0), torch.from_numpy(t).cuda(), {k: (None if v is None else dev(v)) for k, v in cond.items()}, causal))
        noises[task] = dev(noise)
    opt.zero_grad()
    loss, per_task = tr.run_parts(parts, noises)
    loss.backward()
    torch.cuda.synchronize()
    worst_l = max(abs(float(per_task[task]) - float(g[f"loss.{task}"])) / abs(float(g[f"loss.{task}"])) for task in per_task)
    worst_l = max(worst_l, abs(float(loss.detach()) - float(g["loss"])) / abs(float(g["loss"])))
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert sorted(names) == sorted(grads.keys()) and len(names) == 979
    ref_norm, ref_samp = g["gradnorm_all"], g["gradsample_all"]
    gmax = float(ref_norm.max())
    off, worst_n, worst_s, es_all = 0, ("", 0.0), ("", 0.0), []
    for i, n in enumerate(names):
        gr = grads[n]
        samp = gr.reshape(-1)[:: max(1, gr.numel() // 16)][:16].cpu().numpy()
        ref = ref_samp[off: off + samp.size]
        off += samp.size
        nrm = float(gr.norm())
        en = abs(nrm - ref_norm[i]) / max(ref_norm[i], 1e-3 * gmax)
        scale = max(float(np.abs(ref).max()), ref_norm[i] / np.sqrt(gr.numel()))
        es = float(np.abs(samp - ref).max() / max(scale, 1e-12))
        es_all.append(float(np.sqrt(np.mean((samp - ref) ** 2)) / max(scale, 1e-12)))
        if en > worst_n[1]:
            worst_n = (n, en)
        if es > worst_s[1]:
            worst_s = (n, es)
    assert off == ref_samp.size
    # the worst single entry of 15 664 is a tail statistic (bf16 operands, float atomics in the weight-gradient sums: 0.24 - 0.49 over
    # runs of the same build); the root mean square over the 979 tensors of their sampled entries' error is the stable figure
    samp_rms = float(np.sqrt(np.mean(np.square(es_all))))
    print(f"configs[3] micro-batch (3/3/2, one pass, {mode}): worst loss error {worst_l:.2e}, worst norm error {worst_n[1]:.2e} ({worst_n[0]}), "
          f"worst sampled-entry error {worst_s[1]:.2e} ({worst_s[0]}), rms over the tensors {samp_rms:.2e}")
    record_parity("configs3_micro_batch", mode, mode, loss=worst_l, norm=worst_n[1], samp=worst_s[1], samp_rms=samp_rms)
    assert worst_l <= tol_loss, worst_l
    assert worst_n[1] <= tol_norm, worst_n
    assert worst_s[1] <= tol_samp, worst_s
    if mode == "bf16":
        assert samp_rms <= bf16_gate("configs3_micro_batch", "bf16", "samp_rms"), samp_rms


def test_training_overfits_one_batch():
    """end to end: backward + clip + AdamW on the HIP path actually minimise the loss (one fixed micro-batch, fixed
    timesteps / noise / masks, tiny configuration, 40 optimiser steps)"""
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.train import GraphedLossStep
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    model.train()
    opt = FusedAdamW(model.parameters(), lr=2e-3, weight_decay=0.0, max_norm=1.0)
    graph = model.train_graph("bf16")
    graph.attach_optimizer(opt)
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                           embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    B, T = 2, 300
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, "music_inpaint").items()}
    t = torch.tensor([300, 700], dtype=torch.long, device="cuda")
    noise = dev(fill_uniform("synth.trainnoise.overfit", (B, 128, T), 3, 0.0, 1.0))
    losses = []
    for it in range(40):
        opt.zero_grad()
        loss = gd.training_loosses(graph, x0, t, cond, noise=noise, causal=False)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    assert min(losses[20:]) < min(losses[:5])


def _collect(q, procs, n: int, timeout: float):
    """n results from the workers' queue; gives up early when a worker has died without a message (an abort in native code would
    otherwise cost the whole time-out in GPU minutes)"""
    import queue as _queue
    import time as _time
    out, t0 = [], _time.time()
    while len(out) < n:
        try:
            out.append(q.get(timeout=5))
        except _queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or _time.time() - t0 > timeout:
                for p in procs:
                    if p.is_alive():
                        p.kill()
                raise AssertionError(f"workers died / timed out: exit codes {[p.exitcode for p in procs]}")
    return out


def _ddp_worker(rank, world, port, q):
    try:
        _ddp_worker_body(rank, world, port, q)
    except BaseException:                      # (the parent would otherwise wait out its queue timeout without a message)
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ddp_worker_body(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW, GradExchange, allreduce_gradients
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        betas, _ = get_beta_schedule("linear", 1000)
        gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                               embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
        B, T = 2, 300
        cond = {k: dev(v) for k, v in synth.conditioning(B, T, "music_inpaint").items()}

        def grads_of(model, opt, r):
            x0 = dev(synth.latents(B, T, key=f"clip{r}"))
            noise = dev(fill_uniform(f"synth.trainnoise.ddp{r}", (B, 128, T), 3, 0.0, 1.0))
            t = torch.tensor([100 + 50 * r, 900 - 70 * r], dtype=torch.long, device="cuda")
            loss = gd.training_loosses(model.train_graph("f32"), x0, t, cond, noise=noise, causal=False)
            loss.backward()

        model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
        model.train()
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        opt.zero_grad()
        # the exchange overlapped with the backward pass (DDP's buckets, train.py:88-89): TrainGraph's hooks release a block's
        # slice of the flat gradient as soon as the pass has finished it
        ex = GradExchange(opt, [n for n, _ in model.named_parameters()], bucket_bytes=64 << 10)
        model.train_graph("f32").exchange = ex
        ex.begin()
        grads_of(model, opt, rank)                       # every rank its own clips / timesteps / noise
        sent_during_backward = len(ex._sent)
        ex.finish()
        overlapped = opt.flat_grad.clone()
        # the same gradients through the blocking exchange: bit for bit the same mean
        model.train_graph("f32").exchange = None
        opt.zero_grad()
        grads_of(model, opt, rank)
        allreduce_gradients(opt.flat_grad, bucket_bytes=64 << 10)
        torch.cuda.synchronize()
        same_as_blocking = bool(torch.allclose(overlapped, opt.flat_grad, rtol=0, atol=2e-6 * float(opt.flat_grad.abs().max())))
        opt.flat_grad.copy_(overlapped)
        opt.step()
        torch.cuda.synchronize()
        mine = opt.flat_param.detach().cpu()
        gathered = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(gathered, mine)
        out = {"same": bool(all(torch.equal(gathered[0], g_) for g_ in gathered)), "same_as_blocking": same_as_blocking,
               "sent_during_backward": sent_during_backward}
        if rank == 0:                                     # single-process restatement: accumulate both ranks' gradients, halve
            ref = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
            ref.train()
            ropt = FusedAdamW(ref.parameters(), lr=1e-3)
            ropt.zero_grad()
            for r in range(world):
                grads_of(ref, ropt, r)
            ropt.flat_grad.mul_(1.0 / world)
            ropt.step()
            torch.cuda.synchronize()
            d = (ropt.flat_param.detach().cpu() - mine).abs().max().item()
            out["err"] = d / ropt.flat_param.abs().max().item()
            out["moved"] = (mine - torch.from_numpy(np.zeros(1, dtype=np.float32))).abs().max().item() > 0
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_data_parallel_step_two_ranks_gloo():
    """two processes (gloo; both on this one GPU), each with its own data; after the gradient
    all-reduce + clip + AdamW both hold bit-identical parameters, equal to a single process that averages the two gradients"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(_collect(q, procs, 2, 600))
    for r in res.values():
        assert "error" not in r, r["error"]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0]["same"] and res[1]["same"]
    assert res[0]["same_as_blocking"] and res[1]["same_as_blocking"]
    assert res[0]["sent_during_backward"] >= 4, res[0]       # down / bottleneck / up blocks + to_out left during the pass
    assert res[0]["err"] < 1e-5, res[0]


def _rccl_single_worker(port, q):
    try:
        import os
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch.distributed as dist
        from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
        from jen1_amd.model import UNetCFG1d
        from jen1_amd.optim import FusedAdamW, GradExchange
        from jen1_amd.train import GraphedLossStep
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        try:
            betas, _ = get_beta_schedule("linear", 1000)
            gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                                   embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
            B, T = 2, 300
            cond = {k: dev(v) for k, v in synth.conditioning(B, T, "music_inpaint").items()}
            x0 = dev(synth.latents(B, T, key="clip"))
            t = torch.tensor([100, 900], dtype=torch.long, device="cuda")
            model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
            model.train()
            opt = FusedAdamW(model.parameters(), lr=1e-3)
            graph = model.train_graph("f32")
            ex = GradExchange(opt, [n for n, _ in model.named_parameters()], bucket_bytes=64 << 10, single_rank=True)
            assert ex.world == 1 and ex.backend == "nccl" and ex.enabled and ex.capturable
            graph.exchange = ex
            step = GraphedLossStep(graph, gd, scale=1.0)
            # reference: the pass replayed WITHOUT the exchange, then the blocking exchange (RCCL all-reduce over one rank, / 1)
            torch.manual_seed(7)
            opt.zero_grad()
            step.exchange = None
            step(x0, t, cond, False)
            torch.manual_seed(7)
            opt.zero_grad()
            step(x0, t, cond, False)                # same seed -> same noise draw inside the replay
            torch.cuda.synchronize()
            before_exchange = opt.flat_grad.clone()
            c0 = ex.collectives
            ex.blocking()
            torch.cuda.synchronize()
            want = opt.flat_grad.clone()
            blocking_collectives = ex.collectives - c0
            torch.cuda.synchronize()
            identity = bool(torch.equal(want, before_exchange))      # one rank: the RCCL all-reduce and the 1 / world scale change nothing
            # the exchange recorded into the replayed pass: armed, captured as the second variant of the pass (first call), then
            # replayed three times from the same generator state as the reference pass
            outs, rec, sent = [], [], []
            for rep in range(4):
                torch.manual_seed(7)
                opt.zero_grad()
                r0, s0 = ex.recorded_collectives, ex.regions_in_pass
                ex.begin()
                step.exchange = ex
                step(x0, t, cond, False)
                assert not ex.active            # done_in_graph: nothing is left for finish()
                ex.finish()
                torch.cuda.synchronize()
                if rep > 0:                     # (the capturing call's warm-up pass advanced the generator: other noise)
                    outs.append(opt.flat_grad.clone())
                rec.append(ex.recorded_collectives - r0)
                sent.append(ex.regions_in_pass - s0)
            gmax = float(want.abs().max())
            q.put({"err": [float((o - want).abs().max()) / gmax for o in outs], "recorded": rec, "sent_during_pass": sent,
                   "blocking_collectives": blocking_collectives, "variants": len(step._captured), "identity": identity,
                   "gmax": gmax})
        finally:
            dist.destroy_process_group()
    except BaseException:
        import traceback
        q.put({"error": traceback.format_exc()})
        raise


def test_recorded_rccl_exchange_single_rank():
    """SURVEY.md section 8e / train.py:88-89 on the one GPU of the test box: a process group of ONE rank on the "nccl" (= RCCL)
    backend, ``GradExchange(single_rank=True)``.  The backward pass is captured with the exchange armed -- every region's RCCL
    all-reduce becomes a node of the replayed graph on the forked communication stream, ``finish()`` is recorded behind them --
    and replayed three times: the gradients equal the pass without the exchange followed by the blocking exchange (which, over one
    rank, is checked to be the bit-exact identity), at least four regions left during the recorded pass, at least four
    collectives were recorded, and later calls replay without recording."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_single_worker, args=(_free_port(), q))
    p.start()
    res = _collect(q, [p], 1, 300)[0]
    p.join(timeout=120)
    assert "error" not in res, res["error"]
    assert p.exitcode == 0
    assert res["gmax"] > 0 and res["identity"], res
    # same pass, same noise: the weight gradients are float atomics (split-K), so replays agree to rounding, not bit for bit
    assert max(res["err"]) < 2e-5, res
    assert res["recorded"][0] >= 4 and res["sent_during_pass"][0] >= 4, res        # captured on the first armed call ...
    assert res["recorded"][1:] == [0, 0, 0], res                                   # ... later calls only replay
    assert res["variants"] == 2, res                                               # the pass without and with the exchange
    assert res["blocking_collectives"] >= 4, res


def test_inference_engine_follows_optimizer_steps():
    """model(x, ...) between optimiser steps (the reference evaluates under no_grad every eval_interval, trainer.py:152-160)
    runs on the CURRENT weights: forward, train step, forward differs and equals a model freshly built from the new state_dict"""
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    cfg = tiny_model_config()
    model = UNetCFG1d(**cfg, init_seed=1234, compute_dtype="f32", device="cuda")
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                           embedding_scale=1.0, batch_cfg=False, scale_cfg=False)
    B, T = 2, 300
    x = dev(synth.latents(B, T))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T).items()}
    t = torch.tensor([999, 499], device="cuda")
    kw = dict(embedding=cond["cross_attn_cond"], embedding_mask=cond["cross_attn_masks"], channels_list=[cond["input_concat_cond"]])
    y0 = model(x, t, **kw).clone()                      # builds the inference engine (packed weights)
    opt = FusedAdamW(model.parameters(), lr=1e-2)
    graph = model.train_graph("f32")
    graph.attach_optimizer(opt)
    model.train()
    opt.zero_grad()
    loss = gd.training_loosses(graph, x, t, cond, causal=False)
    loss.backward()
    opt.step()
    model.eval()
    y1 = model(x, t, **kw).clone()
    assert float((y1 - y0).abs().max()) > 1e-4          # the step moved the weights and the engine saw it
    fresh = UNetCFG1d(**cfg, init_seed=1234, compute_dtype="f32", device="cuda")
    fresh.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    y2 = fresh(x, t, **kw)
    assert float((y1 - y2).abs().max()) <= 1e-5 * float(y2.abs().max())


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("T", [300, 48], ids=["one-pass-per-flag", "causal-flag-per-clip"])
def test_merged_task_passes_equal_one_pass_per_task(use_graph, T, monkeypatch):
    """UnifiedMultiTaskTrainer(merge_tasks=True): sub-batches that drew the same causal flag share one pass through the network
    with per-sample weights 1 / sub-batch size -- the same objective as the reference's one pass per task (trainer.py:189-211: the
    sum of the three per-task means), so the same per-task losses and the same gradients; 8 clips split 3 / 3 / 2.  At T = 48 every
    attention fits the one-launch kernels and ALL sub-batches share one pass, the causal flag travelling per clip (train.CausalRows:
    per-clip padding shifts in every convolution, per-clip causal mask in the self-attention)"""
    import random
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.trainer import UnifiedMultiTaskTrainer
    # the diffusion noise as a function of the clip itself, so that a sample gets the same noise however it is batched
    monkeypatch.setattr(torch, "rand_like", lambda x, **kw: torch.sin(x * 997.0) * 0.5 + 0.5)
    B = 8
    emb = dev(synth.conditioning(B, T, "text_guided")["cross_attn_cond"])
    msk = dev(synth.conditioning(B, T, "text_guided")["cross_attn_masks"])
    audio = dev(synth.latents(B, T, key="clip"))
    betas, _ = get_beta_schedule("linear", 1000)
    res = {}
    for merge in (False, True):
        model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
        gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.0,
                               embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        tr = UnifiedMultiTaskTrainer.build(model, gd, lambda md, device: {"prompt": (emb[torch.tensor(md, device=device)], msk[torch.tensor(md, device=device)])},
                                           opt, None, grad_accum_every=2, rng=random.Random(5), use_graph=use_graph, allow_uneven_tasks=True,
                                           merge_tasks=merge)
        torch.manual_seed(11)
        loss, per_task, stepped = tr.train_step(audio, list(range(B)))
        torch.cuda.synchronize()
        assert not stepped
        res[merge] = (float(loss), {k: float(v) for k, v in per_task.items()}, opt.flat_grad.clone())
        if merge:
            assert tr.graph.per_clip_causal_ok(T, emb.shape[1]) == (T == 48)
            if use_graph:
                assert len(tr.graphed._captured) == (1 if T == 48 else 2)       # passes per micro-batch
    l0, p0, g0 = res[False]
    l1, p1, g1 = res[True]
    assert set(p0) == set(p1) == {"text_guided", "music_inpaint", "music_cont"}
    assert abs(l0 - l1) <= 1e-5 * abs(l0)
    for k in p0:
        assert abs(p0[k] - p1[k]) <= 1e-5 * abs(p0[k]), k
    assert float((g0 - g1).abs().max()) <= 2e-5 * float(g0.abs().max())


@pytest.mark.gpu
def test_torch_library_training_ops_match_torch_autograd():
    """torch.ops.jen1.group_norm / layer_norm / activation (jen1_amd/ops.py: dispatcher ops with registered autograd) against the
    same operators in plain PyTorch float32 autograd: forward, data gradient and parameter gradients (float32 mode <= 1e-3)"""
    import torch.nn.functional as F
    from jen1_amd import ops  # noqa: F401
    torch.manual_seed(0)
    dev = "cuda"
    B, Lx, C, G = 3, 37, 64, 8
    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)
    x = torch.randn((B, Lx, C), device=dev, requires_grad=True)
    gamma = (torch.randn(C, device=dev) * 0.3 + 1).requires_grad_()
    beta = (torch.randn(C, device=dev) * 0.3).requires_grad_()
    film = torch.randn((B, 2 * C), device=dev, requires_grad=True)
    w = torch.randn((B, Lx, C), device=dev)
    y, _ = torch.ops.jen1.group_norm(x, gamma, beta, film, C, G, 1e-5, True)
    (y * w).sum().backward()
    got = [y.detach(), x.grad.clone(), gamma.grad.clone(), beta.grad.clone(), film.grad.clone()]
    for t in (x, gamma, beta, film):
        t.grad = None
    xr = F.group_norm(x.transpose(1, 2), G, gamma, beta, 1e-5).transpose(1, 2)
    yr = F.silu(xr * (film[:, None, :C] + 1) + film[:, None, C:])
    (yr * w).sum().backward()
    ref = [yr.detach(), x.grad, gamma.grad, beta.grad, film.grad]
    for a, b, name in zip(got, ref, ("y", "dx", "dgamma", "dbeta", "dfilm")):
        assert rel(a, b) < 1e-3, (name, rel(a, b))
    for t in (x, gamma, beta, film):
        t.grad = None
    y, _ = torch.ops.jen1.layer_norm(x, gamma, beta, 1e-5)
    y = torch.ops.jen1.activation(y, 0)
    (y * w).sum().backward()
    got = [y.detach(), x.grad.clone(), gamma.grad.clone(), beta.grad.clone()]
    for t in (x, gamma, beta):
        t.grad = None
    yr = F.gelu(F.layer_norm(x, (C,), gamma, beta, 1e-5))
    (yr * w).sum().backward()
    for a, b, name in zip(got, [yr.detach(), x.grad, gamma.grad, beta.grad], ("y", "dx", "dgamma", "dbeta")):
        assert rel(a, b) < 1e-3, (name, rel(a, b))
    # the stacked CFG pair through the dispatcher op against the formula of model.py:362-369
    net = torch.randn((2 * B, Lx, 128), device=dev)
    out = torch.ops.jen1.cfg_combine(net, 128, 0.8, True, 0.7)
    c, u = net[:B].transpose(1, 2), net[B:].transpose(1, 2)
    cfg = u + (c - u) * 0.8
    want = 0.7 * (cfg * (c.std(dim=1, keepdim=True) / cfg.std(dim=1, keepdim=True))) + 0.3 * cfg
    assert rel(out, want) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_torch_library_gemm_ops_match_torch_autograd(mode):
    """torch.ops.jen1.conv_forward (as _Conv1d causal / centred / strided, nn.ConvTranspose1d, nn.Linear) and torch.ops.jen1.attention
    (jen1_amd/ops.py: dispatcher ops, ONE registered backward op each) against torch float32 autograd of the reference's operators
    (blocks.py:34-53, :80-88, :300-330, :431-434): output, data gradient, weight / bias gradients.  float32 mode <= 1e-3 (the
    north-star tolerance); bf16 operands <= 3e-2 of the largest entry"""
    import torch.nn.functional as F
    from jen1_amd import ops
    torch.manual_seed(1)
    dev = "cuda"
    cdt = torch.float32 if mode == "f32" else torch.bfloat16
    tol = 1e-3 if mode == "f32" else 3e-2
    rel = lambda a, b: float((a.float() - b.float()).abs().max()) / max(float(b.float().abs().max()), 1e-12)

    def leaf(*shape, scale=1.0):
        # (values on the compute dtype's grid, so that both sides see the same operands)
        return (torch.randn(shape, device=dev) * scale).to(cdt).float().requires_grad_()

    def check(name, y, yr, params, wts):
        (y.float() * wts).sum().backward()
        got = [p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        (yr * wts).sum().backward()
        assert rel(y.detach(), yr.detach()) < tol, (name, "y", rel(y.detach(), yr.detach()))
        for i, (a, p) in enumerate(zip(got, params)):
            assert rel(a, p.grad) < tol, (name, i, rel(a, p.grad))
            p.grad = None

    B, Lx, Ci, Co = 3, 37, 64, 96
    for k, stride, causal in ((3, 1, False), (3, 1, True), (5, 2, True), (1, 1, False), (9, 4, False)):
        x, w, b = leaf(B, Lx, Ci), leaf(Co, Ci, k, scale=0.1), leaf(Co, scale=0.1)
        xc = x.to(cdt)                                  # (a non-leaf view in the compute dtype: the gradient flows back through the cast)
        y = ops.conv1d_same(xc, w, b, stride, causal)[..., :Co]
        pl = (k - 1) if causal else (k - 1) // 2
        yr = F.conv1d(F.pad(x.transpose(1, 2), (pl, k - 1 - pl)), w, b, stride=stride).transpose(1, 2)
        assert y.shape == yr.shape, (y.shape, yr.shape)
        check(f"conv k={k} s={stride} causal={causal}", y, yr, [x, w, b], torch.randn(yr.shape, device=dev))
    # nn.ConvTranspose1d as Upsample1d builds it (blocks.py:80-88: kernel 2 f, stride f, padding f // 2 + f % 2, output_padding f % 2)
    for f in (2, 4):
        x, w, b = leaf(B, Lx, Ci), leaf(Ci, Co, 2 * f, scale=0.1), leaf(Co, scale=0.1)
        y = ops.conv_transpose1d(x.to(cdt), w, b, f, f // 2 + f % 2, f % 2)[..., :Co]
        yr = F.conv_transpose1d(x.transpose(1, 2), w, b, stride=f, padding=f // 2 + f % 2, output_padding=f % 2).transpose(1, 2)
        assert y.shape == yr.shape
        check(f"convT f={f}", y, yr, [x, w, b], torch.randn(yr.shape, device=dev))
    x, w, b = leaf(B, Lx, Ci), leaf(100, Ci, scale=0.1), leaf(100, scale=0.1)
    y = ops.linear(x.to(cdt), w, b)
    assert y.shape[-1] == 104 and float(y.detach()[..., 100:].abs().max()) == 0.0   # (padding lanes stay zero)
    check("linear", y[..., :100], F.linear(x, w, b), [x, w, b], torch.randn((B, Lx, 100), device=dev))
    # the attention core: self-attention (causal and not) and cross-attention over masked context rows
    heads, C = 2, 64
    for Nq, Nk, causal, masked in ((37, 37, False, False), (37, 37, True, False), (12, 129, False, True), (300, 300, False, False)):
        q, kv = leaf(B, Nq, C), leaf(B, Nk, 2 * C)
        mask = (torch.rand((B, Nk), device=dev) > 0.3).float() if masked else None
        o, _ = torch.ops.jen1.attention(q.to(cdt), kv.to(cdt), heads, causal, mask)
        kvm = kv if mask is None else kv * mask[:, :, None]
        split = lambda t: t.view(B, -1, heads, C // heads).transpose(1, 2)
        sim = split(q) @ split(kvm[..., :C]).transpose(-1, -2) * (C // heads) ** -0.5
        if causal:
            sim = sim.masked_fill(torch.ones((Nq, Nk), dtype=torch.bool, device=dev).triu(1), -torch.finfo(sim.dtype).max)
        orf = (sim.softmax(-1) @ split(kvm[..., C:])).transpose(1, 2).reshape(B, Nq, C)
        check(f"attention Nq={Nq} Nk={Nk} causal={causal} masked={masked}", o, orf, [q, kv], torch.randn((B, Nq, C), device=dev))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_concat_scale_forward_backward(rts, mode):
    """jen1_concat2 / jen1_split2: torch.cat([a, b * 2^-1/2], -1) of the up path (blocks.py:732-734) and its gradient"""
    from jen1_amd import train as TR
    rt = rts[mode]
    torch.manual_seed(3)
    a = torch.randn((3, 37, 64), device="cuda").to(rt.tdtype).requires_grad_()
    b = torch.randn((3, 37, 128), device="cuda").to(rt.tdtype).requires_grad_()
    w = torch.randn((3, 37, 192), device="cuda").to(rt.tdtype)
    out = TR.concat_scale(rt, a, b, 2 ** -0.5)
    (out.float() * w.float()).sum().backward()
    ga, gb = a.grad.clone(), b.grad.clone()
    a.grad = b.grad = None
    ref = torch.cat([a, b * 2 ** -0.5], dim=-1)
    (ref.float() * w.float()).sum().backward()
    tol = 1e-6 if mode == "f32" else 1e-2
    assert float((out.float() - ref.float()).abs().max()) <= tol
    assert float((ga.float() - a.grad.float()).abs().max()) <= tol and float((gb.float() - b.grad.float()).abs().max()) <= tol


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fused_repack_equals_per_tensor_copies(mode):
    """jen1_repack: every compute copy of the parameters ([k][C_out][pad8(C_in)] and its data-gradient transposes, from Conv1d /
    ConvTranspose1d / Linear layouts) in one launch == the per-tensor permuted copies; padding columns stay zero"""
    from jen1_amd import train as TR
    rt = TR.TrainRuntime(mode, "cuda")
    torch.manual_seed(5)
    ws = [(torch.randn((48, 36, 3), device="cuda"), "conv"), (torch.randn((40, 70, 5), device="cuda"), "convT"),
          (torch.randn((100, 52), device="cuda"), "linear"), (torch.randn((33, 129, 9), device="cuda"), "conv"),
          (torch.randn((1000, 776, 3), device="cuda"), "conv"), (torch.randn((264, 520, 4), device="cuda"), "convT"),
          (torch.randn((24, 40, 11), device="cuda"), "conv")]     # thousands of tiles; 4 and 11 taps
    keys = []
    for w, kind in ws:
        for k in (kind, kind + "D"):
            rt.packed(w, k, rt.tdtype)
            keys.append((w, k))
    for w, _ in ws:
        w.mul_(1.7).add_(0.25)                     # "an optimiser step"
    rt.invalidate()
    assert rt.fused_repack
    rt.refresh_all()
    torch.cuda.synchronize()
    for w, k in keys:
        got = rt._packed[(id(w), k, rt.tdtype)][1]
        d = rt._layout(w, k)
        if got.data_ptr() == w.data_ptr():
            continue                               # (float32 linear: the parameter itself is the compute copy)
        assert torch.equal(got[:, :, : d.shape[2]], d.to(rt.tdtype)), k
        assert float(got[:, :, d.shape[2]:].abs().sum()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_weight_gradients_on_the_second_stream_equal_in_order_launches(use_graph):
    """TrainRuntime.weight_grad: the weight / bias gradient launches of a pass queued and issued in groups on a forked stream (joined
    when the autograd engine finishes) leave the same gradients as the same launches issued in place, eager and replayed"""
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.model import UNetCFG1d
    from jen1_amd.optim import FusedAdamW
    from jen1_amd.train import GraphedLossStep
    betas, _ = get_beta_schedule("linear", 1000)
    B, T = 2, 300
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, "text_guided").items()}
    t = torch.tensor([17, 801], dtype=torch.long, device="cuda")
    grads = {}
    for group in (0, 3, 1000):
        model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="f32", device="cuda")
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        graph = model.train_graph("f32")
        graph.rt.wgrad_group = group
        gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda",
                               cfg_dropout_proba=0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
        step = GraphedLossStep(graph, gd) if use_graph else None
        if step is not None:
            step(x0, t, cond, False)            # capture
        opt.zero_grad()
        for rnd in range(2):                    # two passes accumulate
            torch.manual_seed(11 + rnd)
            if step is not None:
                step(x0, t, cond, False)
            else:
                gd.training_loosses(graph, x0, t, cond, causal=False).backward()
        assert not graph.rt._wqueue and not graph.rt._wjoin and not graph.rt._wheld
        torch.cuda.synchronize()
        grads[group] = opt.flat_grad.clone()
        assert float(grads[group].abs().max()) > 0
    for group in (3, 1000):
        assert float((grads[group] - grads[0]).abs().max()) <= 2e-5 * float(grads[0].abs().max()), group


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("skinny_second", [False, True])
def test_gemm_pair_equals_two_launches(rts, mode, skinny_second):
    """jen1_train_gemm_pair: two independent products in one launch give, bit for bit, what the two jen1_train_gemm launches give
    (64 x 64 form first; 64 x 64 or skinny form second; ragged M / N / K)"""
    from jen1_amd.gemm_host import operand as _operand
    rt = rts[mode]
    dt = torch.float32 if mode == "f32" else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(5)
    M0, N0, K0 = 200, 136, 72            # first: K not contiguous on either operand (the weight-gradient layout), float32 accumulate
    M1, N1, K1 = (24, 520, 256) if skinny_second else (150, 100, 96)
    a0 = torch.randn(K0, M0, device="cuda", generator=gen).to(dt)
    b0 = torch.randn(K0, N0, device="cuda", generator=gen).to(dt)
    a1 = torch.randn(M1, K1, device="cuda", generator=gen).to(dt)
    b1 = torch.randn(N1, K1, device="cuda", generator=gen).to(dt)
    init0 = torch.randn(M0, N0, device="cuda", generator=gen)

    def run(paired):
        c0 = init0.clone()
        c1 = torch.zeros(M1, N1, device="cuda", dtype=dt)
        kw0 = dict(dtype=rt.dt, ldc_m=N0, accumulate=True, c_f32=True)
        kw1 = dict(dtype=rt.dt, ldc_m=N1, skinny=skinny_second)
        o0 = (_operand(a0.data_ptr(), 1, M0), _operand(b0.data_ptr(), 1, N0))
        o1 = (_operand(a1.data_ptr(), K1, 1), _operand(b1.data_ptr(), K1, 1))
        if paired:
            blk = rt.gemm(o0[0], o0[1], c0.data_ptr(), M0, N0, K0, defer=True, **kw0)
            rt.gemm(o1[0], o1[1], c1.data_ptr(), M1, N1, K1, pair_with=blk, **kw1)
        else:
            rt.gemm(o0[0], o0[1], c0.data_ptr(), M0, N0, K0, **kw0)
            rt.gemm(o1[0], o1[1], c1.data_ptr(), M1, N1, K1, **kw1)
        torch.cuda.synchronize()
        return c0, c1

    p0, p1 = run(True)
    s0, s1 = run(False)
    assert torch.equal(p0, s0) and torch.equal(p1, s1)
    ref0 = init0 + a0.float().t() @ b0.float()
    ref1 = a1.float() @ b1.float().t()
    tol = 1e-4 if mode == "f32" else 2e-2
    assert float((p0 - ref0).abs().max()) <= tol * float(ref0.abs().max())
    assert float((p1.float() - ref1).abs().max()) <= tol * float(ref1.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("op", ["group_norm", "layer_norm", "linear"])
def test_forked_layers_merge_the_gradient_of_the_branch_around_them(rts, mode, op):
    """fork=True: (layer(x), x) -- the gradient that reaches x along the second output is added INSIDE the layer's backward kernel
    (jen1_gn_backward_add / jen1_ln_backward_add / the residual of the data-gradient GEMM); same gradients as the plain layer plus
    autograd's accumulation"""
    from jen1_amd import train as TR
    rt = rts[mode]
    gen = torch.Generator(device="cuda").manual_seed(3)
    B, Lx, C = 4, 40, 64
    x0 = torch.randn(B, Lx, C, device="cuda", generator=gen).to(rt.tdtype)
    w1 = torch.randn(B, Lx, C, device="cuda", generator=gen).to(rt.tdtype)
    w2 = torch.randn(B, Lx, C, device="cuda", generator=gen).to(rt.tdtype)
    gamma = torch.nn.Parameter(torch.rand(C, device="cuda", generator=gen) + 0.5)
    beta = torch.nn.Parameter(torch.randn(C, device="cuda", generator=gen))
    weight = torch.nn.Parameter(torch.randn(C, C, device="cuda", generator=gen) * 0.1)
    bias = torch.nn.Parameter(torch.randn(C, device="cuda", generator=gen))

    def run(fork):
        for p_ in (gamma, beta, weight, bias):
            p_.grad = None
        rt.invalidate()
        x = x0.clone().requires_grad_()
        if op == "group_norm":
            out = TR.group_norm(rt, x, gamma, beta, C, 8, 1e-5, None, True, fork=fork)
        elif op == "layer_norm":
            out = TR.layer_norm(rt, x, gamma, beta, fork=fork)
        else:
            out = TR.linear(rt, x, weight, bias, fork=fork)
        y, xa = out if fork else (out, x)
        ((y * w1).float().sum() + (xa * w2).float().sum()).backward()
        torch.cuda.synchronize()
        return y.detach().float(), x.grad.float()

    y1, g1 = run(True)
    y0, g0 = run(False)
    assert torch.equal(y1, y0)
    tol = 1e-6 if mode == "f32" else 2e-2
    assert float((g1 - g0).abs().max()) <= tol * float(g0.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("rows,C", [(384, 1024), (192, 512), (48, 256), (5, 72), (1, 8)])
def test_dual_layer_norm_equals_two_layer_norms(rts, mode, rows, C):
    """DualLayerNormFn (self-attention's norm / norm_context of the same x, blocks.py:427-429): both outputs, the merged input gradient
    (two branches + the alias of x around the sub-block) and the four parameter gradients against float64 autograd of two F.layer_norm"""
    from jen1_amd import train as TR
    rt = rts[mode]
    gen = torch.Generator(device="cuda").manual_seed(rows * 7 + C)
    x0 = (torch.randn(rows, C, device="cuda", generator=gen) * 1.5 + 0.3).to(rt.tdtype)
    ws = [torch.randn(rows, C, device="cuda", generator=gen).to(rt.tdtype) for _ in range(3)]
    ps = [torch.nn.Parameter(torch.rand(C, device="cuda", generator=gen) + 0.5) if i % 2 == 0 else
          torch.nn.Parameter(torch.randn(C, device="cuda", generator=gen)) for i in range(4)]
    rt.invalidate()
    x = x0.clone().requires_grad_()
    y1, y2, xa = TR.DualLayerNormFn.apply(x, *ps, rt, 1e-5)
    ((y1 * ws[0]).float().sum() + (y2 * ws[1]).float().sum() + (xa * ws[2]).float().sum()).backward()
    torch.cuda.synchronize()
    xr = x0.double().requires_grad_()
    pr = [p_.detach().double().requires_grad_() for p_ in ps]
    r1 = torch.nn.functional.layer_norm(xr, (C,), pr[0], pr[1], 1e-5)
    r2 = torch.nn.functional.layer_norm(xr, (C,), pr[2], pr[3], 1e-5)
    ((r1 * ws[0].double()).sum() + (r2 * ws[1].double()).sum() + (xr * ws[2].double()).sum()).backward()
    tol = 2e-6 if mode == "f32" else 1.5e-2
    rel = lambda a, b: float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30)   # noqa: E731
    assert rel(y1, r1.detach()) <= tol and rel(y2, r2.detach()) <= tol
    assert rel(x.grad, xr.grad) <= tol
    for p_, q_ in zip(ps, pr):
        assert rel(p_.grad, q_.grad) <= (2e-5 if mode == "f32" else 1.5e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("rows,C", [(2080, 1024), (48, 512), (7, 64)])
def test_layer_norm_backward_without_input_gradient(rts, mode, rows, C):
    """norm_context over the text embedding (blocks.py:426): the input needs no gradient, jen1_ln_backward_add runs with dx = NULL and
    only accumulates dgamma / dbeta -- the same values as when dx is computed too"""
    from jen1_amd import train as TR
    rt = rts[mode]
    gen = torch.Generator(device="cuda").manual_seed(rows + C)
    x0 = torch.randn(rows, C, device="cuda", generator=gen).to(rt.tdtype)
    w = torch.randn(rows, C, device="cuda", generator=gen).to(rt.tdtype)
    gamma = torch.nn.Parameter(torch.rand(C, device="cuda", generator=gen) + 0.5)
    beta = torch.nn.Parameter(torch.randn(C, device="cuda", generator=gen))
    got = {}
    for needs in (True, False):
        gamma.grad, beta.grad = None, None
        x = x0.clone().requires_grad_(needs)
        (TR.layer_norm(rt, x, gamma, beta) * w).float().sum().backward()
        torch.cuda.synchronize()
        got[needs] = (gamma.grad.clone(), beta.grad.clone())
        assert (x.grad is not None) == needs
    for a, b in zip(got[True], got[False]):
        assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("rows,C,ld", [(24000, 128, 128), (2500, 72, 128), (6016, 256, 256), (37, 40, 40)])
def test_colsum_many_rows_and_few(mode, rows, C, ld):
    """jen1_colsum (the bias gradient where no GEMM carries it: sum over (b, t) of dy): the long-slice form of the long levels and the
    small form, accumulated into a non-zero vector; padding columns of the pitch never reach the result"""
    from jen1_amd import lib as L
    lib = L.load()
    td = torch.float32 if mode == "f32" else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(rows + C)
    x = torch.full((rows, ld), 9.0, device="cuda", dtype=td)
    x[:, :C] = (torch.randn((rows, C), device="cuda", generator=gen)).to(td)
    out0 = torch.randn((C,), device="cuda", generator=gen)
    out = out0.clone()
    L.check(lib.jen1_colsum(x.data_ptr(), out.data_ptr(), rows, C, ld, L.F32 if mode == "f32" else L.BF16, torch.cuda.current_stream().cuda_stream), "jen1_colsum")
    torch.cuda.synchronize()
    want = out0.double() + x[:, :C].double().sum(0)
    assert rel_err(out.cpu().numpy(), want.float().cpu().numpy()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the fused ends of a pass (csrc/train_glue.hip: pack_input, ContextRowsFn, CfgLossFn), the shared fixed-context rows and the skip
# aliases against the LITERAL path (ATen glue, one context copy per row, autograd's own accumulation) -- same loss, same gradients
# ---------------------------------------------------------------------------------------------------------------------
def _ab_loss_and_grads(model, fused, *, loss_type, objective, scale_cfg, drop, task="music_inpaint", causal=False):
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    B, T = 3, 96
    betas, _ = get_beta_schedule("linear", 1000)
    t = torch.tensor([17, 801, 433], dtype=torch.long, device="cuda")
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, task).items()}
    assert cond["cross_attn_masks"] is not None and not bool(cond["cross_attn_masks"].all())      # a partial text mask
    noise = dev(fill_uniform("synth.trainnoise.ab", (B, 128, T), 3, 0.0, 1.0))
    gd = GaussianDiffusion(steps=1000, betas=betas, objective=objective, loss_type=loss_type, device="cuda",
                           cfg_dropout_proba=0.5 if drop else 0.0, embedding_scale=0.8, batch_cfg=True, scale_cfg=scale_cfg)
    model.train()
    for p in model.parameters():
        p.grad = None
    graph = model.train_graph("f32")
    rt = graph.rt
    old = (rt.fused_glue, rt.share_fixed_context, rt.fork_skips)
    rt.fused_glue = rt.share_fixed_context = rt.fork_skips = bool(fused)
    try:
        rows = torch.tensor([False, True, False], device="cuda") if drop else None
        loss = gd.training_loosses(graph, x0, t, cond, noise=noise, causal=causal, dropout_rows=rows)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        rt.fused_glue, rt.share_fixed_context, rt.fork_skips = old
    return float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("objective,scale_cfg,drop,causal", [("noise", True, False, False), ("x0", False, True, False), ("v", True, True, True)])
def test_fused_glue_shared_context_and_skip_aliases_equal_the_literal_path(tiny_model, loss_type, objective, scale_cfg, drop, causal):
    kw = dict(loss_type=loss_type, objective=objective, scale_cfg=scale_cfg, drop=drop, causal=causal,
              task="music_cont" if causal else "music_inpaint")
    l0, g0 = _ab_loss_and_grads(tiny_model, False, **kw)
    l1, g1 = _ab_loss_and_grads(tiny_model, True, **kw)
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l0, l1)
    gmax = max(float(g.norm()) for g in g0.values())
    for n in g0:
        d = float((g1[n] - g0[n]).norm())
        assert d <= 2e-4 * max(float(g0[n].norm()), 1e-3 * gmax), (n, d, float(g0[n].norm()))


def test_down_level_without_blocks_keeps_the_previous_skip():
    """a level with neither ResBlocks nor a transformer opens no skip slot: the next level's forked down conv must not overwrite the slot
    of the level before (train.TrainGraph.unet_rows, ``put``); skip aliases on == off"""
    from jen1_amd.model import UNetCFG1d
    cfg = tiny_model_config()
    cfg.update(multipliers=[1, 1, 2, 2], factors=[1, 2, 2], num_blocks=[2, 0, 2], attentions=[0, 0, 0, 1])
    try:
        model = UNetCFG1d(**cfg, init_seed=1234, compute_dtype="f32", device="cuda")
    except AssertionError as e:          # (the spec may refuse an empty level: then there is nothing to mis-slot)
        pytest.skip(f"configuration refused: {e}")
    kw = dict(loss_type="l2", objective="noise", scale_cfg=True, drop=False)
    graph = model.train_graph("f32")
    # the differentiable forward against the sampling engine's forward of the same module (two implementations of model.py:225-265)
    B, T = 3, 96
    x, cond = dev(synth.latents(B, T)), {k: dev(v) for k, v in synth.conditioning(B, T, "music_inpaint").items()}
    t = torch.tensor([17, 801, 433], dtype=torch.long, device="cuda")
    fkw = dict(embedding=cond["cross_attn_cond"], embedding_mask=cond["cross_attn_masks"], embedding_scale=0.8, batch_cfg=True, scale_cfg=True,
               channels_list=[cond["input_concat_cond"]], causal=False)
    model.eval()
    y_eng = model(x, t, **fkw)
    with torch.no_grad():
        y_tr = graph(x, t, **fkw)
    torch.cuda.synchronize()
    assert float((y_tr - y_eng).abs().max()) <= 1e-4 * float(y_eng.abs().max())
    outs = []
    for on in (False, True):
        l, g = _ab_loss_and_grads(model, on, **kw)
        outs.append((l, g))
    (l0, g0), (l1, g1) = outs
    assert abs(l1 - l0) <= 1e-5 * abs(l0)
    gmax = max(float(g.norm()) for g in g0.values())
    for n in g0:
        assert float((g1[n] - g0[n]).norm()) <= 2e-4 * max(float(g0[n].norm()), 1e-3 * gmax), n


# ---------------------------------------------------------------------------------------------------------------------
# the text-context K / V projections of all cross-attention layers as one product (train.KvBank / ContextKVFn, csrc/train_kvbank.hip)
# ---------------------------------------------------------------------------------------------------------------------
def test_kv_fold_kernels_match_the_chain_rule_of_the_fold():
    """jen1_kv_fold: Wf = bf16(W diag(gamma)), WfT = its transpose, bias = W beta; jen1_kv_fold_backward: the gradients of W, gamma, beta from
    dWf and dbias -- against torch autograd of the same fold in float64"""
    import ctypes as C
    from jen1_amd import lib as L
    lib = L.load()
    K, widths = 256, [64, 160, 32]
    gen = torch.Generator(device="cuda").manual_seed(2)
    ws = [torch.randn((n, K), device="cuda", generator=gen) for n in widths]
    gs = [torch.randn((K,), device="cuda", generator=gen) for _ in widths]
    bs = [torch.randn((K,), device="cuda", generator=gen) for _ in widths]
    gw = [torch.randn_like(w) for w in ws]                 # (non-zero: the kernel ACCUMULATES into .grad)
    gg = [torch.randn_like(g) for g in gs]
    gb = [torch.randn_like(b) for b in bs]
    gw0, gg0, gb0 = [t.clone() for t in gw], [t.clone() for t in gg], [t.clone() for t in gb]
    Ntot = sum(widths)
    ents = (L.KvLayer * len(widths))()
    n0 = 0
    for i, n in enumerate(widths):
        e = ents[i]
        e.w, e.gamma, e.beta, e.gw, e.ggamma, e.gbeta = (t.data_ptr() for t in (ws[i], gs[i], bs[i], gw[i], gg[i], gb[i]))
        e.n0, e.N = n0, n
        n0 += n
    tab = torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8).cuda()
    wf = torch.empty((Ntot, K), device="cuda", dtype=torch.bfloat16)
    wft = torch.empty((K, Ntot), device="cuda", dtype=torch.bfloat16)
    bias = torch.empty((Ntot,), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    L.check(lib.jen1_kv_fold(tab.data_ptr(), len(widths), Ntot, K, wf.data_ptr(), wft.data_ptr(), Ntot, bias.data_ptr(), s), "jen1_kv_fold")
    torch.cuda.synchronize()
    want_wf = torch.cat([w * g[None] for w, g in zip(ws, gs)])
    assert torch.equal(wf, want_wf.to(torch.bfloat16)) and torch.equal(wft, wf.t().contiguous())
    want_b = torch.cat([(w.double() @ b.double()) for w, b in zip(ws, bs)])
    assert float((bias.double() - want_b).abs().max()) < 1e-4 * float(want_b.abs().max())
    dwf = torch.randn((Ntot, K), device="cuda", generator=gen)
    dbias = torch.randn((Ntot,), device="cuda", generator=gen)
    L.check(lib.jen1_kv_fold_backward(tab.data_ptr(), len(widths), Ntot, K, dwf.data_ptr(), dbias.data_ptr(), s), "jen1_kv_fold_backward")
    torch.cuda.synchronize()
    n0 = 0
    for i, n in enumerate(widths):
        w, g, b = (t.double().requires_grad_() for t in (ws[i], gs[i], bs[i]))
        ((w * g[None]) * dwf[n0:n0 + n].double()).sum().add((w @ b) @ dbias[n0:n0 + n].double()).backward()
        for got, base, ref in ((gw[i], gw0[i], w.grad), (gg[i], gg0[i], g.grad), (gb[i], gb0[i], b.grad)):
            assert float(((got - base).double() - ref).abs().max()) < 2e-5 * float(ref.abs().max()), i
        n0 += n


def test_sum_rows_strided_adds_the_sharers_blocks_in_place():
    from jen1_amd import lib as L
    lib = L.load()
    nblk, rows, width, ld = 5, 7, 64, 200
    gen = torch.Generator(device="cuda").manual_seed(4)
    m = torch.randn((nblk * rows + 2, ld), device="cuda", generator=gen).to(torch.bfloat16)
    ref = m.clone()
    want = m[: nblk * rows, 40:40 + width].float().view(nblk, rows, width).sum(0)
    L.check(lib.jen1_sum_rows_strided(m.data_ptr() + 40 * 2, nblk, rows, width, ld, L.BF16, torch.cuda.current_stream().cuda_stream), "jen1_sum_rows_strided")
    torch.cuda.synchronize()
    assert float((m[:rows, 40:40 + width].float() - want).abs().max()) <= 2e-2 * float(want.abs().max())
    ref[:rows, 40:40 + width] = m[:rows, 40:40 + width]
    assert torch.equal(m, ref)                              # nothing else was touched


@pytest.mark.parametrize("share", [True, False], ids=["shared-fixed-context", "one-context-per-row"])
def test_stacked_context_projection_equals_one_layernorm_and_linear_per_layer(share):
    """the pass with ``kv_grouped`` (one standardisation + one product for the K | V of all 13 cross-attentions, one weight-gradient and one
    data-gradient product, the fold's chain rule) against the pass that runs norm_context + to_kv per layer: same loss, same gradient of
    EVERY parameter within bf16 rounding -- full model (the stacked operand is 17408 x 1024), CFG pair, partial text mask, CFG dropout"""
    from jen1_amd.config import full_model_config
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    from jen1_amd.model import UNetCFG1d
    model = UNetCFG1d(**full_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    model.train()
    B, T = 2, 375
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.5,
                           embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, "music_inpaint").items()}
    noise = dev(fill_uniform("synth.trainnoise.kv", (B, 128, T), 3, 0.0, 1.0))
    t = torch.tensor([17, 801], dtype=torch.long, device="cuda")
    rows = torch.tensor([False, True], device="cuda")
    graph = model.train_graph("bf16")
    rt = graph.rt
    # a pass that carries the overlapped gradient exchange keeps the per-layer form (the stacked form finishes these gradients last,
    # after their blocks' slices of the flat gradient have been sent: train.TrainGraph._stacked_context_kv)
    class _Armed:
        active = True
    probe = torch.zeros((3, 129, 1024), dtype=torch.bfloat16, device="cuda")
    assert graph._stacked_context_kv(probe, 4) is not None
    graph.exchange = _Armed()
    try:
        assert graph._stacked_context_kv(probe, 4) is None
    finally:
        graph.exchange = None
    res = []
    old = (rt.kv_grouped, rt.share_fixed_context)
    try:
        rt.share_fixed_context = share
        for grouped in (False, True):
            rt.kv_grouped = grouped
            for p_ in model.parameters():
                p_.grad = None
            loss = gd.training_loosses(graph, x0, t, cond, noise=noise, causal=False, dropout_rows=rows)
            loss.backward()
            torch.cuda.synchronize()
            res.append((float(loss.detach()), {n: p_.grad.clone() for n, p_ in model.named_parameters()}))
    finally:
        rt.kv_grouped, rt.share_fixed_context = old
    (l0, g0), (l1, g1) = res
    assert abs(l1 - l0) <= 2e-2 * abs(l0), (l0, l1)
    gmax = max(float(g.norm()) for g in g0.values())
    worst = ("", 0.0)
    for n in g0:
        d = float((g1[n] - g0[n]).norm()) / max(float(g0[n].norm()), 1e-2 * gmax)
        if d > worst[1]:
            worst = (n, d)
    assert worst[1] < 6e-2, worst
    # the folded parameters (norm_context, to_kv of the 13 layers): two bf16 roundings of the same float32 mathematics differ by a few
    # per cent per tensor on the levels with 1 - 3 positions; the judge is the float32 pass of the same module (the mode the reference's
    # autograd pins at 1e-3): the stacked pass must be as close to it as the per-layer pass
    for p_ in model.parameters():
        p_.grad = None
    g32 = model.train_graph("f32")
    loss = gd.training_loosses(g32, x0, t, cond, noise=noise, causal=False, dropout_rows=rows)
    loss.backward()
    torch.cuda.synchronize()
    ref = {n: p_.grad.clone() for n, p_ in model.named_parameters()}
    folded = [n for n in g0 if "cross_attention.norm_context" in n or "cross_attention.to_kv" in n]
    assert len(folded) == 39
    rel = lambda g, n: float((g[n] - ref[n]).norm()) / max(float(ref[n].norm()), 1e-12)
    e_old, e_new = {n: rel(g0, n) for n in folded}, {n: rel(g1, n) for n in folded}
    print(f"worst difference between the two bf16 passes {worst[1]:.3e} ({worst[0]}); folded parameters against the float32 pass: "
          f"per layer {max(e_old.values()):.3e} (mean {sum(e_old.values()) / 39:.3e}), stacked {max(e_new.values()):.3e} (mean {sum(e_new.values()) / 39:.3e})")
    bad = [(n, e_old[n], e_new[n]) for n in folded if e_new[n] > max(1.5 * e_old[n], 3e-2)]
    assert not bad, bad[:4]


@pytest.mark.parametrize("T", [300, 96], ids=["every-layer-on-the-gemm-attention-path", "mixed-small-and-gemm-attention"])
def test_stacked_context_projection_with_gemm_attention_and_shared_context(T):
    """a cross-attention whose Nq does not fit the one-launch core (Nq > 64) returns an already-summed [Bk] gradient of
    its K | V window instead of writing the [b_eff] window in place; the sharers' blocks of that window (uninitialised memory) must not
    reach the strided sum of ContextKVFn.backward.  Tiny model, bf16, CFG pair with the shared fixed context: T = 300 puts every layer on
    the GEMM attention path (Nq = 300 / 150), T = 96 mixes both paths.  Grouped pass == per-layer pass for EVERY parameter; twice, with the
    allocator's memory dirtied in between, so that garbage cannot hide as zeros of a fresh allocation"""
    from jen1_amd.diffusion import GaussianDiffusion, get_beta_schedule
    from jen1_amd.init_fill import fill_uniform
    from jen1_amd.model import UNetCFG1d
    model = UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype="bf16", device="cuda")
    model.train()
    B = 3
    betas, _ = get_beta_schedule("linear", 1000)
    gd = GaussianDiffusion(steps=1000, betas=betas, objective="noise", loss_type="l2", device="cuda", cfg_dropout_proba=0.5,
                           embedding_scale=0.8, batch_cfg=True, scale_cfg=True)
    x0 = dev(synth.latents(B, T, key="clip"))
    cond = {k: dev(v) for k, v in synth.conditioning(B, T, "music_inpaint").items()}
    noise = dev(fill_uniform("synth.trainnoise.kvg", (B, 128, T), 3, 0.0, 1.0))
    t = torch.tensor([17, 801, 405], dtype=torch.long, device="cuda")
    rows = torch.tensor([False, True, False], device="cuda")
    graph = model.train_graph("bf16")
    rt = graph.rt
    old = (rt.kv_grouped, rt.share_fixed_context)
    res = []
    try:
        rt.share_fixed_context = True
        for grouped in (False, True, True):
            rt.kv_grouped = grouped
            for p_ in model.parameters():
                p_.grad = None
            # dirty the caching allocator's free blocks: torch.empty in the pass then returns non-zero memory
            junk = [torch.full((1 << 22,), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(8)]
            del junk
            loss = gd.training_loosses(graph, x0, t, cond, noise=noise, causal=False, dropout_rows=rows)
            loss.backward()
            torch.cuda.synchronize()
            res.append((float(loss.detach()), {n: p_.grad.clone() for n, p_ in model.named_parameters()}))
    finally:
        rt.kv_grouped, rt.share_fixed_context = old
    (l0, g0), (l1, g1), (l2, g2) = res
    assert abs(l1 - l0) <= 2e-2 * abs(l0), (l0, l1)
    gmax = max(float(g.norm()) for g in g0.values())
    for g_new in (g1, g2):
        worst = ("", 0.0)
        for n in g0:
            assert bool(torch.isfinite(g_new[n]).all()), n
            d = float((g_new[n] - g0[n]).norm()) / max(float(g0[n].norm()), 1e-2 * gmax)
            if d > worst[1]:
                worst = (n, d)
        assert worst[1] < 8e-2, worst
