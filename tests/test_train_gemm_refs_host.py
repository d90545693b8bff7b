"""CPU-only: the float64 model of jen1_train_gemm's descriptor (tests/train_gemm_common.py) against torch, fed by the project's own host
code, and the kernel forms the case table of tests/test_gpu_train_gemm_forms.py expects, asked of jen1_train_gemm_form (host code).

``ModelRuntime`` stands in for GemmRuntime: ``conv_forward`` / ``conv_dgrad`` / ``conv_wgrad`` of jen1_amd/gemm_host.py run unchanged on
float64 CPU tensors, and every ``gemm`` they issue -- the operands ``gemm_host.operand`` and ``ConvGeom.fwd_map`` / ``bwd_map`` describe --
is carried out by the model on the memory the pointers name.  Agreement with F.conv1d / F.conv_transpose1d / F.linear and their autograd
gradients to 1e-12 pins the model and ConvGeom's maps together.
"""
import ctypes as C
import os
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_gemm_common as T
from helpers import ROOT
from jen1_amd import gemm_host as G
from jen1_amd import lib as L

TOL = 1e-12


def _view(ptr, n):
    return np.ctypeslib.as_array((C.c_double * n).from_address(ptr))


def _at_zero(op):
    o = L.GemmOperand.from_buffer_copy(op)
    o.p = 0
    return o


class ModelRuntime(SimpleNamespace):
    """the switches of GemmRuntime + a ``gemm`` that is the float64 model on host memory (every dtype is float64 here)"""

    def __init__(self, **over):
        super().__init__(**dict(dict(skinny_gemm=True, skinny_max_steps=64, target_wgs=256, min_steps=4, big_convs=True, big_conv_rows=4096,
                                     big_wgrads=True, big_wgrad_rows=4096, wgrad_plain_rmw=True, stats=None), **over))
        self.calls = []
        self._acc = torch.zeros(1 << 16, dtype=torch.float64)

    def dt_of(self, t):
        assert t.dtype == torch.float64
        return L.F32

    def split_accumulator(self, n):
        assert n <= self._acc.numel()
        return self._acc

    def hand_over(self, acc, out, residual=None):
        n = out.numel()
        out.view(-1)[:] = acc[:n] + (0 if residual is None else residual.reshape(-1))
        acc[:n] = 0
        return out

    def gemm(self, a, b, c_ptr, M, N, K, *, dtype, bias=None, rowsum=None, residual=None, shift_b=None, skinny=False, defer=False,
             pair_with=None, **kw):
        assert not defer and pair_with is None
        g = dict(M=M, N=N, K=K, **kw)
        taps, batches = g.get("taps", 1), g.get("batches", 1)
        sb = None if shift_b is None else shift_b.numpy()
        bufs = []
        for op, rows in ((a, M), (b, N)):
            off, ok = T.operand_offsets(_at_zero(op), rows, K, taps, batches, sb)
            assert off[ok].min() >= 0
            bufs.append(_view(op.p, int(off[ok].max()) + 1))
        oc = T.c_offsets(dict(g, taps=taps, batches=batches))
        assert oc.min() >= 0
        cv = _view(c_ptr, int(oc.max()) + 1)
        r = T.gemm_model(_at_zero(a), _at_zero(b), bufs[0], bufs[1], cv, g, bias=None if bias is None else bias.numpy(),
                         residual=None if residual is None else _view(residual.data_ptr(), int(oc.max()) + 1),
                         rowsum=None if rowsum is None else rowsum.numpy()[:M], shift_b=sb)
        cv[r["touched"]] = r["c"][r["touched"]]
        if rowsum is not None:
            rowsum.numpy()[:M] = r["rowsum"]
        self.calls.append(dict(g, skinny=skinny))


def _rows(x_bcl):
    """[B, C, L] -> channel-last [B, L, pad8(C)] with zero padding columns"""
    B, Cc, Lx = x_bcl.shape
    out = torch.zeros((B, Lx, G.pad8(Cc)), dtype=torch.float64)
    out[:, :, :Cc] = x_bcl.detach().transpose(1, 2)
    return out


def _back(rows, Cc):
    return rows[:, :, :Cc].transpose(1, 2)


def _close(got, ref):
    got, ref = torch.as_tensor(got), torch.as_tensor(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert float((got - ref).abs().max()) <= TOL * float(ref.abs().max()), float((got - ref).abs().max() / ref.abs().max())


CONVS = [
    # kind, B, Ci, Co, L, k, stride, causal (True / False / one flag per clip)
    ("conv", 2, 16, 24, 37, 3, 1, False),
    ("conv", 3, 13, 40, 50, 3, 1, True),                     # padded channel columns
    ("conv", 2, 8, 12, 101, 9, 4, False),
    ("conv", 2, 8, 12, 94, 5, 2, True),
    ("conv", 16, 128, 72, 6, 3, 1, False),                   # few rows, skinny form off: the host splits K (atomics + hand-over)
    ("conv", 3, 8, 12, 20, 5, 1, (True, False, True)),       # causal and non-causal clips side by side
    ("conv", 2, 8, 12, 21, 3, 2, (False, True)),
    ("convT", 2, 24, 16, 19, 4, 2, False),
    ("convT", 2, 16, 8, 23, 8, 4, False),
    ("linear", 2, 48, 20, 29, 1, 1, False),
]


@pytest.mark.parametrize("case", CONVS, ids=lambda c: "-".join(str(v) for v in c))
def test_model_reproduces_the_conv_family_and_its_gradients(case):
    kind, B, Ci, Co, Lx, k, stride, causal = case
    gen = torch.Generator().manual_seed(7 * Lx + k)
    x = torch.randn((B, Ci, Lx), generator=gen, dtype=torch.float64).requires_grad_()
    w = torch.randn((Ci, Co, k) if kind == "convT" else (Co, Ci, k), generator=gen, dtype=torch.float64).requires_grad_()
    bias = torch.randn((Co,), generator=gen, dtype=torch.float64).requires_grad_()
    pads = lambda c: (k - 1, 0) if c else ((k - 1) // 2, (k - 1) - (k - 1) // 2)
    pad_b = None
    if kind == "convT":
        pad = stride // 2 + stride % 2
        y_ref = F.conv_transpose1d(x, w, bias, stride=stride, padding=pad, output_padding=stride % 2)
    elif kind == "linear":
        pad = 0
        y_ref = F.linear(x.transpose(1, 2), w[:, :, 0], bias).transpose(1, 2)
    elif isinstance(causal, tuple):
        pad = 0
        y_ref = torch.cat([F.conv1d(F.pad(x[i:i + 1], pads(c)), w, bias, stride=stride) for i, c in enumerate(causal)])
        neg = torch.tensor([-pads(c)[0] for c in causal] + [-pads(causal[0])[0]], dtype=torch.int32)       # B + 1 entries
        pad_b = (neg, -neg)
    else:
        pad = pads(causal)[0]
        y_ref = F.conv1d(F.pad(x, pads(causal)), w, bias, stride=stride)
    dy = torch.randn(y_ref.shape, generator=gen, dtype=torch.float64)
    y_ref.backward(dy)
    L_out = y_ref.shape[2]
    rt = ModelRuntime(**(dict(skinny_gemm=False, min_steps=1) if B == 16 else {}))       # (B == 16: the host splits K)
    g = G.ConvGeom(kind, k, stride, pad, Lx, L_out, Ci, Co, pad_b=pad_b)
    wk = w.detach() if kind != "linear" else w.detach()[:, :, 0]
    wp, wd = G.compute_copy(wk, kind, torch.float64), G.compute_copy(wk, kind + "D", torch.float64)
    xr, dyr = _rows(x), _rows(dy)
    _close(_back(G.conv_forward(rt, xr, wp, bias.detach(), g), Co), y_ref.detach())
    res = torch.randn(xr.shape, generator=gen, dtype=torch.float64)
    res[:, :, Ci:] = 0
    _close(_back(G.conv_dgrad(rt, dyr, wp, g, wd=wd, residual=res), Ci), x.grad + _back(res, Ci))
    _close(_back(G.conv_dgrad(rt, dyr, wp, g), Ci), x.grad)            # without the transposed copy: the weight read across its rows
    gw0 = torch.randn(w.shape, generator=gen, dtype=torch.float64)
    gb0 = torch.randn((Co,), generator=gen, dtype=torch.float64)
    gw, gb = gw0.clone(), gb0.clone()
    fused = G.conv_wgrad(rt, xr, dyr, gw if kind != "linear" else gw[:, :, 0], g, gb)
    _close(gw - gw0, w.grad)
    assert fused == (kind != "convT")
    if fused:
        _close(gb - gb0, bias.grad)                                    # the bias gradient through rowsum
    assert B != 16 or sum(c.get("splitk", 1) > 1 for c in rt.calls) >= 3


@pytest.mark.parametrize("k,stride", [(7, 1), (3, 1), (5, 2)])
def test_model_reproduces_reflect_padding(k, stride):
    """F.pad(mode="reflect") followed by the convolution (the SEANet layers): the padding is the index map's mirror"""
    gen = torch.Generator().manual_seed(k)
    B, Ci, Co, Lx = 2, 8, 12, 33
    x = torch.randn((B, Ci, Lx), generator=gen, dtype=torch.float64)
    w = torch.randn((Co, Ci, k), generator=gen, dtype=torch.float64)
    bias = torch.randn((Co,), generator=gen, dtype=torch.float64)
    pad = (k - 1) // 2
    y_ref = F.conv1d(F.pad(x, (pad, pad), mode="reflect"), w, bias, stride=stride)
    g = G.ConvGeom("conv", k, stride, pad, Lx, y_ref.shape[2], Ci, Co, reflect=True)
    _close(_back(G.conv_forward(ModelRuntime(), _rows(x), G.compute_copy(w, "conv", torch.float64), bias, g), Co), y_ref)


@pytest.mark.parametrize("d", [16, 12, 4])
def test_model_reproduces_the_attention_products(d):
    """the products of the attention GEMM path as AttentionCoreFn describes them: the heads side by side in the rows of q, K | V and dO
    (zs1 = d, zdiv = heads), one matrix per (batch element, head) in S, P, dP and dS"""
    B, H, Nq, Nk = 2, 3, 7, 10
    Cq, ldS, Z = H * d, G.pad8(Nk), B * H
    gen = torch.Generator().manual_seed(d)
    q = torch.randn((B, Nq, Cq), generator=gen, dtype=torch.float64)
    kv = torch.randn((B, Nk, 2 * Cq), generator=gen, dtype=torch.float64)
    P = torch.zeros((Z, Nq, ldS), dtype=torch.float64)
    P[:, :, :Nk] = torch.randn((Z, Nq, Nk), generator=gen, dtype=torch.float64)
    heads = lambda t, n: t.reshape(B, n, H, d).transpose(1, 2)            # [B][H][n][d]
    k_, v_ = kv[..., :Cq], kv[..., Cq:]
    rt = ModelRuntime()
    op = G.operand
    es = 8
    scale = d ** -0.5
    S = torch.full((Z, Nq, ldS), 7.0, dtype=torch.float64)
    rt.gemm(op(q.data_ptr(), Cq, 1, zs0=Nq * Cq, zs1=d, zdiv=H), op(kv.data_ptr(), 2 * Cq, 1, zs0=Nk * 2 * Cq, zs1=d, zdiv=H), S.data_ptr(), Nq, Nk, d,
            dtype=L.F32, batches=Z, ldc_m=ldS, c_zs0=Nq * ldS, c_f32=True, alpha=scale)
    _close(S[:, :, :Nk].reshape(B, H, Nq, Nk), torch.einsum("bhnd,bhmd->bhnm", heads(q, Nq), heads(k_, Nk)) * float(np.float32(scale)))
    assert bool((S[:, :, Nk:] == 7.0).all())
    O = torch.zeros((B, Nq, Cq), dtype=torch.float64)
    rt.gemm(op(P.data_ptr(), ldS, 1, zs0=Nq * ldS), op(kv.data_ptr() + Cq * es, 1, 2 * Cq, zs0=Nk * 2 * Cq, zs1=d, zdiv=H), O.data_ptr(), Nq, d, Nk,
            dtype=L.F32, batches=Z, ldc_m=Cq, c_zs0=Nq * Cq, c_zs1=d, c_zdiv=H)
    _close(heads(O, Nq), torch.einsum("bhnm,bhmd->bhnd", P[:, :, :Nk].reshape(B, H, Nq, Nk), heads(v_, Nk)))
    dKV = torch.zeros((B, Nk, 2 * Cq), dtype=torch.float64)
    rt.gemm(op(P.data_ptr(), 1, ldS, zs0=Nq * ldS), op(q.data_ptr(), 1, Cq, zs0=Nq * Cq, zs1=d, zdiv=H), dKV.data_ptr(), Nk, d, Nq,
            dtype=L.F32, batches=Z, ldc_m=2 * Cq, c_zs0=Nk * 2 * Cq, c_zs1=d, c_zdiv=H, alpha=scale)
    _close(heads(dKV[..., :Cq], Nk), torch.einsum("bhnm,bhnd->bhmd", P[:, :, :Nk].reshape(B, H, Nq, Nk), heads(q, Nq)) * float(np.float32(scale)))
    assert float(dKV[..., Cq:].abs().max()) == 0.0


def test_model_counts_magnitudes_and_leaves_the_rest_alone():
    """S = |alpha| sum |a||b| + |bias| + |old C| + |residual| on a product small enough to write out; untouched elements stay"""
    a, b = np.array([1.0, -2.0, 3.0, np.nan]), np.array([-4.0, 5.0, 0.5, np.nan])       # M = N = 1, K = 3, a pitch of 4
    c = np.array([9.0, 10.0, 11.0])
    g = dict(M=1, N=1, K=3, ldc_m=1, alpha=-0.5, accumulate=True)
    r = T.gemm_model(G.operand(0, 4, 1), G.operand(0, 4, 1), a, b, c, g, bias=np.array([0.25]), residual=np.array([0.0, -1.0, 0.0]), c_p=1)
    assert r["c"].tolist() == [9.0, -0.5 * (-4 - 10 + 1.5) + 0.25 + 10.0 - 1.0, 11.0]
    assert r["S"].tolist() == [0.0, 0.5 * (4 + 10 + 1.5) + 0.25 + 10.0 + 1.0, 0.0] and r["touched"].tolist() == [False, True, False]
    assert T.gate(2.0, 3.0, 10, True) == 4 * (10 * 2.0 ** -24 * 3.0 + 2.0 ** -8 * 2.0) and T.gate(2.0, 3.0, 10, False) == 4 * 10 * 2.0 ** -24 * 3.0
    with pytest.raises(AssertionError):
        T.gemm_model(G.operand(0, 4, 1), G.operand(0, 4, 1), a, b, c, dict(g, K=4), c_p=1)      # the model itself never reads past K


@pytest.mark.parametrize("mode", T.MODES)
def test_check_rejects_what_a_wrong_kernel_leaves(mode):
    """Built.check on a built case: the model's own result rounded to C's dtype passes; one element off by a bf16 ulp (bf16) or by
    2^-16 relative (float32), one NaN, one column of the next head added in, one element outside the output changed -- each fails"""
    case = next(c for c in T.CASES if c.id == "direct-lean.attention-d12")
    bt = T.Built(case, mode)
    ref = bt.reference()
    good = T.round_to(ref["c"], bt.c_mode).astype(np.float64)
    assert bt.check(good) <= 0.25
    first = int(np.flatnonzero(ref["touched"])[5])
    bad = good.copy()
    bad[first] += max(abs(bad[first]), 1.0) * 2.0 ** -16
    assert bt.check(bad) > 1.0
    bad = good.copy()
    bad[first] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        bt.check(bad)
    bad = good.copy()
    bad[int(np.flatnonzero(~ref["touched"])[3])] += 1.0
    with pytest.raises(AssertionError, match="outside the output changed"):
        bt.check(bad)
    # head h with the first four channels of head h + 1 multiplied in (what an unmasked 8-element fragment at K - 4 does)
    a, b = bt.operands()
    wide = T.gemm_model(a, b, np.nan_to_num(bt.bufs["a"]), np.nan_to_num(bt.bufs["b"]), bt.bufs["c"], dict(bt.g, K=case.K + 4), c_p=T.GUARD)
    assert bt.check(T.round_to(wide["c"], bt.c_mode).astype(np.float64)) > 100.0


# ------------------------------------------------------------------ which body a call runs (jen1_train_gemm_form: host code, no GPU)
@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.load()


def _args(a, b, c_ptr, M, N, K, *, dtype, taps=1, batches=1, taps_in_z=False, ldc_m, ldc_n=1, c_tap_stride=0, c_zs0=0, c_zs1=0, c_zdiv=1,
          bias=None, splitk=1, atomic=False, accumulate=False, c_f32=False, alpha=1.0, rowsum=None, residual=None, skinny=False, shift_b=None):
    """GemmRuntime.gemm(defer=True) without a runtime: the pointers are numbers nothing reads"""
    g = L.GemmArgs()
    g.a, g.b, g.c, g.bias = a, b, c_ptr, bias
    g.c_zs0, g.c_zs1, g.ldc_m, g.ldc_n, g.c_tap_stride, g.c_zdiv = c_zs0, c_zs1, ldc_m, ldc_n, c_tap_stride, c_zdiv
    g.M, g.N, g.K, g.taps, g.batches = M, N, K, taps, batches
    g.taps_in_z, g.splitk, g.atomic, g.accumulate, g.c_f32, g.dtype = int(taps_in_z), splitk, int(atomic), int(accumulate), int(c_f32), dtype
    g.alpha, g.reserved = alpha, int(skinny)
    g.rowsum, g.residual, g.map_shift_b = rowsum, residual, shift_b
    return g


def _case_form(lib, case, mode):
    es = 4 if mode == T.F32 else 2
    P = 1 << 20
    a, b = case.a.desc(P + case.a.off * es), case.b.desc(2 * P + case.b.off * es)
    g = _args(a, b, 3 * P, case.M, case.N, case.K, dtype=L.F32 if mode == T.F32 else L.BF16, ldc_m=case.ldc_m,
              bias=4 * P if case.bias else None, rowsum=5 * P if case.rowsum else None, residual=6 * P if case.residual else None,
              shift_b=7 * P if case.shift_b is not None else None, **case.kw)
    return lib.jen1_train_gemm_form(g)


@pytest.mark.parametrize("mode", T.MODES)
def test_every_case_reaches_the_form_it_is_named_for(lib, mode):
    wrong = {c.id: (T.form_name(_case_form(lib, c, mode)), T.form_name(c.expected_form(mode)))
             for c in T.CASES + list(T.pair_cases(mode)) if mode in c.modes and _case_form(lib, c, mode) != c.expected_form(mode)}
    assert not wrong, wrong
    ids = [c.id for c in T.CASES]
    assert len(set(ids)) == len(ids)


def test_form_refuses_what_the_launch_refuses(lib):
    assert lib.jen1_train_gemm_form(None) < 0 and b"args is NULL" in lib.jen1_last_error()
    g = _args(G.operand(4096, 8, 1), G.operand(8192, 8, 1), 16384, 4, 4, 8, dtype=L.F32, ldc_m=4, splitk=2)
    assert lib.jen1_train_gemm_form(g) < 0 and b"atomic" in lib.jen1_last_error()
    g.atomic, g.c_f32 = 1, 1
    assert lib.jen1_train_gemm_form(g) == T.D | T.TALL | T.LEAN


def test_float32_direct_path_keeps_its_routes(lib):
    """the register-direct path takes float32 products with K % 4 == 0 (the upper half of the last fragment is masked in the kernel, not
    routed away); bf16 needs K % 8 == 0; one element off the alignment sends either to the staged body"""
    for dt, es in ((L.F32, 4), (L.BF16, 2)):
        for K in (4, 8, 12, 16, 36, 40):
            g = _args(G.operand(4096, 48, 1), G.operand(8192, 48, 1), 16384, 70, 70, K, dtype=dt, ldc_m=72)
            want = T.D | T.LEAN if K % (16 // es) == 0 else 0
            assert lib.jen1_train_gemm_form(g) == want, (dt, K)
            g.a.p = 4096 + es
            assert lib.jen1_train_gemm_form(g) == 0


def test_recorded_launches_keep_their_forms(lib, golden_dir):
    """every jen1_train_gemm launch of the committed record of the training pass (tests/golden/train_record.json, the shapes bench.py
    times among them) by the form jen1_train_gemm_form gives it: the counts below were taken when the query was added, with the launch
    decision moved into it unchanged"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_record", os.path.join(ROOT, "tools", "train_record.py"))
    tr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tr)
    rec = tr.load_fixture(os.path.join(golden_dir, "train_record.json"))
    ptr = lambda v, i: None if v == "null" else (i + 1) << 20

    def operand_of(f, i):
        o = L.GemmOperand()
        for (name, _), v in zip(L.GemmOperand._fields_, f):
            setattr(o, name, ptr(v, i) if name == "p" else v)
        return o

    def args_of(f):
        g = L.GemmArgs()
        for i, ((name, _), v) in enumerate(zip(L.GemmArgs._fields_, f)):
            setattr(g, name, operand_of(v, i) if name in ("a", "b") else ptr(v, i) if isinstance(v, str) else v)
        return g

    count = Counter()
    for case in rec.values():
        for name, args in case["launches"]:
            blocks = [args[0]] if name == "jen1_train_gemm" else args[:2] if name == "jen1_train_gemm_pair" else []
            for f in blocks:
                form = lib.jen1_train_gemm_form(args_of(f))
                assert form >= 0, (f, lib.jen1_last_error())
                count[("f32" if f[20] == L.F32 else "bf16", T.form_name(form))] += 1
    assert dict(count) == RECORDED_FORMS, dict(count)


RECORDED_FORMS = {("bf16", "fastw"): 305, ("bf16", "direct+lean"): 29, ("bf16", "direct+tall+lean"): 6, ("bf16", "direct+skinny+4waves"): 401,
                  ("bf16", "staged"): 29, ("f32", "direct+lean"): 4, ("f32", "staged"): 184, ("f32", "direct+skinny+4waves"): 308}
