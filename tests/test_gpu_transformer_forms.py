"""-m gpu: the launch forms of the inference transformer one by one, against float64 (references, inputs and tolerances:
tests/transformer_forms_common.py; tests/test_transformer_forms_host.py shows that each mistake named there would be seen here).

``OpBuilder.transformer`` issues four dual-range GEMMs (``jen1_conv_args.m_split / k_split``: pqkv, o1q2, o2f1 and the
single-position fold s1q2), finishes the LayerNorm of their high rows in ``jen1_attention_fin`` and reads FiLM rows and the time
token's K / V row from per-step tables through one device scalar.  Each form is driven here with the options ``transformer`` passes,
in both launch dtypes; the float64 reference is computed on the CPU from the operands as the kernel receives them (inputs and weights
rounded to the launch dtype), so what is left is summation order, the output rounding and, where a prologue stores a normalised tile,
that one rounding.  Every output has one guard row behind it and, where its pitch is wider than its channels, zero padding columns:
neither may change.  Gates: 1e-4 (float32) / 3e-2 (bf16) of the largest reference entry for outputs, 2e-3 / 1e-2 for the epilogue's
row statistics -- the kernel tier's own figures (tests/test_gpu_kernels.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import transformer_forms_common as TC
from helpers import BF16_TOL, F32_TOL, record_parity, rel_err
from jen1_amd import lib as L
from jen1_amd import synth
from jen1_amd.config import tiny_model_config

pytestmark = pytest.mark.gpu

GUARD = -1024.0            # exact in bf16
PAD = 32                   # padding columns behind every output's channels


@pytest.fixture(scope="module", params=["f32", "bf16"])
def ctx(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.engine import KernelCtx
    return KernelCtx(request.param, "cuda", target_wgs=256), request.param


def dev(t, dtype=None):
    return None if t is None else t.to(device="cuda", dtype=dtype or t.dtype).contiguous()


def stats32(t64):
    return dev(t64.float().reshape(-1))


def act(x, kc, mode, ld=None, gn=False, rs_C=None):
    """float32 CPU [B][L][C] -> Act in the launch dtype (pitch ld >= C, zero padding) with the statistics a producer's epilogue would have
    left for it: fine-group sums (gn) and row sums over the first rs_C channels"""
    from jen1_amd.engine import Act
    B, Ln, Cx = x.shape
    ld = ld or Cx
    t = torch.zeros((B, Ln, ld), dtype=kc.tdtype, device="cuda")
    t[:, :, :Cx] = dev(x, kc.tdtype)
    xr = TC.rounded(x, mode)
    return Act(t, B, Ln, Cx, ld, stats32(TC.fine_group_sums(xr)) if gn else None, stats32(TC.row_sums(xr, rs_C)) if rs_C else None, cp=Cx)


def guarded(kc, B, Ln, Cx, rs=False, pad=PAD):
    """an output Act of Cx channels at pitch Cx + pad, zeroed, with one guard row of GUARD behind it (and behind its row statistics)"""
    from jen1_amd.engine import Act
    ld = Cx + pad
    buf = torch.zeros((B * Ln + 1) * ld, dtype=kc.tdtype, device="cuda")
    buf[B * Ln * ld:] = GUARD
    rsb = None
    if rs:
        rsb = torch.zeros(B * Ln * 2 + 2, device="cuda")
        rsb[B * Ln * 2:] = GUARD
    a = Act(buf[: B * Ln * ld].view(B, Ln, ld), B, Ln, Cx, ld, None, None if rsb is None else rsb[: B * Ln * 2], cp=Cx)
    return a, buf, rsb


def check_guards(a, buf, rsb, what):
    n = a.B * a.L * a.ld
    assert bool((buf[n:] == GUARD).all()), f"{what}: the guard row behind the output changed"
    assert a.ld == a.C or float(a.t[:, :, a.C:].float().abs().max()) == 0.0, f"{what}: padding columns of the output changed"
    if rsb is not None:
        assert bool((rsb[a.B * a.L * 2:] == GUARD).all()), f"{what}: the guard behind the row statistics changed"


def run(ob):
    ob.finalize_workspace()
    ob.run()
    torch.cuda.synchronize()


def packed(W, kc):
    from jen1_amd.packing import pack_gemm_weight
    return pack_gemm_weight(dev(W)[None], kc.tdtype).flatten(0, 1).contiguous()


# ------------------------------------------------------------------ (a) the dual-range GEMM forms
def add_gemm(ob, kc, mode, c, out, force):
    """the launch of form c["form"] with the options OpBuilder.transformer passes (the builder keeps its operands alive)"""
    form, Cc, mid = c["form"], c["Cc"], c["mid"]
    w, bias = packed(c["W"], kc), dev(c["bias"])
    split = dict(m_split=Cc, k_split=c["k_split"], force=force)
    if form == "pqkv":
        groups, gamma, beta, eps = c["gn"]
        src = act(c["src"], kc, mode, gn=True)
        r = ob.conv(ob.ops, src0=src, w=w, bias=bias, out=out, pro=L.PRO_GN, gn=(groups, Cc, dev(gamma), dev(beta), eps), flat_w=True, **split)
    elif form == "s1q2":
        groups, gamma, beta, eps = c["gn"]
        x1 = act(c["wide"], kc, mode).cols(0, Cc)
        x1.gn = stats32(TC.fine_group_sums(TC.rounded(c["src"], mode)))
        r = ob.conv(ob.ops, src0=x1, w=w, bias=bias, out=out, pro=L.PRO_GN, gn=(groups, Cc, dev(gamma), dev(beta), eps), residual=x1,
                    extra_segs=[(x1, 0)], flat_w=True, **split)
    else:
        x1 = act(c["wide"], kc, mode).cols(0, Cc)
        r = ob.conv(ob.ops, src0=act(c["src"], kc, mode), w=w, bias=bias, out=out, residual=x1, extra_segs=[(x1, 0)], act=c["act"], **split)
    assert r is out


def forces(G):
    for cfg in (None, L.CFG_S16x16, L.CFG_S16x32, L.CFG_S16x64):
        for sk in (1, 2, 3):
            if TC.splitk_ok(G, sk):
                yield {k: v for k, v in (("cfg", cfg), ("splitk", sk)) if v is not None and (k == "cfg" or sk > 1)}


@pytest.mark.parametrize("case", TC.GEMM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_dual_range_gemm(ctx, case):
    """pqkv / o1q2 / o2f1 / s1q2 on the streaming kernel: automatic and forced S16 tiles, split-K 1 .. 3 wherever no K slice is empty
    (o1q2 / o2f1 with k_split = 1 and split-K 2: the second slice lies wholly above k_split for the low rows).

    Measured on MI355X: float32 <= 4e-7 everywhere except pqkv with Cc = 32 at B = L = 1 (5.4e-5 low, 6.9e-5 high rows), bf16 <= 4.3e-3;
    row statistics <= 2e-7 / 2.5e-3.  The exception is the prologue's, not the GEMM's: 32 groups over 32 channels at one position leave
    ONE value per group, the variance is 0 and rstd = eps^-1/2 = 1000, so a float32 evaluation of x A + (beta - mean A) carries
    2^-24 |x| 1000 gamma where the exact result is beta; the same formula evaluated in float32 on the CPU gives 7.4e-5 / 8.2e-5 for
    this case and 6e-8 for (B, L) = (3, 5).  No JEN-1 shape has one value per group."""
    from jen1_amd.engine import OpBuilder
    kc, mode = ctx
    c = TC.gemm_case(*case)
    B, Ln, M, m = c["B"], c["L"], c["M"], c["m_split"]
    y_ref, _ = TC.gemm_ref(c, mode)
    worst = dict(low=0.0, high=0.0, stats=0.0)
    n = 0
    for force in forces(c["G"]):
        ob = OpBuilder(kc)
        out, buf, rsb = guarded(kc, B, Ln, M, rs=c["rs"])
        add_gemm(ob, kc, mode, c, out, force or None)
        convs = [op for op in ob.ops if op.kind == "conv_gemm"]
        assert len(convs) == 1 and "direct=1" in convs[0].label and f"sk={force.get('splitk', 1)} " in convs[0].label, convs[0].label
        assert ("norm_apply" in [op.kind for op in ob.ops]) == (c["gn"] is not None)
        run(ob)
        what = f"{case} {force}"
        check_guards(out, buf, rsb, what)
        if force.get("splitk", 1) > 1:
            assert int(ob.counters.abs().sum().item()) == 0, f"{what}: split-K counters must be left at zero"
        y = out.t[:, :, :M].double().cpu()
        e_lo, e_hi = TC.rel(y[..., :m], y_ref[..., :m]), TC.rel(y[..., m:], y_ref[..., m:])
        # the statistics against float64 sums over the first m_split columns of the stored output
        e_st = TC.rel(out.rs.double().cpu().reshape(B, Ln, 2), TC.row_sums(y, m)) if c["rs"] else 0.0
        print(f"{what} [{mode}]: low rows {e_lo:.3e}, high rows {e_hi:.3e}, row statistics {e_st:.3e}")
        worst = dict(low=max(worst["low"], e_lo), high=max(worst["high"], e_hi), stats=max(worst["stats"], e_st))
        assert e_lo < TC.TOL[mode] and e_hi < TC.TOL[mode], (what, e_lo, e_hi)
        assert e_st < TC.STAT_TOL[mode], (what, e_st)
        n += 1
    assert n >= 4
    if not c["rs"]:
        del worst["stats"]
    record_parity("transformer_forms." + c["form"], "-".join(map(str, case[1:])), mode, **worst)


@pytest.mark.parametrize("mid,H,d", [(32, 4, 8), (160, 5, 32)])
def test_single_position_fold_equals_the_three_launch_route(ctx, mid, H, d):
    """JEN1_FOLD_N1 at kernel level (the tiny configuration never has T' = 1 with Cc % 256 == 0): at L = 1 the two launches proj, s1q2
    give the [x2 | q2_raw] that pqkv, self-attention over one key, o1q2 give on the same data, and both are the unfused sub-block's"""
    from jen1_amd.engine import Act, OpBuilder
    from jen1_amd.packing import conv_weight_to_gemm, o1q2_matrix, pack_gemm_weight, pqkv_matrix, s1q2_matrix
    kc, mode = ctx
    Cc, B = 256, 3
    p = TC.block_params(C=Cc, H=H, d=d, FF=Cc, ctxf=32, seed=mid)
    g = torch.Generator().manual_seed(mid)
    x = torch.randn(B, 1, Cc, generator=g) * 1.4 + 0.3
    xr = TC.rounded(x, mode)
    want = TC.block_unfused(p, xr.permute(0, 2, 1), torch.zeros(B, 2, 32, dtype=torch.float64), False, H, d)
    wqkv, bqkv, wq2, bq2 = TC.block_folded(p)
    f32 = lambda t: dev(t.float())
    rowsum = lambda w: f32(w.to(kc.tdtype).double().sum(1))
    zc = torch.zeros(Cc, device="cuda")
    gn_in = (32, Cc, f32(p["gn.g"]), f32(p["gn.b"]), 1e-6)
    wm2, bm2 = o1q2_matrix(p["wo"], p["bo"], wq2)
    fin_u, fin_b = torch.cat([zc, rowsum(wq2)]), torch.cat([zc, f32(bq2)])
    outs = {}
    # the three-launch route
    ob = OpBuilder(kc)
    xq1, buf1, rsb1 = guarded(kc, B, 1, Cc + 3 * mid, rs=True)
    wm, bm = pqkv_matrix(p["P"], p["pb"], wqkv)
    ob.conv(ob.ops, src0=act(x, kc, mode, gn=True), w=packed(wm.float(), kc), bias=f32(bm), out=xq1, pro=L.PRO_GN, gn=gn_in,
            m_split=Cc, k_split=Cc // 32, flat_w=True)
    a1, bufa, _ = guarded(kc, B, 1, mid)
    ob.attention(ob.ops, q=xq1, q_off=Cc, kv_t=xq1.t, ldkv=xq1.ld, k_off=Cc + mid, v_off=Cc + 2 * mid, out=a1, H=H, d=d, Nk=1, causal=False,
                 fin=(xq1.rs, torch.cat([zc, rowsum(wqkv)]), torch.cat([zc, f32(bqkv)]), Cc, 1e-5, 1, 1))
    x1 = xq1.cols(0, Cc)
    xq2, buf2, rsb2 = guarded(kc, B, 1, Cc + mid, rs=True)
    ob.conv(ob.ops, src0=Act(a1.t, B, 1, mid, a1.ld, cp=mid), w=packed(wm2.float(), kc), bias=f32(bm2), out=xq2, residual=x1,
            extra_segs=[(x1, 0)], m_split=Cc, k_split=mid // 32)
    run(ob)
    for a, b_, r_ in ((xq1, buf1, rsb1), (a1, bufa, None), (xq2, buf2, rsb2)):
        check_guards(a, b_, r_, "three launches")
    outs["three"] = (xq2.t[:, :, : Cc + mid].double().cpu(), xq2.rs.double().cpu().reshape(B, 1, 2))
    # the fold: proj (with the fine-group sums of x1 in its epilogue), then s1q2 with norm_context as a one-group GroupNorm
    ob = OpBuilder(kc)
    x1f, bufx, _ = guarded(kc, B, 1, Cc, pad=0)             # (fine-group sums need a pitch of 32 whole groups)
    x1f = Act(x1f.t, B, 1, Cc, x1f.ld, torch.zeros(B * 64, device="cuda"), None, cp=Cc)
    ob.conv(ob.ops, src0=act(x, kc, mode, gn=True), w=pack_gemm_weight(conv_weight_to_gemm(dev(p["P"].float())[:, :, None]), kc.tdtype),
            bias=f32(p["pb"]), out=x1f, pro=L.PRO_GN, gn=gn_in)
    xq2f, buf3, rsb3 = guarded(kc, B, 1, Cc + mid, rs=True)
    ob.conv(ob.ops, src0=x1f, w=packed(s1q2_matrix(p["wo"], p["wkv"][mid:], wq2).float(), kc), bias=f32(bm2), out=xq2f, pro=L.PRO_GN,
            gn=(1, Cc, f32(p["nctx.g"]), f32(p["nctx.b"]), 1e-5), residual=x1f, extra_segs=[(x1f, 0)], m_split=Cc, k_split=Cc // 32, flat_w=True)
    assert [op.kind for op in ob.ops].count("conv_gemm") == 2
    run(ob)
    check_guards(x1f, bufx, None, "fold: proj")
    check_guards(xq2f, buf3, rsb3, "fold: s1q2")
    outs["fold"] = (xq2f.t[:, :, : Cc + mid].double().cpu(), xq2f.rs.double().cpu().reshape(B, 1, 2))
    # the unfused block: x2, and q2 through the finish
    errs = {}
    for name, (y, st) in outs.items():
        q2 = TC.ln_finish(y[..., Cc:], st, fin_u.double().cpu()[Cc:], fin_b.double().cpu()[Cc:], Cc, 1e-5)
        errs[name + "_x2"], errs[name + "_q2"] = TC.rel(y[..., :Cc], want["x2"]), TC.rel(q2, want["q2"])
    errs["routes_x2"] = TC.rel(outs["fold"][0][..., :Cc], outs["three"][0][..., :Cc])
    errs["routes_q2raw"] = TC.rel(outs["fold"][0][..., Cc:], outs["three"][0][..., Cc:])
    errs["routes_stats"] = TC.rel(outs["fold"][1], outs["three"][1])
    print(f"mid={mid} [{mode}]: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    record_parity("transformer_forms.fold_n1", f"mid{mid}", mode, **errs)
    for k, v in errs.items():
        assert v < (TC.STAT_TOL if k.endswith("stats") else TC.TOL)[mode], (k, v)


# ------------------------------------------------------------------ (b) the cross-attention form of jen1_attention_fin
@pytest.mark.parametrize("case", TC.XATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_cross_attention_form(ctx, case):
    """finish on Q only, K / V through a kv_row map that is not the identity, the last key of the batch elements with extra_row >= 0 from
    row extra_step of the per-step table; the same built launch again after the scalar changed on the device"""
    from jen1_amd.engine import OpBuilder
    kc, mode = ctx
    c = TC.xattn_case(*case)
    B, Nq, Nk, Cc, mid = c["B"], c["Nq"], c["Nk"], c["Cc"], c["mid"]
    q = act(c["q"], kc, mode, rs_C=Cc)
    kv, ext = dev(c["kv"], kc.tdtype), dev(c["kv_extra"], kc.tdtype)
    step = torch.tensor([TC.XATTN_STEPS[0]], dtype=torch.int32, device="cuda")
    out, buf, _ = guarded(kc, B, Nq, mid)
    ob = OpBuilder(kc)
    ob.attention(ob.ops, q=q, q_off=Cc, kv_t=kv, ldkv=2 * mid, k_off=0, v_off=mid, out=out, H=c["H"], d=c["d"], Nk=Nk, causal=False,
                 kv_row=dev(c["kv_row"]), kv_extra=ext, extra_row=dev(c["extra_row"]), ld_extra=c["ld_extra"], kx_off=c["kx_off"],
                 vx_off=c["vx_off"], extra_step=step, fin=(q.rs, dev(c["u"]), dev(c["b"]), Cc, 1e-5, 1, 0))
    ys, errs = [], []
    for s in TC.XATTN_STEPS:
        step.fill_(s)
        run(ob)
        check_guards(out, buf, None, f"{case} step {s}")
        ys.append(out.t[:, :, :mid].clone())
        errs.append(TC.rel(ys[-1].double().cpu(), TC.xattn_ref(c, mode, s)))
    print(f"{case} [{mode}]: " + ", ".join(f"step {s}: {e:.3e}" for s, e in zip(TC.XATTN_STEPS, errs)))
    record_parity("transformer_forms.xattn", "-".join(map(str, case)), mode, out=max(errs))
    assert max(errs) < TC.TOL[mode], errs
    dead = (c["extra_row"] < 0).cuda()
    assert torch.equal(ys[0][dead].view(torch.uint8), ys[1][dead].view(torch.uint8)), "a batch element without a per-step row changed with the step"
    assert not torch.equal(ys[0][~dead], ys[1][~dead])


# ------------------------------------------------------------------ (c) film_step on every path that reads FiLM
FILM_PATHS = [(None, True), ({"cfg": L.CFG_S16x32}, True),                                   # jen1_norm_apply + direct streaming
              ({"cfg": L.CFG_S16x64, "direct": False}, False), ({"cfg": L.CFG_W64x64}, False),   # the LDS-staged prologue
              ({"cfg": L.CFG_T128x16}, False)]                                              # the tile kernel


@pytest.mark.parametrize("case", TC.FILM_CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_film_step_overrides_film_row(ctx, case):
    """GroupNorm -> FiLM -> SiLU -> conv with film = (table, film_row, off, C, step): every batch element uses row step[0], whatever
    film_row says, on each kernel that reads FiLM; the same built launch again after the scalar changed on the device"""
    from jen1_amd.engine import OpBuilder
    from jen1_amd.packing import conv_weight_to_gemm, pack_gemm_weight
    kc, mode = ctx
    c = TC.film_conv_case(*case)
    B, Ln, c0, c1, Cx = c["B"], c["L"], c["c0"], c["c1"], c["C"]
    refs = {s: TC.film_conv_ref(c, mode, s) for s in TC.FILM_STEPS}
    worst = 0.0
    for force, pre_pass in FILM_PATHS:
        step = torch.tensor([TC.FILM_STEPS[0]], dtype=torch.int32, device="cuda")
        out, buf, _ = guarded(kc, B, Ln, 128)
        ob = OpBuilder(kc)
        r = ob.conv(ob.ops, src0=act(c["x0"], kc, mode, gn=True), src1=act(c["x1"], kc, mode, gn=True) if c1 else None, src1_scale=c["src1_scale"],
                    w=pack_gemm_weight(conv_weight_to_gemm(dev(c["w"])), kc.tdtype), bias=dev(c["bias"]), out=out, taps=3, pad_left=1,
                    pro=L.PRO_GN_SILU, gn=(c["groups"], Cx, dev(c["gamma"]), dev(c["beta"]), c["eps"]),
                    film=(dev(c["film"]), dev(c["film_row"]), TC.FILM_OFF, Cx, step), force=force)
        assert r is out and ("norm_apply" in [op.kind for op in ob.ops]) == pre_pass, (force, [op.label for op in ob.ops])
        for s in TC.FILM_STEPS:
            step.fill_(s)
            run(ob)
            check_guards(out, buf, None, f"{case} {force} step {s}")
            e = TC.rel(out.t[:, :, :128].double().cpu(), refs[s])
            print(f"{case} {force} step {s} [{mode}]: {e:.3e}")
            worst = max(worst, e)
            assert e < TC.TOL[mode], (force, s, e)
    record_parity("transformer_forms.film_step", "-".join(map(str, case)), mode, out=worst)


# ------------------------------------------------------------------ (d) jen1_norm_apply through the C ABI
@pytest.mark.parametrize("name", list(TC.NORM_CASES))
def test_norm_apply_modes(ctx, name):
    """GN, GN + SiLU (one and two sources, a group ending at the source boundary, groups narrower than a vector, one group), FiLM by batch
    element / film_row / film_step, LN with and without gamma / beta, a source pitch wider than its channels, L = 1 and B = 1"""
    kc, mode = ctx
    c = TC.norm_case(name, **TC.NORM_CASES[name])
    B, Ln, c0, c1, Cx = c["B"], c["L"], c["c0"], c["c1"], c["C"]
    x0 = act(c["x0"], kc, mode, ld=c["ld0"], gn=c["mode"] != L.PRO_LN, rs_C=c0 if c["mode"] == L.PRO_LN else None)
    x1 = act(c["x1"], kc, mode, ld=c1 + 8, gn=True) if c1 else None
    out, buf, _ = guarded(kc, B, Ln, Cx)
    keep = [dev(c["gamma"]), dev(c["beta"]), dev(c["film"]), dev(c["film_row"])]
    step = torch.tensor([TC.FILM_STEPS[0]], dtype=torch.int32, device="cuda")
    na = L.NormArgs()
    na.x0, na.y = x0.t.data_ptr(), out.t.data_ptr()
    na.dtype, na.mode, na.B, na.L, na.c0, na.c1, na.ld0, na.ld_y = kc.dt, c["mode"], B, Ln, c0, c1, x0.ld, out.ld
    na.gamma, na.beta = (None, None) if keep[0] is None else (keep[0].data_ptr(), keep[1].data_ptr())
    na.eps, na.src1_scale = c["eps"], c["src1_scale"]
    if x1 is not None:
        na.x1, na.ld1, na.gn_stats1 = x1.t.data_ptr(), x1.ld, x1.gn.data_ptr()
    if c["mode"] == L.PRO_LN:
        na.ln_rowstats, na.count = x0.rs.data_ptr(), c0
    else:
        G = c["groups"]
        na.gn_stats0, na.groups, na.cpg, na.count = x0.gn.data_ptr(), G, Cx // G if G > 1 else Cx, (Cx // G) * Ln
    if keep[2] is not None:
        na.film, na.film_off, na.film_C, na.film_ld = keep[2].data_ptr(), TC.FILM_OFF, Cx, keep[2].shape[-1]
        na.film_row = None if keep[3] is None else keep[3].data_ptr()
        na.film_step = step.data_ptr() if c["film_kind"] == "step" else None
    worst = 0.0
    for s in TC.FILM_STEPS if c["film_kind"] == "step" else (None,):
        if s is not None:
            step.fill_(s)
        L.check(kc.lib.jen1_norm_apply(C.byref(na), torch.cuda.current_stream().cuda_stream), "jen1_norm_apply")
        torch.cuda.synchronize()
        check_guards(out, buf, None, f"{name} step {s}")
        e = TC.rel(out.t[:, :, :Cx].double().cpu(), TC.norm_ref(c, mode, s))
        print(f"{name} step {s} [{mode}]: {e:.3e}")
        worst = max(worst, e)
        assert e < TC.TOL[mode], (name, s, e)
    record_parity("transformer_forms.norm_apply", name, mode, out=worst)


# ------------------------------------------------------------------ (e) knobs off equals knobs on, at model level
KNOBS = ("JEN1_FUSE_LN_PROJ", "JEN1_FUSE_O2_FF1", "JEN1_FUSE_FF_OUT")


def _tiny(mode):
    from jen1_amd.model import UNetCFG1d
    return UNetCFG1d(**tiny_model_config(), init_seed=1234, compute_dtype=mode, device="cuda")


def _forward(model, **kw):
    B, T = 2, 300                  # the inputs of tests/test_gpu_model.py::test_tiny_unet_all_cfg_branches_vs_golden
    x, cond = synth.latents(B, T), synth.conditioning(B, T, "text_guided")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    y = model(d(x), d(np.array([999, 499], dtype=np.int64)), embedding=d(cond["cross_attn_cond"]), embedding_mask=d(cond["cross_attn_masks"]),
              channels_list=[d(cond["input_concat_cond"])], embedding_mask_proba=0.0, **kw)
    torch.cuda.synchronize()
    return y.float().cpu().numpy()


def _conv_rows(plan, Ln):
    """M of every 1x1 launch over Ln positions, in order"""
    labels = [getattr(op, "label", "") for op in plan.ops if getattr(op, "kind", "") == "conv_gemm"]
    return [int(l.split(" M=")[1].split()[0]) for l in labels if f" Lin={Ln} " in l and " taps=1 " in l]


@pytest.fixture(scope="module")
def tiny_default():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return {m: _tiny(m) for m in ("f32", "bf16")}


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_knob_off_equals_knob_on(tiny_default, monkeypatch, mode, knob):
    """a tiny-configuration engine built with one fusion knob set to 0 computes what the default engine computes (the knobs-off
    engine is the reference), and the launch list shows that the default plan holds the fused forms and the other one does not"""
    on = tiny_default[mode]
    monkeypatch.setenv(knob, "0")
    off = _tiny(mode)
    assert getattr(off.engine(), {"JEN1_FUSE_LN_PROJ": "fuse_ln_proj", "JEN1_FUSE_O2_FF1": "fuse_o2_ff1", "JEN1_FUSE_FF_OUT": "fuse_ff_out"}[knob]) is False
    monkeypatch.delenv(knob)
    tol = F32_TOL if mode == "f32" else BF16_TOL
    worst = 0.0
    for kw in (dict(embedding_scale=1.0, causal=False), dict(embedding_scale=1.0, causal=True),
               dict(embedding_scale=0.8, batch_cfg=True, scale_cfg=True, causal=False)):
        e = rel_err(_forward(on, **kw), _forward(off, **kw))
        print(f"{knob}=0 against the default [{mode}] {kw}: {e:.3e}")
        worst = max(worst, e)
        assert e < tol, (kw, e)
    record_parity("transformer_forms.knobs", knob, mode, out=worst)
    # the transformers of the tiny configuration (Cc = 128, mid = 128, FeedForward 128) run over 150 positions; without the CFG pair
    # those 300 rows stream, so the default plan holds per transformer one launch of Cc + 3 mid rows (pqkv) and two of Cc + mid = Cc + F
    # rows (o1q2, o2f1)
    t = on.spec.transformers()[0]
    Cc, mid, n_tr = t.channels, t.heads * t.head_features, len(on.spec.transformers())
    assert Cc * t.multiplier == mid
    Ln = on.spec.level_lengths(300)[-1]
    for causal in (False, True):
        p_on, p_off = on.engine().plan(2, 300, 1, causal), off.engine().plan(2, 300, 1, causal)
        m_on, m_off = _conv_rows(p_on, Ln), _conv_rows(p_off, Ln)
        assert m_on.count(Cc + 3 * mid) == n_tr and m_on.count(Cc + mid) == 2 * n_tr and m_on.count(3 * mid) == 0, m_on
        if knob == "JEN1_FUSE_LN_PROJ":
            assert m_off.count(Cc + 3 * mid) == 0 and m_off.count(3 * mid) == n_tr and m_off.count(Cc + mid) == n_tr, m_off
            assert len(m_off) == len(m_on) + 2 * n_tr
        else:
            assert m_off.count(Cc + 3 * mid) == n_tr and m_off.count(Cc + mid) == n_tr, m_off
            assert len(m_off) == len(m_on) + (1 if knob == "JEN1_FUSE_O2_FF1" else 2) * n_tr
