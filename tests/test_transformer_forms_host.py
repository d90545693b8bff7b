"""The inference transformer's fused forms on the host, in float64 (jen1_amd/packing.py: pqkv_matrix, o1q2_matrix, s1q2_matrix,
o2f1_matrix; references and inputs: tests/transformer_forms_common.py).

Composition: the unfused sub-block -- conv1d projection, LayerNorm, Linear, attention, to_out, residual, the first FeedForward layer,
step by step as reference blocks.py:427-446, :483-489, :528-537 writes them -- equals each composed matrix evaluated as a dual-range
GEMM with the LayerNorm finish applied afterwards, to 1e-12 (the figure of tests/test_fold_up_cpu.py).

Power of the check: on the inputs of tests/test_gpu_transformer_forms.py every deliberately wrong variant is at least 10 times the
GPU test's tolerance away from the right answer, in both launch dtypes.
"""
import pytest
import torch
import torch.nn.functional as F

import transformer_forms_common as TC
from jen1_amd import lib as L
from jen1_amd.packing import o1q2_matrix, o2f1_matrix, pqkv_matrix, s1q2_matrix

EXACT = 1e-12
C_, H_, D_, FF, NCTX, CTXF = 64, 4, 8, 128, 5, 48
MID = H_ * D_
DIMS = dict(C=C_, H=H_, d=D_, FF=FF, ctxf=CTXF)


def params(seed=3):
    return TC.block_params(seed=seed, **DIMS)


def unfused(p, x, ctx, causal):
    return TC.block_unfused(p, x, ctx, causal, H_, D_)


folded = TC.block_folded


def inputs(B, Ln, seed=5):
    g = torch.Generator().manual_seed(seed + Ln)
    x = torch.randn(B, C_, Ln, generator=g, dtype=torch.float64) * 1.4 + 0.3
    return x, torch.randn(B, NCTX, CTXF, generator=g, dtype=torch.float64)


def close(a, b):
    e = TC.rel(a, b)
    assert e <= EXACT, e


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Ln", [1, 6])
def test_composed_forms_equal_the_unfused_sub_block(Ln, causal):
    p = params()
    x, ctx = inputs(2, Ln)
    want = unfused(p, x, ctx, causal)
    wqkv, bqkv, wq2, bq2 = folded(p)
    zc = torch.zeros(C_, dtype=torch.float64)
    # pqkv: [x1 | qkv_raw] over GN(x); the finish of q, k and v is the self-attention launch's
    xh = TC.norm_apply_ref(x.permute(0, 2, 1), mode=L.PRO_GN, groups=32, gamma=p["gn.g"], beta=p["gn.b"], eps=1e-6)
    close(xh, want["xh"])
    wm, bm = pqkv_matrix(p["P"][:, :, None], p["pb"], wqkv)
    assert wm.shape == (C_ + 3 * MID, C_) and wm.dtype == torch.float64
    y1, st1 = TC.dual_range_ref([xh], wm, bm, None, C_, C_ // 32, L.ACT_NONE, None)
    close(y1[..., :C_], want["x1"])
    close(st1, TC.row_sums(want["x1"]))
    fin1 = (st1, torch.cat([zc, wqkv.sum(1)]), torch.cat([zc, bqkv]), C_, 1e-5, 1, 1)
    close(TC.ln_finish(y1[..., C_:], st1, fin1[1][C_:], fin1[2][C_:], C_, 1e-5), torch.cat([want["q"], want["k"], want["v"]], -1))
    a1 = TC.attention_ref(y1, y1, q_off=C_, k_off=C_ + MID, v_off=C_ + 2 * MID, H=H_, d=D_, Nk=Ln, causal=causal, fin=fin1)
    close(a1, want["a1"])
    # o1q2: [x2 | q2_raw] over [a1 | x1]; the finish of q2 is the cross-attention launch's, K and V come finished from the context
    wm, bm = o1q2_matrix(p["wo"], p["bo"], wq2)
    assert wm.shape == (C_ + MID, MID + C_) and not wm[:C_, MID:].any()
    y2, st2 = TC.dual_range_ref([a1, y1[..., :C_]], wm, bm, y1[..., :C_], C_, MID // 32, L.ACT_NONE, None)
    close(y2[..., :C_], want["x2"])
    close(st2, TC.row_sums(want["x2"]))
    fin2 = (st2, torch.cat([zc, wq2.sum(1)]), torch.cat([zc, bq2]), C_, 1e-5, 1, 0)
    close(TC.ln_finish(y2[..., C_:], st2, fin2[1][C_:], fin2[2][C_:], C_, 1e-5), want["q2"])
    a2 = TC.attention_ref(y2, want["kv2"], q_off=C_, k_off=0, v_off=MID, H=H_, d=D_, Nk=NCTX, fin=fin2)
    close(a2, want["a2"])
    # o2f1: [x3 | gelu(f)] over [a2 | x2]
    wm, bm = o2f1_matrix(p["wo2"], p["bo2"], p["w1"], p["b1"])
    assert wm.shape == (C_ + FF, MID + C_) and not wm[:C_, MID:].any()
    y3, _ = TC.dual_range_ref([a2, y2[..., :C_]], wm, bm, y2[..., :C_], C_, MID // 32, L.ACT_GELU, None)
    close(y3[..., :C_], want["x3"])
    close(y3[..., C_:], want["f"])


@pytest.mark.parametrize("causal", [False, True])
def test_single_position_fold_equals_the_general_block(causal):
    """s1q2: softmax over one key is 1 and LayerNorm over the channels of one position is a one-group GroupNorm, so at L = 1 the
    self-attention sub-block is one dual-range GEMM over [LN_ctx(x1) | x1] with no attention at all"""
    p = params(4)
    x, ctx = inputs(3, 1)
    want = unfused(p, x, ctx, causal)
    _, _, wq2, bq2 = folded(p)
    x1 = want["x1"]
    _, bm = o1q2_matrix(p["wo"], p["bo"], wq2)
    wm = s1q2_matrix(p["wo"], p["wkv"][MID:], wq2)
    assert wm.shape == (C_ + MID, 2 * C_) and not wm[:C_, C_:].any()
    nc = TC.norm_apply_ref(x1, mode=L.PRO_GN, groups=1, gamma=p["nctx.g"], beta=p["nctx.b"], eps=1e-5)
    close(nc, F.layer_norm(x1, (C_,), p["nctx.g"], p["nctx.b"], 1e-5))
    y, st = TC.dual_range_ref([nc, x1], wm, bm, x1, C_, C_ // 32, L.ACT_NONE, None)
    close(y[..., :C_], want["x2"])
    close(TC.ln_finish(y[..., C_:], st, wq2.sum(1), bq2, C_, 1e-5), want["q2"])


def test_references_against_torch():
    """the references themselves against torch's own operators (float64)"""
    g = torch.Generator().manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B, N, H, d = 2, 7, 4, 8
    t = r(B, N, 3 * H * d)
    for causal in (False, True):
        got = TC.attention_ref(t, t, q_off=0, k_off=H * d, v_off=2 * H * d, H=H, d=d, Nk=N, causal=causal)
        qh, kh, vh = (z.reshape(B, N, H, d).transpose(1, 2) for z in t.split(H * d, -1))
        want = F.scaled_dot_product_attention(qh, kh, vh, is_causal=causal).transpose(1, 2).reshape(B, N, H * d)
        assert TC.rel(got, want) <= EXACT
    x, w, b, res = r(2, 5, 96), r(64, 96), r(64), r(2, 5, 32)
    y, st = TC.dual_range_ref([x[..., :32], x[..., 32:]], w, b, res, 32, 1, L.ACT_GELU, None)
    assert TC.rel(y[..., :32], F.linear(x[..., :32], w[:32, :32], b[:32]) + res) <= EXACT
    assert TC.rel(y[..., 32:], F.gelu(F.linear(x, w[32:], b[32:]))) <= EXACT
    assert TC.rel(st, TC.row_sums(y, 32)) <= EXACT
    assert TC.rel(TC.gelu(x), F.gelu(x)) <= EXACT
    gam, bet = r(96) + 1.5, r(96)
    for groups in (1, 3, 32):
        want = F.group_norm(x.permute(0, 2, 1), groups, gam, bet, 1e-6).permute(0, 2, 1)
        assert TC.rel(TC.norm_apply_ref(x, mode=L.PRO_GN, groups=groups, gamma=gam, beta=bet, eps=1e-6), want) <= EXACT
        two = TC.norm_apply_ref(x[..., :64], x[..., 64:] * 2.0, mode=L.PRO_GN_SILU, src1_scale=0.5, groups=groups, gamma=gam, beta=bet, eps=1e-6)
        assert TC.rel(two, F.silu(want)) <= EXACT
    # fine-group sums add up to GroupNorm's statistics
    fg = TC.fine_group_sums(x[..., :64])
    assert TC.rel(fg[:, :, 0].sum(1), x[..., :64].sum((1, 2))) <= EXACT


def test_case_list_covers_what_the_kernel_branches_on():
    assert TC.splitk_ok(3, 2) and TC.splitk_ok(3, 3) and not TC.splitk_ok(1, 2) and not TC.splitk_ok(4, 3) and TC.splitk_ok(6, 3)
    forms = {c[0] for c in TC.GEMM_CASES}
    assert forms == {"pqkv", "o1q2", "o2f1", "s1q2"}
    # a K slice of a split-K launch that lies wholly above k_split for the low rows (the kernel's ``any == false`` path)
    dead = [(c, sk) for c in map(lambda a: TC.gemm_case(*a), TC.GEMM_CASES) for sk in (2, 3)
            if TC.splitk_ok(c["G"], sk) and (sk - 1) * -(-c["G"] // sk) >= c["k_split"]]
    assert dead, "no split-K case with a K slice wholly above k_split"
    # every mistake of the dual-range list can show in some form (each form shows the ones it has the operands for)
    shown = {k for a in TC.GEMM_CASES for k in TC.gemm_wrong_kinds(TC.gemm_case(*a))}
    assert shown == set(TC.DUAL_RANGE_WRONG)
    # chunks below the four waves of a workgroup, and a count that is no multiple of them
    assert {TC.gemm_case(*a)["k_split"] for a in TC.GEMM_CASES if a[0] == "o1q2"} == {1, 5}
    for step in TC.XATTN_STEPS:
        assert step not in TC.xattn_case(8, 1, 2)["extra_row"].tolist()
    for step in TC.FILM_STEPS:
        assert step not in (4, 0, 2) and step < TC.FILM_ROWS


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", TC.GEMM_CASES, ids=lambda c: "-".join(map(str, c)))
def test_power_dual_range(case, mode):
    c = TC.gemm_case(*case)
    y, st = TC.gemm_ref(c, mode)
    m = c["m_split"]
    assert torch.isfinite(y).all() and y.shape == (c["B"], c["L"], c["M"])
    for kind in TC.gemm_wrong_kinds(c):
        yw, sw = TC.gemm_wrong(c, mode, kind)
        if kind == "stats_all_columns":
            gap, need = TC.rel(sw, st), TC.POWER * TC.STAT_TOL[mode]
        elif kind == "residual_high_rows":
            gap, need = TC.rel(yw[..., m:], y[..., m:]), TC.POWER * TC.TOL[mode]
        else:
            gap, need = TC.rel(yw[..., :m], y[..., :m]), TC.POWER * TC.TOL[mode]
        assert gap >= need, (kind, gap, need)
        # ... and the mistake touches nothing else
        if kind in ("gelu_low_rows", "k_split_ignored"):
            assert torch.equal(yw[..., m:], y[..., m:])
        if kind == "residual_high_rows":
            assert torch.equal(yw[..., :m], y[..., :m]) and torch.equal(sw, st)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case", TC.XATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_power_cross_attention(case, mode):
    c = TC.xattn_case(*case)
    live = c["extra_row"] >= 0
    assert live.any() and not live.all() and c["kv_row"].tolist() != list(range(c["B"]))
    outs = [TC.xattn_ref(c, mode, s) for s in TC.XATTN_STEPS]
    need = TC.POWER * TC.TOL[mode]
    # the two values of the scalar give different outputs where the row is live, the same where it is not
    assert TC.rel(outs[1][live], outs[0][live]) >= need
    assert torch.equal(outs[0][~live], outs[1][~live])
    for s, y in zip(TC.XATTN_STEPS, outs):
        assert TC.rel(TC.xattn_ref(c, mode, s, wrong="extra_row_as_row")[live], y[live]) >= need
        assert TC.rel(TC.xattn_ref(c, mode, s, wrong="finish_kv"), y) >= need


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_power_film_step(mode):
    need = TC.POWER * TC.TOL[mode]
    cases = [(TC.norm_case(n, **kw), TC.norm_ref) for n, kw in TC.NORM_CASES.items() if kw.get("film") == "step"]
    cases += [(TC.film_conv_case(*a), TC.film_conv_ref) for a in TC.FILM_CONV_CASES]
    assert len(cases) >= 6
    for c, ref in cases:
        outs = [ref(c, mode, s) for s in TC.FILM_STEPS]
        assert TC.rel(outs[1], outs[0]) >= need, c["name"]
        for s, y in zip(TC.FILM_STEPS, outs):
            gap = TC.rel(ref(c, mode, s, wrong="film_row"), y)
            assert gap >= need, (c["name"], s, gap)


def test_one_value_per_group_is_the_ill_conditioned_pqkv_case():
    """pqkv with Cc = 32 at B = L = 1: every one of the 32 groups holds ONE value, so the variance is 0, rstd = eps^-1/2 = 1000 and the
    exact result is beta.  The prologue's formula x A + (beta - mean A) evaluated in float32 then carries 2^-24 |x| 1000 gamma into the
    GEMM: a few 1e-5 of the largest output, still inside the float32 gate, where every other shape of the list is at 1e-7"""
    def float32_form(case):
        c = TC.gemm_case(*case)
        groups, gamma, beta, eps = c["gn"]
        x = TC.rounded(c["src"], "f32")
        xg = x.reshape(c["B"], c["L"], groups, -1)
        mean = xg.mean((1, 3), keepdim=True).expand_as(xg).reshape(x.shape)
        rstd = ((xg.var((1, 3), unbiased=False, keepdim=True) + eps) ** -0.5).expand_as(xg).reshape(x.shape)
        A = rstd.float() * gamma
        xh32 = (x.float() * A + (beta - mean.float() * A)).double()
        y, _ = TC.gemm_ref(c, "f32")
        yw, _ = TC.dual_range_ref([xh32], c["W"], c["bias"], None, c["m_split"], c["k_split"], c["act"], None)
        return TC.rel(yw, y), float(rstd.max())

    e11, rstd11 = float32_form(("pqkv", 32, 32, 1, 1))
    e35, rstd35 = float32_form(("pqkv", 32, 32, 3, 5))
    assert rstd11 > 999.0 and rstd35 < 50.0
    assert 100 * e35 < e11 < TC.TOL["f32"], (e11, e35)
