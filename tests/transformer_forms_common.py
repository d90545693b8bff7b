"""Float64 references of the inference transformer's fused launch forms, the inputs the GPU tests drive them with and the tolerances
they compare with; importable without a GPU (tests/test_transformer_forms_host.py pins the references and the inputs).

``OpBuilder.transformer`` (jen1_amd/engine.py) runs its projections as dual-range GEMMs (``jen1_conv_args.m_split / k_split``,
include/jen1_hip.h): output rows below ``m_split`` sum only the first ``k_split`` 32-channel chunks of K, take the residual and feed
``out_rowstats``; rows at or above it sum all of K and take ``act``.  The LayerNorm of the projection in the high rows is finished by
the attention launch (``jen1_attention_fin``), FiLM rows and the time token's K / V row are read from per-step tables through one
device scalar (``film_step`` / ``extra_step``).

Every reference here is written the way the model writes the operation (reference blocks.py:355-380, :427-446, :483-489, :528-537),
on channel-last tensors, in float64.  The ``*_wrong`` functions are deliberately wrong variants of the same operations: the host
tests require that on the GPU tests' inputs each of them is at least ``POWER`` times the GPU tolerance away from the right answer, so
a kernel that made that mistake could not pass.
"""
import zlib

import torch
import torch.nn.functional as F

from jen1_amd import lib as L
from jen1_amd.packing import fold_layernorm

TOL = {"f32": 1e-4, "bf16": 3e-2}            # outputs: the kernel tier's figures (tests/test_gpu_kernels.py TOL)
STAT_TOL = {"f32": 2e-3, "bf16": 1e-2}       # epilogue statistics (test_gpu_kernels.py::test_extra_k_segments_fused_shortcut)
POWER = 10.0
TDTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}


def rounded(t, mode):
    """``t`` as a launch in ``mode`` receives it (rounded to the launch dtype), in float64"""
    return None if t is None else t.to(TDTYPE[mode]).double()


def rel(a, b) -> float:
    """max-abs(a - b) / max-abs(b) (helpers.rel_err on tensors)"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * 2 ** -0.5))


def row_sums(x, C=None):
    """(sum, sumsq) over the first ``C`` channels of every row: [..., 2] float64 (the layout of ln_rowstats / out_rowstats)"""
    x = x.double()[..., :C]
    return torch.stack([x.sum(-1), (x * x).sum(-1)], -1)


def fine_group_sums(x):
    """GroupNorm statistics as a producer's epilogue leaves them: (sum, sumsq) per batch element and fine group (32 per tensor,
    C / 32 channels each) of a channel-last [B][L][C] tensor -> [B][32][2] float64"""
    B, Ln, C = x.shape
    g = x.double().reshape(B, Ln, 32, C // 32)
    return torch.stack([g.sum(dim=(1, 3)), (g * g).sum(dim=(1, 3))], -1)


# ---------------------------------------------------------------------------------------------- the dual-range GEMM
def _dual_range(x_segments, W, bias, residual, m_split, k_split, act, row_scale, *, stats_all=False, gelu_low=False, res_rows=None,
                k_all=False):
    x = torch.cat([s.double() for s in x_segments], -1)
    W = W.double()
    kl = x.shape[-1] if k_all else 32 * k_split
    lo = x[..., :kl] @ W[:m_split, :kl].T
    hi = x @ W[m_split:].T
    if bias is not None:
        lo, hi = lo + bias.double()[:m_split], hi + bias.double()[m_split:]
    if act == L.ACT_GELU:
        hi = gelu(hi)
        if gelu_low:
            lo = gelu(lo)
    if residual is not None:
        lo = lo + residual.double()[..., :m_split]
    if res_rows is not None:
        # the residual operand read for the high rows too: element [row][co] of the tensor the residual is a column window of, wherever
        # that lands (zero past its end)
        rows, ld = res_rows.shape
        flat = torch.cat([res_rows.double().reshape(-1), torch.zeros(W.shape[0], dtype=torch.float64)])
        idx = torch.arange(rows)[:, None] * ld + torch.arange(m_split, W.shape[0])[None, :]
        hi = hi + flat[idx].reshape(hi.shape)
    y = torch.cat([lo, hi], -1)
    if row_scale is not None:
        y = y * row_scale.double()[..., None]
    return y, row_sums(y, None if stats_all else m_split)


def dual_range_ref(x_segments, W, bias, residual, m_split, k_split, act, row_scale):
    """Two dependent layers as one linear map over the K concat of ``x_segments`` ([B][L][32 n] each; W [M][K]):
        y[..., :m_split] = W[:m_split, :32 k_split] x[..., :32 k_split] + bias + residual
        y[..., m_split:] = act(W[m_split:] x + bias)
    both times ``row_scale``.  Returns (y [B][L][M], row statistics [B][L][2] = (sum, sumsq) over the columns < m_split of y)."""
    return _dual_range(x_segments, W, bias, residual, m_split, k_split, act, row_scale)


DUAL_RANGE_WRONG = ("stats_all_columns", "gelu_low_rows", "residual_high_rows", "k_split_ignored")


def dual_range_wrong(kind, x_segments, W, bias, residual, m_split, k_split, act, row_scale, res_rows=None):
    """``dual_range_ref`` with one mistake.  residual_high_rows: ``res_rows`` is the [rows][ld] tensor the residual is a window of"""
    kw = {"stats_all_columns": dict(stats_all=True), "gelu_low_rows": dict(gelu_low=True), "residual_high_rows": dict(res_rows=res_rows),
          "k_split_ignored": dict(k_all=True)}[kind]
    return _dual_range(x_segments, W, bias, residual, m_split, k_split, act, row_scale, **kw)


# ---------------------------------------------------------------------------------------------- LayerNorm finish + attention
def ln_finish(raw, stats, u, b, ln_C, eps):
    """Linear(LayerNorm(x)) from raw = W' x and the row sums of x:  rstd (raw - mean u) + b  (reference blocks.py:427-429 with gamma
    folded into W' and b = W beta)"""
    mean = stats[..., 0].double() / ln_C
    rstd = (stats[..., 1].double() / ln_C - mean * mean + eps) ** -0.5
    return rstd[..., None] * (raw.double() - mean[..., None] * u.double()) + b.double()


def attention_ref(q, kv, *, q_off, k_off, v_off, H, d, Nk, causal=False, kv_row=None, kv_extra=None, extra_row=None, extra_step=None,
                  kx_off=0, vx_off=0, fin=None, wrong=None):
    """AttentionBase.forward (reference blocks.py:355-380) on the operands ``jen1_attention_fin`` takes.  q: [B][Nq][ldq], head h at
    columns q_off + h d; kv: [rows][Nk][ldkv], batch element b reads row kv_row[b] (b when None).  Where extra_row[b] >= 0 the last key
    / value row comes from kv_extra[extra_row[b]] -- from kv_extra[extra_step] when extra_step is given.  fin = (row statistics
    [B Nq][2], u, b, ln_C, eps, finish_q, finish_kv): ``ln_finish`` of Q (u, b at Q's columns) and, for self-attention, of K and V.
    wrong: "extra_row_as_row" ignores extra_step; "finish_kv" finishes K and V of the cross-attention form as well.
    Returns [B][Nq][H d] float64."""
    B, Nq, _ = q.shape
    mid = H * d
    q, kv = q.double(), kv.double()
    rows = torch.arange(B) if kv_row is None else kv_row.long()
    k, v = kv[rows][:, :, k_off: k_off + mid].clone(), kv[rows][:, :, v_off: v_off + mid].clone()
    if kv_extra is not None and extra_row is not None:
        for b in range(B):
            r = int(extra_row[b])
            if r >= 0:
                if extra_step is not None and wrong != "extra_row_as_row":
                    r = int(extra_step)
                k[b, Nk - 1] = kv_extra.double()[r, kx_off: kx_off + mid]
                v[b, Nk - 1] = kv_extra.double()[r, vx_off: vx_off + mid]
    qq = q[:, :, q_off: q_off + mid]
    if fin is not None:
        stats, u, bb, ln_C, eps, fq, fkv = fin
        stats = stats.double().reshape(-1, 2)
        if fq:
            qq = ln_finish(qq, stats.reshape(B, Nq, 2), u[q_off: q_off + mid], bb[q_off: q_off + mid], ln_C, eps)
        if fkv or wrong == "finish_kv":
            n = stats.shape[0]
            st = stats[(rows[:, None] * Nk + torch.arange(Nk)[None, :]) % n]            # the statistics of K / V's own rows
            col = lambda off: (off + torch.arange(mid)) % u.numel()
            k = ln_finish(k, st, u[col(k_off)], bb[col(k_off)], ln_C, eps)
            v = ln_finish(v, st, u[col(v_off)], bb[col(v_off)], ln_C, eps)
    heads = lambda t: t.reshape(B, -1, H, d).transpose(1, 2)
    qh, kh, vh = heads(qq), heads(k), heads(v)
    sim = torch.einsum("bhnd,bhmd->bhnm", qh, kh) * d ** -0.5
    if causal:
        keep = ~torch.ones(Nq, Nk, dtype=torch.bool).triu(Nk - Nq + 1)
        sim = sim.masked_fill(~keep, -torch.finfo(sim.dtype).max)
    out = torch.einsum("bhnm,bhmd->bhnd", sim.softmax(-1), vh)
    return out.transpose(1, 2).reshape(B, Nq, mid)


# ---------------------------------------------------------------------------------------------- jen1_norm_apply
def norm_apply_ref(x0, x1=None, *, mode, src1_scale=1.0, groups=1, gamma=None, beta=None, eps=1e-5, film=None, film_row=None,
                   film_step=None, film_off=0, wrong=None):
    """Every mode of ``jen1_norm_args`` on channel-last [B][L][c] sources: GroupNorm over the channel concat [x0, x1 * src1_scale]
    (+ FiLM x (scale + 1) + shift, + SiLU; reference blocks.py:140-144, :530, :732-734) or LayerNorm with optional gamma / beta
    (blocks.py:427).  FiLM: scale at film[row, film_off + c], shift at film[row, film_off + C + c]; row = film_step for every batch
    element when given, else film_row[b], else b.  wrong: "film_row" ignores film_step."""
    x = x0.double() if x1 is None else torch.cat([x0.double(), x1.double() * src1_scale], -1)
    B, _, C = x.shape
    g64 = None if gamma is None else gamma.double()
    b64 = None if beta is None else beta.double()
    if mode == L.PRO_LN:
        return F.layer_norm(x, (C,), g64, b64, eps)
    # nn.GroupNorm's formula (F.group_norm itself refuses a single value per channel, B = L = 1): biased variance over the
    # positions and the C / groups channels of a group
    Ln = x.shape[1]
    xg = x.reshape(B, Ln, groups, C // groups)
    mean, var = xg.mean(dim=(1, 3), keepdim=True), xg.var(dim=(1, 3), unbiased=False, keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + eps)).reshape(B, Ln, C) * g64 + b64
    if film is not None:
        if film_step is not None and wrong != "film_row":
            rows = torch.full((B,), int(film_step), dtype=torch.long)
        else:
            rows = torch.arange(B) if film_row is None else film_row.long()
        f = film.double()[rows]
        y = y * (f[:, None, film_off: film_off + C] + 1.0) + f[:, None, film_off + C: film_off + 2 * C]
    return F.silu(y) if mode == L.PRO_GN_SILU else y


# ---------------------------------------------------------------------------------------------- the unfused sub-block
def block_params(*, C, H, d, FF, ctxf, seed=3):
    """float64 parameters of one Transformer1d with one block (reference blocks.py:497-526), Linear weights N(0, 1 / fan-in)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    lin = lambda o, i: r(o, i) / i ** 0.5
    aff = lambda n: (torch.rand(n, generator=g, dtype=torch.float64) + 0.5, r(n) * 0.3)
    mid = H * d
    p = dict(P=lin(C, C), pb=r(C) * 0.2, wq=lin(mid, C), wkv=lin(2 * mid, C), wo=lin(C, mid), bo=r(C) * 0.2,
             wq2=lin(mid, C), wkv2=lin(2 * mid, ctxf), wo2=lin(C, mid), bo2=r(C) * 0.2, w1=lin(FF, C), b1=r(FF) * 0.2)
    for k, n in (("gn", C), ("norm", C), ("nctx", C), ("norm2", C), ("nctx2", ctxf)):
        p[k + ".g"], p[k + ".b"] = aff(n)
    return p


def block_unfused(p, x, ctx, causal, H, d):
    """Transformer1d.forward up to the first FeedForward layer, layer by layer (reference blocks.py:528-532, :483-487, :427-437,
    :355-380, :440-444); x: [B][C][L], ctx: [B][n][ctxf]; every intermediate channel-last, by name"""
    mid = H * d

    def attend(q, k, v, is_causal):
        B, n, m = q.shape[0], q.shape[1], k.shape[1]
        h = lambda t: t.reshape(B, -1, H, d).transpose(1, 2)
        sim = torch.einsum("bhnd,bhmd->bhnm", h(q), h(k)) * d ** -0.5
        if is_causal:
            sim = sim.masked_fill(torch.ones(n, m, dtype=torch.bool).triu(m - n + 1), -torch.finfo(sim.dtype).max)
        return torch.einsum("bhnm,bhmd->bhnd", sim.softmax(-1), h(v)).transpose(1, 2).reshape(B, n, mid)

    ln = lambda t, k: F.layer_norm(t, (t.shape[-1],), p[k + ".g"], p[k + ".b"], 1e-5)
    o = {}
    o["xh"] = F.group_norm(x, 32, p["gn.g"], p["gn.b"], 1e-6).permute(0, 2, 1)
    o["x1"] = F.conv1d(o["xh"].permute(0, 2, 1), p["P"][:, :, None], p["pb"]).permute(0, 2, 1)
    o["q"] = ln(o["x1"], "norm") @ p["wq"].T
    o["k"], o["v"] = (ln(o["x1"], "nctx") @ p["wkv"].T).chunk(2, -1)
    o["a1"] = attend(o["q"], o["k"], o["v"], causal)
    o["x2"] = o["a1"] @ p["wo"].T + p["bo"] + o["x1"]
    o["q2"] = ln(o["x2"], "norm2") @ p["wq2"].T
    o["kv2"] = ln(ctx, "nctx2") @ p["wkv2"].T
    k2, v2 = o["kv2"].chunk(2, -1)
    o["a2"] = attend(o["q2"], k2, v2, False)
    o["x3"] = o["a2"] @ p["wo2"].T + p["bo2"] + o["x2"]
    o["f"] = F.gelu(o["x3"] @ p["w1"].T + p["b1"])
    return o


def block_folded(p):
    """the LayerNorm-folded projections as ``Weights`` builds them: (Wqkv' [3 mid][C], its bias, Wq2', its bias)"""
    wq, bq = fold_layernorm(p["wq"], p["norm.g"], p["norm.b"])
    wkv, bkv = fold_layernorm(p["wkv"], p["nctx.g"], p["nctx.b"])
    wq2, bq2 = fold_layernorm(p["wq2"], p["norm2.g"], p["norm2.b"])
    return torch.cat([wq, wkv], 0), torch.cat([bq, bkv]), wq2, bq2


# ---------------------------------------------------------------------------------------------- inputs of the GPU tests
CCS, MIDS = (32, 96), (32, 160)
BLS = ((1, 1), (3, 5), (2, 19), (5, 13))
GEMM_CASES = [(form, Cc, mid, B, Ln) for form in ("pqkv", "o1q2", "o2f1") for Cc in CCS for mid in MIDS for B, Ln in BLS] + \
             [("s1q2", 256, mid, B, 1) for mid in MIDS for B in (1, 3, 5)]


def splitk_ok(G: int, splitk: int) -> bool:
    """what jen1_conv_gemm's validation accepts: no K slice may be empty"""
    return 1 <= splitk <= G and (splitk - 1) * -(-G // splitk) < G


def gemm_case(form, Cc, mid, B, Ln):
    """float32 operands of one dual-range launch as ``OpBuilder.transformer`` issues it (the weights are random, NOT a composition: the
    block that the low rows must skip is non-zero, three times the rest, so that skipping it matters):
      src     [B][L][K0]   the launch's src0 (pqkv: x, GroupNorm of 32 groups; o1q2 / o2f1: the attention output; s1q2: x1, one group)
      wide    [B][L][ldw]  the tensor whose first Cc columns are the extra K segment and the residual (o1q2: [x1 | qkv_raw], o2f1:
                           [x2 | q2_raw]; s1q2: a tensor of 2 Cc columns that starts with x1, so that a read past x1 meets data;
                           pqkv: none)
      W [M][K], bias [M], gn = (groups, gamma, beta, eps) or None, m_split, k_split (chunks), act."""
    g = _gen("gemm", form, Cc, mid, B, Ln)
    r = lambda *s: torch.randn(*s, generator=g)
    K0 = mid if form in ("o1q2", "o2f1") else Cc
    Kx = 0 if form == "pqkv" else Cc
    M = {"pqkv": Cc + 3 * mid, "o1q2": Cc + mid, "s1q2": Cc + mid, "o2f1": Cc + 2 * Cc}[form]
    K = K0 + Kx
    c = dict(form=form, Cc=Cc, mid=mid, B=B, L=Ln, M=M, K0=K0, m_split=Cc, k_split=K0 // 32, G=K // 32,
             act=L.ACT_GELU if form == "o2f1" else L.ACT_NONE, rs=form != "o2f1")
    c["src"] = r(B, Ln, K0) * 1.3 + (0.3 if form in ("pqkv", "s1q2") else 0.0)
    ldw = {"pqkv": 0, "o1q2": Cc + 3 * mid, "o2f1": Cc + mid, "s1q2": 2 * Cc}[form]
    c["wide"] = r(B, Ln, ldw) if ldw else None
    if form == "s1q2":
        c["wide"] = c["wide"] * 1.3 + 0.3
        c["src"] = c["wide"][..., :Cc]
    W = r(M, K) / K ** 0.5
    W[Cc:] *= 0.5
    W[:Cc, K0:] *= 3.0
    c["W"], c["bias"] = W, r(M) * 0.5
    if form == "s1q2":
        c["bias"][Cc:] += 4.0         # 32 high columns beside 256 low ones: large enough to show in statistics taken over all of them
    c["gn"] = None
    if form in ("pqkv", "s1q2"):
        c["gn"] = (32 if form == "pqkv" else 1, torch.rand(Cc, generator=g) + 0.5, r(Cc) * 0.5, 1e-6 if form == "pqkv" else 1e-5)
    return c


def gemm_operands(c, mode):
    """the launch's operands rounded to ``mode``, float64: (x_segments with the prologue applied, W, residual, the [rows][ld] tensor the
    residual is a window of)"""
    src, wide = rounded(c["src"], mode), rounded(c["wide"], mode)
    xh = src
    if c["gn"] is not None:
        groups, gamma, beta, eps = c["gn"]
        xh = norm_apply_ref(src, mode=L.PRO_GN, groups=groups, gamma=gamma, beta=beta, eps=eps)
    if c["form"] == "pqkv":
        return [xh], rounded(c["W"], mode), None, None
    x1 = wide[..., : c["Cc"]]
    return [xh, x1], rounded(c["W"], mode), x1, wide.reshape(-1, wide.shape[-1])


def gemm_ref(c, mode):
    segs, W, res, _ = gemm_operands(c, mode)
    return dual_range_ref(segs, W, c["bias"], res, c["m_split"], c["k_split"], c["act"], None)


def gemm_wrong(c, mode, kind):
    segs, W, res, res_rows = gemm_operands(c, mode)
    return dual_range_wrong(kind, segs, W, c["bias"], res, c["m_split"], c["k_split"], c["act"], None, res_rows=res_rows)


def gemm_wrong_kinds(c):
    """the mistakes this form can show at all: GELU on the low rows needs an activation, a leaking residual a residual, an ignored
    k_split chunks above it"""
    return ["stats_all_columns"] * c["rs"] + ["gelu_low_rows"] * (c["act"] == L.ACT_GELU) + \
           ["residual_high_rows", "k_split_ignored"] * (c["form"] != "pqkv")


XATTN_CASES = [(d, Nq, Nk) for d in (8, 64) for Nq in (1, 7) for Nk in (2, 9)]
XATTN_STEPS = (5, 1)                 # the device scalar's two values: neither is an entry of extra_row


def xattn_case(d, Nq, Nk):
    """float32 operands of the cross-attention launch of ``OpBuilder.transformer``: Q arrives as the raw high columns of [x2 | q2_raw]
    (finish on Q only, statistics of x2), K / V of batch element b are row kv_row[b] of a cached table, the last key of the batch
    elements with extra_row >= 0 is row ``extra_step`` of the per-step table kv_extra.  x2 is wide (std 3), so that a finish applied to
    K and V by mistake -- a factor rstd of about 1 / 3 -- is far outside the tolerance."""
    g = _gen("xattn", d, Nq, Nk)
    r = lambda *s: torch.randn(*s, generator=g)
    B, H, Cc = 3, 4, 64
    mid = H * d
    c = dict(d=d, Nq=Nq, Nk=Nk, B=B, H=H, Cc=Cc, mid=mid, ld_extra=2 * mid + 16, kx_off=8, vx_off=8 + mid)
    q = r(B, Nq, Cc + mid)
    q[:, :, :Cc] = q[:, :, :Cc] * 3.0 + 0.5
    c["q"], c["kv"], c["kv_extra"] = q, r(2 * B, Nk, 2 * mid), r(6, c["ld_extra"]) * 2.5
    c["kv_row"] = torch.tensor([4, 0, 3], dtype=torch.int32)
    c["extra_row"] = torch.tensor([-1, 2, 4], dtype=torch.int32)
    c["u"] = torch.cat([torch.zeros(Cc), r(mid) * 0.7])
    c["b"] = torch.cat([torch.zeros(Cc), r(mid) * 0.3])
    return c


def xattn_ref(c, mode, step, wrong=None):
    q = rounded(c["q"], mode)
    stats = row_sums(q, c["Cc"]).float()                # the statistics a float32 epilogue leaves
    return attention_ref(q, rounded(c["kv"], mode), q_off=c["Cc"], k_off=0, v_off=c["mid"], H=c["H"], d=c["d"], Nk=c["Nk"],
                         kv_row=c["kv_row"], kv_extra=rounded(c["kv_extra"], mode), extra_row=c["extra_row"], extra_step=step,
                         kx_off=c["kx_off"], vx_off=c["vx_off"], fin=(stats, c["u"], c["b"], c["Cc"], 1e-5, 1, 0), wrong=wrong)


# ``jen1_norm_apply`` called directly: name -> keywords of ``norm_case``
NORM_CASES = {
    "gn":               dict(mode=L.PRO_GN, B=3, Ln=5, c0=64, groups=8),
    "gn_silu_ld":       dict(mode=L.PRO_GN_SILU, B=2, Ln=7, c0=64, groups=8, ld0=96),
    "gn_one_group":     dict(mode=L.PRO_GN, B=3, Ln=1, c0=256, groups=1, eps=1e-5),
    "gn_narrow_groups": dict(mode=L.PRO_GN, B=2, Ln=3, c0=96, groups=32, eps=1e-6),
    "gn_two_sources":   dict(mode=L.PRO_GN_SILU, B=3, Ln=5, c0=64, c1=64, groups=8, src1_scale=2 ** -0.5),      # group 3 ends at the boundary
    "gn_two_film_row":  dict(mode=L.PRO_GN_SILU, B=3, Ln=5, c0=64, c1=64, groups=8, src1_scale=2 ** -0.5, film="row"),
    "gn_film_step":     dict(mode=L.PRO_GN_SILU, B=3, Ln=29, c0=64, groups=8, film="step"),
    "gn_film_b":        dict(mode=L.PRO_GN, B=3, Ln=2, c0=64, groups=8, film="b"),
    "gn_L1_B1":         dict(mode=L.PRO_GN_SILU, B=1, Ln=1, c0=64, c1=32, groups=3, src1_scale=2 ** -0.5, film="step"),
    "ln_affine":        dict(mode=L.PRO_LN, B=2, Ln=19, c0=160, affine=True),
    "ln_plain":         dict(mode=L.PRO_LN, B=2, Ln=19, c0=160, affine=False, ld0=192),
    "ln_L1_B1":         dict(mode=L.PRO_LN, B=1, Ln=1, c0=96, affine=True),
}
FILM_ROWS, FILM_OFF = 6, 8
FILM_STEPS = (5, 1)                  # the device scalar's two values: neither is an entry of film_row


def norm_case(name, *, mode, B, Ln, c0, c1=0, groups=1, src1_scale=1.0, eps=1e-5, film=None, affine=True, ld0=None):
    """float32 operands of one ``jen1_norm_apply`` call.  film: None, "b" (row = batch element), "row" (film_row), "step" (film_step
    given beside a film_row it must override)"""
    g = _gen("norm", name)
    r = lambda *s: torch.randn(*s, generator=g)
    C = c0 + c1
    c = dict(name=name, mode=mode, B=B, L=Ln, c0=c0, c1=c1, C=C, groups=groups, src1_scale=src1_scale, eps=eps, film_kind=film,
             ld0=ld0 or c0)
    c["x0"] = r(B, Ln, c0) * 1.5 + 0.3
    c["x1"] = r(B, Ln, c1) * 0.7 - 0.2 if c1 else None
    c["gamma"] = torch.rand(C, generator=g) + 0.5 if affine else None
    c["beta"] = r(C) * 0.3 if affine else None
    c["film"] = r(FILM_ROWS, 2 * C + FILM_OFF + 3) * 0.5 if film else None
    c["film_row"] = torch.tensor([4, 0, 2][:B], dtype=torch.int32) if film in ("row", "step") else None
    return c


def norm_ref(c, mode, step=None, wrong=None):
    """float64 reference of a ``norm_case`` on operands rounded to ``mode``; step: the value of the film_step scalar (film == "step")"""
    return norm_apply_ref(rounded(c["x0"], mode), rounded(c["x1"], mode), mode=c["mode"], src1_scale=c["src1_scale"], groups=c["groups"],
                          gamma=c["gamma"], beta=c["beta"], eps=c["eps"], film=c["film"], film_row=c["film_row"],
                          film_step=step if c["film_kind"] == "step" else None, film_off=FILM_OFF, wrong=wrong)


# GroupNorm -> FiLM -> SiLU -> conv with the FiLM row taken through the device scalar: (L, c0, c1)
FILM_CONV_CASES = [(5, 64, 0), (29, 64, 0), (5, 64, 64), (29, 64, 64)]


def film_conv_case(Ln, c0, c1):
    """ConvBlock1d (reference blocks.py:137-145) over [x0, x1 2^-1/2] with B = 3, 8 groups, k = 3, 128 output channels"""
    g = _gen("film_conv", Ln, c0, c1)
    c = norm_case(f"film_conv.{Ln}.{c0}.{c1}", mode=L.PRO_GN_SILU, B=3, Ln=Ln, c0=c0, c1=c1, groups=8,
                  src1_scale=2 ** -0.5 if c1 else 1.0, film="step")
    C = c0 + c1
    c["w"] = torch.randn(128, C, 3, generator=g) / (3 * C) ** 0.5
    c["bias"] = torch.randn(128, generator=g) * 0.1
    return c


def film_conv_ref(c, mode, step, wrong=None):
    """[B][L][128] float64: conv k = 3, zero padding 1 after the prologue"""
    h = norm_ref(c, mode, step, wrong).permute(0, 2, 1)
    return F.conv1d(F.pad(h, (1, 1)), rounded(c["w"], mode), c["bias"].double()).permute(0, 2, 1)
