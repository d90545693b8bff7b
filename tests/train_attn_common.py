"""Float64 references, float32 restatements, the metric, the gates and the case table of the one-launch attention core of the training
pass (csrc/train_attn.hip: jen1_attn_small_forward[_rows], jen1_attn_small_backward[_rows], jen1_attn_small_fits); importable without a
GPU.  tests/test_train_attn_refs_host.py pins the references and shows that the gates reject wrong kernels; tests/test_gpu_train_attn.py
runs the same cases through the C ABI and through train.attention_core.  The metric's helpers, ``rounded``, ``out_rounding``,
``norm_gate`` and ``capped`` are those of tests/train_ops_common.py.

References (``attn_ref``), float64, written out from the reference model's lines (blocks.py:315-319 the causal rule j <= i + (Nk - Nq),
:355-380 the attention core, :431-434 the padding mask multiplied into k and v).  Inputs are rounded to the mode's dtype first.  K and V
of batch element b are row kv_row[b] of the table times kv_mask[b], the product rounded to the dtype as the kernel's staging rounds it.
``p`` is the softmax over the kept keys; ``p_in`` is p rounded to the dtype -- what the kernel stores, what P V multiplies and what the
backward pass reads -- and ``o`` = p_in V.  The backward reference is the kernel's CONTRACT in float64 on p_in (never on a kernel's
output): dP = dO V^T, dS = P (dP - sum_j P dP), dQ = scale dS K, dK_b = scale mask_b dS^T Q, dV_b = mask_b P^T dO, per batch element, not
summed over the batch elements that share K / V rows.  ``attn_ref_autograd`` is torch.autograd on the float64 forward with the gather
kv[kv_row] inside it; on the unrounded p and after the sharers' sum it equals the contract (pinned on the host).

Restatements (``attn_fwd_emul``, ``attn_bwd_emul``): the same steps with every operation in float32 and P rounded to the dtype before
P V, as in the kernel.  Run in float64 they equal the references; run in float32 their error against float64 is the yardstick of the
gates; and each takes a ``fault`` (``FAULTS``) that makes it wrong in one of the ways this kernel or its callers can be wrong.

Metric: elementwise |got - ref| / (|ref| + s + FLOOR), the maximum over the elements.  s of ``p`` is the RMS of its row; s of ``o``,
``dq``, ``dk``, ``dv`` is the root of the sum of squares of the terms summed into that element (the convention tests/train_ops_common.py
uses for sums; a term dS_ij K_jc of dq, dS_ij Q_ic of dk, counts as the two terms p_ij dP_ij and p_ij sum_j p_ij dP_ij whose difference dS_ij
is: they cancel where one key holds all the weight).  A wrong last key, a wrong last row or one head's dK is then measured against its own neighbourhood.

Gates (``attn_gates``): the output's rounding + 4 x the float32 restatement's error against float64 on the same inputs (``norm_gate``),
no looser than ``capped`` allows against tests/test_gpu_train.py's tolerances.  bf16 ``o`` takes one further term: the kernel's float32
p and the reference's float64 p can round to neighbouring bf16 values, and then one term p_ij v_jc of the sum differs by one bf16 ulp of
p_ij, at most 2 x 2^-8 |p_ij v_jc|: against the denominator that is 2 x 2^-8 max over the elements of max_j |p_ij v_jc| / (|o_ic| + s_ic)
(``one_ulp_term``; it is at most 2^-8, reached where one key holds all the weight).

Form rule: the file has no ``*_form`` query.  ``rows_aligned`` restates the kernel's: an operand is staged with 16-byte vectors when
d % V == 0, ld % V == 0 and the pointer is 16-byte aligned, V = 16 / sizeof(T).  ``AttnCase.forms`` names the intended form of q, k, v and
dO per mode; ``operand_forms`` computes it from pointers and pitches.

Measured on MI355X (profiles/train_attn_parity.txt), the worst measured / gate ratio per quantity over all cases, no gate beyond the
rule above:
    C ABI, f32:   p 0.39 (hot-row-causal), o 0.40 (hot-row-causal), dq 0.44 (rows-2021), dk 0.41 (causal-b101/flag1), dv 0.25
    C ABI, bf16:  p 0.84 (lds-24x110-d128), o 0.56 (coherent-6x60), dq 0.70 (lds-64x121-d64), dk 0.67 (rows-01222), dv 0.67
                  (what the output's own rounding to bf16 takes: the float32 restatement rounded to bf16 measures the same figures)
    backward on the forward's own P:  f32 dq 0.45, dk 0.24, dv 0.27;  bf16 dq 0.70, dk 0.65, dv 0.66
    train.attention_core vs autograd: f32 o 0.21, dq 0.28, dK | dV 0.59;  bf16 o 0.27, dq 0.55, dK | dV 0.52
No case exposed a fault in csrc/train_attn.hip or in AttentionCoreFn.
"""
import functools
from dataclasses import dataclass

import torch

from train_ops_common import (BF16, BIG, F32, FLOOR, MODES, OLD_TOL, U8, U24, _gen, capped, compare, failures, metric, norm_gate,  # noqa: F401
                              out_rounding, rounded, tdtype)

OTHER = 5.5                     # columns of a shared output matrix that belong to somebody else
FWD_Q = ("p", "o")
BWD_Q = ("dq", "dk", "dv")
QUANTITIES = FWD_Q + BWD_Q
INPUT_OPERANDS = ("q", "k", "v", "do")
FAULTS = ("causal_off_by_one", "causal_b_ignored", "kv_row_ignored", "mask_by_kv_row", "mask_not_in_dk", "p_unrounded_in_pv",
          "scale_missing_dq", "scale_missing_dk", "dv_from_ds", "last_key_dropped", "last_query_row_stale", "head_stride_wrong")
LDS_MAX = 160 * 1024


def pad8(n):
    return (n + 7) // 8 * 8


def esize(mode):
    return 4 if mode == F32 else 2


def rows_aligned(ptr, ld, d, esz):
    """csrc/train_attn.hip rows_aligned: the rows of one head are read as 16-byte vectors"""
    v = 16 // esz
    return d % v == 0 and ld % v == 0 and ptr % 16 == 0


def bwd_lds(Nq, Nk, d):
    """bytes of LDS of the backward kernel (csrc/train_attn.hip bwd_lds): Q, dO [Nq][d + 4], K, V [Nk][d + 4], P, dS [Nq][Nk | 1], float32"""
    return ((2 * Nq + 2 * Nk) * (d + 4) + 2 * Nq * (Nk | 1)) * 4


def fits(Nq, Nk, d):
    return Nq <= 64 and Nk <= 512 and d <= 128 and d % 4 == 0 and bwd_lds(Nq, Nk, d) <= LDS_MAX


@dataclass(frozen=True)
class AttnCase:
    name: str
    B: int
    H: int
    Nq: int
    Nk: int
    d: int
    causal: int = 0               # the scalar flag
    causal_b: tuple = None        # the flag per batch element (overrides the scalar flag)
    mask: str = ""                # kv_mask: "01" 0 / 1 entries that differ between batch elements, "full" batch element 1 fully masked too,
    #                               "frac" one fractional entry (0.625: three bits, the product needs rounding in both dtypes)
    kv_row: tuple = None          # K / V row map; the table then has Bk rows
    Bk: int = 0
    extra: tuple = ()             # ((operand, columns), ...): the pitch of q, k, v, do (and o), dq, dk, dv is H d + columns
    off: tuple = ()               # ((operand, bytes), ...): q, k, v, do start that many bytes past a 16-byte boundary
    kv_joint: int = -1            # >= 0: K | V are two column windows of ONE matrix of pitch 2 H d + kv_joint
    dkv_window: tuple = None      # (W, c0): dK | dV are columns [c0, c0 + 2 H d) of one matrix of pitch W
    ldp: int = 0                  # 0: pad8(Nk)
    hot: bool = False             # the last query row of every head is scaled so that its scores reach about +-80
    coherent: bool = False        # q is zero (uniform p) and v has mean 1.5: every term of o has the sign and the
    #                               rounding of its neighbours
    forms: tuple = ("vvvv", "vvvv")   # the intended staging form of q, k, v, dO (v vector, s scalar) in f32 and in bf16

    @property
    def C(self):
        return self.H * self.d

    @property
    def rows(self):
        return self.Bk if self.kv_row is not None else self.B

    @property
    def scale(self):
        """the float32 value the entry points are given"""
        return float(torch.tensor(float(self.d) ** -0.5, dtype=torch.float32))

    @property
    def p_ld(self):
        return self.ldp or pad8(self.Nk)

    def form(self, mode):
        return self.forms[MODES.index(mode)]


def _wide(n, ops=("q", "k", "v", "do", "dq", "dk", "dv")):
    return tuple((o, n) for o in ops)


_SV = ("vvvv", "ssss")
_SS = ("ssss", "ssss")
CASES = [
    # sizes
    AttnCase("1x1", 2, 2, 1, 1, 8),
    AttnCase("5x7", 2, 3, 5, 7, 8),
    AttnCase("24x24", 2, 4, 24, 24, 16, ldp=27),                                       # ldp = Nk + 3
    AttnCase("24x24-causal", 2, 4, 24, 24, 16, causal=1),
    AttnCase("64x64-causal", 1, 2, 64, 64, 8, causal=1),                               # the 8-wave row loop eight times; B = 1
    AttnCase("5x129", 2, 2, 5, 129, 8),                                                # three lane strides; ldp = pad8(129) = 136
    AttnCase("7x130-causal", 1, 2, 7, 130, 8, causal=1, ldp=133),
    AttnCase("1x512-d32", 1, 2, 1, 512, 32),
    AttnCase("d4", 2, 2, 5, 7, 4, forms=_SV),
    AttnCase("d128-H1", 1, 1, 3, 9, 128),
    # the LDS edge: the largest Nk that jen1_attn_small_fits accepts
    AttnCase("lds-24x110-d128", 1, 1, 24, 110, 128),
    AttnCase("lds-64x121-d64", 1, 2, 64, 121, 64, causal=1),
    # causal
    AttnCase("9x13-causal", 2, 2, 9, 13, 8, causal=1),
    AttnCase("causal-b101/flag0", 3, 2, 9, 13, 8, causal=0, causal_b=(1, 0, 1)),
    AttnCase("causal-b101/flag1", 3, 2, 9, 13, 8, causal=1, causal_b=(1, 0, 1)),
    AttnCase("causal-b010/flag1", 3, 2, 6, 6, 8, causal=1, causal_b=(0, 1, 0)),
    AttnCase("9x13-causal-mask", 2, 2, 9, 13, 8, causal=1, mask="01"),
    # kv_mask
    AttnCase("mask-01", 2, 2, 5, 7, 8, mask="01"),
    AttnCase("mask-full", 3, 2, 5, 7, 8, mask="full"),
    AttnCase("mask-frac", 2, 2, 5, 7, 8, mask="frac"),
    # kv_row
    AttnCase("rows-01222", 5, 1, 5, 7, 16, mask="01", kv_row=(0, 1, 2, 2, 2), Bk=3),
    AttnCase("rows-0111-H2", 4, 2, 5, 7, 16, mask="01", kv_row=(0, 1, 1, 1), Bk=2),
    AttnCase("rows-2021", 4, 2, 5, 7, 8, mask="01", kv_row=(2, 0, 2, 1), Bk=3),
    # staging forms
    AttnCase("d12", 2, 2, 5, 7, 12, forms=_SV),
    AttnCase("d20", 2, 2, 5, 9, 20, forms=_SV),
    AttnCase("d8-ld+4", 2, 2, 5, 7, 8, extra=_wide(4, INPUT_OPERANDS), forms=_SV),
    AttnCase("d8-ld+2", 2, 2, 5, 7, 8, extra=_wide(2, INPUT_OPERANDS), forms=_SS),
    AttnCase("d8-off4", 2, 2, 5, 7, 8, off=tuple((o, 4) for o in INPUT_OPERANDS), forms=_SS),
    AttnCase("d8-off8", 2, 2, 5, 7, 8, off=tuple((o, 8) for o in INPUT_OPERANDS), forms=_SS),
    AttnCase("mixed-vsvs", 2, 2, 5, 7, 8, off=(("k", 8),), extra=(("do", 2),), forms=("vsvs", "vsvs")),
    # pitches
    AttnCase("wide", 2, 2, 5, 7, 8, extra=_wide(8)),
    AttnCase("kv-joint-window", 3, 2, 5, 7, 8, mask="01", kv_joint=8, dkv_window=(48, 8), extra=(("q", 8), ("do", 16), ("dq", 24))),
    AttnCase("rows-window", 4, 2, 5, 9, 8, mask="01", kv_row=(0, 1, 2, 2), Bk=3, kv_joint=0, dkv_window=(40, 0), ldp=12),
    # scores
    AttnCase("hot-row", 2, 2, 6, 65, 16, hot=True),
    AttnCase("hot-row-causal", 2, 2, 6, 6, 16, causal=1, hot=True),
    # uniform rows over a V with an offset
    AttnCase("coherent-6x60", 2, 2, 6, 60, 8, coherent=True),                            # bf16(1 / 60) = 1.0034 / 60: 0.875 x 2^-8 off
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and all(c.B * c.H <= 8 and fits(c.Nq, c.Nk, c.d) for c in CASES)
LDS_EDGE = [("lds-24x110-d128", 110), ("lds-64x121-d64", 121)]       # (case, the largest Nk that fits by the file's formula)
# chained forward -> backward (the backward reads the forward's own P): both ldp forms, a row map, the LDS edge
CHAINED = ["24x24", "5x129", "rows-window", "9x13-causal-mask", "lds-64x121-d64"]


# =====================================================================================================================
# inputs
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def attn_inputs(case: AttnCase, mode: str):
    """float32 tensors as the kernel sees them (rounded to bf16 where it reads bf16): q, do [B, Nq, C], k, v [rows, Nk, C], mask [B, Nk] or
    None, flags [B] (the causal flag the kernel must apply to each batch element), kv_row [B] (the identity when the case has none)"""
    B, Nq, Nk, C = case.B, case.Nq, case.Nk, case.C
    g = _gen(B, case.H, Nq, Nk, case.d, len(case.name))
    q = torch.randn((B, Nq, C), generator=g)
    k = torch.randn((case.rows, Nk, C), generator=g)
    v = torch.randn((case.rows, Nk, C), generator=g)
    do = torch.randn((B, Nq, C), generator=g)
    if case.hot:
        # the last row's scores get a standard deviation of 40: they reach +-80 and beyond; only the max-subtraction keeps exp finite
        # (and its dO scaled down as much: its terms p dP q in dK stay the size of the other rows')
        q[:, -1] *= 40.0
        do[:, -1] /= 40.0
    if case.coherent:
        q[:] = 0.0
        v = v * 0.25 + 1.5
    mask = None
    if case.mask:
        mask = (torch.rand((B, Nk), generator=g) > 0.35).float()
        mask[:, 0] = 1.0
        for b in range(B):                                       # (every batch element differs from the one before it)
            mask[b, (b + 1) % Nk] = float(b % 2)
        if case.mask == "full":
            mask[1] = 0.0
        if case.mask == "frac":
            mask[0, Nk - 1] = 0.625
    flags = torch.tensor(case.causal_b if case.causal_b is not None else [case.causal] * B, dtype=torch.int32)
    rows = torch.tensor(case.kv_row if case.kv_row is not None else list(range(B)), dtype=torch.int64)
    return {"q": rounded(q, mode), "k": rounded(k, mode), "v": rounded(v, mode), "do": rounded(do, mode), "mask": mask, "flags": flags,
            "kv_row": rows}


def keep_mask(case: AttnCase, flags, off=0):
    """[B, Nq, Nk] bool: the keys a query keeps"""
    i, j = torch.arange(case.Nq)[:, None], torch.arange(case.Nk)[None, :]
    causal = j <= i + (case.Nk - case.Nq) + off
    return torch.where(flags.bool()[:, None, None], causal[None], torch.ones_like(causal)[None])


# =====================================================================================================================
# float64 references
# =====================================================================================================================
def _split(t, H):
    B, N, C = t.shape
    return t.view(B, N, H, C // H).permute(0, 2, 1, 3)            # [B, H, N, d]


def _merge(t):
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * d)


def _row_rms(t):
    return torch.sqrt((t * t).mean(dim=-1, keepdim=True)).expand_as(t)


def staged_kv(case: AttnCase, d, mode):
    """float64 [B, Nk, C] K and V as the kernel stages them: row kv_row[b] times kv_mask[b], rounded to the dtype"""
    k, v = d["k"].double()[d["kv_row"]], d["v"].double()[d["kv_row"]]
    if d["mask"] is not None:
        m = d["mask"].double()[:, :, None]
        k, v = rounded(k * m, mode).double(), rounded(v * m, mode).double()
    return k, v


def attn_bwd_ref(case: AttnCase, mode: str, p_in):
    """the backward kernel's contract in float64 on ``p_in`` [B, H, Nq, Nk], and the scales of the metric"""
    d = attn_inputs(case, mode)
    H, sc = case.H, case.scale
    k, v = staged_kv(case, d, mode)
    q4, k4, v4, g4 = _split(d["q"].double(), H), _split(k, H), _split(v, H), _split(d["do"].double(), H)
    m = d["mask"].double()[:, None, :, None] if d["mask"] is not None else torch.ones((1, 1, 1, 1), dtype=torch.float64)
    p = p_in.double()
    dp = torch.einsum("bhid,bhjd->bhij", g4, v4)
    t = (p * dp).sum(dim=-1, keepdim=True)
    ds = p * (dp - t)
    rss = lambda a, b, eq: torch.sqrt(torch.einsum(eq, a * a, b * b))          # noqa: E731
    # the summed terms of dq and dk: dS_ij is itself the difference of p_ij dP_ij and p_ij t_i, t_i = sum_j p_ij dP_ij, which cancel where
    # one key holds all the weight (dS -> 0 while both stay of order |dP|): each dS_ij K_jc (Q_ic) counts as those two terms
    ds2 = torch.sqrt((p * dp) ** 2 + (p * t) ** 2)
    return {"dq": _merge(torch.einsum("bhij,bhjd->bhid", ds, k4) * sc), "s:dq": _merge(rss(ds2, k4, "bhij,bhjd->bhid") * sc),
            "dk": _merge(torch.einsum("bhij,bhid->bhjd", ds, q4) * sc * m), "s:dk": _merge(rss(ds2, q4, "bhij,bhid->bhjd") * sc * m),
            "dv": _merge(torch.einsum("bhij,bhid->bhjd", p, g4) * m), "s:dv": _merge(rss(p, g4, "bhij,bhid->bhjd") * m)}


@functools.lru_cache(maxsize=None)
def attn_ref(case: AttnCase, mode: str):
    d = attn_inputs(case, mode)
    H = case.H
    k, v = staged_kv(case, d, mode)
    q4, k4, v4 = _split(d["q"].double(), H), _split(k, H), _split(v, H)
    sim = torch.einsum("bhid,bhjd->bhij", q4, k4) * case.scale
    keep = keep_mask(case, d["flags"])[:, None]
    p = torch.softmax(sim.masked_fill(~keep, -float("inf")), dim=-1)
    p_in = rounded(p, mode).double()
    ref = {"p": p, "s:p": _row_rms(p), "p_in": p_in, "keep": keep.expand_as(p),
           "o": _merge(torch.einsum("bhij,bhjd->bhid", p_in, v4)),
           "s:o": _merge(torch.sqrt(torch.einsum("bhij,bhjd->bhid", p_in * p_in, v4 * v4)))}
    ref.update(attn_bwd_ref(case, mode, p_in))
    return ref


def sum_sharers(t, kv_row, rows):
    """[B, Nk, C] per batch element -> [rows, Nk, C]: the blocks of the batch elements that read the same K / V rows added up"""
    return torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype).index_add_(0, kv_row, t)


@functools.lru_cache(maxsize=None)
def attn_ref_autograd(case: AttnCase, mode: str):
    """torch.autograd on the float64 forward with the gather kv[kv_row] inside (the staging's rounding of k mask passes the gradient
    through: d(k mask) / dk = mask); o from the UNROUNDED p.  dk, dv: [rows, Nk, C], the sharers summed; dk_b, dv_b: per batch element"""
    d = attn_inputs(case, mode)
    H = case.H
    q, kt, vt = (d[n].double().requires_grad_() for n in ("q", "k", "v"))
    kb, vb = kt[d["kv_row"]], vt[d["kv_row"]]
    kb.retain_grad(), vb.retain_grad()
    ks, vs = kb, vb
    if d["mask"] is not None:
        m = d["mask"].double()[:, :, None]
        ks, vs = kb * m, vb * m
        ks = ks + (rounded(ks.detach(), mode).double() - ks.detach())
        vs = vs + (rounded(vs.detach(), mode).double() - vs.detach())
    sim = torch.einsum("bhid,bhjd->bhij", _split(q, H), _split(ks, H)) * case.scale
    p = torch.softmax(sim.masked_fill(~keep_mask(case, d["flags"])[:, None], -float("inf")), dim=-1)
    o = _merge(torch.einsum("bhij,bhjd->bhid", p, _split(vs, H)))
    o.backward(d["do"].double())
    return {"o": o.detach(), "p": p.detach(), "dq": q.grad, "dk": kt.grad, "dv": vt.grad, "dk_b": kb.grad, "dv_b": vb.grad}


# =====================================================================================================================
# restatements: every operation in ``dtype``; ``fault``: one of FAULTS
# =====================================================================================================================
def _heads_in(t, H, d, fault):
    """[B, N, C] -> [B, H, N, d] as the kernel reads an input"""
    if fault == "head_stride_wrong":
        idx = (torch.arange(H)[:, None] * (d + 4) + torch.arange(d)[None, :]) % t.shape[-1]
        return t[:, :, idx].permute(0, 2, 1, 3)
    return _split(t, H)


def _emul_mask(case, d, fault):
    m = d["mask"]
    if m is not None and fault == "mask_by_kv_row":
        m = m[d["kv_row"]]
    return m


def _emul_kv(case, d, mode, dtype, fault):
    rows = d["kv_row"]
    if fault == "kv_row_ignored":
        rows = torch.arange(case.B).clamp_max(case.rows - 1)
    k, v = d["k"].to(dtype)[rows], d["v"].to(dtype)[rows]
    m = _emul_mask(case, d, fault)
    if m is not None:
        k, v = rounded(k * m.to(dtype)[:, :, None], mode).to(dtype), rounded(v * m.to(dtype)[:, :, None], mode).to(dtype)
    return k, v


def attn_fwd_emul(case: AttnCase, d, mode, dtype=torch.float32, fault=None):
    """-> p [B, H, Nq, Nk] (before its rounding to the dtype) and o [B, Nq, C]"""
    H, dd = case.H, case.d
    k, v = _emul_kv(case, d, mode, dtype, fault)
    q4, k4, v4 = (_heads_in(t, H, dd, fault) for t in (d["q"].to(dtype), k, v))
    s = torch.einsum("bhid,bhjd->bhij", q4, k4) * case.scale
    flags = torch.full_like(d["flags"], case.causal) if fault == "causal_b_ignored" else d["flags"]
    keep = keep_mask(case, flags, -1 if fault == "causal_off_by_one" else 0)[:, None].expand_as(s).clone()
    if fault == "last_key_dropped":
        keep[..., -1] = False
    mx = torch.where(keep, s, torch.full_like(s, -3.0e38)).max(dim=-1, keepdim=True).values
    e = torch.where(keep, torch.exp(s - mx), torch.zeros_like(s))
    p = e * (1 / e.sum(dim=-1, keepdim=True))
    pr = p if fault == "p_unrounded_in_pv" else rounded(p, mode).to(dtype)
    o = _merge(torch.einsum("bhij,bhjd->bhid", pr, v4))
    if fault == "last_query_row_stale":
        p, o = p.clone(), o.clone()
        p[:, :, -1], o[:, -1] = 0, 0
    return {"p": p, "o": o}


def attn_bwd_emul(case: AttnCase, d, mode, p_in, dtype=torch.float32, fault=None):
    """-> dq [B, Nq, C], dk, dv [B, Nk, C] per batch element"""
    H, dd = case.H, case.d
    sc = case.scale
    k, v = _emul_kv(case, d, mode, dtype, fault)
    q4, k4, v4, g4 = (_heads_in(t, H, dd, fault) for t in (d["q"].to(dtype), k, v, d["do"].to(dtype)))
    m = _emul_mask(case, d, fault)
    m = m.to(dtype)[:, None, :, None] if m is not None else torch.ones((1, 1, 1, 1), dtype=dtype)
    p = p_in.to(dtype)
    dp = torch.einsum("bhid,bhjd->bhij", g4, v4)
    ds = p * (dp - (p * dp).sum(dim=-1, keepdim=True))
    dq = torch.einsum("bhij,bhjd->bhid", ds, k4) * (1 if fault == "scale_missing_dq" else sc)
    dk = torch.einsum("bhij,bhid->bhjd", ds, q4) * ((1 if fault == "scale_missing_dk" else sc) * (1 if fault == "mask_not_in_dk" else m))
    dv = torch.einsum("bhij,bhid->bhjd", ds if fault == "dv_from_ds" else p, g4) * m
    if fault == "last_query_row_stale":
        dq = dq.clone()
        dq[:, :, -1] = 0
    return {"dq": _merge(dq), "dk": _merge(dk), "dv": _merge(dv)}


def attn_emul(case: AttnCase, mode: str, dtype=torch.float32, fault=None):
    """both restatements on the case's inputs, the backward on the reference's p_in"""
    d = attn_inputs(case, mode)
    out = attn_fwd_emul(case, d, mode, dtype, fault)
    out.update(attn_bwd_emul(case, d, mode, attn_ref(case, mode)["p_in"], dtype, fault))
    return out


# =====================================================================================================================
# gates
# =====================================================================================================================
def one_ulp_term(ref, d, case, mode):
    """bf16 o: one term p_ij v_jc off by one bf16 ulp of p_ij (<= 2 x 2^-8 p_ij), against the metric's denominator"""
    if mode != BF16:
        return 0.0
    k, v = staged_kv(case, d, mode)
    big = _merge((ref["p_in"][..., None] * _split(v, case.H)[:, :, None].abs()).amax(dim=3))         # max_j |p_ij v_jc|
    return 2.0 * U8 * float((big / (ref["o"].abs() + ref["s:o"] + FLOOR)).max())


@functools.lru_cache(maxsize=None)
def attn_yards(case: AttnCase, mode: str):
    """the float32 restatement's error against float64, per quantity"""
    ref, emul = attn_ref(case, mode), attn_emul(case, mode)
    return {q: metric(emul[q], ref[q], ref["s:" + q]) for q in QUANTITIES}


@functools.lru_cache(maxsize=None)
def attn_gates(case: AttnCase, mode: str):
    ref, yards = attn_ref(case, mode), attn_yards(case, mode)
    extra = {"o": one_ulp_term(ref, attn_inputs(case, mode), case, mode)}
    # (1x1: one key, p = 1 and dS = 0 exactly -- dq and dk are all zeros, nothing to take the old tolerance relative to)
    return {q: capped(g, ref, q, mode) if float(ref[q].abs().max()) > 0 else g
            for q, g in ((q, norm_gate(mode, yards[q], extra=extra.get(q, 0.0))) for q in QUANTITIES)}


# =====================================================================================================================
# memory layout of a case: matrices, operands, forms
# =====================================================================================================================
def layout(case: AttnCase, mode: str):
    """{operand: (matrix, first column, pitch)} and {matrix: (shape, byte offset past a 16-byte boundary)}.  Operands: q, k, v, do, o, p,
    dq, dk, dv; o has do's pitch (the entry points take one ``ldo`` each)"""
    B, Nq, Nk, C = case.B, case.Nq, case.Nk, case.C
    ex, off = dict(case.extra), dict(case.off)
    ops, mats = {}, {}

    def own(op, rows, n, extra_of=None):
        ld = C + ex.get(extra_of or op, 0)
        ops[op], mats[op] = (op, 0, ld), ((rows, n, ld), off.get(op, 0))

    own("q", B, Nq)
    own("do", B, Nq)
    own("o", B, Nq, "do")
    own("dq", B, Nq)
    if case.kv_joint >= 0:
        ld = 2 * C + case.kv_joint
        mats["kv"] = ((case.rows, Nk, ld), off.get("k", 0))
        ops["k"], ops["v"] = ("kv", 0, ld), ("kv", C, ld)
    else:
        own("k", case.rows, Nk)
        own("v", case.rows, Nk)
    if case.dkv_window is not None:
        w, c0 = case.dkv_window
        assert c0 + 2 * C <= w
        mats["dkv"] = ((B, Nk, w), 0)
        ops["dk"], ops["dv"] = ("dkv", c0, w), ("dkv", c0 + C, w)
    else:
        own("dk", B, Nk)
        own("dv", B, Nk)
    assert case.p_ld >= Nk
    ops["p"], mats["p"] = ("p", 0, case.p_ld), ((B * case.H, Nq, case.p_ld), 0)
    return ops, mats


def operand_forms(case: AttnCase, mode: str, base):
    """the staging form of q, k, v, dO ('v' or 's' each) when matrix m starts at address base[m]"""
    ops, _ = layout(case, mode)
    esz = esize(mode)
    return "".join("v" if rows_aligned(base[ops[o][0]] + ops[o][1] * esz, ops[o][2], case.d, esz) else "s" for o in INPUT_OPERANDS)


def host_fill(case: AttnCase, mode: str, p_in=None):
    """{matrix: float32 fill}: inputs hold their data and BIG in the columns no head reads; outputs NaN where a kernel writes and OTHER
    in the columns that belong to somebody else; ``p``: NaN everywhere (the forward writes the padding columns too), or ``p_in`` with
    BIG padding when given (the backward's input)"""
    d = attn_inputs(case, mode)
    ops, mats = layout(case, mode)
    C = case.C
    fill = {}
    for m, (shape, _) in mats.items():
        fill[m] = torch.full(shape, OTHER if m in ("o", "dq", "dk", "dv", "dkv") else BIG)
    for op, src in (("q", d["q"]), ("k", d["k"]), ("v", d["v"]), ("do", d["do"])):
        m, c0, _ = ops[op]
        fill[m][..., c0:c0 + C] = src
    for op in ("o", "dq", "dk", "dv"):
        m, c0, _ = ops[op]
        fill[m][..., c0:c0 + C] = float("nan")
    if p_in is None:
        fill["p"][:] = float("nan")
    else:
        fill["p"][..., :case.Nk] = p_in.reshape(case.B * case.H, case.Nq, case.Nk).float()
    return fill
