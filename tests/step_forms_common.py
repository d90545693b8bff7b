"""Shared by test_step_forms_host.py and test_gpu_step_forms.py: one sampler step (csrc/elementwise.hip, cfg_step_kernel and
cfg_step_vec_body) restated in numpy, independent of the package.

``step_model``  float64, written from the lines the kernel comments cite: the CFG combine and std rescale of model.py:362-369,
                model_predictions and the DDIM / ancestral updates of gdm.py:128-163 and :202-222, the VDM update of vdm/vdm.py:52-55, and
                the kind-4 (DPM-Solver++(2M)) and known-region blend formulas of include/jen1_hip.h.  Next to every value it returns an
                elementwise error bound for a float32 evaluation (below).
``step_f32``    the same step in float32, in the kernels' documented operand order, one rounding per operation.
case tables     the smallest shapes that reach each edge of the two kernels, the row kinds, and a sparse crossing of both with the
                objectives and switches, per entry point.

The bounds.  Every float32 operation (sum, difference, product, quotient, square root) is allowed one ulp: a relative error of
u = 2 * 2^-24 (``OP``).  A correctly rounded operation uses at most half of that, so a float32 evaluation that rounds to nearest stays
inside half of every bound whatever its summation order (test_step_forms_host.py asserts it), and the other half is the kernel's.  Errors
are carried to first order: an input with the absolute error e contributes |factor| e to a product and e to a sum, and the operation's own
rounding adds u |result|.  A sum of n terms in ANY order is within (n - 1) u sum|terms|.  A fused multiply-add rounds once where the
restatement rounds twice, so a kernel that contracts stays inside the same bound.  Every bound has the form k 2^-24 (sum of |terms|) +
(carried input errors) with k = 2 x (operations on the path of a term); each count is derived where it is used.  Nothing here was tuned on
GPU output.
"""
import zlib
from collections import namedtuple

import numpy as np

U24, U8 = 2.0 ** -24, 2.0 ** -8
OP = 2 * U24                                # u: what one operation may be off by, relatively (one ulp; see above)
TB = 32                                     # time steps per workgroup = per entry of ``parts``
OBJECTIVES = ("noise", "x0", "v")
OBJ_ID = {"noise": 0, "x0": 1, "v": 2}
F = np.float32


def bf16_round(a):
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(a.shape)


class Step:
    """what one step gives: ``val[name]`` and, from the float64 model, ``err[name]`` (the elementwise bound) for name in
    o (the guided output) / x0 / eps / x_next / hist / rows / parts.  Layouts: [B][C][T]; rows [nrep B][T][C]; parts [B][ceil(T / 32)][C][2]"""

    def __init__(self):
        self.val, self.err = {}, {}


# ---------------------------------------------------------------------------------------------------------------------
# float64 model with bounds
# ---------------------------------------------------------------------------------------------------------------------
def _rel_std(v, e_in):
    """relative error bound of the unbiased std over axis 1 of v [B][C][T] as float32 computes it from inputs that are off by e_in.
    mean: a sum of C terms ((C - 1) u sum|v|) and a division (u |m|) -> e_m.  A perturbed mean changes sum (v - m)^2 by exactly
    C e_m^2 (the first-order term is sum (v - m) = 0).  Each d = v - m' rounds once (its square carries 2 u), the square once (u), the
    sum of C non-negative terms (C - 1) u: (C + 2) u.  The division by C - 1: u.  The square root halves the relative error and adds
    u.  The inputs: std is a seminorm, so |std(v + e) - std(v)| <= ||e|| / sqrt(C - 1)."""
    C = v.shape[1]
    m = v.mean(axis=1, keepdims=True)
    ss = ((v - m) ** 2).sum(axis=1, keepdims=True)
    e_m = OP * ((C - 1) * np.abs(v).sum(axis=1, keepdims=True) / C + np.abs(m))
    rel = ((C + 3) * OP + C * e_m ** 2 / ss) / 2 + OP
    return rel + np.sqrt((e_in ** 2).sum(axis=1, keepdims=True) / ss)


def _guided64(net_rows, B, C, nrep, scale, scale_cfg, phi):
    """model.py:362-369 -> (o, e_o), [B][C][T]"""
    n = np.asarray(net_rows, dtype=np.float64)[:, :, :C]
    oc = n[:B].transpose(0, 2, 1)
    if nrep == 1:
        return oc.copy(), np.zeros_like(oc)                     # the network output itself: no arithmetic
    ou = n[B:2 * B].transpose(0, 2, 1)
    ds = (oc - ou) * float(F(scale))
    og = ou + ds
    # difference, product, sum: the difference's and the product's roundings are relative to |ds| (2 u |ds|), the sum's to |og| <= |ou| + |ds|
    e_og = 3 * OP * (np.abs(ou) + np.abs(ds))
    if not scale_cfg:
        return og, e_og
    p = float(F(phi))
    q = 1.0 - p
    ratio = oc.std(axis=1, ddof=1, keepdims=True) / og.std(axis=1, ddof=1, keepdims=True)
    a, b = p * (og * ratio), q * og
    # ratio: the two standard deviations and one division (u).  a = phi (og ratio): two products (2 u) on top of the ratio's error, and
    # og's own error times |phi ratio|.  b = (1 - phi) og: 1 - phi rounds (u), the product (u), and og's error times |1 - phi|.  The last
    # sum rounds once more, relative to |o| <= |a| + |b|: + u on both.
    rel = _rel_std(oc, np.zeros_like(oc)) + _rel_std(og, e_og) + OP
    e_o = (rel + 3 * OP) * np.abs(a) + 3 * OP * np.abs(b) + (np.abs(p * ratio) + abs(q)) * e_og
    return a + b, e_o


def step_model(net_rows, x, noise, hist, coef_row, blend, B, C, nrep, scale, scale_cfg, phi, objective, clip_x0, rows_bf16=False):
    """One step in float64.  net_rows [nrep B][T][>= C] (cond rows, then the uncond rows); x, noise, hist [B][C][T] (noise None: none
    drawn; hist not None: a multistep form, which draws no noise); coef_row the 8 floats of include/jen1_hip.h; blend None or
    (known, eps_k, keep [B][T], p, q).  Inputs are taken as exact: round them to the storage type first."""
    st = Step()
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[2]
    sr, srm1, sa_n, cc, sg, kind, sa_t, s1m_t = (float(F(v)) for v in coef_row)
    obj = OBJ_ID.get(objective, objective)
    clip = (lambda v: np.clip(v, -1.0, 1.0)) if clip_x0 else (lambda v: v)         # exact, and 1-Lipschitz: a bound passes through
    o, e_o = _guided64(net_rows, B, C, nrep, scale, scale_cfg, phi)
    ms = hist is not None
    zero = np.zeros_like(x)
    nz = zero if (noise is None or ms or sg == 0.0) else np.asarray(noise, dtype=np.float64)     # (a sigma == 0 row reads no noise)
    if obj == 0:                                            # gdm.py:128-131
        eps, e_eps = o, e_o
        a, b = sr * x, srm1 * eps
        x0 = clip(a - b)
        e_x0 = 2 * OP * (np.abs(a) + np.abs(b)) + abs(srm1) * e_o           # each product u, the difference u (|a| + |b|)
    else:
        if obj == 1:                                        # gdm.py:133-136
            x0, e_x0 = clip(o), e_o
        else:                                               # gdm.py:138-142
            a2, b2 = sa_t * x, s1m_t * o
            x0 = clip(a2 - b2)
            e_x0 = 2 * OP * (np.abs(a2) + np.abs(b2)) + abs(s1m_t) * e_o
        a = sr * x
        eps = (a - x0) / srm1
        # numerator: the product u |a|, the difference u (|a| + |x0|), x0's own error; through 1 / srm1; the division u |eps|
        e_eps = (2 * OP * np.abs(a) + OP * np.abs(x0) + e_x0) / abs(srm1) + OP * np.abs(eps)
    if kind == 4.0:                                         # include/jen1_hip.h: x_next = (b0 x0 + a x_t) + b1 x0_prev
        if not ms:
            raise ValueError("a kind-4 row needs a multistep form")
        hp = zero if sg == 0.0 else np.asarray(hist, dtype=np.float64)          # (a b1 == 0 row reads no history)
        p = (sa_n * x0, cc * x, sg * hp)
        x_next = (p[0] + p[1]) + p[2]
        e_xn = 3 * OP * sum(np.abs(v) for v in p) + abs(sa_n) * e_x0          # a term: its product and at most two sums
    elif kind == 3.0:                                       # vdm/vdm.py:52-55, evaluated as written, no clamp
        t = (sr * x, srm1 * o, srm1 * x, sr * o)
        x0, eps = t[0] - t[1], t[2] + t[3]
        e_x0 = 2 * OP * (np.abs(t[0]) + np.abs(t[1])) + abs(srm1) * e_o
        e_eps = 2 * OP * (np.abs(t[2]) + np.abs(t[3])) + abs(sr) * e_o
        p = (sa_n * x0, cc * eps)
        x_next = p[0] + p[1]
        e_xn = 2 * OP * (np.abs(p[0]) + np.abs(p[1])) + abs(sa_n) * e_x0 + abs(cc) * e_eps
    elif kind == 1.0:                                       # gdm.py:207-209
        x_next, e_xn = x0, e_x0
    elif kind == 2.0:                                       # gdm.py:144-163: posterior mean + sd noise
        p = (x0 * sa_n, cc * x, sg * nz)
        x_next = (p[0] + p[1]) + p[2]
        e_xn = 3 * OP * sum(np.abs(v) for v in p) + abs(sa_n) * e_x0
    else:                                                   # gdm.py:212-222
        p = (x0 * sa_n, cc * eps, sg * nz)
        x_next = (p[0] + p[1]) + p[2]
        e_xn = 3 * OP * sum(np.abs(v) for v in p) + abs(sa_n) * e_x0 + abs(cc) * e_eps
    if blend is not None:                                   # include/jen1_hip.h: keep (p known + q eps_k) + (1 - keep) x_next
        known, eps_k, keep, bp, bq = blend
        k1, k2 = float(F(bp)) * np.asarray(known, np.float64), float(F(bq)) * np.asarray(eps_k, np.float64)
        kn = k1 + k2
        e_kn = 2 * OP * (np.abs(k1) + np.abs(k2))                            # each product u, the sum u (|k1| + |k2|)
        kw = np.asarray(keep, np.float64)[:, None, :]
        t1, t2 = kw * kn, (1.0 - kw) * x_next
        # t1: its product u, the last sum u.  t2: 1 - keep rounds (u), the product (u), the last sum (u).  The carried errors by their weights.
        e_xn = np.abs(kw) * e_kn + np.abs(1.0 - kw) * e_xn + 2 * OP * np.abs(t1) + 3 * OP * np.abs(t2)
        x_next = t1 + t2
    st.val.update(o=o, x0=x0, eps=eps, x_next=x_next)
    st.err.update(o=e_o, x0=e_x0, eps=e_eps, x_next=e_xn)
    if ms:
        st.val["hist"], st.err["hist"] = x0, e_x0                               # the unblended, clipped x0
    rows = np.concatenate([x_next.transpose(0, 2, 1)] * nrep, axis=0)
    e_rows = np.concatenate([e_xn.transpose(0, 2, 1)] * nrep, axis=0)
    st.val["rows"] = rows
    st.err["rows"] = e_rows + (U8 * np.abs(rows) if rows_bf16 else 0.0)         # 2^-8 |value| covers the rounding to bf16 (2^-9 (|value| + e))
    nb = (T + TB - 1) // TB
    xp, ep = np.zeros((B, C, nb * TB)), np.zeros((B, C, nb * TB))              # columns past T count as zeros
    xp[:, :, :T], ep[:, :, :T] = x_next, e_xn
    xp, ep = xp.reshape(B, C, nb, TB), ep.reshape(B, C, nb, TB)
    s, q = xp.sum(-1), (xp * xp).sum(-1)
    # sum of 32 terms, any order: 31 u sum|v|, and every term's own error.  sum of squares: each square u (none inside a fused multiply-add)
    # and 31 u for the sum: 32 u q; a term off by e moves its square by 2 |v| e + e^2.
    e_s = ep.sum(-1) + (TB - 1) * OP * np.abs(xp).sum(-1)
    e_q = (2 * np.abs(xp) * ep + ep * ep).sum(-1) + TB * OP * q
    st.val["parts"] = np.stack([s, q], axis=-1).transpose(0, 2, 1, 3)
    st.err["parts"] = np.stack([e_s, e_q], axis=-1).transpose(0, 2, 1, 3)
    return st


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatement in the kernels' operand order
# ---------------------------------------------------------------------------------------------------------------------
def _sum32(a, axis, order):
    """float32 sum along ``axis``: "seq" adds the terms one by one from 0, "pairwise" adds neighbours level by level"""
    a = np.moveaxis(np.asarray(a, dtype=F), axis, 0)
    if order == "seq":
        s = np.zeros(a.shape[1:], dtype=F)
        for i in range(a.shape[0]):
            s = s + a[i]
        return s
    terms = [a[i] for i in range(a.shape[0])]
    while len(terms) > 1:
        nxt = [terms[i] + terms[i + 1] for i in range(0, len(terms) - 1, 2)]
        if len(terms) % 2:
            nxt.append(terms[-1])
        terms = nxt
    return terms[0]


def step_f32(net_rows, x, noise, hist, coef_row, blend, B, C, nrep, scale, scale_cfg, phi, objective, clip_x0, rows_bf16=False, sums="seq"):
    """The step as the kernels evaluate it (cfg_step_vec_body; cfg_step_kernel has the same expressions): numpy float32 scalars and
    arrays, so every product, sum, quotient and root is rounded to float32 by itself.  ``sums``: the order of the reductions over the
    channels (the kernels' own orders are neither; the bound holds for any)."""
    st = Step()
    x = np.asarray(x, dtype=F)
    T = x.shape[2]
    sr, srm1, sa_n, cc, sg, kind, sa_t, s1m_t = (F(v) for v in coef_row)
    obj = OBJ_ID.get(objective, objective)
    one = F(1.0)
    clip = (lambda v: np.minimum(np.maximum(v, F(-1.0)), one)) if clip_x0 else (lambda v: v)
    n = np.asarray(net_rows, dtype=F)[:, :, :C]
    oc = np.ascontiguousarray(n[:B].transpose(0, 2, 1))
    if nrep == 2:
        ou = np.ascontiguousarray(n[B:2 * B].transpose(0, 2, 1))
        og = ou + (oc - ou) * F(scale)
        if scale_cfg:
            Cf, C1 = F(C), F(C - 1)
            m_c, m_g = _sum32(oc, 1, sums) / Cf, _sum32(og, 1, sums) / Cf
            dc, dg = oc - m_c[:, None, :], og - m_g[:, None, :]
            v_c, v_g = _sum32(dc * dc, 1, sums), _sum32(dg * dg, 1, sums)
            ratio = (np.sqrt(v_c / C1) / np.sqrt(v_g / C1))[:, None, :]
            og = F(phi) * (og * ratio) + (one - F(phi)) * og
        o = og
    else:
        o = oc
    ms = hist is not None
    zero = np.zeros_like(x)
    nz = zero if (noise is None or ms or sg == 0.0) else np.asarray(noise, dtype=F)
    if obj == 0:
        eps = o
        x0 = clip(sr * x - srm1 * eps)
    elif obj == 1:
        x0 = clip(o)
        eps = (sr * x - x0) / srm1
    else:
        x0 = clip(sa_t * x - s1m_t * o)
        eps = (sr * x - x0) / srm1
    if kind == 4.0:
        if not ms:
            raise ValueError("a kind-4 row needs a multistep form")
        hp = zero if sg == 0.0 else np.asarray(hist, dtype=F)
        x_next = (sa_n * x0 + cc * x) + sg * hp
    elif kind == 3.0:
        x0 = sr * x - srm1 * o
        eps = srm1 * x + sr * o
        x_next = sa_n * x0 + cc * eps
    elif kind == 1.0:
        x_next = x0
    elif kind == 2.0:
        x_next = x0 * sa_n + cc * x + sg * nz
    else:
        x_next = x0 * sa_n + cc * eps + sg * nz
    if blend is not None:
        known, eps_k, keep, bp, bq = blend
        kn = F(bp) * np.asarray(known, F) + F(bq) * np.asarray(eps_k, F)
        kw = np.asarray(keep, F)[:, None, :]
        x_next = kw * kn + (one - kw) * x_next
    assert all(v.dtype == F for v in (o, x0, eps, x_next))
    st.val.update(o=o, x0=x0, eps=eps, x_next=x_next)
    if ms:
        st.val["hist"] = x0
    r = x_next.transpose(0, 2, 1)
    st.val["rows"] = np.concatenate([bf16_round(r) if rows_bf16 else r] * nrep, axis=0)
    nb = (T + TB - 1) // TB
    xp = np.zeros((B, C, nb * TB), dtype=F)
    xp[:, :, :T] = x_next
    xp = xp.reshape(B, C, nb, TB)
    s, q = np.zeros((B, C, nb), dtype=F), np.zeros((B, C, nb), dtype=F)
    for j in range(TB):                                      # one lane per channel walks its 32 time steps; the square is fused
        v = xp[..., j]
        s = s + v
        q = (v.astype(np.float64) * v.astype(np.float64) + q.astype(np.float64)).astype(F)
    st.val["parts"] = np.stack([s, q], axis=-1).transpose(0, 2, 1, 3)
    return st


# ---------------------------------------------------------------------------------------------------------------------
# coefficient rows: magnitudes like those of the product's tables (alphas_cumprod 0.35 -> 0.55: sqrt_recipm1 = 1.36)
# ---------------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("k0", "k0_det", "k1", "k2", "k3", "k4_first", "k4")
ROW_KIND_ID = {"k0": 0, "k0_det": 0, "k1": 1, "k2": 2, "k3": 3, "k4_first": 4, "k4": 4}
A_PREV2, A_T, A_NEXT = 0.20, 0.35, 0.55       # alphas_cumprod two steps apart: before this step (for the multistep ratio), at it, after it


def coef_row(name, variant=0):
    """the 8 floats of a row of kind ``name`` (float32): k0 DDIM at eta = 1, k0_det DDIM at eta = 0 (sigma == 0), k1 DDIM's last step,
    k2 the ancestral row, k3 a VDM row, k4_first / k4 DPM-Solver++(2M) without / with the history term.  ``variant`` moves the
    noise levels a little: a second row of the same kind with other numbers (two consecutive launches)."""
    a, an, ap = A_T + 0.04 * variant, A_NEXT + 0.03 * variant, A_PREV2 + 0.02 * variant
    head = [np.sqrt(1.0 / a), np.sqrt(1.0 / a - 1.0)]
    tail = [np.sqrt(a), np.sqrt(1.0 - a)]
    if name in ("k0", "k0_det"):
        sigma = 0.0 if name == "k0_det" else np.sqrt((1.0 - a / an) * (1.0 - an) / (1.0 - a))
        mid = [np.sqrt(an), np.sqrt(1.0 - an - sigma ** 2), sigma, 0.0]
    elif name == "k1":
        mid = [0.0, 0.0, 0.0, 1.0]
    elif name == "k2":                        # t - 1 is the level ``an``: beta = 1 - a / an
        beta = 1.0 - a / an
        mid = [beta * np.sqrt(an) / (1.0 - a), (1.0 - an) * np.sqrt(1.0 - beta) / (1.0 - a), np.sqrt(beta * (1.0 - an) / (1.0 - a)), 2.0]
    elif name == "k3":
        t, tn = 0.6 - 0.05 * variant, 0.5 - 0.05 * variant
        return np.array([np.cos(t * np.pi / 2), np.sin(t * np.pi / 2), np.cos(tn * np.pi / 2), np.sin(tn * np.pi / 2), 0.0, 3.0, 0.0, 0.0],
                        dtype=F)
    elif name in ("k4_first", "k4"):
        lam = lambda v: np.log(np.sqrt(v) / np.sqrt(1.0 - v))
        h = lam(an) - lam(a)
        E = -np.sqrt(an) * np.expm1(-h)
        if name == "k4_first":
            b0, b1 = E, 0.0
        else:
            r = (lam(a) - lam(ap)) / h
            b0, b1 = E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r)
        mid = [b0, np.sqrt(1.0 - an) / np.sqrt(1.0 - a), b1, 4.0]
    else:
        raise KeyError(name)
    return np.array(head + mid + tail, dtype=F)


def blend_level(variant=0):
    """(p, q) of the known-region blend: the level the latents are at after the step"""
    an = A_NEXT + 0.03 * variant
    return F(np.sqrt(an)), F(np.sqrt(1.0 - an))


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
VEC_SHAPES = [            # (B, C, T, ld, ld_rows, nrep): what the vector form serves
    (1, 8, 1, 8, 8, 1),               # the smallest of everything; one lane of a half wave holds channels, 31 clamped columns
    (3, 64, 31, 64, 72, 2),           # one full 64-channel block, T % 32 == 31; context columns behind the latents
    (2, 72, 33, 80, 72, 2),           # C ends inside the second block; T % 32 == 1: a block of one column and 31 zero columns
    (2, 128, 75, 136, 264, 2),        # the product's C with its concat context behind it
    (1, 136, 32, 136, 144, 1),        # C ends inside the third block; T % 32 == 0; no CFG pair
    (2, 256, 65, 256, 256, 2),        # the widest C
]
SCALAR_SHAPES = [         # (B, C, T, ld, nrep): what only the general kernel serves
    (1, 2, 1, 2, 1),
    (2, 5, 33, 7, 2),
    (3, 63, 31, 63, 2),
    (2, 65, 64, 72, 1),
    (2, 100, 75, 100, 2),
    (1, 255, 40, 255, 2),
    (2, 128, 50, 132, 2),             # C % 8 == 0, but ld % 8 != 0 forces the general kernel
]
ENTRY_POINTS = ("cfg_combine", "cfg_ddim_step", "cfg_ddim_step_adv", "cfg_ddim_step_pack", "cfg_ddim_step_pack_blend",
                "cfg_ddim_step_pack_ms", "step_tail", "step_tail_blend", "step_tail_ms")
PACKING = ENTRY_POINTS[3:]                                      # need the vector form
ADVANCING = ENTRY_POINTS[2:]                                    # advance the step counter
NOISE_ROWS = ("k0", "k0_det", "k1", "k2", "k3")                 # what the forms with a noise table take
MS_ROWS = ("k4_first", "k4", "k1", "k0")                        # the multistep forms: kind 4, DDIM's last step, another kind without its noise
SCALE = 0.8                                                     # embedding_scale of the configurations
PHIS = (0.7, 1.0)

Case = namedtuple("Case", "entry shape row objective clip scale_cfg phi blend outs indexed")
# shape: a VEC_SHAPES / SCALAR_SHAPES entry.  blend: the form is given the known-region blend (always for *_blend, alternating for *_ms).
# outs: eps_out / x0_out are passed (the unpacked forms).  indexed: coefficients and noise as tables behind a step counter (the forms
# that do not advance may also be given one row directly).


def case_id(c):
    return "%s-%s-%s-%s-clip%d-cfg%d-phi%s%s%s%s" % (c.entry, "x".join(str(v) for v in c.shape), c.row, c.objective, c.clip, c.scale_cfg,
                                                     c.phi, "-blend" if c.blend else "", "-outs" if c.outs else "",
                                                     "" if c.indexed else "-direct")


def shape_fields(shape):
    """-> (B, C, T, ld, ld_rows or None, nrep)"""
    return shape if len(shape) == 6 else shape[:4] + (None, shape[4])


def is_vector(shape, esz=2):
    """the entry points' rule for the vector form (step_run in csrc/elementwise.hip, with an aligned base pointer): C % 8 == 0,
    ld % 8 == 0, rows of a multiple of 16 bytes; for the packed rows: ld_rows >= C and rows of a multiple of 16 bytes in the compute type
    (esz: its size -- 2 is the stricter one)"""
    B, C, T, ld, ld_rows, nrep = shape_fields(shape)
    ok = C % 8 == 0 and ld % 8 == 0 and (ld * esz) % 16 == 0 and 8 <= C <= 256 and ld >= C
    if ld_rows is not None:
        ok = ok and ld_rows >= C and (ld_rows * esz) % 16 == 0
    return ok


def _cross(entry, shapes, rows, n):
    """n cases of one entry point: every list is walked at its own pace, so that n >= the longest list shows every value of every list
    and the values meet in changing combinations; not the full product"""
    out = []
    for i in range(n):
        shape = shapes[i % len(shapes)]
        row = rows[(i + i // len(rows)) % len(rows)] if rows else None
        objective = OBJECTIVES[(i + i // 3) % 3]
        clip = (i // 2 + 1) % 2
        if row == "k3":
            objective, clip = "v", 0                           # the VDM trajectory: v objective, no clamp
        blend = entry.endswith("_blend") or (entry.endswith("_ms") and i % 2 == 1)
        outs = entry in ("cfg_ddim_step", "cfg_ddim_step_adv") and i % 2 == 0
        indexed = entry != "cfg_ddim_step" or i % 3 != 2
        out.append(Case(entry, shape, row, objective, clip, (i + i // 6) % 2, PHIS[(i // 2) % 2], blend, outs, indexed))
    return out


def _combine_cases(shapes):
    out = []
    for i, shape in enumerate(shapes):                        # cfg_combine always has the pair: nrep = 2 whatever the shape says
        shape = shape[:-1] + (2,)
        out.append(Case("cfg_combine", shape, None, None, 0, (i + 1) % 2, PHIS[(i // 2) % 2], False, False, False))
    return out


N_CROSS = 14                                                   # two passes over the longest list (7 scalar shapes)
SCALAR_CASES = (_combine_cases(SCALAR_SHAPES) + _cross("cfg_ddim_step", SCALAR_SHAPES, NOISE_ROWS, N_CROSS) +
                _cross("cfg_ddim_step_adv", SCALAR_SHAPES, NOISE_ROWS, N_CROSS))
VEC_UNPACKED_CASES = (_combine_cases(VEC_SHAPES) + _cross("cfg_ddim_step", VEC_SHAPES, NOISE_ROWS, N_CROSS) +
                      _cross("cfg_ddim_step_adv", VEC_SHAPES, NOISE_ROWS, N_CROSS))
PACK_CASES = (_cross("cfg_ddim_step_pack", VEC_SHAPES, NOISE_ROWS, N_CROSS) + _cross("cfg_ddim_step_pack_blend", VEC_SHAPES, NOISE_ROWS, N_CROSS) +
              _cross("cfg_ddim_step_pack_ms", VEC_SHAPES, MS_ROWS, N_CROSS))
TAIL_CASES = (_cross("step_tail", VEC_SHAPES, NOISE_ROWS, N_CROSS) + _cross("step_tail_blend", VEC_SHAPES, NOISE_ROWS, N_CROSS) +
              _cross("step_tail_ms", VEC_SHAPES, MS_ROWS, N_CROSS))
ALL_CASES = SCALAR_CASES + VEC_UNPACKED_CASES + PACK_CASES + TAIL_CASES


def bit_exact(c):
    """the cases in which the header promises bits that a float32 restatement can state: no reduction over the channels (nrep == 1 or no
    std rescale) and no division (objective noise; a VDM row divides nothing either)"""
    nrep = shape_fields(c.shape)[5]
    return (nrep == 1 or not c.scale_cfg) and (c.objective == "noise" or c.row == "k3")


# the tail's sentinel tables and zeroed areas: (entry sizes in bytes, zeroed bytes).  4112 = 257 x 16: an odd number of 16-byte words;
# 1 MiB + 16: more than one pass of the 8 x 256 threads of a row; the zeroed area at 1, 2 and 65 (capped to 64) rows of 256 KiB.
TAIL_FILLS = [
    ((4112,), 16),
    ((16, 4112, (1 << 20) + 16), (1 << 18) + 16),
    ((4112, (1 << 20) + 16, 16), (1 << 24) + 16),
]


# ---------------------------------------------------------------------------------------------------------------------
# inputs of a case (float32; the GPU test rounds the network output to the compute type before either side reads it)
# ---------------------------------------------------------------------------------------------------------------------
BIG = 3.0e4               # padding columns [C, ld) of the network output: finite in bf16 too, and nothing may depend on them
N_TABLE, S_ROW = 5, 1     # rows of the coefficient / noise / kb tables, and the row the counter points at (rows S_ROW and S_ROW + 1 hold data)


def keep_mask(B, T, rng):
    """keep [B][T]: 0, 1 and fractional values, one mask per sample"""
    k = rng.choice(np.array([0.0, 1.0, 0.25, 0.625], dtype=F), size=(B, T)).astype(F)
    k[:, 0] = [(1.0, 0.0, 0.375)[b % 3] for b in range(B)]
    if T > 2:
        k[:, 1], k[:, 2] = 1.0, 0.0
    return k


def case_inputs(c, bf16=False, variant=0):
    """-> dict of float32 arrays: net [nrep B][T][ld] (padding BIG), x, noise, hist, known, eps_k [B][C][T], keep [B][T].  Every channel
    has its own offset and spread, so that the std rescale has something to do; x is wide enough for the clamp to act on part of x0"""
    B, C, T, ld, _, nrep = shape_fields(c.shape)
    # (seeded by what the inputs depend on, not by the entry point: the forms that must agree bit for bit are given the same numbers)
    rng = np.random.default_rng([zlib.crc32(case_id(c._replace(entry="", blend=False, outs=False, indexed=True)).encode()), variant])
    r = lambda *s: rng.standard_normal(s).astype(F)
    net = np.full((nrep * B, T, ld), BIG, dtype=F)
    net[:, :, :C] = r(nrep * B, T, C) * (0.6 + 0.8 * rng.random((1, 1, C))).astype(F) + 0.3 * r(1, 1, C)
    if bf16:
        net = bf16_round(net)
    d = dict(net=net, x=r(B, C, T), noise=r(B, C, T), hist=np.clip(r(B, C, T) * 0.8, -1.0, 1.0).astype(F), known=r(B, C, T) * F(0.5),
             eps_k=r(B, C, T), keep=keep_mask(B, T, rng))
    return d


def model_args(c, d, variant=0, bf16=False, blend=None, x=None, hist=None):
    """positional and keyword arguments of step_model / step_f32 for case c on inputs d (x / hist: override, for a second launch)"""
    B, C, T, ld, _, nrep = shape_fields(c.shape)
    row = coef_row(c.row or "k1", variant)
    ms = c.entry.endswith("_ms")
    use_blend = c.blend if blend is None else blend
    bl = (d["known"], d["eps_k"], d["keep"]) + blend_level(variant) if use_blend else None
    noise = None if (ms or c.row == "k3") else d["noise"]
    h = (d["hist"] if hist is None else hist) if ms else None
    return ((d["net"], d["x"] if x is None else x, noise, h, row, bl, B, C, nrep, SCALE, c.scale_cfg, c.phi, c.objective or "noise", c.clip),
            dict(rows_bf16=bf16))
