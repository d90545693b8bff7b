"""Float64 references, float32 restatements, the metric, the gates and the case tables of the training pass's GroupNorm, LayerNorm,
activation and softmax kernels (csrc/train_ops.hip); importable without a GPU.  tests/test_train_ops_refs_host.py pins the references and
shows that the gates reject wrong kernels; tests/test_gpu_train_ops.py runs the same cases through the C ABI.

References: the forward is written out from the reference model's lines (GroupNorm -> FiLM -> SiLU: blocks.py:137-143 and :158; LayerNorm:
blocks.py:400-401; the two LayerNorms of one input: blocks.py:427-429; GELU(erf): blocks.py:443; softmax with the causal rule
j <= i + (Nk - Nq): blocks.py:315-319 and :367-371) in float64 torch; every backward reference is torch.autograd on that forward.

Restatements (``*_emul``, the pattern of ``lstm_layer_emul`` in encodec_common.py): the same mathematics with every operation in float32,
reductions included, the backward written out by hand.  Run in float64 the hand-written backward must agree with autograd (pinned on the
host), run in float32 its error against the float64 reference is the yardstick of the GPU gates; and it takes a ``fault`` that makes it
wrong in one of the ways a kernel goes wrong, which the gates must reject.

Metric: elementwise |got - ref| / (|ref| + s), the maximum over the elements.  s is the RMS of the reference over the element's own
reduction unit: the row for LayerNorm and softmax, the (batch element, group) for GroupNorm.  For a sum over a column or a group
(dgamma, dbeta, dfilm, GroupNorm's sums, the LayerNorm mean) the unit is the column, and s is the RMS of the summed terms times
sqrt(their number) = the root of the sum of their squares: the size a sum of that many terms of either sign has (for dfilm, a sum
over t alone, at least the RMS of the group's FiLM gradients as well).  That is larger than an RMS of neighbouring results would
be, so a sum is measured against the scale on which it can be computed, not against its neighbours.  A wrong last row, a
wrong last vector of a group or one wrong dbeta entry is then measured against its own neighbourhood, not against the largest entry of
the tensor.  Activations have no reduction unit: s = 0 plus an absolute floor per element, the size of the terms that cancel in it
(see ``act_ref``).  Every denominator also carries FLOOR = 2^-102: a result in float32's denormal range may be flushed to 0, an
absolute error of up to 2^-126 = 2^-24 x 2^-102.
"""
import functools
import math
from dataclasses import dataclass

import torch

U24, U23, U8 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -8
TINY = 2.0 ** -126                       # the smallest normal number of float32 and of bf16
FLOOR = TINY * 2.0 ** 24                 # added to every denominator of the metric (denormal results may be flushed)
BIG = 3.0e4                              # padding columns of inputs (finite in bf16 too)
F32, BF16 = "f32", "bf16"
MODES = [F32, BF16]
OLD_TOL = {F32: 1e-3, BF16: 5e-2}        # what tests/test_gpu_train.py asks of max-abs error / max-abs reference


def tdtype(mode):
    return torch.float32 if mode == F32 else torch.bfloat16


def rounded(t, mode):
    """a tensor the kernel reads in the compute dtype, as the kernel sees it (float32 values)"""
    return None if t is None else (t.float() if mode == F32 else t.to(torch.bfloat16).float())


def out_rounding(mode, f32_output=False):
    """half an ulp of the output's format, relative to |ref|"""
    return U24 if (mode == F32 or f32_output) else U8


def _gen(*key):
    return torch.Generator().manual_seed(4321 + sum((i + 1) * int(v) for i, v in enumerate(key)))


def metric(got, ref, s=0.0):
    """max over the elements of |got - ref| / (|ref| + s + FLOOR); NaN or inf anywhere in ``got`` is inf"""
    got = torch.as_tensor(got).double()
    ref = torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    s = torch.as_tensor(s, dtype=torch.float64)
    if ref.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (ref.abs() + s + FLOOR)).max())


def old_metric(got, ref):
    """tests/helpers.py rel_err: max-abs error over the largest reference entry"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def norm_gate(mode, yard, f32_output=False, extra=0.0, least=0.0):
    """the gate of a norm's output or gradient: the rounding of the output plus 4 x the error of the float32 restatement against
    float64 at the same inputs (the 4 covers what the restatement does not model: the order of the reductions and float atomics).
    ``least``: a lower limit of the yardstick, 0 except for GroupNorm's sums (``sum_yard_least``)."""
    return out_rounding(mode, f32_output) + 4.0 * max(yard, least) + extra


def capped(gate, ref, q, mode):
    """no gate looser than what tests/test_gpu_train.py implies for the same quantity: |err| <= gate (|ref| + s) gives
    max|err| / max|ref| <= gate (1 + max s / max|ref|), which stays at or under its tolerance.  (It binds where one ill-conditioned
    element sets the restatement's error for a whole tensor: dfilm at L = 1, one term per sum, next to the zero of SiLU'.)"""
    s = torch.as_tensor(ref.get("s:" + q, 0.0), dtype=torch.float64)
    return min(gate, OLD_TOL[mode] / (1.0 + float(s.max() / ref[q].abs().max())))


def sum_yard_least(terms):
    """the least a float32 sum of ``terms`` terms can be held to, as a yardstick: sqrt(ceil(log2 terms)) roundings of 2^-24.  In the
    best order there is, a balanced tree, every term passes through ceil(log2 terms) additions; each level rounds partial sums
    whose squares add up to the terms' own, so the sum's error is 2^-24 sqrt(levels / 3) of their root-sum-square at one sigma and
    sqrt(levels) within two.  torch's float32 sum, which the restatement uses, IS that best order, and its measured error on one
    sample says little: 0.7 roundings on the 10 280 terms of the pad257 cases.  jen1_gn_sums adds 16 rows per thread in sequence and
    then with float atomics in an order that changes from run to run: the same input measured between 0.06e-6 and 0.31e-6 in
    different runs against 0.26e-6 - 0.28e-6 for 4 x the restatement alone.  This widens the gate of ``sums``, and of nothing else,
    by up to 3.7x (pad257: 0.95e-6); every other quantity passed 4 x its restatement with no lower limit at 0.61 of it or less."""
    return U24 * math.sqrt(math.ceil(math.log2(max(terms, 2))))


# bf16 mode of the one-launch GroupNorm kernels with SiLU: the sigmoid is v_rcp(1 + v_exp(..)) -- two uses, 2 ulp of float32 each
GN_FUSED_BF16_EXTRA = 2 * 2 * U23


def compare(got, ref, gates):
    """{quantity: metric} for every quantity that has a gate; the scale of quantity q is ref['s:' + q] (0 when absent)"""
    return {q: metric(got[q], ref[q], ref.get("s:" + q, 0.0)) for q in gates}


def failures(metrics, gates):
    return {q: (metrics[q], gates[q]) for q in gates if not metrics[q] <= gates[q]}


def _rss(t, dims):
    return torch.sqrt((t * t).sum(dim=dims))


# =====================================================================================================================
# GroupNorm (+ FiLM) (+ SiLU)
# =====================================================================================================================
@dataclass(frozen=True)
class GnCase:
    name: str
    B: int
    C: int
    ld: int
    L: int
    G: int
    fwd: str                  # the form jen1_gn_forward is meant to run: scalar | vector (two launches), fused256 | fused1024
    bwd: str                  # ... jen1_gn_backward_add2: scalar | vector (three launches), fused256 | fused1024
    sums: str = "vector"      # ... jen1_gn_sums on the same x
    film: str = ""            # "f": film_ld = 2C; "wide": 2C + 8; "odd": 2C + 3 (not a multiple of 8: scalar)
    silu: bool = True
    adds: str = ""            # "a": dx_add, "b": dx_add2, "ab": both
    mirror: bool = False      # flags bit 1: dfilm mirrors film
    mis: str = ""             # the tensor that starts one element off a 16-byte boundary: x, y (y forward, dx backward), gamma, film
    fused0: bool = False      # run with JEN1_GN_FUSED=0
    ratio: float = 0.2        # mean / std of x
    eps: float = 1e-5

    @property
    def cpg(self):
        return self.C // self.G

    @property
    def film_ld(self):
        return {"": 0, "f": 2 * self.C, "wide": 2 * self.C + 8, "odd": 2 * self.C + 3}[self.film]

    @property
    def flags(self):
        return (1 if self.silu else 0) | (2 if self.mirror else 0)


_V = dict(fwd="vector", bwd="vector")
_S = dict(fwd="scalar", bwd="scalar")
_F256 = dict(fwd="fused256", bwd="fused256")
_F1024 = dict(fwd="fused1024", bwd="fused1024")
GN_CASES = [
    # scalar by padding / by channels per group
    GnCase("pad257", 3, 257, 264, 40, 1, sums="scalar", film="f", adds="a", **_S),
    GnCase("cpg5", 2, 20, 24, 7, 4, sums="scalar", silu=False, **_S),
    GnCase("cpg1-global-atomics", 1, 256, 256, 5, 256, sums="scalar", **_S),          # one block covers 256 groups: gi >= 32
    # vector, three launches
    GnCase("vec-cpg24", 2, 96, 96, 33, 4, film="f", adds="b", **_V),                   # vpg = 3: no power of two
    GnCase("vec-16pairs", 2, 128, 128, 75, 8, film="wide", mirror=True, adds="ab", **_V),
    GnCase("vec-plain", 2, 128, 128, 75, 8, silu=False, **_V),
    # one launch, 256 threads
    GnCase("f256-vpg1", 4, 64, 64, 19, 8, film="f", adds="a", **_F256),                # B % 8 != 0
    GnCase("f256-vpg1-plain", 4, 64, 64, 19, 8, silu=False, **_F256),
    GnCase("f256-vpg16-L1", 16, 1024, 1024, 1, 8, film="wide", mirror=True, **_F256),  # B % 8 == 0
    GnCase("f256-below-long", 1, 256, 256, 1499, 32, film="f", adds="ab", **_F256),    # L cpg = 11 992
    GnCase("f256-b8-long-rows", 8, 128, 128, 375, 8, film="f", adds="b", **_F256),     # L cpg = 6 000, B % 8 == 0
    # one launch, 1024 threads
    GnCase("f1024-exact", 1, 256, 256, 1500, 32, film="f", adds="ab", **_F1024),       # L cpg = 12 000 exactly
    GnCase("f1024-b8", 8, 32, 32, 1500, 4, **_F1024),                                  # B % 8 == 0, no FiLM
    # the fused shapes with JEN1_GN_FUSED=0
    GnCase("f256-vpg1/off", 4, 64, 64, 19, 8, film="f", adds="a", fused0=True, **_V),
    GnCase("f256-vpg16-L1/off", 16, 1024, 1024, 1, 8, film="wide", mirror=True, fused0=True, **_V),
    GnCase("f1024-exact/off", 1, 256, 256, 1500, 32, film="f", adds="ab", fused0=True, **_V),
    # scalar by alignment
    GnCase("vec-cpg24/x+1", 2, 96, 96, 33, 4, film="f", adds="b", mis="x", sums="scalar", **_S),
    GnCase("vec-cpg24/y+1", 2, 96, 96, 33, 4, film="f", adds="b", mis="y", **_S),
    GnCase("vec-cpg24/gamma+1", 2, 96, 96, 33, 4, film="f", adds="b", mis="gamma", **_S),
    GnCase("vec-cpg24/film+1", 2, 96, 96, 33, 4, film="f", adds="b", mis="film", **_S),
    GnCase("f256-vpg1/x+1", 4, 64, 64, 19, 8, film="f", adds="a", mis="x", sums="scalar", **_S),
    GnCase("vec-cpg24/film-odd", 2, 96, 96, 33, 4, film="odd", **_S),
    # inputs with an offset: the kernels take the variance as E[x^2] - mean^2 from float32 sums.  At mean / std = 4 - 8 every form
    # missed these gates (the three-launch form by up to 4x: f32 dgamma 4.1e-5 against 1.0e-5), the scalar form from mean / std = 1
    # on (1.5 - 2.5x in dx, cause not isolated); mean / std = 0.5 is the largest offset of the sweep at which all three pass, which
    # is the range include/jen1_train.h states.  The whole sweep: profiles/train_ops_parity.txt
    GnCase("f256-ratio0.5", 4, 64, 64, 19, 8, film="f", ratio=0.5, **_F256),
    GnCase("vec-ratio0.5", 2, 128, 128, 75, 8, film="f", ratio=0.5, **_V),
    GnCase("pad257-ratio0.5", 3, 257, 264, 40, 1, sums="scalar", film="f", ratio=0.5, **_S),
]
# groups of 2048 channels: the one-launch backward's LDS does not fit (host query only, never launched)
GN_CPG2048 = [GnCase("cpg2048-short", 32, 2048, 2048, 2, 1, fwd="vector", bwd="vector"),
              GnCase("cpg2048-long", 32, 2048, 2048, 8, 1, fwd="vector", bwd="vector")]

GN_FORWARD_Q = ("y", "sums")
GN_BACKWARD_Q = ("dx", "dgamma", "dbeta", "dfilm")


@functools.lru_cache(maxsize=None)
def gn_inputs(case: GnCase, mode: str):
    """float32 tensors as the kernel sees them (rounded to bf16 where it reads bf16), rows without padding"""
    B, C, L = case.B, case.C, case.L
    g = _gen(B, C, L, case.G, len(case.film), int(case.ratio * 10))
    sd = 1.5
    d = {"x": rounded(torch.randn((B, L, C), generator=g) * sd + sd * case.ratio, mode),
         "gamma": torch.randn((C,), generator=g), "beta": torch.randn((C,), generator=g) * 0.2,
         "dy": rounded(torch.randn((B, L, C), generator=g), mode),
         "film": rounded(torch.randn((B, case.film_ld), generator=g) * 0.5, mode) if case.film else None,
         "dx_add": rounded(torch.randn((B, L, C), generator=g), mode) if "a" in case.adds else None,
         "dx_add2": rounded(torch.randn((B, L, C), generator=g), mode) if "b" in case.adds else None,
         "dgamma0": torch.randn((C,), generator=g) * 3.0, "dbeta0": torch.randn((C,), generator=g) * 3.0}
    return d


def _silu_grad(f, fault=None):
    s = torch.sigmoid(f)
    return s if fault == "silu_no_term" else s * (1 + f * (1 - s))


def gn_emul(case: GnCase, d, dtype=torch.float32, fault=None):
    """GroupNorm -> FiLM -> SiLU and its backward, every operation in ``dtype``; returns y, sums, dx, dgamma, dbeta, dfilm [B][2C] and the
    root-sum-squares of the terms of every sum ('s:' entries).  ``fault``: one of the mistakes the gates must reject."""
    B, C, L, G, cpg = case.B, case.C, case.L, case.G, case.cpg
    c = lambda t: None if t is None else t.to(dtype)       # noqa: E731
    x, gamma, beta, dy, film = c(d["x"]), c(d["gamma"]), c(d["beta"]), c(d["dy"]), c(d["film"])
    xs = x
    if fault == "last_vec_next_group":                     # statistics: the last 8 channels of a group read from the next group
        w = min(8, cpg)
        xs = x.clone()
        for grp in range(G - 1):
            xs[:, :, (grp + 1) * cpg - w:(grp + 1) * cpg] = x[:, :, (grp + 2) * cpg - w:(grp + 2) * cpg]
    xg = xs.reshape(B, L, G, cpg)
    if fault == "skip_last_row":
        xg = xg[:, :L - 1]
    count = L * cpg - (1 if fault == "count_minus_1" else 0)
    s1, s2 = xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))
    mean = (s1 / count)[:, None, :, None]
    var = (((xg - mean) ** 2).sum(dim=(1, 3)) / count)[:, None, :, None]
    rstd = 1 / torch.sqrt(var + case.eps)
    if fault == "gamma_off_by_one":
        gamma = torch.roll(gamma, 1)
    xh = ((x.reshape(B, L, G, cpg) - mean) * rstd).reshape(B, L, C)
    n = xh * gamma + beta
    sc1 = film[:, None, :C] + 1 if film is not None else torch.ones((), dtype=dtype)
    sh = film[:, None, C:2 * C] if film is not None else torch.zeros((), dtype=dtype)
    f = n * sc1 + sh
    y = f * torch.sigmoid(f) if case.silu else f
    out = {"y": y, "sums": torch.stack([s1, s2], dim=-1),
           "s:sums": torch.stack([_rss(xg, (1, 3)), _rss(xg * xg, (1, 3))], dim=-1)}
    df = dy * _silu_grad(f, fault) if case.silu else dy
    dn = df * sc1
    out["dgamma"] = (dn * xh).sum(dim=(0, 1)) + (0 if fault == "dgamma_overwrite" else c(d["dgamma0"]))
    out["dbeta"] = dn.sum(dim=(0, 1)) + c(d["dbeta0"])
    out["s:dgamma"], out["s:dbeta"] = _rss(dn * xh, (0, 1)), _rss(dn, (0, 1))
    if film is not None:
        out["dfilm"] = torch.cat([(df * n).sum(dim=1), df.sum(dim=1)], dim=1)
        out["s:dfilm"] = torch.cat([_rss(df * n, 1), _rss(df, 1)], dim=1)
    dxh = (dn * gamma).reshape(B, L, G, cpg)
    xh4 = xh.reshape(B, L, G, cpg)
    m1 = dxh.sum(dim=(1, 3), keepdim=True) / (L * cpg)
    m2 = (dxh * xh4).sum(dim=(1, 3), keepdim=True) / (L * cpg)
    dx = (rstd * (dxh - m1 - xh4 * m2)).reshape(B, L, C)
    twice = fault == "dx_add_twice"                        # (the first one the case has)
    for k in ("dx_add", "dx_add2"):
        if d[k] is not None:
            dx = dx + c(d[k]) * (2 if twice else 1)
            twice = False
    out["dx"] = dx
    return out


@functools.lru_cache(maxsize=None)
def gn_ref(case: GnCase, mode: str):
    """float64: forward written out, backward by autograd; the scales of the metric"""
    B, C, L, G, cpg = case.B, case.C, case.L, case.G, case.cpg
    d = gn_inputs(case, mode)
    x, gamma, beta = (d[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    film = d["film"].double().requires_grad_() if case.film else None
    xg = x.reshape(B, L, G, cpg)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    h = ((xg - mean) / torch.sqrt(var + case.eps)).reshape(B, L, C) * gamma + beta
    if film is not None:
        h = h * (film[:, None, :C] + 1) + film[:, None, C:2 * C]
    y = h * torch.sigmoid(h) if case.silu else h
    (y * d["dy"].double()).sum().backward()
    man = gn_emul(case, d, torch.float64)
    dx = x.grad
    for k in ("dx_add", "dx_add2"):
        if d[k] is not None:
            dx = dx + d[k].double()
    unit = lambda t: torch.sqrt((t.reshape(B, L, G, cpg) ** 2).mean(dim=(1, 3), keepdim=True)).expand(B, L, G, cpg).reshape(B, L, C)   # noqa: E731
    y = y.detach()
    ref = {"y": y, "s:y": unit(y), "dx": dx, "s:dx": unit(dx),
           "sums": torch.stack([xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))], dim=-1).detach(), "s:sums": man["s:sums"],
           "dgamma": gamma.grad + d["dgamma0"].double(), "s:dgamma": man["s:dgamma"],
           "dbeta": beta.grad + d["dbeta0"].double(), "s:dbeta": man["s:dbeta"]}
    if film is not None:
        # (a FiLM gradient is a sum over t only -- one term at L = 1, where nothing damps an element next to the zero of SiLU': its
        # scale is also at least the RMS of its own group's FiLM gradients, scale and shift halves apart)
        df = film.grad[:, :2 * C]
        grp = torch.sqrt((df.reshape(B, 2, G, cpg) ** 2).mean(dim=3, keepdim=True)).expand(B, 2, G, cpg).reshape(B, 2 * C)
        ref["dfilm"], ref["s:dfilm"] = df, torch.maximum(man["s:dfilm"], grp)
    return ref


def gn_quantities(case):
    return [q for q in GN_FORWARD_Q + GN_BACKWARD_Q if q != "dfilm" or case.film]


def gn_is_fused(form):
    return form in ("fused256", "fused1024")


@functools.lru_cache(maxsize=None)
def gn_gates(case: GnCase, mode: str):
    ref, emul = gn_ref(case, mode), gn_emul(case, gn_inputs(case, mode))
    gates = {}
    for q in gn_quantities(case):
        f32_out = q in ("sums", "dgamma", "dbeta") or (q == "dfilm" and not case.mirror)
        form = case.fwd if q in GN_FORWARD_Q else case.bwd
        extra = GN_FUSED_BF16_EXTRA if (mode == BF16 and case.silu and gn_is_fused(form) and q != "sums") else 0.0
        least = sum_yard_least(case.L * case.cpg) if q == "sums" else 0.0
        gates[q] = capped(norm_gate(mode, metric(emul[q], ref[q], ref.get("s:" + q, 0.0)), f32_out, extra, least), ref, q, mode)
    return gates


FORM_NAMES = {0: "scalar", 1: "vector", 2: "fused256", 3: "fused1024"}
LN_BWD_NAMES = {0: "scalar256", 1: "scalar512", 2: "vector256", 3: "vector512"}


def gn_forms(lib, case: GnCase, ptr):
    """(jen1_gn_sums, jen1_gn_forward, jen1_gn_backward_add2) forms of the case for the addresses ptr[name]"""
    shape = (case.B, case.L, case.C, case.ld, case.G)
    film = ptr["film"] if case.film else None
    return (FORM_NAMES[lib.jen1_gn_sums_form(ptr["x"], *shape)],
            FORM_NAMES[lib.jen1_gn_forward_form(ptr["x"], ptr["gamma"], ptr["beta"], film, case.film_ld, ptr["y"], *shape)],
            FORM_NAMES[lib.jen1_gn_backward_form(ptr["dy"], ptr["x"], ptr["gamma"], ptr["beta"], film, case.film_ld, ptr["dx"], *shape)])


def gn_offsets(case: GnCase):
    """elements by which each tensor starts past a 16-byte boundary"""
    o = {k: 0 for k in ("x", "y", "dy", "dx", "gamma", "beta", "film")}
    if case.mis:
        o[case.mis] = 1
        if case.mis == "y":
            o["dx"] = 1
    return o


# =====================================================================================================================
# LayerNorm and the two LayerNorms of one input
# =====================================================================================================================
@dataclass(frozen=True)
class LnCase:
    name: str
    rows: int
    C: int
    ld: int
    fwd: str                  # scalar | vector
    bwd: str                  # scalar256 | scalar512 | vector256 | vector512
    add: bool = False         # dx_add
    dx_null: bool = False     # dx == NULL: only the column sums
    mis: bool = False         # x one element off a 16-byte boundary
    dual: bool = False        # jen1_ln2_forward / jen1_ln2_backward_add
    eps: float = 1e-5


LN_CASES = [
    LnCase("1x8", 1, 8, 8, "vector", "vector256"),
    LnCase("5x72", 5, 72, 72, "vector", "vector256", add=True),
    LnCase("5x72/dx-null", 5, 72, 72, "vector", "vector256", dx_null=True),
    LnCase("7x2048", 7, 2048, 2048, "vector", "scalar256"),
    LnCase("6x1176", 6, 1176, 1176, "vector", "scalar256", add=True),               # the first C whose 7 waves' sums pass 64 KB
    LnCase("3x65-ld72", 3, 65, 72, "scalar", "scalar256", add=True),
    LnCase("3x65-ld72/dx-null", 3, 65, 72, "scalar", "scalar256", dx_null=True),
    LnCase("600x40/x+1", 600, 40, 40, "scalar", "scalar512", add=True, mis=True),
    LnCase("600x40/x+1/dx-null", 600, 40, 40, "scalar", "scalar512", dx_null=True, mis=True),
    LnCase("600x128", 600, 128, 128, "vector", "vector512", add=True),
    LnCase("600x128/dx-null", 600, 128, 128, "vector", "vector512", dx_null=True),
    LnCase("255x128", 255, 128, 128, "vector", "vector256"),
    LnCase("256x128", 256, 128, 128, "vector", "vector512"),
    LnCase("300x64", 300, 64, 64, "vector", "vector512", add=True),                 # 32 blocks x 8 waves < 300 rows: waves loop
]
LN2_CASES = [LnCase(f"dual-{r}x{c}{'+add' if a else ''}", r, c, c, "vector", "vector256", add=a, dual=True)
             for r, c in ((1, 8), (5, 72), (130, 1024)) for a in (False, True)]


def ln_quantities(case: LnCase):
    q = ["y", "stats", "dgamma", "dbeta"] + ([] if case.dx_null else ["dx"])
    return q + ["y2", "dgamma2", "dbeta2"] if case.dual else q


@functools.lru_cache(maxsize=None)
def ln_inputs(case: LnCase, mode: str):
    R, C = case.rows, case.C
    g = _gen(R, C, int(case.dual), 7)
    d = {"x": rounded(torch.randn((R, C), generator=g) * 2 + 0.5, mode), "dy": rounded(torch.randn((R, C), generator=g), mode),
         "gamma": torch.randn((C,), generator=g), "beta": torch.randn((C,), generator=g) * 0.2,
         "dx_add": rounded(torch.randn((R, C), generator=g), mode) if case.add else None,
         "dgamma0": torch.randn((C,), generator=g) * 3.0, "dbeta0": torch.randn((C,), generator=g) * 3.0}
    if case.dual:
        d.update({"dy2": rounded(torch.randn((R, C), generator=g), mode), "gamma2": torch.randn((C,), generator=g),
                  "beta2": torch.randn((C,), generator=g) * 0.2, "dgamma20": torch.randn((C,), generator=g) * 3.0,
                  "dbeta20": torch.randn((C,), generator=g) * 3.0})
    return d


def ln_emul(case: LnCase, d, dtype=torch.float32, fault=None):
    C = case.C
    c = lambda t: None if t is None else t.to(dtype)       # noqa: E731
    x, dy, gamma, beta = c(d["x"]), c(d["dy"]), c(d["gamma"]), c(d["beta"])
    count = C - (1 if fault == "count_minus_1" else 0)
    mean = x.sum(dim=1, keepdim=True) / count
    rstd = 1 / torch.sqrt(((x - mean) ** 2).sum(dim=1, keepdim=True) / count + case.eps)
    xh = (x - mean) * rstd
    gidx = torch.roll(gamma, 1) if fault == "gamma_off_by_one" else gamma
    out = {"y": xh * gidx + beta, "stats": torch.cat([mean, rstd], dim=1),
           "s:stats": torch.cat([_rss(x, 1)[:, None] / C, torch.zeros_like(rstd)], dim=1)}
    rows = slice(0, case.rows - 1) if fault == "skip_last_row" else slice(None)
    out["dgamma"] = (dy * xh)[rows].sum(dim=0) + (0 if fault == "dgamma_overwrite" else c(d["dgamma0"]))
    out["dbeta"] = dy[rows].sum(dim=0) + c(d["dbeta0"])
    out["s:dgamma"], out["s:dbeta"] = _rss(dy * xh, 0), _rss(dy, 0)
    dh = dy * gidx
    if case.dual:
        dy2, gamma2 = c(d["dy2"]), c(d["gamma2"])
        out["y2"] = xh * gamma2 + c(d["beta2"])
        out["dgamma2"], out["dbeta2"] = (dy2 * xh).sum(dim=0) + c(d["dgamma20"]), dy2.sum(dim=0) + c(d["dbeta20"])
        out["s:dgamma2"], out["s:dbeta2"] = _rss(dy2 * xh, 0), _rss(dy2, 0)
        dh = dh + dy2 * gamma2
    dx = rstd * (dh - dh.sum(dim=1, keepdim=True) / C - xh * ((dh * xh).sum(dim=1, keepdim=True) / C))
    if d["dx_add"] is not None:
        dx = dx + c(d["dx_add"]) * (2 if fault == "dx_add_twice" else 1)
    out["dx"] = dx
    return out


@functools.lru_cache(maxsize=None)
def ln_ref(case: LnCase, mode: str):
    d = ln_inputs(case, mode)
    names = ("x", "gamma", "beta") + (("gamma2", "beta2") if case.dual else ())
    v = {k: d[k].double().requires_grad_() for k in names}
    x = v["x"]
    mean = x.mean(dim=1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mean) ** 2).mean(dim=1, keepdim=True) + case.eps)
    xh = (x - mean) * rstd
    y = xh * v["gamma"] + v["beta"]
    loss = (y * d["dy"].double()).sum()
    if case.dual:
        y2 = xh * v["gamma2"] + v["beta2"]
        loss = loss + (y2 * d["dy2"].double()).sum()
    loss.backward()
    man = ln_emul(case, d, torch.float64)
    row = lambda t: torch.sqrt((t * t).mean(dim=1, keepdim=True)).expand_as(t)       # noqa: E731
    dx = x.grad if d["dx_add"] is None else x.grad + d["dx_add"].double()
    ref = {"y": y.detach(), "s:y": row(y.detach()), "dx": dx, "s:dx": row(dx),
           "stats": torch.cat([mean, rstd], dim=1).detach(), "s:stats": man["s:stats"],
           "dgamma": v["gamma"].grad + d["dgamma0"].double(), "dbeta": v["beta"].grad + d["dbeta0"].double(),
           "s:dgamma": man["s:dgamma"], "s:dbeta": man["s:dbeta"]}
    if case.dual:
        ref.update({"y2": y2.detach(), "s:y2": row(y2.detach()), "dgamma2": v["gamma2"].grad + d["dgamma20"].double(),
                    "dbeta2": v["beta2"].grad + d["dbeta20"].double(), "s:dgamma2": man["s:dgamma2"], "s:dbeta2": man["s:dbeta2"]})
    return ref


@functools.lru_cache(maxsize=None)
def ln_gates(case: LnCase, mode: str):
    ref, emul = ln_ref(case, mode), ln_emul(case, ln_inputs(case, mode))
    return {q: capped(norm_gate(mode, metric(emul[q], ref[q], ref.get("s:" + q, 0.0)), f32_output=q not in ("y", "y2", "dx")), ref, q, mode)
            for q in ln_quantities(case)}


def ln_forms(lib, case: LnCase, ptr):
    """(jen1_ln_forward, jen1_ln_backward_add) forms; dx and dx_add are NULL where the case passes none"""
    dx = None if case.dx_null else ptr["dx"]
    add = ptr["dx_add"] if case.add else None
    return (FORM_NAMES[lib.jen1_ln_forward_form(ptr["x"], ptr["gamma"], ptr["beta"], ptr["y"], case.rows, case.C, case.ld)],
            LN_BWD_NAMES[lib.jen1_ln_backward_form(ptr["dy"], ptr["x"], ptr["gamma"], dx, add, case.rows, case.C, case.ld)])


# =====================================================================================================================
# activations
# =====================================================================================================================
ACT_NAMES = {0: "gelu", 1: "silu", 2: "elu"}
ACT_WRAP_SCALAR = 256 * 32 * 256 + 1          # one element more than the grid cap's threads (odd: the scalar form)
ACT_WRAP_VECTOR = 8 * (256 * 32 * 256 + 1)    # ... 8-element vectors (SiLU only: the loop does not depend on the mode)
# (n, elements x / dy / dx start past a 16-byte boundary, the form)
ACT_CASES = [(1, 0, "scalar"), (7, 0, "scalar"), (8, 0, "vector"), (4999, 0, "scalar"), (5000, 0, "vector"), (5000, 1, "scalar"),
             (ACT_WRAP_SCALAR, 0, "scalar")]
ACT_SPECIALS = [0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, -1.278, 1.0, -5.0]       # the edges of expf / expm1f / erff; silu' = 0 near -1.278


@functools.lru_cache(maxsize=None)
def act_inputs(n: int, mode: str):
    g = _gen(n, 3)
    x = torch.randn((n,), generator=g) * 3.0
    sp = torch.tensor(ACT_SPECIALS)
    k = min(n, len(sp))
    x[n - k:] = sp[:k]                         # (at the END: the tail of the last block and of the last vector)
    return rounded(x, mode), rounded(torch.randn((n,), generator=g) + 0.25, mode)


def act_emul(mode_id: int, x, dy, dtype=torch.float32, fault=None):
    """(y, dx) with every operation in ``dtype``, term by term as the kernels write them"""
    x, dy = x.to(dtype), dy.to(dtype)
    if mode_id == 0:
        cdf = 0.5 * (1 + torch.erf(x * 0.70710678118654752440))
        return 0.5 * x * (1 + torch.erf(x * 0.70710678118654752440)), dy * (cdf + x * (0.39894228040143267794 * torch.exp(-0.5 * x * x)))
    if mode_id == 1:
        return x / (1 + torch.exp(-x)), dy * _silu_grad(x, fault)
    return torch.where(x > 0, x, torch.expm1(x)), dy * torch.where(x > 0, torch.ones_like(x), torch.exp(x))


@functools.lru_cache(maxsize=None)
def act_ref(mode_id: int, n: int, mode: str):
    """float64 (y, dx = autograd) and the absolute floors of the metric: the size of the terms that cancel in an element.
    GELU: x/2 + (x/2) erf(x / sqrt 2) -- for x < 0 two terms of |x| / 2 nearly cancel; its derivative cdf + x pdf likewise
    (1/2 + erf/2 and x pdf).  SiLU': s (1 + x (1 - s)) passes through 0 at x = -1.278: the terms are s and s |x| (1 - s).
    SiLU, ELU and ELU' are products and quotients of positive terms: nothing cancels, the floor is 0."""
    x, dy = act_inputs(n, mode)
    xr = x.double().requires_grad_()
    if mode_id == 0:
        y = 0.5 * xr * (1 + torch.erf(xr / math.sqrt(2.0)))
    elif mode_id == 1:
        y = xr / (1 + torch.exp(-xr))
    else:
        y = torch.where(xr > 0, xr, torch.expm1(xr))
    # (autograd differentiates expm1 as result + 1, which is 0 below x = -37: ELU's gradient comes from the same function written
    # exp(x) - 1, whose derivative autograd takes as exp(x))
    ((torch.where(xr > 0, xr, torch.exp(xr) - 1) if mode_id == 2 else y) * dy.double()).sum().backward()
    xd, dd = x.double(), dy.double().abs()
    zero = torch.zeros_like(xd)
    if mode_id == 0:
        pdf = torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
        fy, fdx = xd.abs() / 2, dd * (0.5 + xd.abs() * pdf)
    elif mode_id == 1:
        s = torch.sigmoid(xd)
        fy, fdx = zero, dd * s * (1 + xd.abs() * (1 - s))
    else:
        fy, fdx = zero, zero
    return {"y": y.detach(), "dx": xr.grad, "s:y": fy, "s:dx": fdx}


# Gates of the pointwise kernels, in float32 roundings (2^-24 each, relative to the element's terms; a correctly rounded operation
# costs 1, a library function its documented ulp bound x 2: expf 1 ulp, expm1f 1 ulp, erff 2 ulp; hipcc divides with IEEE rounding):
#   GELU  y  = 0.5 x (1 + erf(x c)):   x c 1, its effect on erf <= 1 (|t erf'(t)| <= 0.5 erf's scale), erff 4, the sum 1, two products 2   ->  9
#   GELU  dx = dy (cdf + x pdf):       cdf as above 7, x x 1 and its product 1 (|u| e^-u <= 0.37: under 1 through exp), expf 2,
#                                      two products 2, the sum 1, dy . 1                                                                 -> 16
#   SiLU  y  = x / (1 + exp(-x)):      expf 2, the sum 1, the division 1                                                                 ->  4
#   SiLU  dx = dy s (1 + x (1 - s)):   s 4, 1 - s 1 (+ s's 4: within the floor's terms), the product 1, the sum 1, two products 2       -> 13
#   ELU   y  = expm1(x):  2;   ELU dx = dy exp(x):  expf 2, the product 1                                                                ->  2, 3
ACT_ROUNDINGS = {(0, "y"): 9, (0, "dx"): 16, (1, "y"): 4, (1, "dx"): 13, (2, "y"): 2, (2, "dx"): 3}


def act_gates(mode_id: int, mode: str):
    return {q: out_rounding(mode) + ACT_ROUNDINGS[(mode_id, q)] * U24 for q in ("y", "dx")}


# =====================================================================================================================
# softmax over keys
# =====================================================================================================================
# (Z, Nq, Nk, ld_s, ld_p, causal)
SOFTMAX_CASES = [(2, 1, 1, 1, 8, 0), (3, 7, 7, 7, 8, 0), (3, 7, 7, 7, 8, 1), (2, 5, 129, 136, 136, 0), (2, 6, 65, 65, 72, 0),
                 (2, 6, 65, 65, 72, 1), (1, 24, 24, 32, 24, 0), (1, 24, 24, 32, 24, 1)]


@functools.lru_cache(maxsize=None)
def softmax_inputs(case, mode: str):
    Z, Nq, Nk, ld_s, ld_p, causal = case
    g = _gen(*case)
    s = torch.randn((Z * Nq, Nk), generator=g) * 2.0
    if Nk > 1:                                  # the last row: scores near +80 and -80 (nothing but the max-subtraction keeps exp finite)
        s[-1] = torch.where(torch.arange(Nk) % 2 == 0, 80.0, -80.0) + torch.randn((Nk,), generator=g)
    return s, torch.randn((Z * Nq, Nk), generator=g)


def softmax_keep(case, off=0):
    Z, Nq, Nk, ld_s, ld_p, causal = case
    i = torch.arange(Z * Nq) % Nq
    j = torch.arange(Nk)
    return (j[None, :] <= i[:, None] + (Nk - Nq) + off) if causal else torch.ones((Z * Nq, Nk), dtype=torch.bool)


def softmax_emul(case, s, dtype=torch.float32, fault=None):
    """p with every operation in ``dtype``"""
    keep = softmax_keep(case, -1 if fault == "causal_off_by_one" else 0)
    s = s.to(dtype)
    m = torch.where(keep, s, torch.full_like(s, -3.0e38)).max(dim=1, keepdim=True).values
    e = torch.where(keep, torch.exp(s - m), torch.zeros_like(s))
    return e * (1 / e.sum(dim=1, keepdim=True))


def softmax_bwd_emul(p, dp, dtype=torch.float32):
    p, dp = p.to(dtype), dp.to(dtype)
    return p * (dp - (p * dp).sum(dim=1, keepdim=True))


@functools.lru_cache(maxsize=None)
def softmax_ref(case, mode: str):
    """float64 p = softmax over the kept keys.  The backward kernel reads p as the forward stored it, so ``p_in`` is p rounded to the
    mode's dtype and ``ds`` the kernel's contract ds = p (dp - sum_j dp p) in float64 on that p_in; ``ds_autograd`` is autograd on
    the softmax itself (equal to the contract on the unrounded p: pinned on the host)"""
    s, dp = softmax_inputs(case, mode)
    keep = softmax_keep(case)
    sr = s.double().requires_grad_()
    p = torch.softmax(torch.where(keep, sr, torch.full_like(sr, -math.inf)), dim=1)
    (p * dp.double()).sum().backward()
    row = lambda t: torch.sqrt((t * t).mean(dim=1, keepdim=True)).expand_as(t)       # noqa: E731
    p_in = rounded(p.detach(), mode)
    ds = softmax_bwd_emul(p_in, dp, torch.float64)
    return {"p": p.detach(), "s:p": row(p.detach()), "p_in": p_in, "ds": ds, "s:ds": row(ds), "ds_autograd": sr.grad}


# Gates, in float32 roundings (2^-24) relative to the metric's denominator |ref| + rms(row):
#   p_j = exp(s_j - m) / z:  the difference 1, whose absolute error |s_j - m| 2^-24 passes through exp as (m - s_j) e^-(m - s_j)
#     <= 0.37 of the row's largest entry: 1;  expf 2 (1 ulp);  z is a sum of Nk positive terms that carry those 4 each, added in
#     log2(64) = 6 lane steps and Nk / 64 serial ones: 4 + 6 + Nk / 64;  the reciprocal 1, the product 1            -> 16 + Nk / 64
#   ds_j = p_j (dp_j - d), d = sum_j p_j dp_j:  d's products 1 and its tree 6 + Nk / 64, an ABSOLUTE error relative to
#     sum_j |p_j dp_j|, which reaches ds_j multiplied by p_j; the difference 1 and the product 1 are relative to |ds_j|.  Against the
#     denominator: 2 + (7 + Nk / 64) A, A = max over the rows of max_j p_j sum_j |p_j dp_j| / rms_j(ds), a property of the inputs
#     (computed from the float64 reference; rows whose ds is exactly 0 -- one kept key: p = 1, d = dp -- have no error at all)
def softmax_gates(case, mode: str):
    Z, Nq, Nk, ld_s, ld_p, causal = case
    ref = softmax_ref(case, mode)
    _, dp = softmax_inputs(case, mode)
    p = ref["p_in"].double()
    rms = torch.sqrt((ref["ds"] ** 2).mean(dim=1))
    a = torch.where(rms > 0, p.max(dim=1).values * (p * dp.double()).abs().sum(dim=1) / rms.clamp_min(FLOOR), torch.zeros_like(rms))
    return {"p": out_rounding(mode) + (16 + Nk / 64) * U24, "ds": out_rounding(mode) + (2 + (7 + Nk / 64) * float(a.max())) * U24}
