"""A float64 model of jen1_train_gemm's descriptor (include/jen1_train.h), the case table of its kernel forms and the builder of their
buffers; importable without a GPU.  tests/test_train_gemm_refs_host.py pins the model against torch; tests/test_gpu_train_gemm_forms.py
runs the cases on the kernel.

The model is written from the words of the header, not from csrc/train_gemm.hip: the operand address rule, the index map (mul, tapmul,
shift, div, the validity test, reflect, map_shift_b), taps_in_z and the C address rule, alpha, bias, accumulate / atomic, residual and
rowsum.  It works on flat host buffers; an operand's ``p`` is an element offset into its buffer.  For every C element it gives the
float64 result and the float64 sum of magnitudes S = |alpha| sum |a||b| + |bias| + |old C| + |residual| the gate is scaled by.

Buffers (``Built``): every operand lies inside a larger allocation with GUARD elements (>= 256 bytes) on either side; the guards and
every element the descriptor does not address -- columns k >= K up to the pitch, rows beyond M or N, the gaps between heads and taps --
are NaN, so a read the contract does not allow poisons the result.  C lies the same way inside a finite pattern that must come back bit
for bit wherever the call may not write.  Values are drawn in float32 and rounded to the storage dtype before the model sees them: what is
left between model and kernel is the float32 accumulation and the rounding of the output.

The gate, per element (derived, not fitted): |got - ref| <= c (n 2^-24 S + r |ref|) with n = taps K + splitk + 3, r = 2^-8 for a bf16 C
and 0 otherwise, c = 4.  bf16 products are exact in float32, a float32 sum of n terms in any order errs by at most n u S, the output is
rounded once; the factor 4 is margin for the matrix instructions' internal summation.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from helpers import ROOT  # noqa: F401  (puts the package on sys.path)
from jen1_amd import lib as L
from jen1_amd.gemm_host import ConvGeom, Map, operand

U24, U8 = 2.0 ** -24, 2.0 ** -8
GATE_C = 4.0
GUARD = 128                              # elements on either side of every buffer: 256 bytes in bf16, 512 in float32
F32, BF16 = "f32", "bf16"
MODES = [F32, BF16]
D, TALL, FASTW, SKINNY, LEAN = L.GEMM_DIRECT, L.GEMM_TALL, L.GEMM_FASTW, L.GEMM_SKINNY, L.GEMM_LEAN


def skinny_form(waves):
    return D | SKINNY | (waves << L.GEMM_WAVES_SHIFT)


def form_name(form):
    if form < 0:
        return "refused"
    names = [n for bit, n in ((D, "direct"), (TALL, "tall"), (FASTW, "fastw"), (SKINNY, "skinny"), (LEAN, "lean")) if form & bit]
    if form & SKINNY:
        names.append(f"{form >> L.GEMM_WAVES_SHIFT}waves")
    return "+".join(names) or "staged"


# =====================================================================================================================
# the model
# =====================================================================================================================
def map_index(op, idx, tap, shift_b=None):
    """the index map of jen1_gemm_operand along its mapped axis: indices ``idx`` (int array) -> (mapped index, valid)"""
    b, t = np.divmod(np.asarray(idx, dtype=np.int64), op.map_L)
    shift = np.asarray(shift_b, dtype=np.int64)[b] if op.reserved == 1 else op.map_shift
    s = t * op.map_mul + tap * op.map_tapmul + shift
    if op.map_reflect:
        s = np.where(s < 0, -s, s)
        s = np.where(s >= op.map_Lsrc, 2 * (op.map_Lsrc - 1) - s, s)
    ok = np.ones(s.shape, dtype=bool)
    if op.map_div > 1:
        ok &= s % op.map_div == 0
        s = s // op.map_div
    ok &= (s >= 0) & (s < op.map_Lsrc)
    return b * op.map_Lsrc + s, ok


def operand_offsets(op, rows, K, taps, batches, shift_b=None):
    """element offsets [batches][taps][rows][K] into the operand's flat buffer and which of them the product reads (the others read as 0)"""
    z = np.arange(batches, dtype=np.int64)
    base = (op.p or 0) + (z // op.zdiv) * op.zs0 + (z % op.zdiv) * op.zs1
    r, k = np.arange(rows, dtype=np.int64), np.arange(K, dtype=np.int64)
    off = np.empty((batches, taps, rows, K), dtype=np.int64)
    ok = np.empty((batches, taps, rows, K), dtype=bool)
    for tap in range(taps):
        R, okr = (map_index(op, r, tap, shift_b) if op.map_axis == 1 else (r, np.ones(rows, dtype=bool)))
        Kk, okk = (map_index(op, k, tap, shift_b) if op.map_axis == 2 else (k, np.ones(K, dtype=bool)))
        off[:, tap] = base[:, None, None] + tap * op.tap_stride + R[None, :, None] * op.ld_r + Kk[None, None, :] * op.ld_k
        ok[:, tap] = okr[:, None] & okk[None, :]
    return off, ok


def c_offsets(g, c_p=0):
    """element offsets [batches][taps or 1][M][N] of the C elements the call stores"""
    z = np.arange(g["batches"], dtype=np.int64)
    base = c_p + (z // g.get("c_zdiv", 1)) * g.get("c_zs0", 0) + (z % g.get("c_zdiv", 1)) * g.get("c_zs1", 0)
    tap = np.arange(g["taps"] if g.get("taps_in_z") else 1, dtype=np.int64) * g.get("c_tap_stride", 0)
    m = np.arange(g["M"], dtype=np.int64) * g["ldc_m"]
    n = np.arange(g["N"], dtype=np.int64) * g.get("ldc_n", 1)
    return base[:, None, None, None] + tap[None, :, None, None] + m[None, None, :, None] + n[None, None, None, :]


def _gather(buf, off, ok):
    v = np.where(ok, np.asarray(buf, dtype=np.float64)[np.where(ok, off, 0)], 0.0)
    assert np.isfinite(v).all(), "the model read an element outside what the builder filled"
    return v


def gemm_model(a, b, A, B, C, g, bias=None, residual=None, rowsum=None, shift_b=None, c_p=0):
    """``a`` / ``b``: jen1_gemm_operand mirrors whose ``p`` is an element offset into the flat arrays ``A`` / ``B``; ``C`` (``residual``):
    the flat C buffer before the call with C's element 0 at ``c_p``; ``g``: M, N, K and the keyword arguments of GemmRuntime.gemm.
    Returns {"c": the float64 C buffer after the call, "S": the magnitude sums (0 where nothing is stored), "touched": where the call
    stores, "rowsum", "rowsum_S"}."""
    M, N, K, taps, batches = g["M"], g["N"], g["K"], g.get("taps", 1), g.get("batches", 1)
    g = dict(g, taps=taps, batches=batches)
    alpha = float(np.float32(g.get("alpha", 1.0)))          # the descriptor's alpha is a float
    oa, ka = operand_offsets(a, M, K, taps, batches, shift_b)
    ob, kb = operand_offsets(b, N, K, taps, batches, shift_b)
    Av, Bv = _gather(A, oa, ka), _gather(B, ob, kb)
    prod = np.einsum("ztmk,ztnk->ztmn", Av, Bv)
    mag = np.einsum("ztmk,ztnk->ztmn", np.abs(Av), np.abs(Bv))
    if not g.get("taps_in_z"):
        prod, mag = prod.sum(1, keepdims=True), mag.sum(1, keepdims=True)
    val, S = alpha * prod, abs(alpha) * mag
    if bias is not None:
        bv = np.asarray(bias, dtype=np.float64)[:N]
        val, S = val + bv, S + np.abs(bv)
    oc = c_offsets(g, c_p)
    assert np.unique(oc).size == oc.size, "two output elements share an address"
    out = np.array(C, dtype=np.float64)
    if g.get("accumulate") or g.get("atomic"):
        val, S = val + out[oc], S + np.abs(out[oc])
    if residual is not None:
        rv = np.asarray(residual, dtype=np.float64)[oc]
        val, S = val + rv, S + np.abs(rv)
    assert np.isfinite(val).all()
    out[oc] = val
    Sf = np.zeros(out.shape)
    Sf[oc] = S
    touched = np.zeros(out.shape, dtype=bool)
    touched[oc] = True
    res = {"c": out, "S": Sf, "touched": touched}
    if rowsum is not None:
        old = np.asarray(rowsum, dtype=np.float64)
        res["rowsum"] = old + alpha * Av[:, 0].sum(axis=(0, 2))
        res["rowsum_S"] = np.abs(old) + abs(alpha) * np.abs(Av[:, 0]).sum(axis=(0, 2))
    return res


def gate(ref, S, n, c_bf16, c=GATE_C):
    """the per-element bound of the module docstring"""
    return c * (n * U24 * S + (U8 if c_bf16 else 0.0) * np.abs(ref))


def gate_terms(g):
    return g.get("taps", 1) * g["K"] + g.get("splitk", 1) + 3


# =====================================================================================================================
# the cases
# =====================================================================================================================
@dataclass
class Opnd:
    """what gemm_host.operand takes besides the pointer; ``off``: elements the operand's base lies behind the 16-byte aligned start"""
    ld_r: int
    ld_k: int
    tap_stride: int = 0
    zs0: int = 0
    zs1: int = 0
    zdiv: int = 1
    m: Optional[Map] = None
    off: int = 0

    def desc(self, p):
        return operand(p, self.ld_r, self.ld_k, self.tap_stride, self.zs0, self.zs1, self.zdiv, self.m)


@dataclass
class Case:
    group: str                  # the form family the parity file lists the case under
    name: str
    form: object                # the expected jen1_train_gemm_form: an int, or {mode: int}
    M: int
    N: int
    K: int
    a: Opnd
    b: Opnd
    ldc_m: int
    modes: tuple = (F32, BF16)
    shift_b: Optional[list] = None
    bias: bool = False
    residual: bool = False
    rowsum: bool = False
    kw: dict = field(default_factory=dict)      # the other keyword arguments of GemmRuntime.gemm

    @property
    def id(self):
        return f"{self.group}.{self.name}"

    def expected_form(self, mode):
        return self.form[mode] if isinstance(self.form, dict) else self.form

    def scalars(self):
        return dict(M=self.M, N=self.N, K=self.K, ldc_m=self.ldc_m, **self.kw)


def _conv(kind, taps, stride, L_in, L_out, causal=False, reflect=False, per_batch=None):
    """ConvGeom of a _Conv1d (pad (k - 1) / 2, or k - 1 on the left when causal), with ``per_batch`` = the causal flag of every clip"""
    pad = taps - 1 if causal else (taps - 1) // 2
    pad_b = None
    if per_batch is not None:
        neg = torch.tensor([-(taps - 1) if c else -((taps - 1) // 2) for c in per_batch], dtype=torch.int32)
        pad_b = (neg, -neg)
    return ConvGeom(kind, taps, stride, pad, L_in, L_out, 8, 8, reflect=reflect, pad_b=pad_b)


def _fwd_case(group, name, form, K, *, stride=1, taps=3, causal=False, reflect=False, per_batch=None, N=72, f32_tight=False, Lo=37, nb=2,
              skinny=False, **over):
    """forward convolution: A = the activation rows [nb][L_in][pitch] mapped along the rows, B = the weight [tap][N][ldb]"""
    L_in = Lo * stride
    g = _conv("conv", taps, stride, L_in, Lo, causal, reflect, per_batch)
    lda, ldb = (K + 4, K) if f32_tight else (K + 8, K + 8)
    kw = dict(taps=taps, skinny=skinny)
    shift = None
    if per_batch is not None:
        shift = g.fwd_shift_b.tolist() + [g.fwd_shift_b.tolist()[0]]      # one entry more than there are batch elements
    fields = dict(modes=(F32,) if f32_tight else (F32, BF16), shift_b=shift)
    for k in ("bias", "residual", "modes"):
        if k in over:
            fields[k] = over.pop(k)
    kw.update(over)
    return Case(group, name, form, nb * Lo, N, K, Opnd(lda, 1, m=g.fwd_map(1)), Opnd(ldb, 1, tap_stride=N * ldb), ldc_m=N + 8, kw=kw, **fields)


def _wgrad_case(group, name, form, M, N, K, g: Optional[ConvGeom], taps, modes, shift_b=None, rowsum=False, **over):
    """weight gradient: A = dY [K][lda] and B = the layer's input [rows][ldb], both with contiguous rows, B mapped along k;
    one matrix per tap, C float32 laid out [M][N][tap]"""
    kw = dict(taps=taps, taps_in_z=True, ldc_n=taps, c_tap_stride=1, c_f32=True)
    kw.update(over)
    m = None if g is None else g.fwd_map(2)
    return Case(group, name, form, M, N, K, Opnd(1, M), Opnd(1, N, m=m), ldc_m=N * taps, modes=modes, shift_b=shift_b, rowsum=rowsum, kw=kw)


def _cases():
    cs = []
    # ---- staged body --------------------------------------------------------------------------------------------------
    cs.append(Case("staged", "pv-65x33x70", 0, 65, 33, 70, Opnd(72, 1), Opnd(1, 40), ldc_m=40))        # A k-contiguous, B row-contiguous (P V)
    wg = _conv("conv", 3, 1, 37, 37)
    for name, over, rs in (("store", {}, False), ("rowsum-accumulate", dict(accumulate=True), True),
                           ("rowsum-splitk3", dict(atomic=True, splitk=3), True), ("splitk4-empty-slice", dict(atomic=True, splitk=4), False)):
        cs.append(_wgrad_case("staged", "wgrad-72x40x74." + name, 0, 72, 40, 74, wg, 3, (F32,), rowsum=rs, **over))
    for K in (5, 1):
        cs.append(Case("staged", f"K{K}", 0, 65, 33, K, Opnd(8, 1), Opnd(8, 1), ldc_m=40))
    cs.append(Case("staged", "base-off-by-one", 0, 65, 33, 70, Opnd(72, 1, off=1), Opnd(72, 1, off=1), ldc_m=40))     # the scalar fallback of fetch
    # ---- the bf16 weight-gradient loop ----------------------------------------------------------------------------------
    fw = dict(M=136, N=24, K=74, modes=(BF16,))
    cs.append(_wgrad_case("fastw", "unmapped.rowsum", FASTW, g=None, taps=1, rowsum=True, accumulate=True, alpha=0.5, **fw))
    cs.append(_wgrad_case("fastw", "mul2", FASTW, g=_conv("conv", 3, 2, 74, 37), taps=3, **fw))
    cs.append(_wgrad_case("fastw", "div2", FASTW, g=ConvGeom("convT", 4, 2, 1, 19, 37, 8, 8), taps=4, rowsum=True, accumulate=True, **fw))
    pb = _conv("conv", 3, 1, 37, 37, per_batch=[False, True])
    cs.append(_wgrad_case("fastw", "per-batch-shifts", FASTW, g=pb, taps=3, shift_b=pb.fwd_shift_b.tolist() + [-1], accumulate=True, alpha=-1.5, **fw))
    for rs in (True, False):
        cs.append(_wgrad_case("fastw", f"K300-splitk2{'.rowsum' if rs else ''}", FASTW, 136, 24, 300, _conv("conv", 3, 1, 100, 100), 3, (BF16,),
                              rowsum=rs, atomic=True, splitk=2, alpha=0.75))
    # ---- register-direct, the lean kernel ---------------------------------------------------------------------------------
    maps = (("stride1", {}), ("stride2", dict(stride=2)), ("stride4", dict(stride=4, taps=5)), ("causal", dict(causal=True)),
            ("reflect7", dict(taps=7, reflect=True)), ("per-batch", dict(per_batch=[True, False])))
    for mname, mk in maps:
        for K in (40, 96):
            cs.append(_fwd_case("direct-lean", f"{mname}.K{K}", D | LEAN, K, **mk))
        for K in (4, 12, 36):           # float32, K % 8 == 4: the last fragment has no upper half; B's rows K apart, A's K + 4
            cs.append(_fwd_case("direct-lean", f"{mname}.K{K}.tight", D | LEAN, K, f32_tight=True, **mk))
    dg = _conv("conv", 3, 2, 37, 19)        # the data gradient of a stride-2 convolution: rows of dx from rows of dy
    cs.append(Case("direct-lean", "dgrad-div2", D | LEAN, 74, 72, 40, Opnd(48, 1, m=dg.bwd_map(1)), Opnd(48, 1, tap_stride=72 * 48), ldc_m=80,
                   kw=dict(taps=3)))
    cs.append(_fwd_case("direct-lean", "bias.alpha", D | LEAN, 40, bias=True, alpha=0.375))
    cs.append(_fwd_case("direct-lean", "residual", D | LEAN, 40, residual=True))
    cs.append(_fwd_case("direct-lean", "accumulate", D | LEAN, 40, accumulate=True))
    for d in (16, 12):                      # Q K^T of the attention GEMM path: 2 x 3 heads side by side in rows of 3 d channels
        C3, Nq, Nk = 3 * d, 37, 40
        cs.append(Case("direct-lean", f"attention-d{d}", {F32: D | LEAN, BF16: (D | LEAN) if d % 8 == 0 else 0}, Nq, Nk, d,
                       Opnd(C3, 1, zs0=Nq * C3, zs1=d, zdiv=3), Opnd(C3, 1, zs0=Nk * C3, zs1=d, zdiv=3), ldc_m=Nk,
                       kw=dict(batches=6, c_zs0=Nq * Nk, c_f32=True, alpha=d ** -0.5)))
    # ---- register-direct, the full kernel (float32 read-modify-write of C) --------------------------------------------------
    cs.append(_fwd_case("direct-full", "c_f32-accumulate", D, 40, c_f32=True, accumulate=True))
    # (split-K with atomics has no read-modify-write of its own: it runs the lean kernel; the bias must land once)
    cs.append(_fwd_case("direct-full", "splitk2-bias", D | LEAN, 40, c_f32=True, atomic=True, splitk=2, bias=True))
    # ---- tall -------------------------------------------------------------------------------------------------------------
    for N in (1, 8, 32, 33):
        cs.append(Case("tall", f"130x{N}x40", (D | TALL | LEAN) if N <= 32 else (D | LEAN), 130, N, 40, Opnd(48, 1), Opnd(48, 1), ldc_m=N + 3))
    # ---- skinny -------------------------------------------------------------------------------------------------------------
    # (taps, K): 3, 47, 48, 63, 64 and 96 steps of 32 -- either side of the switches to 8 and to 16 waves -- and 7 taps of one step,
    # where one stride of a wave's walk crosses several taps.  N <= 32 is a narrow output: the tall layout takes it whatever the
    # caller prefers ("ignored when the operands do not allow it"), so those cases pin that; N = 33 has a last tile of one column.
    for taps, K, waves in ((3, 32, 4), (1, 1504, 4), (3, 512, 8), (3, 672, 8), (1, 2048, 16), (3, 1024, 16), (7, 32, 4)):
        for M in (1, 33):
            for N in (16, 17, 33, 40):
                form = skinny_form(waves) if N > 32 else D | TALL | LEAN
                cs.append(Case("skinny", f"{M}x{N}.{taps}x{K}", form, M, N, K, Opnd(K + 8, 1, tap_stride=M * (K + 8)),
                               Opnd(K, 1, tap_stride=N * K), ldc_m=N + 8, kw=dict(taps=taps, skinny=True)))
    for K in (36, 100):                     # float32, K % 8 == 4 in the skinny walk: the same half fragment as on the lean kernel
        cs.append(Case("skinny", f"33x40.3x{K}.tight", skinny_form(4), 33, 40, K, Opnd(K + 4, 1, tap_stride=33 * (K + 4)),
                       Opnd(K, 1, tap_stride=40 * K), ldc_m=48, modes=(F32,), kw=dict(taps=3, skinny=True)))
    cs.append(_fwd_case("skinny", "rows-mapped.L6x4", skinny_form(8), 512, Lo=6, nb=4, N=40, skinny=True))
    sk = dict(Lo=11, nb=3, N=40, skinny=True)       # 33 rows, 3 x 512: 48 steps
    cs.append(_fwd_case("skinny", "bias", skinny_form(8), 512, bias=True, **sk))
    cs.append(_fwd_case("skinny", "residual", skinny_form(8), 512, residual=True, **sk))
    cs.append(_fwd_case("skinny", "accumulate", skinny_form(8), 512, accumulate=True, **sk))
    cs.append(_fwd_case("skinny", "c_f32-accumulate", skinny_form(8), 512, c_f32=True, accumulate=True, **sk))
    cs.append(_fwd_case("skinny", "splitk2", skinny_form(4), 512, c_f32=True, atomic=True, splitk=2, **sk))
    return cs


CASES = _cases()


def pair_cases(mode):
    """jen1_train_gemm_pair: a mapped weight gradient with rowsum (first) and a skinny data gradient (second)"""
    first = _wgrad_case("pair", "wgrad-rowsum", FASTW if mode == BF16 else 0, 72, 40, 74, _conv("conv", 3, 1, 37, 37), 3, (mode,), rowsum=True,
                        accumulate=True)
    dg = _conv("conv", 3, 2, 12, 6)
    second = Case("pair", "skinny-dgrad", skinny_form(4), 24, 40, 256, Opnd(256, 1, m=dg.bwd_map(1)), Opnd(256, 1, tap_stride=40 * 256), ldc_m=40,
                  modes=(mode,), kw=dict(taps=3, skinny=True))
    return first, second


# =====================================================================================================================
# the builder
# =====================================================================================================================
def round_to(x, mode):
    x = np.asarray(x, dtype=np.float32)
    return x if mode == F32 else torch.from_numpy(x).to(torch.bfloat16).float().numpy()


def _pattern(n, mode):
    """a finite pattern no product of the cases gives, exact in bf16"""
    return round_to(-(3.0 + 0.25 * (np.arange(n) % 7)) * 64.0, mode)


class Built:
    """the host side of one case in one mode: flat float32 arrays holding values of the storage dtype, the descriptors and the reference"""

    def __init__(self, case: Case, mode: str, seed: int = 0):
        self.case, self.mode = case, mode
        rng = np.random.default_rng(1000 + seed)
        g = self.g = case.scalars()
        taps, batches = g.get("taps", 1), g.get("batches", 1)
        self.c_mode = F32 if (mode == F32 or g.get("c_f32")) else BF16
        self.shift_b = None if case.shift_b is None else np.asarray(case.shift_b, dtype=np.int32)
        self.bufs, self.base = {}, {}
        for key, op, rows in (("a", case.a, case.M), ("b", case.b, case.N)):
            off, ok = operand_offsets(op.desc(0), rows, case.K, taps, batches, self.shift_b)
            assert off[ok].min() >= 0
            buf = np.full(GUARD + op.off + int(off[ok].max()) + 1 + GUARD, np.nan, dtype=np.float32)
            used = np.unique(off[ok]) + GUARD + op.off
            buf[used] = round_to(rng.standard_normal(used.size), mode)
            self.bufs[key], self.base[key] = buf, GUARD + op.off
        oc = c_offsets(dict(g, taps=taps, batches=batches))
        n_c = GUARD + int(oc.max()) + 1 + GUARD
        c = _pattern(n_c, self.c_mode)
        if g.get("accumulate") or g.get("atomic"):
            c[oc + GUARD] = round_to(rng.standard_normal(oc.shape), self.c_mode)
        self.bufs["c"], self.base["c"] = c, GUARD
        if case.residual:
            res = np.full(n_c, np.nan, dtype=np.float32)
            res[oc + GUARD] = round_to(rng.standard_normal(oc.shape), self.c_mode)
            self.bufs["residual"] = res
        if case.bias:
            self.bufs["bias"] = np.concatenate([rng.standard_normal(case.N).astype(np.float32), np.full(GUARD, np.nan, dtype=np.float32)])
        if case.rowsum:
            self.bufs["rowsum"] = np.concatenate([rng.standard_normal(case.M).astype(np.float32), _pattern(GUARD, F32)])

    def operands(self, a_ptr=0, b_ptr=0, es=1):
        """the two descriptors as gemm_host.operand gives them; (0, 0, 1): ``p`` is the element offset into the flat buffers"""
        return (self.case.a.desc(a_ptr + self.base["a"] * es), self.case.b.desc(b_ptr + self.base["b"] * es))

    def reference(self):
        a, b = self.operands()
        bf = self.bufs
        r = gemm_model(a, b, bf["a"], bf["b"], bf["c"], self.g, bias=bf.get("bias"), residual=bf.get("residual"),
                       rowsum=None if "rowsum" not in bf else bf["rowsum"][:self.case.M], shift_b=self.shift_b, c_p=GUARD)
        return r

    def check(self, got_c, got_rowsum=None, c=GATE_C):
        """the worst error / bound ratio over every stored element; raises on a NaN in the stored region, a changed untouched element or
        an element over its bound"""
        ref = self.reference()
        got = np.asarray(got_c, dtype=np.float64)
        t = ref["touched"]
        assert np.isfinite(got[t]).all(), f"{self.case.id} {self.mode}: {int((~np.isfinite(got[t])).sum())} stored elements are not finite"
        same = got[~t] == self.bufs["c"][~t].astype(np.float64)
        assert same.all(), f"{self.case.id} {self.mode}: {int((~same).sum())} elements outside the output changed"
        n = gate_terms(self.g)
        err, bound = np.abs(got[t] - ref["c"][t]), gate(ref["c"][t], ref["S"][t], n, self.c_mode == BF16, c)
        worst = _worst(err, bound)
        if got_rowsum is not None:
            M = self.case.M
            gr = np.asarray(got_rowsum, dtype=np.float64)
            assert (gr[M:] == self.bufs["rowsum"][M:].astype(np.float64)).all(), f"{self.case.id} {self.mode}: rowsum's guard changed"
            assert np.isfinite(gr[:M]).all()
            n_r = self.g["K"] + self.g.get("splitk", 1) + 3
            worst = max(worst, _worst(np.abs(gr[:M] - ref["rowsum"]), gate(ref["rowsum"], ref["rowsum_S"], n_r, False, c)))
        return worst


def _worst(err, bound):
    """max err / bound; an error where the bound is 0 (nothing but padding was summed: the result must be exactly 0) counts as inf"""
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
    ratio = np.where((bound == 0) & (err > 0), np.inf, ratio)
    return float(ratio.max()) if ratio.size else 0.0
