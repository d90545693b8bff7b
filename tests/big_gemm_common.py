"""A float64 model of the big GEMM family (csrc/big_gemm.hip), its case tables, the builder of their buffers and the deliberately wrong
variants; importable without a GPU.  tests/test_big_gemm_refs_host.py pins the model against torch and the variants' power;
tests/test_gpu_big_gemm_forms.py runs the cases on the kernels.

The model is written from the words of include/jen1_hip.h (jen1_big_gemm with a group table or the inline group, jen1_big_gemm_tn,
jen1_big_gemm_tn_store, jen1_big_gemm_conv, jen1_big_gemm_tn_conv), not from the kernels.  It works in float64 on operands rounded to the
launch dtype and gives, for every output element, the value and the sum of magnitudes the gate is scaled by:

    S = (|alpha| sum |a||b| + |bias|) |row_scale| + |old C| + |residual|

(row_scale multiplies everything in front of it, so it scales the error of what it multiplies; a masked row has S = |old C| and must
come out exactly: zeros, bias included, when nothing is accumulated.)

The gate, per element, is train_gemm_common's (derived there, not fitted): |got - ref| <= 4 (n 2^-24 S + r |ref|), n = the reduction
length + 3 (+ the number of reduction slices where slices are added with float atomics), r = 2^-8 for a bf16 output and 0 for float32.

Buffers: every operand lies inside a larger allocation; guards, pitch columns, rows past the matrix and everything else the contract
does not let a call read are NaN.  Every output lies in a finite pattern (exact in bf16) that must come back bit for bit wherever the call
may not write; where a call stores without accumulating, the writable region is NaN before the call and must be finite after it -- that is
what shows that the tile orders and the column cut reach every tile once.

Wrong variants: every model takes ``wrong=``; a variant changes the result only in the cases that list it (``Case.wrong``).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from helpers import ROOT  # noqa: F401  (puts the package on sys.path)
from train_gemm_common import BF16, F32, GATE_C, GUARD, U8, U24, _pattern, _worst, gate, round_to  # noqa: F401
from transformer_forms_common import POWER  # noqa: F401

ROW_LIMIT = 1 << 22                 # jen1_big_gemm with a row map, and the convolution forms: M below this


# =====================================================================================================================
# restatements of host-side decisions (the expectation a GPU case states before it launches)
# =====================================================================================================================
def route(M, Ntot, K, bf16, n_groups, group_align, n_cu=256, wm=0, t256=-1, s4=-1):
    """which tile forms a jen1_big_gemm call runs on: {"s272": the whole product on 256 x 272 tiles, "n_big": columns [0, n_big) on
    256 x 256 tiles, "wm": 2 / 4 = 128 x 128 / 256 x 128 tiles for the rest}.  wm / t256 / s4: JEN1_BGEMM_WM / _T256 / _S4 (-1: unset)"""
    bf = bf16 and not wm
    tm, tn_all = -(-M // 256), -(-Ntot // 256)
    n_big = 0
    if bf and s4 != 0 and t256 != 1 and K >= 32 and K % 32 == 0 and Ntot % 272 == 0 and (n_groups == 1 or (group_align >= 16 and group_align % 16 == 0)):
        t272, t256n = tm * (Ntot // 272), tm * tn_all
        c272, c256 = -(-t272 // n_cu) * 272.0, -(-t256n // n_cu) * 256.0
        if s4 == 272 or (t272 >= (n_cu * 3) // 4 and c272 < c256 and K >= 512):
            return dict(s272=True, n_big=0, wm=2)
    if bf and t256 != 0 and (n_groups == 1 or (group_align >= 256 and group_align % 256 == 0)):
        if t256 == 1:
            n_big = Ntot
        elif tm * tn_all >= (n_cu * 3) // 4 and K >= 512:
            rounds, tail = divmod(tm * tn_all, n_cu)
            tn_big = tn_all
            if tail > 0 and tail * 4 < n_cu * 3 and rounds >= 1:
                tn_big = (rounds * n_cu) // tm
            n_big = Ntot if tn_big >= tn_all else tn_big * 256
            if n_groups > 1 and n_big < Ntot and n_big % group_align:
                n_big -= n_big % group_align
    t = tm * (-(-(Ntot - n_big) // 128))
    return dict(s272=False, n_big=n_big, wm=wm or (4 if (t >= 512 and K >= 2048) else 2))


def tn_splits(tiles, M):
    """slices of the reduction of a TN product over ``tiles`` output tiles (JEN1_BGEMM_TN_SPLITS unset)"""
    MT = -(-M // 64)
    s_min = -(-128 // tiles)
    best, splits = 1e30, 1
    for s in range(min(s_min, MT), MT + 1):
        t = float(np.float32(0.5) * np.float32(-(-MT // s)) + np.float32(0.058) * np.float32(s) * np.float32(tiles))
        if t < best:
            best, splits = t, s
    splits = max(1, min(splits, MT))
    per = -(-MT // splits)
    return -(-MT // per)


def tn_conv_tiles(co, ci, taps):
    cpt = 16 // taps if taps > 1 else 16
    tiles_k = -(-(-(-ci // 8)) // cpt) if taps > 1 else -(-ci // 128)
    return -(-co // 128) * tiles_k


def bias_slices(M):
    """(rows per slice, slices) of the bias gradient of jen1_big_gemm_tn_conv"""
    nbk = max(1, min(32, M // 1536))
    rows = -(-M // nbk)
    return rows, -(-M // rows)


def row_map_f32(m, rows_in):
    """the float32 expression the kernels divide a row index with, emulated in numpy: (int)((m + 0.5f) * (1.0f / rows_in))"""
    inv = np.float32(1.0) / np.float32(rows_in)
    return ((np.asarray(m).astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)


# =====================================================================================================================
# buffers
# =====================================================================================================================
class Mat:
    """a rows x cols matrix at pitch ld inside a flat float32 buffer: GUARD elements on either side and ``extra`` rows behind it.
    Everything is NaN (an operand), or with ``pattern`` the finite pattern (an output).  ``all`` views rows + extra rows at the pitch, ``v``
    the matrix"""

    def __init__(self, rows, cols, ld, mode, pattern=False, extra=2):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.mode = rows, cols, ld, mode
        n = (rows + extra) * ld
        self.flat = _pattern(GUARD + n + GUARD, mode).copy() if pattern else np.full(GUARD + n + GUARD, np.nan, dtype=np.float32)
        self.all = self.flat[GUARD:GUARD + n].reshape(rows + extra, ld)
        self.v = self.all[:rows, :cols]

    def fill(self, rng, mode, scale=0.5):
        self.v[...] = round_to(rng.standard_normal(self.v.shape) * scale, mode)
        return self


def vec(rng, n, scale=1.0):
    """a float32 vector with NaN guards on either side (a bias, a gradient accumulator's neighbourhood)"""
    flat = np.full(GUARD + n + GUARD, np.nan, dtype=np.float32)
    flat[GUARD:GUARD + n] = (rng.standard_normal(n) * scale).astype(np.float32)
    return flat


class Out:
    """one output buffer of a built case: the whole flat buffer before the call (guards included), the model's result, S, where the call
    stores, and the gate's n.  The model's arrays cover the region behind the front guard; the rest of the buffer may not change"""

    def __init__(self, name, before, mode, n, at=GUARD):
        self.name, self.before, self.mode, self.n, self.at = name, np.asarray(before, dtype=np.float32).reshape(-1), mode, n, at
        self.ref = self.S = self.touched = None

    def _embed(self, arr, base):
        arr = np.asarray(arr).reshape(-1)
        out = np.array(base)
        out[self.at:self.at + arr.size] = arr
        return out

    def set(self, ref, S, touched):
        self.ref = self._embed(ref, self.before.astype(np.float64))
        self.S = self._embed(S, np.zeros(self.before.size))
        self.touched = self._embed(touched, np.zeros(self.before.size, dtype=bool))
        return self

    def _ratio(self, got):
        t = self.touched
        return _worst(np.abs(got[t] - self.ref[t]), gate(self.ref[t], self.S[t], self.n, self.mode == BF16))

    def judge(self, got, what=""):
        """the worst error / bound over the stored elements of the whole buffer after the call; raises on a stored NaN or a change
        outside the stored region"""
        got = np.asarray(got, dtype=np.float64).reshape(-1)
        t = self.touched
        assert got.size == t.size
        assert np.isfinite(got[t]).all(), f"{what} {self.name}: {int((~np.isfinite(got[t])).sum())} of {int(t.sum())} stored elements are not finite"
        same = got[~t] == self.before[~t].astype(np.float64)
        assert same.all(), f"{what} {self.name}: {int((~same).sum())} elements outside the output changed"
        return self._ratio(got)

    def distance(self, other):
        """how far a wrong variant's result (the model's region) lies from the right one, in units of the gate; inf: it leaves a stored
        element unwritten or not finite, or changes an element outside the output"""
        o = self._embed(other, self.before.astype(np.float64))
        t = self.touched
        if not np.isfinite(o[t]).all():
            return np.inf
        b = self.before.astype(np.float64)
        if not ((o[~t] == b[~t]) | (np.isnan(o[~t]) & np.isnan(b[~t]))).all():
            return np.inf
        return self._ratio(o)


# =====================================================================================================================
# NT: jen1_big_gemm
# =====================================================================================================================
@dataclass(frozen=True)
class Form:
    env: dict               # the switches that force the form (JEN1_BGEMM_WM is read once per process: a child of its own)
    nstage: int             # LDS stages of the K ring
    bk_bytes: int           # bytes of a K step
    rowwise: bool           # bf16 stores without accumulation leave row-wise

    def bk(self, mode):
        return self.bk_bytes // (4 if mode == F32 else 2)


FORMS = {
    "t128": Form(dict(JEN1_BGEMM_T256="0", JEN1_BGEMM_S4="0"), 2, 128, False),
    "t256x128": Form(dict(JEN1_BGEMM_WM="4"), 3, 128, False),
    "t256": Form(dict(JEN1_BGEMM_T256="1", JEN1_BGEMM_S4="0"), 2, 128, True),
    "s272": Form(dict(JEN1_BGEMM_T256="0", JEN1_BGEMM_S4="272"), 4, 64, True),
}


def forced(form):
    e = FORMS[form].env
    return dict(wm=int(e.get("JEN1_BGEMM_WM", 0)), t256=int(e.get("JEN1_BGEMM_T256", -1)), s4=int(e.get("JEN1_BGEMM_S4", -1)))


@dataclass(frozen=True)
class Grp:
    N: int
    ldc: int
    bias: bool = False


@dataclass(frozen=True)
class NT:
    form: str
    name: str
    M: int
    K: int
    groups: tuple
    lda: int = 0            # 0: K
    ldb: int = 0
    rows_in: int = 0
    rows_out: int = 0
    scale: bool = False
    alpha: float = 1.0
    c_f32: bool = False
    accumulate: bool = False
    group_align: int = 0
    inline: bool = False    # groups == NULL: the one group in the inline fields
    wrong: tuple = ()

    @property
    def Ntot(self):
        return sum(g.N for g in self.groups)

    @property
    def id(self):
        return f"{self.form}.{self.name}"

    def modes(self):
        return (F32, BF16) if self.form in ("t128", "t256x128") else (BF16,)

    def K_of(self, mode):
        """the table states K in bf16 steps; float32 runs the same number of K steps (a step is 128 bytes)"""
        return self.K // 2 if mode == F32 else self.K

    def pitch(self, ld, mode):
        return self.K_of(mode) + (ld - self.K if ld else 0)


def out_row(m, rows_in, rows_out, wrong=None):
    """orow(m) = (m / rows_in) * rows_out + m % rows_in; rows_in = 0: m"""
    m = np.asarray(m, dtype=np.int64)
    if rows_in <= 0:
        return m
    q = m // rows_in
    if wrong == "rowmap_off_by_one":            # the quotient one too large on the last row of a block
        q = (m + 1) // rows_in
    r = m - q * rows_in
    return q * (rows_in if wrong == "rowmap_in_for_out" else rows_out) + r


def nt_model(case: NT, mode, A, Bw, biases, scale, c_before, wrong=None):
    """A [M][K], Bw [Ntot][K] float64; biases: per group [N] or None; scale: indexed by the OUTPUT row, or None; c_before: per group
    the [rows][ldc] buffer before the call.  Returns per group (c after the call, S, touched), all [rows][ldc]"""
    f = FORMS[case.form]
    K, bk = A.shape[1], f.bk(mode)
    alpha = float(np.float32(case.alpha))
    if wrong == "drop_last_k":
        A = A.copy()
        A[:, K - bk:] = 0.0
    if wrong == "swap_k_ring" and K // bk > f.nstage:        # A's K steps nstage - 1 and nstage change places, B's stay
        A = A.copy()
        s = f.nstage
        A[:, (s - 1) * bk:s * bk], A[:, s * bk:(s + 1) * bk] = A[:, s * bk:(s + 1) * bk].copy(), A[:, (s - 1) * bk:s * bk].copy()
    prod, mag = A @ Bw.T, np.abs(A) @ np.abs(Bw).T
    m = np.arange(case.M)
    orow_true = out_row(m, case.rows_in, case.rows_out)
    orow = out_row(m, case.rows_in, case.rows_out, wrong)
    rs = np.ones(case.M)
    if scale is not None:
        rs = np.asarray(scale, dtype=np.float64)[m if wrong == "scale_at_gemm_row" else orow_true]
        rs = np.where(np.isfinite(rs), rs, 1.0e3)         # (only a wrong variant reads an entry nobody filled)
    rs = rs[:, None]
    c_mode = F32 if (mode == F32 or case.c_f32) else BF16
    starts = np.cumsum([0] + [g.N for g in case.groups])
    res = []
    for gi, g in enumerate(case.groups):
        n0 = int(starts[gi])
        cols = slice(0, g.N) if (wrong == "stacked_column") else slice(n0, n0 + g.N)      # (the group's own column where the stacked one belongs)
        p, s = prod[:, cols], mag[:, cols]
        b = np.zeros(g.N) if biases[gi] is None else np.asarray(biases[gi], dtype=np.float64)[:g.N]
        if wrong == "alpha_on_bias":
            val = alpha * (p + b) * rs
        elif wrong == "mask_before_bias":
            val = alpha * p * rs + b
        else:
            val = (alpha * p + b) * rs
        S = (abs(alpha) * s + np.abs(b)) * np.abs(rs)
        before = np.asarray(c_before[gi], dtype=np.float64)
        out, Sf, touched = before.copy(), np.zeros(before.shape), np.zeros(before.shape, dtype=bool)
        if case.accumulate:
            old = before[orow, :g.N]
            val, S = val + old, S + np.abs(old)
        keep = np.zeros(val.shape, dtype=bool)             # elements a wrong variant leaves unwritten
        if wrong == "group_by_tile" and case.form == "s272":
            n = n0 + np.arange(g.N)
            t0 = (n // 272) * 272
            keep |= ((t0 < n0) | (t0 >= n0 + g.N))[None, :]
        if wrong == "ragged_half_dropped" and f.rowwise and c_mode == BF16 and not case.accumulate:
            odd = (orow * g.ldc) % 8 != 0
            keep |= odd[:, None] & ((np.arange(g.N) % 8) >= 4)[None, :]
        out[orow, :g.N] = np.where(keep, before[orow, :g.N], val)
        Sf[orow_true, :g.N] = S
        touched[orow_true, :g.N] = True
        if wrong is None:
            assert np.isfinite(out[touched]).all()
        res.append((out, Sf, touched))
    return res


class BuiltNT:
    """the host side of one NT case in one mode"""

    def __init__(self, case: NT, mode, seed=0):
        self.case, self.mode = case, mode
        rng = np.random.default_rng(7000 + seed)
        M, K = case.M, case.K_of(mode)
        self.K, self.lda, self.ldb = K, case.pitch(case.lda, mode), case.pitch(case.ldb, mode)
        self.c_mode = F32 if (mode == F32 or case.c_f32) else BF16
        self.a = Mat(M, K, self.lda, mode).fill(rng, mode)
        self.b = Mat(case.Ntot, K, self.ldb, mode).fill(rng, mode, 0.25)
        self.orow = out_row(np.arange(M), case.rows_in, case.rows_out)
        rows_c = (-(-M // case.rows_in) * case.rows_out) if case.rows_in else M
        self.rows_c = rows_c
        self.scale = None
        if case.scale:                                     # indexed by the output row; entries no GEMM row maps to are NaN
            self.scale = np.full(GUARD + rows_c + GUARD, np.nan, dtype=np.float32)
            vals = rng.choice(np.array([0.0, 0.5, 1.0, 1.75, -1.25], dtype=np.float32), size=M, p=[0.3, 0.2, 0.2, 0.15, 0.15])
            vals[:2] = (0.0, 1.75)
            self.scale[GUARD + self.orow] = vals
        self.c, self.bias = [], []
        for g in case.groups:
            c = Mat(rows_c, g.N, g.ldc, self.c_mode, pattern=True)
            c.all[self.orow, :g.N] = round_to(rng.standard_normal((M, g.N)), self.c_mode) if case.accumulate else np.nan
            self.c.append(c)
            self.bias.append(vec(rng, g.N) if g.bias else None)
        self.outs = [Out(f"group{gi}", c.flat.copy(), self.c_mode, K + 3) for gi, c in enumerate(self.c)]
        for o, r in zip(self.outs, self.model()):
            o.set(*r)

    def model(self, wrong=None):
        return nt_model(self.case, self.mode, self.a.v.astype(np.float64), self.b.v.astype(np.float64),
                        [None if b is None else b[GUARD:] for b in self.bias], None if self.scale is None else self.scale[GUARD:],
                        [c.all for c in self.c], wrong)

    def judge(self, got_all):
        """got_all: per group the whole flat buffer after the call"""
        return max(o.judge(g, f"{self.case.id} {self.mode}") for o, g in zip(self.outs, got_all))

    def distance(self, wrong):
        return max(o.distance(r[0]) for o, r in zip(self.outs, self.model(wrong)))


def _nt_cases():
    cs = []
    small = (("t128", 132), ("t256x128", 132), ("t256", 132), ("s272", 272))
    for form, N in small:
        rw = FORMS[form].rowwise
        # K steps (prologue, first refill, ring wrap) x ragged M, pitched operands, ragged columns at a pitch 4 past the width
        for K in (64, 128, 192, 320):
            for M in (1, 129, 257, 300):
                w = ("drop_last_k",) + (("swap_k_ring",) if K // (FORMS[form].bk_bytes // 2) > FORMS[form].nstage else ())
                w += ("ragged_half_dropped",) if (rw and (N + 4) % 8 == 4 and M > 1) else ()
                cs.append(NT(form, f"K{K}.M{M}", M, K, (Grp(N, N + 4),), lda=K + 8, ldb=K + 24, inline=(M != 257), wrong=w))
        # one group, ragged columns.  N % 8 == 4: ldc = N is the pitch that puts every other row start off 16 bytes, ldc = N + 4 the aligned one
        widths = (272, 544) if form == "s272" else (4, 132, 260)
        for Nr in widths:
            for ldc in (Nr, Nr + 4):
                w = ("ragged_half_dropped",) if (rw and ldc % 8 == 4 and Nr > 4) else ()
                cs.append(NT(form, f"N{Nr}.ldc{ldc}", 300, 128, (Grp(Nr, ldc, bias=True),), alpha=0.75, inline=True, wrong=w))
        # row map
        for ri, ro, M in ((3, 4, 301), (77, 82, 300), (129, 130, 300)):
            cs.append(NT(form, f"rows{ri}to{ro}", M, 128, (Grp(N, N + 4, bias=True),), rows_in=ri, rows_out=ro, scale=True, alpha=-1.5, inline=True,
                         wrong=("alpha_on_bias", "mask_before_bias", "scale_at_gemm_row", "rowmap_in_for_out", "rowmap_off_by_one")))
        # group tables: per-group pitch, bias on some groups, alpha; each output mode once
        if form in ("t128", "t256x128"):
            grps, ga = (Grp(128, 128, True), Grp(384, 392), Grp(256, 256, True)), 0
        elif form == "t256":
            grps, ga = (Grp(256, 264, True), Grp(512, 512)), 256
        else:       # 2176 = 8 x 272 columns; the boundaries 384 and 512 lie inside the tile [272, 544): three groups in one tile
            grps, ga = (Grp(384, 384, True), Grp(128, 136), Grp(1664, 1664, True)), 128
        for name, kw in (("store", {}), ("f32-out", dict(c_f32=True)), ("f32-accumulate", dict(c_f32=True, accumulate=True)),
                         ("accumulate", dict(accumulate=True))):
            w = ("stacked_column", "alpha_on_bias", "mask_before_bias") + (("group_by_tile",) if form == "s272" else ())
            cs.append(NT(form, f"groups.{name}", 300, 128, grps, rows_in=77, rows_out=82, scale=True, alpha=0.625, group_align=ga, wrong=w, **kw))
    # tile order of the 256-row forms: the blocked branch (tiles_m even, tiles_n a multiple of 32 / bm), the plain one (M = 513: 3 tiles
    # along m) and tile counts below 8 / no multiple of 8 for the XCD deal
    cs.append(NT("t256", "tiles.2x16", 300, 64, (Grp(4096, 4096),)))
    cs.append(NT("t256", "tiles.4x8", 770, 64, (Grp(2048, 2048),)))
    cs.append(NT("t256", "tiles.8x4", 1800, 64, (Grp(1024, 1024),)))
    cs.append(NT("t256", "tiles.3x2", 513, 64, (Grp(512, 512),)))
    cs.append(NT("t256", "tiles.1x3", 200, 64, (Grp(768, 768),)))
    cs.append(NT("s272", "tiles.8x4", 1800, 64, (Grp(1088, 1088),)))
    cs.append(NT("s272", "tiles.3x2", 513, 64, (Grp(544, 544),)))
    cs.append(NT("s272", "tiles.1x3", 200, 64, (Grp(816, 816),)))
    return cs


NT_CASES = _nt_cases()


# =====================================================================================================================
# TN: jen1_big_gemm_tn / jen1_big_gemm_tn_store
# =====================================================================================================================
@dataclass(frozen=True)
class TN:
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    ldc: int
    alpha: float = 0.375
    wrong: tuple = ()

    @property
    def id(self):
        return f"M{self.M}.N{self.N}.K{self.K}"


def tn_model(A, Bm, c_before, alpha, store, wrong=None):
    """C[n][k] (+)= alpha sum_m A[m][n] B[m][k]; c_before [N + extra][ldc].  Returns (c after, S, touched)"""
    alpha = float(np.float32(alpha))
    M, N, K = A.shape[0], A.shape[1], Bm.shape[1]
    if wrong == "drop_last_k":                              # the last 64-row step of the reduction
        A = A.copy()
        A[((M - 1) // 64) * 64:] = 0.0
    if wrong == "swap_k_ring" and M > 128:                  # A's second and third 64-row steps change places
        A = A.copy()
        hi = min(M, 192)
        blk = A[128:hi].copy()
        A[128:hi] = A[64:64 + hi - 128]
        A[64:64 + hi - 128] = blk
    val, S = alpha * (A.T @ Bm), abs(alpha) * (np.abs(A).T @ np.abs(Bm))
    before = np.asarray(c_before, dtype=np.float64)
    out, Sf, touched = before.copy(), np.zeros(before.shape), np.zeros(before.shape, dtype=bool)
    if not store:
        val, S = val + before[:N, :K], S + np.abs(before[:N, :K])
    out[:N, :K], Sf[:N, :K], touched[:N, :K] = val, S, True
    return out, Sf, touched


class BuiltTN:
    def __init__(self, case: TN, store, seed=0):
        self.case, self.store = case, store
        rng = np.random.default_rng(8000 + seed)
        self.a = Mat(case.M, case.N, case.lda, BF16).fill(rng, BF16)
        self.b = Mat(case.M, case.K, case.ldb, BF16).fill(rng, BF16)
        self.c = Mat(case.N, case.K, case.ldc, F32, pattern=True)
        self.c.v[...] = np.nan if store else rng.standard_normal((case.N, case.K)).astype(np.float32)
        self.splits = 1 if store else tn_splits(-(-case.N // 128) * -(-case.K // 128), case.M)
        self.out = Out("c", self.c.flat.copy(), F32, case.M + 3 + (0 if store else self.splits)).set(*self.model())

    def model(self, wrong=None):
        return tn_model(self.a.v.astype(np.float64), self.b.v.astype(np.float64), self.c.all, self.case.alpha, self.store, wrong)

    def distance(self, wrong):
        return self.out.distance(self.model(wrong)[0])


# (N, K) with pitches that keep a partial 128-column tile inside the row; ldc > K
TN_CASES = [TN(M, N, K, lda, ldb, K + 4, wrong=(("drop_last_k",) if M > 1 else ()) + (("swap_k_ring",) if M > 128 else ()))
            for (N, K, lda, ldb) in ((8, 8, 128, 136), (136, 264, 256, 384), (128, 384, 136, 392)) for M in (1, 63, 64, 65, 300)]


# =====================================================================================================================
# convolution forms: jen1_big_gemm_conv, jen1_big_gemm_tn_conv
# =====================================================================================================================
def conv_rows(B, T_in, T_out, taps, stride, pad, shift_b=None, div=1, wrong=None):
    """input row (into [B T_in]) of output row m = b T_out + t and tap, and whether it is read (else it counts as zeros)"""
    m = np.arange(B * T_out, dtype=np.int64)
    b, t = np.divmod(m, T_out)
    sh = np.zeros(B, dtype=np.int64) if shift_b is None else np.asarray(shift_b, dtype=np.int64)[:B]
    if wrong == "shift_b_neighbour":
        sh = np.roll(sh, -1)
    pos = t[:, None] * stride + np.arange(taps)[None, :] - pad + sh[b][:, None]
    ok = np.ones(pos.shape, dtype=bool)
    if div > 1:
        if wrong != "div_counts_all":
            ok &= pos % div == 0
        pos = pos // div
    row = b[:, None] * T_in + pos
    if wrong == "pad_from_next_batch":                      # the range test against the whole buffer where it belongs to the batch element
        ok &= (row >= 0) & (row < B * T_in)
    else:
        ok &= (pos >= 0) & (pos < T_in)
    return np.where(ok, row, 0), ok


@dataclass(frozen=True)
class Conv:
    name: str
    B: int
    T_in: int
    T_out: int
    ci: int
    co: int
    taps: int
    stride: int
    pad: int
    tap_rev: bool = False
    div: int = 1
    shift_b: Optional[tuple] = None
    bias: bool = True
    residual: bool = False
    ld_x: int = 0
    ld_w: int = 0
    ld_y: int = 0
    wrong: tuple = ()

    @property
    def id(self):
        return self.name


def _im2col(x, rows, ok):
    """[M][taps][ci] with zeros where a tap reads none"""
    return np.where(ok[:, :, None], x[rows], 0.0)


def conv_model(case: Conv, x, w, bias, residual, y_before, wrong=None):
    """x [B T_in][ci], w [taps][co][ci] float64 as they lie in memory; y_before [M + extra][ld_y].  Returns (y after, S, touched)"""
    rows, ok = conv_rows(case.B, case.T_in, case.T_out, case.taps, case.stride, case.pad, case.shift_b, case.div, wrong)
    X = _im2col(x, rows, ok)
    order = np.arange(case.taps)
    if case.tap_rev and wrong != "tap_not_reversed":
        order = order[::-1]
    W = w[order]                                            # [tap][co][ci]: the matrix tap ``tap`` of the sum multiplies
    if wrong == "drop_last_k":
        X = X.copy()
        X[:, -1, ((case.ci - 1) // 64) * 64:] = 0.0
    if wrong == "swap_k_ring" and case.taps >= 3:           # x's taps 1 and 2 change places, W's stay
        X = X.copy()
        X[:, [1, 2]] = X[:, [2, 1]]
    Xf, Wf = X.reshape(X.shape[0], -1), W.transpose(1, 0, 2).reshape(case.co, -1)
    val, S = Xf @ Wf.T, np.abs(Xf) @ np.abs(Wf).T
    if bias is not None:
        val, S = val + bias[None, :case.co], S + np.abs(bias[None, :case.co])
    M = case.B * case.T_out
    if residual is not None:
        val, S = val + residual[:M, :case.co], S + np.abs(residual[:M, :case.co])
    before = np.asarray(y_before, dtype=np.float64)
    out, Sf, touched = before.copy(), np.zeros(before.shape), np.zeros(before.shape, dtype=bool)
    out[:M, :case.co], Sf[:M, :case.co], touched[:M, :case.co] = val, S, True
    return out, Sf, touched


class BuiltConv:
    def __init__(self, case: Conv, seed=0):
        self.case = case
        rng = np.random.default_rng(9000 + seed)
        M = case.B * case.T_out
        self.ld_x, self.ld_w, self.ld_y = case.ld_x or case.ci, case.ld_w or case.ci, case.ld_y or case.co
        self.x = Mat(case.B * case.T_in, case.ci, self.ld_x, BF16).fill(rng, BF16)
        self.w = [Mat(case.co, case.ci, self.ld_w, BF16, extra=1).fill(rng, BF16, 0.125) for _ in range(case.taps)]
        self.w_tap_stride = (case.co + 1) * self.ld_w       # (the tap matrices one NaN row apart)
        self.w_flat = np.concatenate([np.full(GUARD, np.nan, dtype=np.float32)] + [m.all.reshape(-1) for m in self.w] + [np.full(GUARD, np.nan, dtype=np.float32)])
        self.bias = vec(rng, case.co) if case.bias else None
        self.res = Mat(M, case.co, self.ld_y, BF16).fill(rng, BF16) if case.residual else None
        self.y = Mat(M, case.co, self.ld_y, BF16, pattern=True)
        self.y.v[...] = np.nan
        self.shift_b = None if case.shift_b is None else np.asarray(case.shift_b, dtype=np.int32)
        self.out = Out("y", self.y.flat.copy(), BF16, case.taps * case.ci + 3).set(*self.model())

    def model(self, wrong=None):
        return conv_model(self.case, self.x.v.astype(np.float64), np.stack([m.v for m in self.w]).astype(np.float64),
                          None if self.bias is None else self.bias[GUARD:].astype(np.float64),
                          None if self.res is None else self.res.all.astype(np.float64), self.y.all, wrong)

    def distance(self, wrong):
        return self.out.distance(self.model(wrong)[0])


def _conv_cases():
    B, T = 3, 50
    half = lambda t, s: (t - 1) // s + 1
    cs = [
        Conv("centred-k3", B, T, T, 128, 64, 3, 1, 1, wrong=("drop_last_k", "swap_k_ring", "pad_from_next_batch")),
        Conv("causal-k3.residual", B, T, T, 128, 128, 3, 1, 2, bias=False, residual=True, wrong=("pad_from_next_batch",)),
        Conv("stride2-k5", 2, 257, half(257, 2), 256, 96, 5, 2, 2, wrong=("drop_last_k",)),
        Conv("1x1.co72-in-128", 4, 43, 43, 192, 72, 1, 1, 0, ld_y=128, ld_x=200, ld_w=208),
        Conv("ci264.ragged-step", B, T, T, 264, 128, 3, 1, 1, ld_x=272, wrong=("drop_last_k",)),
        Conv("shift_b.stride1", 4, T, T, 128, 128, 3, 1, 0, shift_b=(-2, -1, -2, 0), wrong=("shift_b_neighbour",)),
        Conv("shift_b.stride2", 4, 51, half(51, 2), 128, 64, 5, 2, 0, shift_b=(-4, -2, -3, -2), wrong=("shift_b_neighbour",)),
        Conv("dgrad.tap_rev", B, T, T, 128, 128, 3, 1, 0, tap_rev=True, bias=False, wrong=("tap_not_reversed",)),
    ]
    for stride, k, padding in ((2, 4, 1), (4, 8, 2)):       # ConvTranspose1d forward: stride 1, taps reversed, pad' = k - 1 - padding, div = its stride
        L_in = 43
        L_out = (L_in - 1) * stride - 2 * padding + k
        cs.append(Conv(f"convT-forward.s{stride}", B, L_in, L_out, 128, 64, k, 1, k - 1 - padding, tap_rev=True, div=stride,
                       wrong=("tap_not_reversed", "div_counts_all")))
    return cs


CONV_CASES = _conv_cases()


@dataclass(frozen=True)
class TNConv:
    name: str
    B: int
    T_in: int
    T_out: int
    ci: int
    co: int
    taps: int
    stride: int
    pad: int
    shift_b: Optional[tuple] = None
    gb: bool = True
    alpha: float = 0.5
    wrong: tuple = ()

    @property
    def id(self):
        return self.name


def tn_conv_model(case: TNConv, dy, x, gw_before, gb_before, wrong=None):
    """gw[co][ci][tap] += alpha sum_{b,t} dy[b T_out + t][co] x[b T_in + t stride + tap - pad][ci], gb[co] += alpha sum dy.
    gw_before: flat [co * ci * taps (+ guards behind)]; returns ((gw, S, touched), (gb, S, touched) or None)"""
    alpha = float(np.float32(case.alpha))
    rows, ok = conv_rows(case.B, case.T_in, case.T_out, case.taps, case.stride, case.pad, case.shift_b, 1, wrong)
    X = _im2col(x, rows, ok)                                # [M][tap][ci]
    M = dy.shape[0]
    d = dy
    if wrong == "drop_last_k":
        d = dy.copy()
        d[((M - 1) // 64) * 64:] = 0.0
    Xf = X.reshape(M, -1)
    oct_ = lambda v: v.reshape(case.co, case.taps, case.ci).transpose(0, 2, 1)
    val, S = alpha * oct_(d.T @ Xf), abs(alpha) * oct_(np.abs(dy).T @ np.abs(Xf))
    if wrong == "tap_ci_layout":
        val = np.ascontiguousarray(val.transpose(0, 2, 1)).reshape(val.shape)
    n = case.co * case.ci * case.taps
    before = np.asarray(gw_before, dtype=np.float64)
    out, Sf, touched = before.copy(), np.zeros(before.shape), np.zeros(before.shape, dtype=bool)
    out[:n] = before[:n] + val.reshape(-1)
    Sf[:n], touched[:n] = S.reshape(-1) + np.abs(before[:n]), True
    res_b = None
    if gb_before is not None:
        bb = np.asarray(gb_before, dtype=np.float64)
        d = dy
        if wrong == "bias_tail_dropped":                    # per slice, the rows behind its last whole pass of 128
            per, n_sl = bias_slices(M)
            d = dy.copy()
            for j in range(n_sl):
                r0, r1 = j * per, min(M, (j + 1) * per)
                d[r0 + ((r1 - r0) // 128) * 128:r1] = 0.0
        ob, Sb, tb = bb.copy(), np.zeros(bb.shape), np.zeros(bb.shape, dtype=bool)
        ob[:case.co] = bb[:case.co] + alpha * d.sum(0)
        Sb[:case.co], tb[:case.co] = abs(alpha) * np.abs(dy).sum(0) + np.abs(bb[:case.co]), True
        res_b = (ob, Sb, tb)
    return (out, Sf, touched), res_b


class BuiltTNConv:
    def __init__(self, case: TNConv, seed=0):
        self.case = case
        rng = np.random.default_rng(9500 + seed)
        M = case.B * case.T_out
        self.ld_dy, self.ld_x = -(-case.co // 128) * 128 + 8, -(-case.ci // 8) * 8 + (0 if case.ci % 8 else 8)
        self.dy = Mat(M, case.co, self.ld_dy, BF16).fill(rng, BF16)
        self.x = Mat(case.B * case.T_in, case.ci, self.ld_x, BF16).fill(rng, BF16)
        if "bias_tail_dropped" in case.wrong:
            # the gate grows with the 3 100 rows and a slice's tail is 14 of them: they are drawn 8 x larger (exact in bf16), so that
            # losing them lies well outside the gate
            per, n_sl = bias_slices(M)
            for j in range(n_sl):
                r0, r1 = j * per, min(M, (j + 1) * per)
                self.dy.v[r0 + ((r1 - r0) // 128) * 128:r1] *= 8.0
        n = case.co * case.ci * case.taps
        self.gw = _pattern(n + GUARD, F32).copy()            # (the gradient is contiguous: the pattern lies behind it)
        self.gw[:n] = rng.standard_normal(n).astype(np.float32)
        self.gb = _pattern(case.co + GUARD, F32).copy()
        self.gb[:case.co] = rng.standard_normal(case.co).astype(np.float32)
        self.shift_b = None if case.shift_b is None else np.asarray(case.shift_b, dtype=np.int32)
        splits = tn_splits(tn_conv_tiles(case.co, case.ci, case.taps), M)
        rw, rb = self.model()
        self.out_w = Out("gw", self.gw.copy(), F32, M + 3 + splits, at=0).set(*rw)
        self.out_b = Out("gb", self.gb.copy(), F32, M + 3 + bias_slices(M)[1], at=0).set(*rb) if case.gb else None

    def model(self, wrong=None):
        return tn_conv_model(self.case, self.dy.v.astype(np.float64), self.x.v.astype(np.float64), self.gw, self.gb if self.case.gb else None, wrong)

    def distance(self, wrong):
        rw, rb = self.model(wrong)
        d = self.out_w.distance(rw[0])
        return d if rb is None else max(d, self.out_b.distance(rb[0]))


def _tn_conv_cases():
    cs = []
    for taps in (1, 3, 7, 16):
        for ci in (20, 128, 257):
            pad = (taps - 1) // 2
            w = ("drop_last_k",) + (("tap_ci_layout",) if taps > 1 else ())
            cs.append(TNConv(f"k{taps}.ci{ci}", 3, 50, 50, ci, 72 if ci == 20 else 128, taps, 1, pad, gb=(ci != 128), wrong=w))
    cs.append(TNConv("stride2-k5", 2, 257, 129, 128, 64, 5, 2, 2, wrong=("tap_ci_layout",)))
    cs.append(TNConv("shift_b", 4, 50, 50, 128, 128, 3, 1, 0, shift_b=(-2, -1, -2, 0), wrong=("shift_b_neighbour", "pad_from_next_batch")))
    cs.append(TNConv("rows3100.two-bias-slices", 4, 775, 775, 128, 128, 3, 1, 1, wrong=("bias_tail_dropped",)))
    return cs


TN_CONV_CASES = _tn_conv_cases()


# =====================================================================================================================
# the small kernels
# =====================================================================================================================
def standardize_ref(x, C, eps, mode):
    """float64 (x - mean) / sqrt(var + eps) over the first C columns of the rows, on the values rounded to ``mode``; and the float32
    restatement of the two-moment formula (sum and sum of squares, var = q / C - mean^2 clamped at 0) whose error scales the bound"""
    xr = round_to(np.asarray(x)[:, :C], mode)
    x64 = xr.astype(np.float64)
    mean = x64.mean(1, keepdims=True)
    ref = (x64 - mean) / np.sqrt(((x64 - mean) ** 2).mean(1, keepdims=True) + eps)
    s, q = xr.sum(1, keepdims=True, dtype=np.float32), (xr * xr).sum(1, keepdims=True, dtype=np.float32)
    m32 = s / np.float32(C)
    var = np.maximum(q / np.float32(C) - m32 * m32, np.float32(0))
    emul = (xr - m32) * (np.float32(1) / np.sqrt(var + np.float32(eps)))
    return ref, emul.astype(np.float64)


ALL_WRONG = ("drop_last_k", "swap_k_ring", "alpha_on_bias", "mask_before_bias", "scale_at_gemm_row", "rowmap_in_for_out", "rowmap_off_by_one",
             "group_by_tile", "stacked_column", "ragged_half_dropped", "tap_not_reversed", "shift_b_neighbour", "div_counts_all",
             "pad_from_next_batch", "tap_ci_layout", "bias_tail_dropped")
# which kernels can make which mistake: the host test wants every pair shown by at least one case
NT_ALL = ("drop_last_k", "swap_k_ring", "alpha_on_bias", "mask_before_bias", "scale_at_gemm_row", "rowmap_in_for_out", "rowmap_off_by_one", "stacked_column")
CAN_MAKE = {
    "t128": NT_ALL, "t256x128": NT_ALL, "t256": NT_ALL + ("ragged_half_dropped",), "s272": NT_ALL + ("ragged_half_dropped", "group_by_tile"),
    "tn": ("drop_last_k", "swap_k_ring"), "tn_store": ("drop_last_k", "swap_k_ring"),
    "conv": ("drop_last_k", "swap_k_ring", "tap_not_reversed", "shift_b_neighbour", "div_counts_all", "pad_from_next_batch"),
    "tn_conv": ("drop_last_k", "shift_b_neighbour", "pad_from_next_batch", "tap_ci_layout", "bias_tail_dropped"),
}
