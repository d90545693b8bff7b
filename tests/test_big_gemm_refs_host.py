"""CPU pins of tests/big_gemm_common.py: the float64 model of the big GEMM family against torch float64 (matmul, conv1d,
conv_transpose1d and their autograd), the power of the wrong variants in the GPU test's own metric, the float32 row-map expression of the
kernels swept below the bound jen1_big_gemm now checks, the restated route on the production shapes, and the refusals of the C ABI
(they return before any launch: no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import big_gemm_common as G
from jen1_amd import lib as L

BF16, F32 = G.BF16, G.F32
t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), float(np.abs(a - b).max())


# ---------------------------------------------------------------------------------------------------------------------
# the model against torch
# ---------------------------------------------------------------------------------------------------------------------
def _nt(name):
    return next(c for c in G.NT_CASES if c.id == name)


@pytest.mark.parametrize("name,mode", [("t128.groups.f32-accumulate", BF16), ("t128.groups.store", F32), ("s272.groups.accumulate", BF16),
                                       ("t256.rows129to130", BF16), ("t128.rows3to4", F32), ("t128.N132.ldc132", BF16), ("t256.K320.M257", BF16)])
def test_nt_model_matches_torch(name, mode):
    """C_g[orow(m)][n - n0] (+)= (alpha sum_k A B + bias) row_scale[orow(m)], group by group with torch.matmul; what lies outside stays"""
    case = _nt(name)
    bt = G.BuiltNT(case, mode)
    A, Bw = t64(bt.a.v), t64(bt.b.v)
    alpha = float(np.float32(case.alpha))
    n0 = 0
    for gi, g in enumerate(case.groups):
        want = t64(bt.c[gi].all).clone()
        for m in range(case.M):
            orow = m if not case.rows_in else (m // case.rows_in) * case.rows_out + m % case.rows_in
            v = alpha * (Bw[n0:n0 + g.N] @ A[m])
            if bt.bias[gi] is not None:
                v = v + t64(bt.bias[gi][G.GUARD:G.GUARD + g.N])
            if bt.scale is not None:
                v = v * float(bt.scale[G.GUARD + orow])
            want[orow, :g.N] = v + (want[orow, :g.N] if case.accumulate else 0.0)
        got = bt.outs[gi].ref[G.GUARD:G.GUARD + want.numel()].reshape(want.shape)
        t = bt.outs[gi].touched[G.GUARD:G.GUARD + want.numel()].reshape(want.shape)
        _close(got[t], want.numpy()[t])
        assert int(t.sum()) == case.M * g.N and not bt.outs[gi].touched[:G.GUARD].any() and not bt.outs[gi].touched[G.GUARD + want.numel():].any()
        if case.rows_in:
            assert not t[:bt.rows_c].reshape(-1, case.rows_out, g.ldc)[:, case.rows_in:].any()      # the unmapped rows of every block
        assert not t[bt.rows_c:].any()
        assert not t[:, g.N:].any()
        n0 += g.N


def test_nt_masked_rows_have_a_zero_bound():
    """row_scale == 0: the model's value and S are exactly 0 (bias included), so any non-zero output is over the gate"""
    bt = G.BuiltNT(_nt("t128.rows77to82"), BF16)
    zero = bt.orow[bt.scale[G.GUARD + bt.orow] == 0.0]
    assert zero.size > 10
    o = bt.outs[0]
    ld = bt.c[0].ld
    for r in zero[:5]:
        sl = slice(G.GUARD + r * ld, G.GUARD + r * ld + bt.case.groups[0].N)
        assert o.touched[sl].all() and (o.ref[sl] == 0).all() and (o.S[sl] == 0).all()


@pytest.mark.parametrize("store", [False, True])
def test_tn_model_matches_torch(store):
    bt = G.BuiltTN(G.TN_CASES[9], store)           # M = 300, (136, 264)
    case = bt.case
    want = float(np.float32(case.alpha)) * (t64(bt.a.v).t() @ t64(bt.b.v))
    if not store:
        want = want + t64(bt.c.v)
    ref = bt.out.ref[G.GUARD:G.GUARD + bt.c.all.size].reshape(bt.c.all.shape)
    _close(ref[:case.N, :case.K], want.numpy())
    assert int(bt.out.touched.sum()) == case.N * case.K


def _conv_torch(case, bt):
    """y of the case by torch, one batch element at a time (the per-element shift is a padding of its own)"""
    x = t64(bt.x.v).reshape(case.B, case.T_in, case.ci).permute(0, 2, 1)
    w = torch.stack([t64(m.v) for m in bt.w])                 # [taps][co][ci] as in memory
    ys = []
    for b in range(case.B):
        sh = 0 if case.shift_b is None else case.shift_b[b]
        if case.div > 1:        # ConvTranspose1d forward: stride 1, tap_rev, pad' = k - 1 - padding, div = the layer's stride
            assert case.tap_rev and case.stride == 1 and sh == 0
            wt = w.permute(2, 1, 0)                             # [ci][co][k]
            y = F.conv_transpose1d(x[b:b + 1], wt, None, stride=case.div, padding=case.taps - 1 - case.pad)
        else:
            left = case.pad - sh
            right = (case.T_out - 1) * case.stride + case.taps - left - case.T_in
            xp = F.pad(x[b:b + 1], (max(left, 0), max(right, 0)))
            xp = xp[..., max(-left, 0):xp.shape[-1] - max(-right, 0)]
            wt = w.permute(1, 2, 0)                             # [co][ci][k]
            y = F.conv1d(xp, wt.flip(-1) if case.tap_rev else wt, None, stride=case.stride)
        assert y.shape[-1] == case.T_out, (y.shape, case.T_out)
        ys.append(y[0].t())
    y = torch.cat(ys)
    if bt.bias is not None:
        y = y + t64(bt.bias[G.GUARD:G.GUARD + case.co])
    if bt.res is not None:
        y = y + t64(bt.res.v)
    return y.numpy()


@pytest.mark.parametrize("case", G.CONV_CASES, ids=[c.id for c in G.CONV_CASES])
def test_conv_model_matches_torch(case):
    bt = G.BuiltConv(case)
    M = case.B * case.T_out
    ref = bt.out.ref[G.GUARD:G.GUARD + bt.y.all.size].reshape(bt.y.all.shape)
    _close(ref[:M, :case.co], _conv_torch(case, bt))
    assert int(bt.out.touched.sum()) == M * case.co


def test_conv_model_data_gradient_matches_autograd():
    """the data gradient of a stride-1 convolution is the same form on dy with the taps reversed, pad' = taps - 1 - pad and the
    [taps][ci][co] copy of the weight"""
    rng = np.random.default_rng(3)
    B, T, ci, co, k, pad = 2, 19, 8, 12, 3, 1
    x = torch.from_numpy(rng.standard_normal((B, ci, T))).requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((co, ci, k)))
    dy = rng.standard_normal((B, T, co))
    F.conv1d(F.pad(x, (pad, k - 1 - pad)), w).backward(torch.from_numpy(dy).permute(0, 2, 1))
    case = G.Conv("dgrad", B, T, T, co, ci, k, 1, k - 1 - pad, tap_rev=True, bias=False)
    out, _, _ = G.conv_model(case, dy.reshape(B * T, co), w.permute(2, 1, 0).numpy(), None, None, np.zeros((B * T, ci)))
    _close(out, x.grad.permute(0, 2, 1).reshape(B * T, ci).numpy())


@pytest.mark.parametrize("case", G.TN_CONV_CASES[:-1], ids=[c.id for c in G.TN_CONV_CASES[:-1]])
def test_tn_conv_model_matches_autograd(case):
    bt = G.BuiltTNConv(case)
    x = t64(bt.x.v).reshape(case.B, case.T_in, case.ci).permute(0, 2, 1)
    dy = t64(bt.dy.v).reshape(case.B, case.T_out, case.co).permute(0, 2, 1)
    w = torch.zeros((case.co, case.ci, case.taps), dtype=torch.float64, requires_grad=True)
    bias = torch.zeros((case.co,), dtype=torch.float64, requires_grad=True)
    for b in range(case.B):
        sh = 0 if case.shift_b is None else case.shift_b[b]
        left = case.pad - sh
        right = (case.T_out - 1) * case.stride + case.taps - left - case.T_in
        xp = F.pad(x[b:b + 1], (max(left, 0), max(right, 0)))
        xp = xp[..., max(-left, 0):xp.shape[-1] - max(-right, 0)]
        F.conv1d(xp, w, bias, stride=case.stride).backward(dy[b:b + 1])
    alpha = float(np.float32(case.alpha))
    n = case.co * case.ci * case.taps
    _close(bt.out_w.ref[:n] - bt.gw[:n], alpha * w.grad.reshape(-1).numpy(), 1e-10)
    if case.gb:
        _close(bt.out_b.ref[:case.co] - bt.gb[:case.co], alpha * bias.grad.numpy(), 1e-10)


# ---------------------------------------------------------------------------------------------------------------------
# the wrong variants
# ---------------------------------------------------------------------------------------------------------------------
def _built():
    for i, c in enumerate(G.NT_CASES):
        for mode in c.modes():
            if c.wrong:
                yield c.form, f"{c.id}-{mode}", c.wrong, (lambda c=c, mode=mode, i=i: G.BuiltNT(c, mode, i))
    for i, c in enumerate(G.TN_CASES):
        for store in (False, True):
            yield ("tn_store" if store else "tn"), c.id, c.wrong, (lambda c=c, store=store, i=i: G.BuiltTN(c, store, i))
    for i, c in enumerate(G.CONV_CASES):
        yield "conv", c.id, c.wrong, (lambda c=c, i=i: G.BuiltConv(c, i))
    for i, c in enumerate(G.TN_CONV_CASES):
        yield "tn_conv", c.id, c.wrong, (lambda c=c, i=i: G.BuiltTNConv(c, i))


def test_every_variant_lies_far_outside_the_gate_where_it_is_listed():
    """each variant a case lists lies at least POWER x the GPU gate from the right answer there (or leaves a stored element unwritten /
    writes outside the output: inf), and every kernel shows every mistake it can make in at least one case"""
    shown, weak = set(), []
    for kernel, name, wrong, build in _built():
        if not wrong:
            continue
        bt = build()
        for w in wrong:
            assert w in G.ALL_WRONG and w in G.CAN_MAKE[kernel], (kernel, name, w)
            d = bt.distance(w)
            if d >= G.POWER:
                shown.add((kernel, w))
            else:
                weak.append((kernel, name, w, d))
    assert not weak, weak
    missing = [(k, w) for k, ws in G.CAN_MAKE.items() for w in ws if (k, w) not in shown]
    assert not missing, missing
    assert {w for ws in G.CAN_MAKE.values() for w in ws} == set(G.ALL_WRONG)


def test_the_right_model_is_at_distance_zero_and_unlisted_variants_do_not_matter():
    bt = G.BuiltNT(_nt("t128.N132.ldc132"), BF16)
    assert bt.distance(None) == 0.0
    for w in ("rowmap_in_for_out", "rowmap_off_by_one", "scale_at_gemm_row", "group_by_tile", "ragged_half_dropped", "swap_k_ring"):
        assert bt.distance(w) == 0.0, w          # no row map, no scale, one group, direct stores, two K steps


# ---------------------------------------------------------------------------------------------------------------------
# the row map in float32
# ---------------------------------------------------------------------------------------------------------------------
def test_row_map_expression_is_exact_below_the_bound():
    """q(m) = (int)((m + 0.5f) * (1.0f / rows_in)) for rows_in = 1 .. 4096 and every m < 2^22.  m + 0.5 is exact below 2^23 and a float32
    product with a positive constant, like the truncation, never decreases when m grows: q is right for every m of a block once it is
    right on the block's first row (q = k at m = k rows_in) and on its last (q = k at m = (k + 1) rows_in - 1).  Those two rows of every
    block are evaluated here; a few rows_in are swept over every m as well."""
    lim = G.ROW_LIMIT
    for r in range(1, 4097):
        k = np.arange(0, (lim - 1) // r + 1, dtype=np.int64)
        first = k * r
        last = np.minimum(first + r - 1, lim - 1)
        assert (G.row_map_f32(first, r) == k).all() and (G.row_map_f32(last, r) == k).all(), r
    m = np.arange(lim, dtype=np.int64)
    for r in (3, 77, 128, 129, 141, 1000):
        assert (G.row_map_f32(m, r) == m // r).all(), r


def test_row_map_expression_fails_above_the_bound():
    """what the new check keeps out: the first wrong quotient for rows_in = 1000 lies between 2^22 and the 2^24 rows the operand check allows"""
    m = np.arange(1 << 22, 1 << 23, dtype=np.int64)
    bad = m[G.row_map_f32(m, 1000) != m // 1000]
    assert bad.size and bad[0] == 5386999


# ---------------------------------------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------------------------------------
def test_route_restatement_on_the_production_shapes():
    """the sampling plan's stacked projection at B = 8 (1024 x 17408 x 1024, 13 groups of 256-column multiples) on 256 CUs: one round of
    256 x 272 tiles; with that form switched off, 16384 columns on 256 x 256 tiles and 1024 on the small ones.  The training pass's
    2 x 8 x 129 rows against the same weights as one group: 14336 columns on the big tiles."""
    assert G.route(1024, 17408, 1024, True, 13, 256) == dict(s272=True, n_big=0, wm=2)
    assert G.route(1024, 17408, 1024, True, 13, 256, s4=0) == dict(s272=False, n_big=16384, wm=2)
    assert G.route(2064, 17408, 1024, True, 1, 0) == dict(s272=False, n_big=14336, wm=2)      # 9 x 68 tiles: two whole rounds of big tiles
    # the natural-route cases of the GPU test (the 272 form switched off): the cut at 16384, moved to a group boundary
    assert G.route(770, 17408, 512, True, 1, 0, s4=0) == dict(s272=False, n_big=16384, wm=2)
    assert G.route(770, 17408, 512, True, 4, 4352, s4=0) == dict(s272=False, n_big=13056, wm=2)
    assert G.route(770, 17408, 512, True, 1, 0) == dict(s272=True, n_big=0, wm=2)
    # float32 and small products stay on the 128-column forms
    assert G.route(770, 17408, 512, False, 1, 0) == dict(s272=False, n_big=0, wm=2)
    assert G.route(300, 132, 128, True, 1, 0) == dict(s272=False, n_big=0, wm=2)
    for form, nt in (("t128", (False, 0, 2)), ("t256x128", (False, 0, 4)), ("t256", (False, 2176, 2)), ("s272", (True, 0, 2))):
        r = G.route(300, 2176, 128, True, 3, 256, **G.forced(form))
        assert (r["s272"], r["n_big"], r["wm"]) == nt, (form, r)


# ---------------------------------------------------------------------------------------------------------------------
# refusals of the C ABI: every one returns before anything is launched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return L.load()


def _args(**kw):
    g = L.BGemmArgs()
    g.a, g.b, g.c = 1 << 20, 1 << 21, 1 << 22          # never dereferenced: a refused call launches nothing
    g.M, g.Ntot, g.K, g.lda, g.ldb, g.n_groups, g.ldc = 300, 132, 64, 64, 64, 1, 132
    g.dtype, g.alpha = L.BF16, 1.0
    for k, v in kw.items():
        setattr(g, k, v)
    return g


REFUSED = [
    ("width", dict(Ntot=130, ldc=132), "multiple of 4"),
    ("width-f32", dict(Ntot=131, ldc=132, dtype=L.F32, K=32), "multiple of 4"),
    ("ldc-ragged", dict(ldc=134), "ldc"),
    ("ldc-short", dict(ldc=128), "ldc"),
    ("c-unaligned", dict(c=(1 << 22) + 4), "aligned"),
    ("c-f32-unaligned", dict(c=(1 << 22) + 8, c_f32=1), "aligned"),
    ("bias-unaligned", dict(bias=(1 << 23) + 8), "aligned"),
    ("rows_out-below-rows_in", dict(rows_in=128, rows_out=127), "row map"),
    ("rows_in-negative", dict(rows_in=-1, rows_out=4), "row map"),
    ("row-map-M-2^22", dict(rows_in=128, rows_out=129, M=1 << 22), "row map"),
    ("group_align-16", dict(groups=1 << 22, c=None, n_groups=3, Ntot=2176, group_align=16), "group_align"),
]


@pytest.mark.parametrize("name,kw,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_big_gemm_refuses(lib, name, kw, word):
    """the width / pitch / alignment contract of the 4-wide stores, the row map's bound and rows_out >= rows_in, and group boundaries
    finer than 128 columns (the group table is a made-up address: the call returns before anything reads it)"""
    assert lib.jen1_big_gemm(C.byref(_args(**kw)), None) != 0
    assert word in lib.jen1_last_error().decode(), lib.jen1_last_error()


def test_big_gemm_conv_refuses_ragged_widths_and_unaligned_bases(lib):
    ok = dict(x=1 << 20, w=1 << 21, bias=None, residual=None, y=1 << 22, B=2, T_in=50, T_out=50, ci=64, co=64, taps=3, stride=1, pad=1, tap_rev=0,
              ld_x=64, ld_w=64, w_tap_stride=64 * 64, ld_y=64, shift_b=None, div=1)
    for kw in (dict(co=62), dict(ld_y=66), dict(y=(1 << 22) + 4), dict(residual=(1 << 23) + 2), dict(bias=(1 << 23) + 4), dict(B=1 << 17, T_out=32)):
        a = dict(ok, **kw)
        assert lib.jen1_big_gemm_conv(*a.values(), None) != 0, kw
        assert "big_gemm_conv" in lib.jen1_last_error().decode()


def test_group_table_builder_checks_what_the_library_cannot_read():
    """a device table's widths, pitches and bases are the caller's promise: bgemm_group_table refuses them before it copies anything"""
    for grp in ((4096, None, 0, 130, 132), (4096, None, 0, 128, 130), (4096, None, 0, 128, 124), (4100, None, 0, 128, 128), (4096, 8200, 0, 128, 128)):
        with pytest.raises(L.Jen1HipError):
            L.bgemm_group_table([grp], "cpu")
    assert L.bgemm_group_table([(4096, 8192, 0, 128, 132)], "cpu").numel() == 32
