"""-m gpu: the big GEMM family (csrc/big_gemm.hip) form by form through the C ABI against the float64 model of tests/big_gemm_common.py
(the model, the case tables, the buffers, the gate; tests/test_big_gemm_refs_host.py pins the model against torch and the power of its
wrong variants without a GPU).

Every case is one call.  The NT forms are forced with the switches the library reads (JEN1_BGEMM_T256 / _S4 per call; _WM once per
process: the 256 x 128 table runs in ONE child process with a time limit of its own), and a case first asks the restated route where its
arguments go and fails unless that is the form it is named for.  Every stored element is judged under the per-element gate
|got - ref| <= 4 (n 2^-24 S + r |ref|); a stored element that is not finite (an operand read outside what the contract addresses, or a
tile nobody wrote: both are NaN before the call) and any change outside the stored region fail the case.  The worst error / bound of
every case goes to the parity log (profiles/big_gemm_forms_parity.txt is its summary).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import big_gemm_common as G
from helpers import record_parity
from jen1_amd import lib as L

pytestmark = pytest.mark.gpu
BF16, F32, GUARD = G.BF16, G.F32, G.GUARD


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return L.load()


def _td(mode):
    return torch.float32 if mode == F32 else torch.bfloat16


def _up(flat, mode):
    return torch.from_numpy(np.ascontiguousarray(flat, dtype=np.float32)).to(_td(mode)).cuda()


def _at(t, elems=GUARD):
    return None if t is None else t.data_ptr() + elems * t.element_size()


def _host(t):
    return t.float().cpu().numpy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _verdict(test, case_id, mode, worst, **more):
    print(f"{test} {case_id} {mode}: error / bound = {worst:.3f}")
    record_parity("big_gemm_forms." + test, case_id, mode, err_over_bound=worst, **more)
    assert worst <= 1.0, f"{case_id} {mode}: error / bound = {worst}"


# ---------------------------------------------------------------------------------------------------------------------
# NT: jen1_big_gemm
# ---------------------------------------------------------------------------------------------------------------------
def _assert_route(case: G.NT, mode):
    r = G.route(case.M, case.Ntot, case.K_of(mode), mode == BF16, len(case.groups), case.group_align, **G.forced(case.form))
    want = {"t128": (False, 0, 2), "t256x128": (False, 0, 4), "t256": (False, case.Ntot, 2), "s272": (True, 0, 2)}[case.form]
    assert (r["s272"], r["n_big"], r["wm"]) == want, f"{case.id} {mode}: routed to {r}"


def run_nt(lib, bt: G.BuiltNT):
    """one jen1_big_gemm call on the buffers of a built case; returns the worst error / bound"""
    case, mode = bt.case, bt.mode
    a, b = _up(bt.a.flat, mode), _up(bt.b.flat, mode)
    cs = [_up(c.flat, bt.c_mode) for c in bt.c]
    biases = [None if v is None else _up(v, F32) for v in bt.bias]
    scale = None if bt.scale is None else _up(bt.scale, F32)
    g = L.BGemmArgs()
    g.a, g.b, g.row_scale = _at(a), _at(b), _at(scale)
    g.M, g.Ntot, g.K, g.lda, g.ldb, g.n_groups = case.M, case.Ntot, bt.K, bt.lda, bt.ldb, len(case.groups)
    g.rows_in, g.rows_out, g.c_f32, g.accumulate = case.rows_in, case.rows_out, int(case.c_f32), int(case.accumulate)
    g.dtype, g.alpha, g.group_align = (L.F32 if mode == F32 else L.BF16), case.alpha, case.group_align
    tab = None
    if case.inline:
        assert len(case.groups) == 1
        g.c, g.bias, g.ldc = _at(cs[0]), _at(biases[0]), case.groups[0].ldc
    else:
        rows, n0 = [], 0
        for grp, c, bias in zip(case.groups, cs, biases):
            rows.append((_at(c), _at(bias), n0, grp.N, grp.ldc))
            n0 += grp.N
        tab = L.bgemm_group_table(rows, a.device)
        g.groups = tab.data_ptr()
    L.check(lib.jen1_big_gemm(C.byref(g), _stream()), "jen1_big_gemm")
    torch.cuda.synchronize()
    return bt.judge([_host(c) for c in cs])


NT_GRID = [(c, m) for c in G.NT_CASES if c.form != "t256x128" for m in c.modes()]


@pytest.mark.parametrize("case,mode", NT_GRID, ids=[f"{c.id}-{m}" for c, m in NT_GRID])
def test_nt_form_matches_the_model(lib, monkeypatch, case, mode):
    for k in ("JEN1_BGEMM_T256", "JEN1_BGEMM_S4"):
        monkeypatch.delenv(k, raising=False)
    for k, v in G.FORMS[case.form].env.items():
        monkeypatch.setenv(k, v)
    _assert_route(case, mode)
    worst = run_nt(lib, G.BuiltNT(case, mode, seed=G.NT_CASES.index(case)))
    _verdict("nt." + case.form, case.name, mode, worst)


WM4_LIMIT_S = 120


def _wm4_child():
    """the child: every case of the 256 x 128 form in both dtypes, one JSON line each; stops at the first error that is not a verdict"""
    lib_ = L.load()
    bad = 0
    for i, case in enumerate(G.NT_CASES):
        if case.form != "t256x128":
            continue
        for mode in case.modes():
            _assert_route(case, mode)
            try:
                worst, why = run_nt(lib_, G.BuiltNT(case, mode, seed=i)), ""
            except AssertionError as e:
                worst, why = float("inf"), str(e)
            bad += not worst <= 1.0
            print("WM4 " + json.dumps(dict(case=case.name, mode=mode, worst=worst, why=why)), flush=True)
    print("WM4 DONE", flush=True)
    return bad


def test_256x128_form_matches_the_model_in_one_child_process():
    """JEN1_BGEMM_WM=4 from the start of a child process: big_gemm_nt_kernel<T, 4, 3> in both dtypes over the whole NT table of that form"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = dict(os.environ)
    for k in ("JEN1_BGEMM_T256", "JEN1_BGEMM_S4"):
        env.pop(k, None)
    env["JEN1_BGEMM_WM"] = "4"
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(L.__file__))), os.path.dirname(os.path.abspath(__file__))]
                                        + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=WM4_LIMIT_S, env=env)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the JEN1_BGEMM_WM=4 child did not finish within {WM4_LIMIT_S} s (killed):\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-4000:]}")
    lines = [json.loads(ln[4:]) for ln in r.stdout.splitlines() if ln.startswith("WM4 {")]
    for d in lines:
        record_parity("big_gemm_forms.nt.t256x128", d["case"], d["mode"], err_over_bound=d["worst"])
    want = sum(len(c.modes()) for c in G.NT_CASES if c.form == "t256x128")
    assert r.returncode == 0 and "WM4 DONE" in r.stdout and len(lines) == want, f"exit code {r.returncode}, {len(lines)} of {want} cases\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-4000:]}"
    over = [d for d in lines if not d["worst"] <= 1.0]
    assert not over, over


# the natural route: nothing forced but the 272 form switched off (it would take these shapes whole), so that the columns are cut between
# the 256 x 256 form and the 128 x 128 form; and once with nothing switched at all
NATURAL = [("one-group.cut", 1, dict(JEN1_BGEMM_S4="0"), dict(s272=False, n_big=16384, wm=2)),
           ("four-groups.cut-on-a-boundary", 4, dict(JEN1_BGEMM_S4="0"), dict(s272=False, n_big=13056, wm=2)),
           ("four-groups.auto", 4, {}, dict(s272=True, n_big=0, wm=2))]


@pytest.mark.parametrize("name,n_groups,env,want", NATURAL, ids=[n[0] for n in NATURAL])
def test_natural_route_writes_every_tile_once(lib, monkeypatch, name, n_groups, env, want):
    """M = 770, Ntot = 17408, K = 512 in bf16, stores into NaN: every element finite and inside the gate against a float64 product taken
    on the GPU, rows past M and the pitch columns untouched"""
    for k in ("JEN1_BGEMM_T256", "JEN1_BGEMM_S4"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    M, Ntot, K = 770, 17408, 512
    ga = Ntot // n_groups if n_groups > 1 else 0
    s4 = int(env.get("JEN1_BGEMM_S4", -1))
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert G.route(M, Ntot, K, True, n_groups, ga, 256, s4=s4) == want
    here = G.route(M, Ntot, K, True, n_groups, ga, n_cu, s4=s4)
    if here != want:
        pytest.skip(f"{n_cu} CUs route this product to {here}; the case is stated for 256 CUs ({want})")
    gen = torch.Generator(device="cuda").manual_seed(41)
    a = torch.full((M + 2, K), float("nan"), device="cuda", dtype=torch.bfloat16)
    b = torch.full((Ntot + 2, K), float("nan"), device="cuda", dtype=torch.bfloat16)
    a[:M] = (torch.randn((M, K), device="cuda", generator=gen) * 0.5).to(torch.bfloat16)
    b[:Ntot] = (torch.randn((Ntot, K), device="cuda", generator=gen) * 0.25).to(torch.bfloat16)
    N = Ntot // n_groups
    cs, rows = [], []
    for gi in range(n_groups):
        ldc = N + (8 if gi == 1 else 0)
        c = torch.full((M + 2, ldc), -224.0, device="cuda", dtype=torch.bfloat16)
        c[:M, :N] = float("nan")
        cs.append(c)
        rows.append((c.data_ptr(), None, gi * N, N, ldc))
    tab = L.bgemm_group_table(rows, a.device)
    g = L.BGemmArgs()
    g.a, g.b, g.groups = a.data_ptr(), b.data_ptr(), tab.data_ptr()
    g.M, g.Ntot, g.K, g.lda, g.ldb, g.n_groups = M, Ntot, K, K, K, n_groups
    g.dtype, g.alpha, g.group_align = L.BF16, 1.0, ga
    L.check(lib.jen1_big_gemm(C.byref(g), _stream()), "jen1_big_gemm")
    torch.cuda.synchronize()
    A, Bw = a[:M].double(), b[:Ntot].double()
    worst = 0.0
    for gi, c in enumerate(cs):
        ref = A @ Bw[gi * N:(gi + 1) * N].t()
        S = A.abs() @ Bw[gi * N:(gi + 1) * N].abs().t()
        got = c[:M, :N].double()
        assert bool(torch.isfinite(got).all()), f"{name}: {int((~torch.isfinite(got)).sum())} elements of group {gi} were never written"
        assert bool((c[M:] == -224.0).all()) and bool((c[:, N:] == -224.0).all()), f"{name}: group {gi}: written outside the output"
        bound = G.GATE_C * ((K + 3) * G.U24 * S + G.U8 * ref.abs())
        worst = max(worst, float(((got - ref).abs() / bound).max()))
    _verdict("nt.natural", name, BF16, worst, n_big=want["n_big"], s272=float(want["s272"]))


# ---------------------------------------------------------------------------------------------------------------------
# TN, TN-store
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [False, True], ids=["tn", "tn_store"])
@pytest.mark.parametrize("case", G.TN_CASES, ids=[c.id for c in G.TN_CASES])
def test_tn_forms_match_the_model(lib, case, store):
    bt = G.BuiltTN(case, store, seed=G.TN_CASES.index(case))
    a, b, c = _up(bt.a.flat, BF16), _up(bt.b.flat, BF16), _up(bt.c.flat, F32)
    fn = lib.jen1_big_gemm_tn_store if store else lib.jen1_big_gemm_tn
    L.check(fn(_at(a), _at(b), _at(c), case.M, case.N, case.K, case.lda, case.ldb, case.ldc, case.alpha, _stream()), "jen1_big_gemm_tn")
    torch.cuda.synchronize()
    worst = bt.out.judge(_host(c), case.id)
    _verdict("tn_store" if store else "tn", case.id, BF16, worst, splits=bt.splits)


# ---------------------------------------------------------------------------------------------------------------------
# the convolution forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CONV_CASES, ids=[c.id for c in G.CONV_CASES])
def test_conv_form_matches_the_model(lib, case):
    bt = G.BuiltConv(case, seed=G.CONV_CASES.index(case))
    x, w, y = _up(bt.x.flat, BF16), _up(bt.w_flat, BF16), _up(bt.y.flat, BF16)
    bias = None if bt.bias is None else _up(bt.bias, F32)
    res = None if bt.res is None else _up(bt.res.flat, BF16)
    sh = None if bt.shift_b is None else torch.from_numpy(bt.shift_b).cuda()
    L.check(lib.jen1_big_gemm_conv(_at(x), _at(w), _at(bias), _at(res), _at(y), case.B, case.T_in, case.T_out, case.ci, case.co, case.taps, case.stride,
                                   case.pad, int(case.tap_rev), bt.ld_x, bt.ld_w, bt.w_tap_stride, bt.ld_y, None if sh is None else sh.data_ptr(), case.div,
                                   _stream()), "jen1_big_gemm_conv")
    torch.cuda.synchronize()
    _verdict("conv", case.id, BF16, bt.out.judge(_host(y), case.id))


@pytest.mark.parametrize("case", G.TN_CONV_CASES, ids=[c.id for c in G.TN_CONV_CASES])
def test_tn_conv_form_matches_the_model(lib, case):
    bt = G.BuiltTNConv(case, seed=G.TN_CONV_CASES.index(case))
    dy, x = _up(bt.dy.flat, BF16), _up(bt.x.flat, BF16)
    gw, gb = _up(bt.gw, F32), _up(bt.gb, F32)
    sh = None if bt.shift_b is None else torch.from_numpy(bt.shift_b).cuda()
    L.check(lib.jen1_big_gemm_tn_conv(_at(dy), _at(x), gw.data_ptr(), gb.data_ptr() if case.gb else None, case.B, case.T_out, case.T_in, case.co, case.ci,
                                      case.taps, case.stride, case.pad, bt.ld_dy, bt.ld_x, case.alpha, None if sh is None else sh.data_ptr(), _stream()),
            "jen1_big_gemm_tn_conv")
    torch.cuda.synchronize()
    worst = bt.out_w.judge(_host(gw), case.id)
    if case.gb:
        worst = max(worst, bt.out_b.judge(_host(gb), case.id))
    else:
        assert np.array_equal(_host(gb), bt.gb), "gb is NULL in this call"
    _verdict("tn_conv", case.id, BF16, worst)


# ---------------------------------------------------------------------------------------------------------------------
# the small kernels
# ---------------------------------------------------------------------------------------------------------------------
MARGIN = 8.0            # x the float32 restatement's own error (the margin of test_gpu_codec_segments.py)


@pytest.mark.parametrize("mode", [F32, BF16])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("Cw", [4, 252, 256, 260, 1024])
def test_standardize_rows_matches_float64(lib, Cw, rows, mode):
    """per row: |y - ref| <= 8 e, ref = float64 on the values rounded to the compute dtype, e = the largest error over the row of a
    float32 restatement of the same two-moment formula written in the same dtype; with more than one row the last one is constant (the variance clamp: zeros);
    x and y at pitches wider than C, y inside a pattern"""
    rng = np.random.default_rng(Cw * 7 + rows)
    ldx, ldy, eps = Cw + 4, Cw + 8, 1e-5
    x = G.Mat(rows, Cw, ldx, F32)
    x.v[...] = (rng.standard_normal((rows, Cw)) + 0.5).astype(np.float32)
    if rows > 1:
        x.v[rows - 1] = 1.5
    y = G.Mat(rows, Cw, ldy, mode, pattern=True)
    xd, yd = _up(x.flat, F32), _up(y.flat, mode)
    L.check(lib.jen1_standardize_rows(_at(xd), _at(yd), rows, Cw, ldx, ldy, eps, L.F32 if mode == F32 else L.BF16, _stream()), "jen1_standardize_rows")
    torch.cuda.synchronize()
    got = _host(yd).astype(np.float64)
    ref, emul = G.standardize_ref(x.v, Cw, eps, mode)
    touched = np.zeros(y.flat.shape, dtype=bool)
    touched[GUARD:GUARD + y.all.size].reshape(y.all.shape)[:rows, :Cw] = True
    assert (got[~touched] == y.flat[~touched]).all(), "written outside the rows"
    out = got[GUARD:GUARD + y.all.size].reshape(y.all.shape)[:rows, :Cw]
    assert np.isfinite(out).all()
    e_row = np.abs(G.round_to(emul, mode) - ref).max(1, keepdims=True)
    err = np.abs(out - ref)
    print(f"standardize_rows C{Cw} rows{rows} {mode}: max|y-ref| {err.max():.3e} restatement {e_row.max():.3e}")
    record_parity("big_gemm_forms.standardize_rows", f"C{Cw}.rows{rows}", mode, max_err=err.max(), emul_err=e_row.max())
    assert rows == 1 or (out[rows - 1] == 0).all(), "a constant row standardises to zeros"
    assert (err <= MARGIN * e_row).all(), (float(err.max()), float(e_row.max()))


@pytest.mark.parametrize("mode", [F32, BF16])
def test_kv_fixed_fill_is_the_rounded_product(lib, mode):
    """out_l[b][n][:] = fixed_l[n][:] * mask[b][n], bit for bit the float32 product rounded to the compute dtype; layers of different width,
    one of them with more vectors than one pass of the grid covers (3 x 129 x 512 / 8 = 24 768 > 64 x 256), a mask that is not binary"""
    rng = np.random.default_rng(17)
    B, R = 3, 129
    mask = rng.choice(np.array([0.0, 1.0, 0.5, -1.25, 3.0], dtype=np.float32), size=(B, R))
    md = torch.from_numpy(mask).cuda()
    keep, tab = [], np.zeros((3, 4), dtype=np.int64)
    for i, C2 in enumerate((512, 64, 1024)):
        fixed = G.round_to(rng.standard_normal((R, C2)), mode)
        out = G._pattern(GUARD + B * R * C2 + GUARD, mode).copy()
        fd, od = _up(fixed, mode), _up(out, mode)
        keep.append((fixed, out, fd, od, C2))
        tab[i, 0], tab[i, 1], tab[i, 2] = fd.data_ptr(), _at(od), C2
    td = torch.from_numpy(tab).cuda()
    L.check(lib.jen1_kv_fixed_fill(td.data_ptr(), 3, md.data_ptr(), B, R, L.F32 if mode == F32 else L.BF16, _stream()), "jen1_kv_fixed_fill")
    torch.cuda.synchronize()
    for fixed, out, fd, od, C2 in keep:
        want = out.copy()
        want[GUARD:GUARD + B * R * C2] = G.round_to(fixed[None] * mask[:, :, None], mode).reshape(-1)
        assert np.array_equal(_host(od), want), C2


if __name__ == "__main__":          # the child of test_256x128_form_matches_the_model_in_one_child_process
    assert os.environ.get("JEN1_BGEMM_WM") == "4"
    sys.exit(1 if _wm4_child() else 0)
