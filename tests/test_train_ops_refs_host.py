"""CPU: the float64 references of tests/train_ops_common.py are what torch.nn.functional computes, the gates of
tests/test_gpu_train_ops.py reject kernels that are wrong in the ways kernels go wrong, accept the float32 restatements, and every case
of the tables runs the kernel form it is named for (the jen1_*_form queries of include/jen1_train.h need no GPU)."""
import math

import pytest
import torch
import torch.nn.functional as F

import train_ops_common as T
from jen1_amd import lib as L

PIN = 1e-12


@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.load()


def _close(a, b, tol=PIN):
    return T.old_metric(a, b) <= tol


def _round_out(t, mode, f32_output=False):
    return t.float().double() if (mode == T.F32 or f32_output) else t.to(torch.bfloat16).double()


_GN = {c.name: c for c in T.GN_CASES}
_LN = {c.name: c for c in T.LN_CASES + T.LN2_CASES}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the references are torch.nn.functional in float64, and the hand-written backward in float64 is autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in T.GN_CASES if not c.mis and not c.fused0 and c.L <= 400], ids=lambda c: c.name)
def test_group_norm_reference_is_torch(case):
    d, ref = T.gn_inputs(case, T.F32), T.gn_ref(case, T.F32)
    B, C, L_ = case.B, case.C, case.L
    x, ga, be = (d[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    fl = d["film"].double().requires_grad_() if case.film else None
    h = F.group_norm(x.transpose(1, 2), case.G, ga, be, case.eps)                    # [B, C, L]
    if fl is not None:
        h = h * (fl[:, :C, None] + 1) + fl[:, C:2 * C, None]
    y = F.silu(h) if case.silu else h
    y.backward(d["dy"].double().transpose(1, 2))
    assert _close(ref["y"], y.detach().transpose(1, 2))
    dx = x.grad + sum(d[k].double() for k in ("dx_add", "dx_add2") if d[k] is not None)
    assert _close(ref["dx"], dx)
    assert _close(ref["dgamma"], ga.grad + d["dgamma0"].double()) and _close(ref["dbeta"], be.grad + d["dbeta0"].double())
    if fl is not None:
        assert _close(ref["dfilm"], fl.grad[:, :2 * C])
    man = T.gn_emul(case, d, torch.float64)
    for q in T.gn_quantities(case):
        assert _close(man[q], ref[q], 1e-11), q


@pytest.mark.parametrize("case", T.LN_CASES + T.LN2_CASES, ids=lambda c: c.name)
def test_layer_norm_reference_is_torch(case):
    d, ref = T.ln_inputs(case, T.F32), T.ln_ref(case, T.F32)
    x, ga, be = (d[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    y = F.layer_norm(x, (case.C,), ga, be, case.eps)
    loss = (y * d["dy"].double()).sum()
    if case.dual:
        ga2, be2 = d["gamma2"].double().requires_grad_(), d["beta2"].double().requires_grad_()
        y2 = F.layer_norm(x, (case.C,), ga2, be2, case.eps)
        loss = loss + (y2 * d["dy2"].double()).sum()
    loss.backward()
    assert _close(ref["y"], y.detach())
    assert _close(ref["dx"], x.grad if d["dx_add"] is None else x.grad + d["dx_add"].double())
    assert _close(ref["dgamma"], ga.grad + d["dgamma0"].double()) and _close(ref["dbeta"], be.grad + d["dbeta0"].double())
    xd = d["x"].double()
    assert _close(ref["stats"][:, 0], xd.mean(dim=1)) and _close(ref["stats"][:, 1], 1 / torch.sqrt(xd.var(dim=1, unbiased=False) + case.eps))
    if case.dual:
        assert _close(ref["y2"], y2.detach()) and _close(ref["dgamma2"], ga2.grad + d["dgamma20"].double())
        assert _close(ref["dbeta2"], be2.grad + d["dbeta20"].double())
    man = T.ln_emul(case, d, torch.float64)
    for q in T.ln_quantities(case) + ["dx"]:
        assert _close(man[q], ref[q], 1e-11), q


@pytest.mark.parametrize("mode_id", [0, 1, 2], ids=lambda m: T.ACT_NAMES[m])
def test_activation_reference_is_torch(mode_id):
    n = 5000
    x, dy = T.act_inputs(n, T.F32)
    ref = T.act_ref(mode_id, n, T.F32)
    xr = x.double().requires_grad_()
    y = (F.gelu, F.silu, F.elu)[mode_id](xr)
    y.backward(dy.double())
    # (torch's ELU backward is dy (y + 1) from the stored output, exact to 2^-53 of |dy| and no better: pinned against that scale)
    assert T.metric(ref["y"], y.detach()) <= PIN and T.metric(ref["dx"], xr.grad, ref["s:dx"] + (dy.double().abs() if mode_id == 2 else 0)) <= PIN
    ye, dxe = T.act_emul(mode_id, x, dy, torch.float64)
    assert T.metric(ye, ref["y"], ref["s:y"]) <= 1e-11 and T.metric(dxe, ref["dx"], ref["s:dx"]) <= 1e-11


@pytest.mark.parametrize("case", T.SOFTMAX_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_softmax_reference_is_torch(case):
    s, dp = T.softmax_inputs(case, T.F32)
    ref = T.softmax_ref(case, T.F32)
    sr = s.double().requires_grad_()
    p = F.softmax(sr.masked_fill(~T.softmax_keep(case), -math.inf), dim=-1)
    p.backward(dp.double())
    assert _close(ref["p"], p.detach()) and _close(ref["ds_autograd"], sr.grad)
    assert float((ref["p"].sum(dim=1) - 1).abs().max()) < PIN
    assert float((T.softmax_bwd_emul(ref["p"], dp, torch.float64) - ref["ds_autograd"]).abs().max()) < PIN       # the kernel's contract IS the gradient
    assert float((T.softmax_emul(case, s, torch.float64) - ref["p"]).abs().max()) < PIN


# ---------------------------------------------------------------------------------------------------------------------
# 2. the gates reject wrong kernels and accept the float32 restatements
# ---------------------------------------------------------------------------------------------------------------------
def _gn_got(case, mode, fault=None):
    out = T.gn_emul(case, T.gn_inputs(case, mode), fault=fault)
    return {q: _round_out(out[q], mode, q in ("sums", "dgamma", "dbeta") or (q == "dfilm" and not case.mirror)) for q in T.gn_quantities(case)}


def _ln_got(case, mode, fault=None):
    out = T.ln_emul(case, T.ln_inputs(case, mode), fault=fault)
    return {q: _round_out(out[q], mode, q not in ("y", "y2", "dx")) for q in T.ln_quantities(case)}


GN_FAULTS = ["count_minus_1", "skip_last_row", "last_vec_next_group", "gamma_off_by_one", "silu_no_term", "dx_add_twice", "dgamma_overwrite"]
LN_FAULTS = ["count_minus_1", "skip_last_row", "gamma_off_by_one", "dx_add_twice", "dgamma_overwrite"]


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name,fault", [(n, f) for n in ("f256-vpg1", "vec-cpg24", "f1024-exact", "pad257") for f in GN_FAULTS
                                        if not (f == "last_vec_next_group" and _GN[n].G == 1)])      # (one group has no next group)
def test_group_norm_gates_reject(name, fault, mode):
    case = _GN[name]
    gates = T.gn_gates(case, mode)
    assert T.failures(T.compare(_gn_got(case, mode, fault), T.gn_ref(case, mode), gates), gates)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("fault", LN_FAULTS)
@pytest.mark.parametrize("name", ["5x72", "600x128", "dual-130x1024+add", "3x65-ld72"])
def test_layer_norm_gates_reject(name, fault, mode):
    case = _LN[name]
    gates = T.ln_gates(case, mode)
    assert T.failures(T.compare(_ln_got(case, mode, fault), T.ln_ref(case, mode), gates), gates)


@pytest.mark.parametrize("mode", T.MODES)
def test_activation_gate_rejects_a_silu_derivative_without_its_second_term(mode):
    x, dy = T.act_inputs(5000, mode)
    ref = T.act_ref(1, 5000, mode)
    _, dx = T.act_emul(1, x, dy, fault="silu_no_term")
    assert T.metric(_round_out(dx, mode), ref["dx"], ref["s:dx"]) > T.act_gates(1, mode)["dx"]


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("case", [c for c in T.SOFTMAX_CASES if c[5]], ids=lambda c: "-".join(str(v) for v in c))
def test_softmax_gate_rejects_a_causal_limit_off_by_one(case, mode):
    s, _ = T.softmax_inputs(case, mode)
    ref = T.softmax_ref(case, mode)
    p = _round_out(T.softmax_emul(case, s, fault="causal_off_by_one"), mode)
    assert T.metric(p, ref["p"], ref["s:p"]) > T.softmax_gates(case, mode)["p"]


@pytest.mark.parametrize("mode", T.MODES)
def test_restatements_pass_every_gate_and_no_gate_is_looser_than_the_old_one(mode):
    """the unmodified float32 restatement, rounded to the output's dtype, passes at every case of every table; and every gate of every
    quantity, taken to test_gpu_train.py's metric (|err| <= gate (|ref| + s), so max|err| / max|ref| <= gate (1 + max s / max|ref|)),
    is under its bound"""
    def old(ref, gates):
        return {q: g * (1 + float(torch.as_tensor(ref.get("s:" + q, 0.0)).max() / ref[q].abs().max())) for q, g in gates.items()}
    for case in T.GN_CASES:
        gates, ref = T.gn_gates(case, mode), T.gn_ref(case, mode)
        assert not T.failures(T.compare(_gn_got(case, mode), ref, gates), gates), case.name
        assert all(v <= T.OLD_TOL[mode] for v in old(ref, gates).values()), (case.name, old(ref, gates))
    for case in T.LN_CASES + T.LN2_CASES:
        gates, ref = T.ln_gates(case, mode), T.ln_ref(case, mode)
        assert not T.failures(T.compare(_ln_got(case, mode), ref, gates), gates), case.name
        assert all(v <= T.OLD_TOL[mode] for v in old(ref, gates).values()), (case.name, old(ref, gates))
    for mode_id in (0, 1, 2):
        for n, _, _ in T.ACT_CASES:
            x, dy = T.act_inputs(n, mode)
            ref, gates = T.act_ref(mode_id, n, mode), T.act_gates(mode_id, mode)
            y, dx = T.act_emul(mode_id, x, dy)
            got = {"y": _round_out(y, mode), "dx": _round_out(dx, mode)}
            assert not T.failures(T.compare(got, ref, gates), gates), (mode_id, n)
            assert all(g <= T.OLD_TOL[mode] for g in gates.values())
    for case in T.SOFTMAX_CASES:
        s, dp = T.softmax_inputs(case, mode)
        ref, gates = T.softmax_ref(case, mode), T.softmax_gates(case, mode)
        got = {"p": _round_out(T.softmax_emul(case, s), mode), "ds": _round_out(T.softmax_bwd_emul(ref["p_in"], dp), mode)}
        assert not T.failures(T.compare(got, ref, gates), gates), case
        assert all(2 * g <= T.OLD_TOL[mode] for g in gates.values()), (case, gates)


# ---------------------------------------------------------------------------------------------------------------------
# 3. every case runs the form it is named for
# ---------------------------------------------------------------------------------------------------------------------
BASE = 0x7F0000000000            # an address on a 4 KB boundary; tensors 256 MB apart


def _fake(names, offsets, esize):
    """addresses: an aligned base plus offsets[name] elements of esize[name] bytes"""
    return {k: BASE + i * 0x10000000 + offsets.get(k, 0) * esize.get(k, 4) for i, k in enumerate(names)}


def _gn_ptrs(case, mode):
    es = 4 if mode == T.F32 else 2
    return _fake(("x", "y", "dy", "dx", "gamma", "beta", "film"), T.gn_offsets(case), {"x": es, "y": es, "dy": es, "dx": es, "film": es})


def _ln_ptrs(case, mode):
    es = 4 if mode == T.F32 else 2
    return _fake(("x", "y", "dy", "dx", "dx_add", "gamma", "beta"), {"x": 1} if case.mis else {}, {k: es for k in ("x", "y", "dy", "dx", "dx_add")})


@pytest.mark.parametrize("mode", T.MODES)
def test_every_case_runs_the_form_it_is_named_for(lib, mode, monkeypatch):
    seen_gn, seen_ln, seen_act = set(), set(), set()
    for case in T.GN_CASES:
        if case.fused0:
            monkeypatch.setenv("JEN1_GN_FUSED", "0")
        else:
            monkeypatch.delenv("JEN1_GN_FUSED", raising=False)
        forms = T.gn_forms(lib, case, _gn_ptrs(case, mode))
        assert forms == (case.sums, case.fwd, case.bwd), (case.name, forms)
        seen_gn.update(forms)
    monkeypatch.delenv("JEN1_GN_FUSED", raising=False)
    assert seen_gn == set(T.FORM_NAMES.values())
    for case in T.LN_CASES:
        forms = T.ln_forms(lib, case, _ln_ptrs(case, mode))
        assert forms == (case.fwd, case.bwd), (case.name, forms)
        seen_ln.update(forms)
    assert seen_ln == {"scalar", "vector"} | set(T.LN_BWD_NAMES.values())
    es = 4 if mode == T.F32 else 2
    for n, off, form in T.ACT_CASES + [(T.ACT_WRAP_VECTOR, 0, "vector")]:
        p = _fake(("x", "y", "dy", "dx"), {k: off for k in ("x", "y", "dy", "dx")}, {k: es for k in ("x", "y", "dy", "dx")})
        assert T.FORM_NAMES[lib.jen1_act_form(p["x"], p["y"], None, n)] == form
        assert T.FORM_NAMES[lib.jen1_act_form(p["dy"], p["x"], p["dx"], n)] == form
        seen_act.add(form)
    assert seen_act == {"scalar", "vector"}


@pytest.mark.parametrize("mode", T.MODES)
def test_one_misaligned_tensor_is_enough_for_the_scalar_form(lib, mode):
    """each pointer of a call, alone, one element off a 16-byte boundary"""
    es = 4 if mode == T.F32 else 2
    case = _GN["f256-vpg1"]
    shape = (case.B, case.L, case.C, case.ld, case.G)
    names = ("x", "y", "dy", "dx", "gamma", "beta", "film")
    for k in names:
        p = _fake(names, {k: 1}, {n: es for n in ("x", "y", "dy", "dx", "film")})
        fwd = lib.jen1_gn_forward_form(p["x"], p["gamma"], p["beta"], p["film"], case.film_ld, p["y"], *shape)
        bwd = lib.jen1_gn_backward_form(p["dy"], p["x"], p["gamma"], p["beta"], p["film"], case.film_ld, p["dx"], *shape)
        assert fwd == (L.FORM_FUSED256 if k in ("dy", "dx") else L.FORM_SCALAR), k
        assert bwd == (L.FORM_FUSED256 if k == "y" else L.FORM_SCALAR), k
    ln = _LN["600x128"]
    names = ("x", "y", "dy", "dx", "dx_add", "gamma", "beta")
    for k in names:
        p = _fake(names, {k: 1}, {n: es for n in ("x", "y", "dy", "dx", "dx_add")})
        fwd = lib.jen1_ln_forward_form(p["x"], p["gamma"], p["beta"], p["y"], ln.rows, ln.C, ln.ld)
        bwd = lib.jen1_ln_backward_form(p["dy"], p["x"], p["gamma"], p["dx"], p["dx_add"], ln.rows, ln.C, ln.ld)
        assert fwd == (L.FORM_SCALAR if k in ("x", "y", "gamma", "beta") else L.FORM_VECTOR), k
        assert bwd == (L.LN_BWD_VECTOR512 if k in ("y", "beta") else L.LN_BWD_SCALAR512), k
    for k in ("a", "b", "c"):
        p = _fake(("a", "b", "c"), {k: 1}, {n: es for n in "abc"})
        assert lib.jen1_act_form(p["a"], p["b"], p["c"], 5000) == L.FORM_SCALAR


def test_groups_of_2048_channels_take_the_three_launch_backward(lib, monkeypatch):
    """the one-launch backward would ask for 66 576 bytes of dynamic LDS with 256 threads (no attribute: 65 536 at most) and 168 000
    with 1024 (the attribute allows 163 840): the query, and with it the launch, answers with the three-launch form, and the forward
    with the two launches (the one-launch forms stop at 1024 channels per group).  Half the group width fits both."""
    monkeypatch.delenv("JEN1_GN_FUSED", raising=False)
    for case in T.GN_CPG2048:
        forms = T.gn_forms(lib, case, _gn_ptrs(case, T.F32))
        assert forms == (case.sums, case.fwd, case.bwd), (case.name, forms)
    p = _gn_ptrs(T.GN_CPG2048[0], T.F32)
    for L_, want in ((2, L.FORM_FUSED256), (16, L.FORM_FUSED1024)):
        assert lib.jen1_gn_backward_form(p["dy"], p["x"], p["gamma"], p["beta"], None, 0, p["dx"], 32, L_, 1024, 1024, 1) == want


def test_form_queries_reject_what_the_entry_points_reject(lib):
    p = _gn_ptrs(_GN["vec-plain"], T.F32)
    assert lib.jen1_gn_sums_form(p["x"], 2, 75, 128, 128, 7) == -1                   # 128 channels in 7 groups
    assert lib.jen1_gn_forward_form(p["x"], p["gamma"], p["beta"], None, 0, p["y"], 2, 75, 128, 120, 8) == -1      # ld < C
    assert lib.jen1_ln_forward_form(p["x"], p["gamma"], p["beta"], p["y"], 4, 2056, 2056) == -1
    assert lib.jen1_ln_backward_form(p["dy"], p["x"], p["gamma"], p["dx"], None, 0, 64, 64) == -1
    assert lib.jen1_act_form(p["x"], p["y"], None, 0) == -1
