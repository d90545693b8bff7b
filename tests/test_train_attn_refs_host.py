"""CPU: the float64 references of tests/train_attn_common.py are what torch computes, the kernel's contract backward is the gradient, the
gates of tests/test_gpu_train_attn.py accept the float32 restatements and reject every fault of ``FAULTS`` -- at the (case, quantity)
the tables below name, so that a case that stops exercising what it is in the table for fails here -- and every case's operands take
the staging form it is named for by the restated ``rows_aligned``."""
import pytest
import torch
import torch.nn.functional as F

import train_attn_common as A
from jen1_amd import lib as L

PIN = 1e-11


@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.load()


def _round_out(t, mode):
    return t.float().double() if mode == A.F32 else t.to(torch.bfloat16).double()


def _got(case, mode, fault=None):
    out = A.attn_emul(case, mode, fault=fault)
    return {q: _round_out(out[q], mode) for q in A.QUANTITIES}


def _rejected(case, mode, fault):
    gates = A.attn_gates(case, mode)
    return set(A.failures(A.compare(_got(case, mode, fault), A.attn_ref(case, mode), gates), gates))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the references
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_references_are_torch_and_the_contract_is_the_gradient(case, mode):
    d, ref, auto = A.attn_inputs(case, mode), A.attn_ref(case, mode), A.attn_ref_autograd(case, mode)
    H = case.H
    # the forward: torch's own attention on the gathered, masked, rounded rows
    k, v = A.staged_kv(case, d, mode)
    keep = A.keep_mask(case, d["flags"])[:, None]
    o = F.scaled_dot_product_attention(A._split(d["q"].double(), H), A._split(k, H), A._split(v, H), attn_mask=keep, scale=case.scale)
    assert A.metric(auto["o"], A._merge(o), ref["s:o"]) <= PIN and A.metric(auto["p"], ref["p"], ref["s:p"]) <= PIN
    assert float((ref["p"].sum(dim=-1) - 1).abs().max()) <= PIN and bool((ref["p"][~ref["keep"]] == 0).all())
    # the contract on the UNROUNDED p, the sharers' blocks added up, is autograd with the gather inside; per batch element it is the
    # gradient of the gathered rows
    con = A.attn_bwd_ref(case, mode, ref["p"])
    assert A.metric(con["dq"], auto["dq"], con["s:dq"]) <= PIN
    for q in ("dk", "dv"):
        assert A.metric(con[q], auto[q + "_b"], con["s:" + q]) <= PIN, q
        s = torch.sqrt(A.sum_sharers(con["s:" + q] ** 2, d["kv_row"], case.rows))
        assert A.metric(A.sum_sharers(con[q], d["kv_row"], case.rows), auto[q], s) <= PIN, q
    # the restatements in float64 are the references (o and the backward on p_in)
    man = A.attn_emul(case, mode, torch.float64)
    for q in A.QUANTITIES:
        assert A.metric(man[q], ref[q], ref["s:" + q]) <= PIN, q


def test_a_fully_masked_batch_element():
    """every key's K and V rows are zero: uniform p, o = 0, dK = dV = 0 (and dQ = 0: K is zero)"""
    case = A.BY_NAME["mask-full"]
    for mode in A.MODES:
        d, ref = A.attn_inputs(case, mode), A.attn_ref(case, mode)
        assert float(d["mask"][1].abs().max()) == 0 and all(float(d["mask"][b].sum()) > 0 for b in (0, 2))
        assert A.metric(ref["p"][1], torch.full_like(ref["p"][1], 1.0 / case.Nk)) <= PIN
        assert all(float(ref[q][1].abs().max()) == 0 for q in ("o", "dq", "dk", "dv"))
        assert all(float(ref[q][0].abs().max()) > 0 for q in ("o", "dq", "dk", "dv"))


def test_the_fractional_mask_entry_needs_a_rounding():
    """0.625 k is not a number of the dtype: the reference rounds the PRODUCT (a kernel that rounded first, or not at all, differs)"""
    case = A.BY_NAME["mask-frac"]
    for mode in A.MODES:
        d = A.attn_inputs(case, mode)
        k, _ = A.staged_kv(case, d, mode)
        exact = d["k"].double()[0, -1] * 0.625
        assert float(d["mask"][0, -1]) == 0.625 and bool((k[0, -1] != exact).any())
        assert bool(torch.equal(k[0, -1], A.rounded(exact, mode).double()))


def test_case_table_covers_what_the_kernels_branch_on():
    cs = A.CASES
    assert {(1, 1), (5, 7), (24, 24)} <= {(c.Nq, c.Nk) for c in cs}
    assert any(c.Nq == 64 for c in cs) and any(c.Nk in (129, 130) for c in cs) and any((c.Nq, c.Nk, c.d) == (1, 512, 32) for c in cs)
    assert {4, 128} <= {c.d for c in cs} and any(c.H == 1 for c in cs) and any(c.B == 1 for c in cs)
    assert any(c.causal and c.Nq == c.Nk for c in cs) and any(c.causal and (c.Nq, c.Nk) == (9, 13) for c in cs)
    assert {(c.causal, c.causal_b) for c in cs} >= {(0, (1, 0, 1)), (1, (1, 0, 1))}
    assert any(c.causal and c.mask for c in cs) and {"01", "full", "frac"} <= {c.mask for c in cs}
    assert any(c.kv_row == (0, 1, 2, 2, 2) and c.Bk == 3 and c.B == 5 for c in cs) and any(c.kv_row == (2, 0, 2, 1) for c in cs)
    assert all(c.mask for c in cs if c.kv_row) and all(not (c.causal or c.causal_b) or c.Nq <= c.Nk for c in cs)
    assert any(c.kv_joint >= 0 for c in cs) and any(c.dkv_window for c in cs)
    assert any(c.p_ld == A.pad8(c.Nk) and c.p_ld > c.Nk for c in cs) and any(c.p_ld == c.Nk + 3 for c in cs)
    for c in cs:                                      # sharers have different masks
        if c.kv_row:
            m = A.attn_inputs(c, A.F32)["mask"]
            rows = list(c.kv_row)
            assert any(rows[a] == rows[b] and not torch.equal(m[a], m[b]) for a in range(c.B) for b in range(a)), c.name
    for name, nk in A.LDS_EDGE:
        c = A.BY_NAME[name]
        assert c.Nk == nk and A.fits(c.Nq, nk, c.d) and not A.fits(c.Nq, nk + 1, c.d)
    hot = A.attn_inputs(A.BY_NAME["hot-row"], A.F32)
    sim = torch.einsum("bhid,bhjd->bhij", A._split(hot["q"], 2), A._split(hot["k"], 2)) * A.BY_NAME["hot-row"].scale
    assert float(sim[:, :, -1].max()) > 80 and float(sim[:, :, -1].min()) < -80 and float(sim[:, :, :-1].abs().max()) < 8


def test_fits_restated_is_the_library_s(lib):
    for Nq in (1, 24, 64, 65):
        for d in (4, 6, 64, 128, 132):
            for Nk in (1, 109, 110, 111, 121, 122, 512, 513):
                assert bool(lib.jen1_attn_small_fits(Nq, Nk, d, L.F32)) == A.fits(Nq, Nk, d), (Nq, Nk, d)
    for name, nk in A.LDS_EDGE:                       # the largest Nk the library accepts, found by asking it
        c = A.BY_NAME[name]
        assert max(n for n in range(1, 513) if lib.jen1_attn_small_fits(c.Nq, n, c.d, L.BF16)) == nk


# ---------------------------------------------------------------------------------------------------------------------
# 2. the gates accept the float32 restatements and reject the faults
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.MODES)
def test_restatements_pass_every_gate_and_no_gate_is_looser_than_the_old_one(mode):
    worst = {}
    for case in A.CASES:
        gates, ref = A.attn_gates(case, mode), A.attn_ref(case, mode)
        m = A.compare(_got(case, mode), ref, gates)
        assert not A.failures(m, gates), (case.name, A.failures(m, gates))
        for q, g in gates.items():
            if g > 0 and m[q] / g > worst.get(q, (0.0, ""))[0]:
                worst[q] = (m[q] / g, case.name)
            top = float(ref[q].abs().max())
            # |err| <= gate (|ref| + s): tests/test_gpu_train.py's metric max|err| / max|ref| stays under its tolerance
            assert top == 0 or g * (1 + float(ref["s:" + q].max()) / top) <= A.OLD_TOL[mode] * (1 + 1e-12), (case.name, q)
    print(f"[{mode}] the float32 restatement's worst metric / gate: " + ", ".join(f"{q} {r:.2f} ({n})" for q, (r, n) in worst.items()))
    assert all(r <= 1 for r, _ in worst.values())


# fault -> [(case, modes, the quantities that must reject it there)]
BOTH = tuple(A.MODES)
REJECTED_BY = {
    "causal_off_by_one": [("24x24-causal", BOTH, "p o"), ("9x13-causal", BOTH, "p o"), ("64x64-causal", BOTH, "p o"),
                          ("lds-64x121-d64", BOTH, "p o"), ("causal-b101/flag0", BOTH, "p o"), ("9x13-causal-mask", BOTH, "p o")],
    "causal_b_ignored": [("causal-b101/flag0", BOTH, "p o"), ("causal-b101/flag1", BOTH, "p o"), ("causal-b010/flag1", BOTH, "p o")],
    "kv_row_ignored": [("rows-2021", BOTH, "p o dq dk")],
    "mask_by_kv_row": [("rows-01222", BOTH, "p o dq dk dv"), ("rows-0111-H2", BOTH, "p o dq dk dv"), ("rows-2021", BOTH, "p o dq dk dv"),
                       ("rows-window", BOTH, "p o dq dk dv")],
    "mask_not_in_dk": [("mask-01", BOTH, "dk"), ("mask-full", BOTH, "dk"), ("mask-frac", BOTH, "dk"), ("9x13-causal-mask", BOTH, "dk"),
                       ("kv-joint-window", BOTH, "dk"), ("rows-01222", BOTH, "dk")],
    # (float32 mode rounds nothing; in bf16 the unrounded product is CLOSER to the exact softmax and further from what the backward
    # pass will read: uniform rows over a V with an offset make every term's rounding pull the same way)
    "p_unrounded_in_pv": [("coherent-6x60", (A.BF16,), "o")],
    "scale_missing_dq": [("5x7", BOTH, "dq"), ("d4", BOTH, "dq"), ("d128-H1", BOTH, "dq"), ("1x512-d32", BOTH, "dq")],
    "scale_missing_dk": [("5x7", BOTH, "dk"), ("d4", BOTH, "dk"), ("d128-H1", BOTH, "dk"), ("1x512-d32", BOTH, "dk")],
    "dv_from_ds": [("5x7", BOTH, "dv"), ("24x24", BOTH, "dv"), ("1x512-d32", BOTH, "dv"), ("mask-full", BOTH, "dv")],
    "last_key_dropped": [("5x7", BOTH, "p o"), ("5x129", BOTH, "p o"), ("1x512-d32", BOTH, "p o"), ("lds-24x110-d128", BOTH, "p o"),
                         ("1x1", BOTH, "p o")],
    "last_query_row_stale": [("5x7", BOTH, "p o dq"), ("64x64-causal", BOTH, "p o dq"), ("24x24", BOTH, "p o dq"), ("1x1", BOTH, "p o")],
    "head_stride_wrong": [("5x7", BOTH, "p o dq dk dv"), ("d4", BOTH, "p o dq dk dv"), ("d12", BOTH, "p o dq dk dv"),
                          ("24x24", BOTH, "p o dq dk dv")],
}


def test_the_table_names_every_fault():
    assert set(REJECTED_BY) == set(A.FAULTS)


@pytest.mark.parametrize("fault", A.FAULTS)
def test_gates_reject(fault):
    for name, modes, qs in REJECTED_BY[fault]:
        for mode in modes:
            assert set(qs.split()) <= _rejected(A.BY_NAME[name], mode, fault), (fault, name, mode, _rejected(A.BY_NAME[name], mode, fault))


@pytest.mark.parametrize("mode", A.MODES)
def test_every_case_rejects_the_faults_of_what_it_exercises(mode):
    """whatever a case is in the table for, the gates see when it goes wrong there"""
    for c in A.CASES:
        if c.causal or (c.causal_b and any(c.causal_b)):
            assert "p" in _rejected(c, mode, "causal_off_by_one"), c.name
        if c.causal_b:
            assert "p" in _rejected(c, mode, "causal_b_ignored"), c.name
        if c.mask:
            assert "dk" in _rejected(c, mode, "mask_not_in_dk"), c.name
        if c.kv_row:
            assert {"dk", "dv"} <= _rejected(c, mode, "mask_by_kv_row"), c.name
        if c.H > 1 and not c.coherent:
            assert {"o", "dv"} <= _rejected(c, mode, "head_stride_wrong"), c.name
        assert "p" in _rejected(c, mode, "last_query_row_stale"), c.name
        if c.name != "hot-row-causal":                # (only the hot row keeps the last key, with a weight that may be nothing)
            assert "p" in _rejected(c, mode, "last_key_dropped"), c.name
        if c.Nk > 1 and not c.coherent:               # (one key: dS = 0; q = 0: dK = 0)
            assert "dq" in _rejected(c, mode, "scale_missing_dq") and "dk" in _rejected(c, mode, "scale_missing_dk"), c.name
        assert "dv" in _rejected(c, mode, "dv_from_ds"), c.name


# ---------------------------------------------------------------------------------------------------------------------
# 3. every case's operands take the form it is named for
# ---------------------------------------------------------------------------------------------------------------------
BASE = 0x7F0000000000            # an address on a 4 KB boundary; matrices 256 MB apart


def _fake_bases(case, mode):
    _, mats = A.layout(case, mode)
    return {m: BASE + i * 0x10000000 + off for i, (m, (_, off)) in enumerate(sorted(mats.items()))}


@pytest.mark.parametrize("mode", A.MODES)
def test_every_case_runs_the_forms_it_is_named_for(mode):
    seen = set()
    for c in A.CASES:
        got = A.operand_forms(c, mode, _fake_bases(c, mode))
        assert got == c.form(mode), (c.name, mode, got)
        seen.add(got)
    assert {"vvvv", "ssss", "vsvs"} <= seen


def test_the_form_rule():
    for esz, v in ((4, 4), (2, 8)):
        assert A.rows_aligned(BASE, 8 * v, 2 * v, esz)
        assert not A.rows_aligned(BASE, 8 * v, 2 * v + 4, esz) or esz == 4                 # d % V (float32: every d % 4 == 0 passes)
        assert not A.rows_aligned(BASE, 8 * v + 2, 2 * v, esz)                              # ld % V
        assert not A.rows_aligned(BASE + 4, 8 * v, 2 * v, esz) and not A.rows_aligned(BASE + 8, 8 * v, 2 * v, esz)
    # bf16: d = 12 and 20 are scalar, float32 vector; a pitch of H d + 4 likewise
    by = A.BY_NAME
    assert by["d12"].forms == by["d20"].forms == by["d8-ld+4"].forms == by["d4"].forms == ("vvvv", "ssss")
    assert by["d8-ld+2"].forms == by["d8-off4"].forms == by["d8-off8"].forms == ("ssss", "ssss")


def test_layouts_stay_inside_their_matrices():
    """every address a kernel may touch lies inside the matrix the layout allots (checked before anything runs on a device)"""
    for mode in A.MODES:
        for c in A.CASES:
            ops, mats = A.layout(c, mode)
            for op, (m, c0, ld) in ops.items():
                shape, off = mats[m]
                assert ld == shape[-1] and off % A.esize(mode) == 0
                width = c.p_ld if op == "p" else c.C
                rows = {"q": c.B, "do": c.B, "o": c.B, "dq": c.B, "dk": c.B, "dv": c.B, "k": c.rows, "v": c.rows, "p": c.B * c.H}[op]
                n = c.Nq if op in ("q", "do", "o", "dq", "p") else c.Nk
                assert (rows, n) == shape[:2] and 0 <= c0 and c0 + width <= ld, (c.name, op)
            fill = A.host_fill(c, mode)
            assert all(fill[m].shape == tuple(mats[m][0]) for m in mats)
