"""-m gpu: the one-launch attention core of the training pass (csrc/train_attn.hip) through the C ABI, case by case of
tests/train_attn_common.py in f32 and bf16, and through train.attention_core (the host glue around it).

References, float32 yardsticks, the metric, the gates, the case table and the memory layout of each case are in
tests/train_attn_common.py (pinned on the CPU by tests/test_train_attn_refs_host.py).  Method of tests/test_gpu_train_ops.py, whose
``Buf`` and ``_call`` this module uses: every matrix lies inside a larger allocation with guard elements either side; outputs hold NaN
where a kernel writes and OTHER in the columns that belong to somebody else, which must come back bit-equal; inputs hold large finite
values in the columns no head reads and must come back unchanged.  Each case first asserts, by the restated ``rows_aligned`` on the
pointers it is about to pass, that q, k, v and dO are staged in the form the case is named for.  The forward runs on the case's inputs;
the backward runs on the reference's ``p_in`` (the float64 softmax rounded to the dtype), never on the forward's P, except in the
chained test, where the contract is evaluated on the P the forward wrote.  Every case writes its measured metrics and gates with
record_parity (profiles/train_attn_parity.txt).
"""
import pytest
import torch

import train_attn_common as A
from helpers import record_parity
from test_gpu_train_ops import Buf, _call, _same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rts():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.train import TrainRuntime
    return {"f32": TrainRuntime("f32"), "bf16": TrainRuntime("bf16")}


class AttnRun:
    """the matrices of one case on the device; forward() and backward() call the entry points and return {quantity: result}"""

    def __init__(self, rt, case, mode, p_in=None):
        self.rt, self.case, self.mode = rt, case, mode
        self.ops, mats = A.layout(case, mode)
        fill = A.host_fill(case, mode, p_in)
        self.esz = A.esize(mode)
        self.buf = {m: Buf(shape, rt.tdtype, fill[m], off // self.esz) for m, (shape, off) in mats.items()}
        d = A.attn_inputs(case, mode)
        self.mask = None if d["mask"] is None else Buf(d["mask"].shape, torch.float32, d["mask"])
        self.flags = None if case.causal_b is None else Buf((case.B,), torch.int32, d["flags"])
        self.kv_row = None if case.kv_row is None else Buf((case.B,), torch.int32, d["kv_row"].to(torch.int32))
        self.inputs = [self.buf[self.ops[o][0]] for o in A.INPUT_OPERANDS] + [b for b in (self.mask, self.flags, self.kv_row) if b is not None]

    def arg(self, op):
        """(pointer, pitch) of an operand"""
        m, c0, ld = self.ops[op]
        return self.buf[m].ptr + c0 * self.esz, ld

    def forms(self):
        return A.operand_forms(self.case, self.mode, {m: b.ptr for m, b in self.buf.items()})

    def view(self, op):
        m, c0, _ = self.ops[op]
        return self.buf[m].t[..., c0:c0 + self.case.C].cpu()

    def _others_kept(self, written):
        """the columns of the matrices of ``written`` operands that are not theirs are bit-equal, guards intact"""
        for m in {self.ops[o][0] for o in written}:
            b = self.buf[m]
            mine = torch.zeros(b.t.shape[-1], dtype=torch.bool)
            for o in written:
                if self.ops[o][0] == m:
                    mine[self.ops[o][1]:self.ops[o][1] + self.case.C] = True
            assert b.intact() and _same_bits(b.t[..., ~mine], b.before[..., ~mine]), m

    def _opt(self):
        p = lambda b: None if b is None else b.ptr                                   # noqa: E731
        return p(self.mask), p(self.flags), p(self.kv_row)

    def forward(self):
        c, rt = self.case, self.rt
        mask, flags, rows = self._opt()
        head = (*self.arg("q"), *self.arg("k"), *self.arg("v"), *self.arg("o"), *self.arg("p"), c.B, c.H, c.Nq, c.Nk, c.d, c.scale,
                c.causal, flags, mask)
        if rows is None:
            _call(rt, "jen1_attn_small_forward", *head, rt.dt)
        else:
            _call(rt, "jen1_attn_small_forward_rows", *head, rows, rt.dt)
        assert all(b.unchanged() for b in self.inputs)
        self._others_kept(["o"])
        pb = self.buf["p"]
        assert pb.intact()
        p = pb.t.cpu()
        assert _same_bits(p[..., c.Nk:], torch.zeros_like(p[..., c.Nk:]))           # padding columns [Nk, ldp): exactly 0
        p = p[..., :c.Nk].reshape(c.B, c.H, c.Nq, c.Nk)
        assert bool((p[~A.attn_ref(c, self.mode)["keep"]] == 0).all())               # keys the causal rule drops: exactly 0
        return {"p": p, "o": self.view("o")}

    def backward(self):
        c, rt = self.case, self.rt
        mask, _, rows = self._opt()
        pb = self.buf["p"]
        pb.freeze()
        head = (*self.arg("q"), *self.arg("k"), *self.arg("v"), *self.arg("p"), *self.arg("do"), *self.arg("dq"), *self.arg("dk"),
                *self.arg("dv"), c.B, c.H, c.Nq, c.Nk, c.d, c.scale, mask)
        if rows is None:
            _call(rt, "jen1_attn_small_backward", *head, rt.dt)
        else:
            _call(rt, "jen1_attn_small_backward_rows", *head, rows, rt.dt)
        assert all(b.unchanged() for b in self.inputs) and pb.unchanged()
        self._others_kept(["dq"])
        self._others_kept(["dk", "dv"])
        return {q: self.view(q) for q in A.BWD_Q}


def _report(kind, case, mode, metrics, gates):
    record_parity("train_attn", f"{kind}.{case.name}", mode, **metrics, **{q + ".gate": g for q, g in gates.items()})
    print(f"{kind}.{case.name} [{mode}] " + ", ".join(f"{q} {metrics[q]:.3e} (gate {gates[q]:.3e})" for q in gates))
    bad = A.failures(metrics, gates)
    assert not bad, (kind, case.name, mode, bad)


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_attention_small(rts, mode, case):
    rt = rts[mode]
    assert rt.lib.jen1_attn_small_fits(case.Nq, case.Nk, case.d, rt.dt) == 1
    ref, gates = A.attn_ref(case, mode), A.attn_gates(case, mode)
    fwd = AttnRun(rt, case, mode)
    assert fwd.forms() == case.form(mode)
    got = fwd.forward()
    bwd = AttnRun(rt, case, mode, ref["p_in"])
    assert bwd.forms() == case.form(mode)
    got.update(bwd.backward())
    _report("abi", case, mode, A.compare(got, ref, gates), gates)


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name", A.CHAINED)
def test_backward_on_the_forward_s_own_p(rts, mode, name):
    """forward, then backward on the P it wrote (padding columns and all): the backward is a pure function of (q, k, v, P, dO), so the
    reference is the contract in float64 on THAT P, under the case's gates"""
    case, rt = A.BY_NAME[name], rts[mode]
    run = AttnRun(rt, case, mode)
    p = run.forward()["p"]
    got = run.backward()
    ref = A.attn_bwd_ref(case, mode, p.double())
    gates = {q: g for q, g in A.attn_gates(case, mode).items() if q in A.BWD_Q}
    _report("chained", case, mode, A.compare(got, ref, gates), gates)


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name,nk", A.LDS_EDGE)
def test_one_key_past_the_lds_limit_is_refused(rts, mode, name, nk):
    """the case itself (test_attention_small) runs at the largest Nk that fits; one more and ``fits`` says no and all four entry points
    refuse before anything is launched"""
    case, rt = A.BY_NAME[name], rts[mode]
    assert max(n for n in range(1, 513) if rt.lib.jen1_attn_small_fits(case.Nq, n, case.d, rt.dt)) == nk == case.Nk
    assert rt.lib.jen1_attn_small_fits(case.Nq, nk + 1, case.d, rt.dt) == 0
    run = AttnRun(rt, case, mode)                      # (buffers of the smaller shape: a refusal touches nothing)
    fw = (*run.arg("q"), *run.arg("k"), *run.arg("v"), *run.arg("o"), run.arg("p")[0], A.pad8(nk + 1), case.B, case.H, case.Nq, nk + 1, case.d,
          case.scale, 0, None, None)
    bw = (*run.arg("q"), *run.arg("k"), *run.arg("v"), run.arg("p")[0], A.pad8(nk + 1), *run.arg("do"), *run.arg("dq"), *run.arg("dk"),
          *run.arg("dv"), case.B, case.H, case.Nq, nk + 1, case.d, case.scale, None)
    for fn, args in (("jen1_attn_small_forward", fw + (rt.dt, None)), ("jen1_attn_small_forward_rows", fw + (None, rt.dt, None)),
                     ("jen1_attn_small_backward", bw + (rt.dt, None)), ("jen1_attn_small_backward_rows", bw + (None, rt.dt, None))):
        assert getattr(rt.lib, fn)(*args) != 0 and b"do not fit one workgroup" in rt.lib.jen1_last_error(), fn
    torch.cuda.synchronize()
    assert all(b.unchanged() for b in run.buf.values())


# ---------------------------------------------------------------------------------------------------------------------
# train.attention_core / AttentionCoreFn: the host glue, against float64 autograd with the gather inside
# ---------------------------------------------------------------------------------------------------------------------
def _glue_ref(case, mode, summed):
    """autograd's o, dq and dK | dV (``summed``: [Bk, Nk, 2C], the sharers added up; else per batch element), the metric's scales and
    the gates: the kernel's gates, plus the distance between the two float64 references (autograd differentiates the exact softmax,
    the kernel's contract reads P rounded to the dtype: the saved P's rounding lies between the kernel and autograd whatever the
    kernel does), plus for the sum of the sharers' blocks one more rounding (each block is rounded, then their sum).  A sum's
    denominator is the sum of its blocks' denominators: each block may be off by its gate times its own |ref| + s."""
    d, ref, auto, gates = A.attn_inputs(case, mode), A.attn_ref(case, mode), A.attn_ref_autograd(case, mode), A.attn_gates(case, mode)
    rows, n = d["kv_row"], case.rows
    out = {"o": auto["o"], "s:o": ref["s:o"], "dq": auto["dq"], "s:dq": ref["s:dq"]}
    g = {"o": gates["o"] + A.metric(ref["o"], auto["o"], ref["s:o"]), "dq": gates["dq"] + A.metric(ref["dq"], auto["dq"], ref["s:dq"])}
    for q in ("dk", "dv"):
        if summed:
            den = A.sum_sharers(ref[q].abs() + ref["s:" + q], rows, n)
            out[q], out["s:" + q] = auto[q], den - auto[q].abs()
            dist = A.metric(A.sum_sharers(ref[q], rows, n), auto[q], out["s:" + q])
        else:
            out[q], out["s:" + q] = auto[q + "_b"], ref["s:" + q]
            dist = A.metric(ref[q], auto[q + "_b"], ref["s:" + q])
        g[q] = gates[q] + dist + (A.out_rounding(mode) if summed else 0.0)
    out["dkv"], out["s:dkv"] = torch.cat([out["dk"], out["dv"]], dim=-1), torch.cat([out["s:dk"], out["s:dv"]], dim=-1)
    g["dkv"] = max(g.pop("dk"), g.pop("dv"))
    return out, g


def _glue_inputs(rt, case, mode):
    d = A.attn_inputs(case, mode)
    q = d["q"].to("cuda", rt.tdtype).requires_grad_()
    kv = torch.cat([d["k"], d["v"]], dim=-1).to("cuda", rt.tdtype)
    mask = None if d["mask"] is None else d["mask"].cuda()
    rows = None if case.kv_row is None else d["kv_row"].to(torch.int32).cuda()
    return d, q, kv, mask, rows


def _glue_call(fn):
    from test_gpu_train_ops import _failed_calls
    if _failed_calls:
        pytest.fail(f"not run: {_failed_calls[0]} failed on the device earlier in this session")
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    except Exception:
        _failed_calls.append("train.attention_core")
        raise


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name", ["rows-01222", "rows-0111-H2"])
def test_attention_core_sums_the_sharers_rows(rts, mode, name):
    """kv_row without a slot: dK | dV are written per batch element and the last B - (Bk - 1) blocks summed in place
    (jen1_sum_rows_inplace); the gradient that comes back has Bk rows"""
    from jen1_amd import train as TR
    case, rt = A.BY_NAME[name], rts[mode]
    d, q, kv, mask, rows = _glue_inputs(rt, case, mode)
    kv.requires_grad_()

    def run():
        o = TR.attention_core(rt, q, kv, case.H, False, mask, rows)
        o.backward(d["do"].to("cuda", rt.tdtype))
        return o
    o = _glue_call(run)
    assert kv.grad.shape == (case.Bk, case.Nk, 2 * case.C)
    ref, gates = _glue_ref(case, mode, summed=True)
    got = {"o": o.detach().cpu(), "dq": q.grad.cpu(), "dkv": kv.grad.cpu()}
    _report("core.sum", case, mode, A.compare(got, ref, gates), gates)


@pytest.mark.parametrize("name", ["rows-01222", "rows-window"])
def test_attention_core_writes_a_kv_slot(rts, name):
    """kv_row with a KvSlot over a wider bf16 matrix (ContextKVFn's stacked gradient): K | V are read from a column window of a stacked
    projection, dK | dV come back per batch element in the slot's window, the other columns untouched, and the gradient autograd
    receives is the first Bk blocks of that window"""
    from jen1_amd import train as TR
    mode = A.BF16
    case, rt = A.BY_NAME[name], rts[mode]
    d, q, kv, mask, rows = _glue_inputs(rt, case, mode)
    C2, W, c0 = 2 * case.C, 2 * case.C + 24, 8
    stacked = torch.full((case.Bk, case.Nk, W), A.BIG, dtype=rt.tdtype, device="cuda")
    stacked[:, :, c0:c0 + C2] = kv
    stacked.requires_grad_()
    dall = Buf((case.B, case.Nk, W), rt.tdtype, torch.full((case.B, case.Nk, W), A.OTHER))
    slot = TR.KvSlot(dall.t[:, :, c0:c0 + C2])

    def run():
        o = TR.attention_core(rt, q, stacked[:, :, c0:c0 + C2], case.H, False, mask, rows, slot)
        o.backward(d["do"].to("cuda", rt.tdtype))
        return o
    o = _glue_call(run)
    mine = torch.zeros(W, dtype=torch.bool)
    mine[c0:c0 + C2] = True
    assert dall.intact() and _same_bits(dall.t[..., ~mine], dall.before[..., ~mine])
    g = stacked.grad
    assert g.shape == (case.Bk, case.Nk, W) and float(g[..., ~mine.cuda()].abs().max()) == 0
    assert _same_bits(g[..., c0:c0 + C2], dall.t[:case.Bk, :, c0:c0 + C2])              # the returned view: Bk rows of the slot
    ref, gates = _glue_ref(case, mode, summed=False)
    got = {"o": o.detach().cpu(), "dq": q.grad.cpu(), "dkv": dall.t[..., c0:c0 + C2].cpu()}
    _report("core.slot", case, mode, A.compare(got, ref, gates), gates)


@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name", ["causal-b101/flag0", "causal-b010/flag1"])
def test_attention_core_takes_causal_rows(rts, mode, name):
    """CausalRows with mixed flags: each batch element is masked by its own flag"""
    from jen1_amd import train as TR
    case, rt = A.BY_NAME[name], rts[mode]
    d, q, kv, mask, rows = _glue_inputs(rt, case, mode)
    kv.requires_grad_()

    def run():
        o = TR.attention_core(rt, q, kv, case.H, TR.CausalRows(d["flags"].cuda()))
        o.backward(d["do"].to("cuda", rt.tdtype))
        return o
    o = _glue_call(run)
    ref, gates = _glue_ref(case, mode, summed=True)
    got = {"o": o.detach().cpu(), "dq": q.grad.cpu(), "dkv": kv.grad.cpu()}
    _report("core.causal-rows", case, mode, A.compare(got, ref, gates), gates)
