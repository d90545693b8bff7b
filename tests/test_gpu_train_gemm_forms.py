"""jen1_train_gemm form by form on the GPU against the float64 model of its descriptor (tests/train_gemm_common.py: the model, the
case table, the buffers and the gate; tests/test_train_gemm_refs_host.py pins the model against torch without a GPU).

Every case is one launch through GemmRuntime.gemm (the pair: one launch of two products).  Before it launches, a case asks
jen1_train_gemm_form which body its arguments run and fails unless it is the one the case is named for.  Every element the call stores is
compared with the model under the per-element gate |got - ref| <= 4 (n 2^-24 S + r |ref|); a NaN in the stored region (an operand read
outside what the descriptor addresses: everything there is NaN) and any change to C outside it fail the case.  The worst error / bound
ratio of every case goes to the parity log (profiles/train_gemm_forms_parity.txt is its summary by form and dtype).
"""
import pytest
import torch

import train_gemm_common as T
from helpers import record_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rts():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.gemm_host import GemmRuntime
    return {m: GemmRuntime(m) for m in T.MODES}


def _tdtype(mode):
    return torch.float32 if mode == T.F32 else torch.bfloat16


class OnDevice:
    """the buffers of a built case on the GPU and the arguments of its GemmRuntime.gemm call"""

    def __init__(self, rt, bt: T.Built):
        self.bt = bt
        case, mode = bt.case, bt.mode
        up = lambda key, m: torch.from_numpy(bt.bufs[key]).to(_tdtype(m)).cuda()
        self.a, self.b, self.c = up("a", mode), up("b", mode), up("c", bt.c_mode)
        self.residual = up("residual", bt.c_mode) if case.residual else None
        self.bias = up("bias", T.F32) if case.bias else None
        self.rowsum = up("rowsum", T.F32) if case.rowsum else None
        self.shift_b = None if bt.shift_b is None else torch.from_numpy(bt.shift_b).cuda()
        oa, ob = bt.operands(self.a.data_ptr(), self.b.data_ptr(), self.a.element_size())
        self.args = (oa, ob, self.c.data_ptr() + T.GUARD * self.c.element_size(), case.M, case.N, case.K)
        self.kw = dict(case.kw, dtype=rt.dt, ldc_m=case.ldc_m, bias=self.bias, rowsum=self.rowsum,
                       residual=None if self.residual is None else self.residual[T.GUARD:], shift_b=self.shift_b)

    def block(self, rt):
        return rt.gemm(*self.args, defer=True, **self.kw)

    def check(self):
        got = self.c.float().cpu().numpy()
        return self.bt.check(got, None if self.rowsum is None else self.rowsum.cpu().numpy())


def _assert_form(rt, blk, case, mode):
    form = rt.lib.jen1_train_gemm_form(blk)
    assert form == case.expected_form(mode), f"{case.id} {mode}: runs {T.form_name(form)}, meant for {T.form_name(case.expected_form(mode))}"


GRID = [(c, m) for c in T.CASES for m in c.modes]


@pytest.mark.parametrize("case,mode", GRID, ids=[f"{c.id}-{m}" for c, m in GRID])
def test_form_matches_the_model(rts, case, mode):
    rt = rts[mode]
    dev = OnDevice(rt, T.Built(case, mode, seed=T.CASES.index(case)))
    _assert_form(rt, dev.block(rt), case, mode)
    rt.gemm(*dev.args, **dev.kw)
    torch.cuda.synchronize()
    worst = dev.check()
    print(f"{case.id} {mode}: error / bound = {worst:.3f}")
    record_parity("train_gemm_forms." + case.group, case.name, mode, err_over_bound=worst)
    assert worst <= 1.0, f"{case.id} {mode}: error / bound = {worst}"


@pytest.mark.parametrize("mode", T.MODES)
def test_pair_matches_the_model(rts, mode):
    """jen1_train_gemm_pair against the model, product by product: a mapped weight gradient with rowsum and a skinny data gradient"""
    rt = rts[mode]
    first, second = (OnDevice(rt, T.Built(c, mode, seed=500 + i)) for i, c in enumerate(T.pair_cases(mode)))
    blk = first.block(rt)
    _assert_form(rt, blk, first.bt.case, mode)
    _assert_form(rt, second.block(rt), second.bt.case, mode)
    rt.gemm(*second.args, pair_with=blk, **second.kw)
    torch.cuda.synchronize()
    for dev in (first, second):
        worst = dev.check()
        print(f"{dev.bt.case.id} {mode}: error / bound = {worst:.3f}")
        record_parity("train_gemm_forms.pair", dev.bt.case.name, mode, err_over_bound=worst)
        assert worst <= 1.0, f"{dev.bt.case.id} {mode}: error / bound = {worst}"
