"""-m gpu: the GroupNorm, LayerNorm, activation and softmax kernels of the training pass (csrc/train_ops.hip), entry point by entry
point through the C ABI, every kernel form of every entry point, in f32 and bf16.

References, float32 yardsticks, the metric, the gates and the case tables are in tests/train_ops_common.py (pinned on the CPU by
tests/test_train_ops_refs_host.py).  Method of tests/test_gpu_train_glue.py: every output lies inside a larger allocation with guard
elements either side, NaN where the kernel writes, a non-zero pattern where it accumulates (dgamma, dbeta), NaN in the scratch the
contract says the call resets (P, Gm, sums); padding columns of inputs hold large finite values no result may depend on, padding
columns of y and dx hold 0 and must come back bit-equal; in bf16 mode the inputs are rounded first and then handed to the float64
reference.  Each case first asserts, through the jen1_*_form queries on the pointers it is about to pass, that it runs the kernel
form it is named for.  Every case writes its measured metrics and gates with record_parity (profiles/train_ops_parity.txt).
"""
import pytest
import torch

import train_ops_common as T
from helpers import record_parity

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements either side of a buffer (a multiple of 8: 16-byte alignment survives in both dtypes)
GUARD_VALUE = -7.25
OTHER = 5.5                     # columns of a shared buffer that belong to somebody else


@pytest.fixture(scope="module")
def rts():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.train import TrainRuntime
    return {"f32": TrainRuntime("f32"), "bf16": TrainRuntime("bf16")}


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


class Buf:
    """a tensor of ``shape`` inside a larger allocation, ``off`` elements past a 16-byte boundary.  ``fill`` None: NaN (a buffer the
    kernel writes), else its values (an input, or a buffer that is accumulated into).  ``intact()``: no element outside changed;
    ``unchanged()``: nor any inside (inputs)."""

    def __init__(self, shape, dtype, fill=None, off=0):
        n = 1
        for v in shape:
            n *= int(v)
        self.whole = torch.full((n + 2 * GUARD + 8,), GUARD_VALUE, dtype=dtype, device="cuda")
        self.lo = GUARD + off
        self.t = self.whole[self.lo:self.lo + n].view(*shape)
        assert self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        if fill is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(fill)
        self.before = self.t.clone()
        self.n = n

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        g = torch.cat([self.whole[:self.lo], self.whole[self.lo + self.n:]])
        return _same_bits(g, torch.full_like(g, GUARD_VALUE))

    def unchanged(self):
        return self.intact() and _same_bits(self.t, self.before)

    def freeze(self):
        """what a call wrote becomes the state a later call must leave alone"""
        self.before = self.t.clone()


def _padded(t, ld, pad):
    """[..., C] -> [..., ld] with ``pad`` in the padding columns"""
    out = torch.full(t.shape[:-1] + (ld,), float(pad), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def _inp(t, dtype, ld=None, off=0, pad=T.BIG):
    return Buf(t.shape[:-1] + (ld or t.shape[-1],), dtype, _padded(t, ld or t.shape[-1], pad), off)


def _out(shape, C, dtype, off=0):
    """an output with padding columns: NaN in [..., :C], 0 in [..., C:]"""
    fill = torch.zeros(shape)
    fill[..., :C] = float("nan")
    return Buf(shape, dtype, fill, off)


_failed_calls = []


def _call(rt, name, *args):
    """one entry point, then a synchronize; after a call that failed nothing more of this module is launched on the device"""
    from jen1_amd import lib as L
    if _failed_calls:
        pytest.fail(f"not run: {_failed_calls[0]} failed on the device earlier in this session")
    try:
        L.check(getattr(rt.lib, name)(*args, rt.stream()), name)
        torch.cuda.synchronize()
    except Exception:
        _failed_calls.append(name)
        raise


def _padding_kept(buf, C):
    """padding columns bit-equal to their prefill, guards intact"""
    return buf.intact() and _same_bits(buf.t[..., C:], buf.before[..., C:])


def _report(kind, name, mode, metrics, gates):
    record_parity("train_ops", f"{kind}.{name}", mode, **metrics, **{q + ".gate": g for q, g in gates.items()})
    print(f"{kind}.{name} [{mode}] " + ", ".join(f"{q} {metrics[q]:.3e} (gate {gates[q]:.3e})" for q in gates))
    bad = T.failures(metrics, gates)
    assert not bad, (kind, name, mode, bad)


def _set_fused(monkeypatch, off):
    if off:
        monkeypatch.setenv("JEN1_GN_FUSED", "0")
    else:
        monkeypatch.delenv("JEN1_GN_FUSED", raising=False)


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------
class GnRun:
    """the buffers of one GroupNorm case on the device; forward() and backward() call the entry points and return {quantity: result}"""

    def __init__(self, rt, case, mode):
        self.rt, self.case = rt, case
        B, C, L_, G, ld = case.B, case.C, case.L, case.G, case.ld
        d, o, td = T.gn_inputs(case, mode), T.gn_offsets(case), rt.tdtype
        self.x = _inp(d["x"], td, ld, o["x"])
        self.dy = _inp(d["dy"], td, ld, o["dy"])
        self.gamma, self.beta = _inp(d["gamma"], torch.float32, off=o["gamma"]), _inp(d["beta"], torch.float32, off=o["beta"])
        self.film = None
        if case.film:
            f = d["film"].clone()
            f[:, 2 * C:] = T.BIG                                       # film_ld > 2C: columns that are not this block's
            self.film = Buf(f.shape, td, f, o["film"])
        self.adds = [None if d[k] is None else _inp(d[k], td, ld) for k in ("dx_add", "dx_add2")]
        self.y, self.dx = _out((B, L_, ld), C, td, o["y"]), _out((B, L_, ld), C, td, o["dx"])
        self.sums = Buf((B, G, 2), torch.float32)
        self.dgamma, self.dbeta = Buf((C,), torch.float32, d["dgamma0"]), Buf((C,), torch.float32, d["dbeta0"])
        self.P, self.Gm = Buf((B, C, 4), torch.float32), Buf((B, G, 2), torch.float32)
        self.dfilm = None
        if case.film:
            if case.mirror:
                fill = torch.full((B, case.film_ld), OTHER)
                fill[:, :2 * C] = float("nan")
                self.dfilm = Buf((B, case.film_ld), td, fill)
            else:
                self.dfilm = Buf((B, 2 * C), torch.float32)
        self.shape = (B, L_, C, ld, G)

    def _fp(self):
        return (None, 0) if self.film is None else (self.film.ptr, self.case.film_ld)

    def forms(self):
        ptr = {k: getattr(self, k).ptr for k in ("x", "y", "dy", "dx", "gamma", "beta")}
        ptr["film"] = None if self.film is None else self.film.ptr
        return T.gn_forms(self.rt.lib, self.case, ptr)

    def forward(self):
        c = self.case
        _call(self.rt, "jen1_gn_forward", self.x.ptr, self.sums.ptr, self.gamma.ptr, self.beta.ptr, *self._fp(), self.y.ptr, *self.shape,
              c.eps, c.flags, self.rt.dt)
        assert _padding_kept(self.y, c.C) and self.sums.intact()
        self.sums.freeze()
        assert all(b.unchanged() for b in (self.x, self.gamma, self.beta)) and (self.film is None or self.film.unchanged())
        return {"y": self.y.t[..., :c.C].cpu(), "sums": self.sums.t.cpu()}

    def backward(self, sums=None):
        c = self.case
        sums = self.sums if sums is None else sums
        _call(self.rt, "jen1_gn_backward_add2", self.dy.ptr, self.x.ptr, sums.ptr, self.gamma.ptr, self.beta.ptr, *self._fp(), self.dx.ptr,
              *[None if a is None else a.ptr for a in self.adds], self.dgamma.ptr, self.dbeta.ptr, None if self.dfilm is None else self.dfilm.ptr,
              self.P.ptr, self.Gm.ptr, *self.shape, c.eps, c.flags, self.rt.dt)
        assert _padding_kept(self.dx, c.C)
        assert all(b.intact() for b in (self.dgamma, self.dbeta, self.P, self.Gm))
        assert all(b.unchanged() for b in [self.x, self.dy, sums, self.gamma, self.beta] + [a for a in self.adds if a is not None])
        got = {"dx": self.dx.t[..., :c.C].cpu(), "dgamma": self.dgamma.t.cpu(), "dbeta": self.dbeta.t.cpu()}
        if self.dfilm is not None:
            assert _padding_kept(self.dfilm, 2 * c.C) and self.film.unchanged()              # (mirror: the other blocks' columns)
            got["dfilm"] = self.dfilm.t[:, :2 * c.C].cpu()
        return got


def _split(gates, names):
    return {q: g for q, g in gates.items() if q in names}


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("case", T.GN_CASES, ids=lambda c: c.name)
def test_group_norm(rts, mode, case, monkeypatch):
    _set_fused(monkeypatch, case.fused0)
    run = GnRun(rts[mode], case, mode)
    assert run.forms() == (case.sums, case.fwd, case.bwd)
    ref, gates = T.gn_ref(case, mode), T.gn_gates(case, mode)
    got = run.forward()
    got.update(run.backward())
    _report("gn", case.name, mode, T.compare(got, ref, gates), gates)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("name", ["f256-vpg1", "f256-vpg16-L1", "f1024-exact"])
def test_group_norm_sums_serve_the_other_form(rts, mode, name, monkeypatch):
    """sums written by the one-launch forward and by the two launches agree within the gate, and each backward form passes its gates on
    the sums the OTHER forward form wrote"""
    fused = next(c for c in T.GN_CASES if c.name == name)
    plain = next(c for c in T.GN_CASES if c.name == name + "/off")
    ref = T.gn_ref(fused, mode)
    runs = {}
    for case in (fused, plain):
        _set_fused(monkeypatch, case.fused0)
        runs[case] = GnRun(rts[mode], case, mode)
        assert runs[case].forms() == (case.sums, case.fwd, case.bwd)
        runs[case].forward()
    a, b = runs[fused].sums.t.cpu(), runs[plain].sums.t.cpu()
    gate = max(T.gn_gates(fused, mode)["sums"], T.gn_gates(plain, mode)["sums"])
    m = T.metric(a, b, ref["s:sums"])
    metrics = {"sums_between_forms": m}
    assert m <= gate, (m, gate)
    for case, other in ((fused, plain), (plain, fused)):
        _set_fused(monkeypatch, case.fused0)
        gates = _split(T.gn_gates(case, mode), T.GN_BACKWARD_Q)
        res = T.compare(runs[case].backward(runs[other].sums), ref, gates)
        assert not T.failures(res, gates), (case.name, T.failures(res, gates))
        metrics.update({f"{q}.{case.bwd}": v for q, v in res.items()})
    record_parity("train_ops", f"gn.{name}.crossed-sums", mode, **metrics)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("case", T.LN_CASES, ids=lambda c: c.name)
def test_layer_norm(rts, mode, case):
    rt, td = rts[mode], rts[mode].tdtype
    R, C, ld = case.rows, case.C, case.ld
    d, ref, gates = T.ln_inputs(case, mode), T.ln_ref(case, mode), T.ln_gates(case, mode)
    off = 1 if case.mis else 0
    x, dy = _inp(d["x"], td, ld, off), _inp(d["dy"], td, ld)
    gamma, beta = _inp(d["gamma"], torch.float32), _inp(d["beta"], torch.float32)
    add = _inp(d["dx_add"], td, ld) if case.add else None
    y, dx = _out((R, ld), C, td), _out((R, ld), C, td)
    stats = Buf((R, 2), torch.float32)
    dgamma, dbeta = Buf((C,), torch.float32, d["dgamma0"]), Buf((C,), torch.float32, d["dbeta0"])
    ptr = {"x": x.ptr, "y": y.ptr, "dy": dy.ptr, "dx": dx.ptr, "gamma": gamma.ptr, "beta": beta.ptr, "dx_add": add.ptr if add else None}
    assert T.ln_forms(rt.lib, case, ptr) == (case.fwd, case.bwd)
    _call(rt, "jen1_ln_forward", x.ptr, gamma.ptr, beta.ptr, y.ptr, stats.ptr, R, C, ld, case.eps, rt.dt)
    assert _padding_kept(y, C) and stats.intact() and x.unchanged()
    stats.freeze()
    _call(rt, "jen1_ln_backward_add", dy.ptr, x.ptr, stats.ptr, gamma.ptr, None if case.dx_null else dx.ptr, add.ptr if add else None,
          dgamma.ptr, dbeta.ptr, R, C, ld, rt.dt)
    assert dgamma.intact() and dbeta.intact() and all(b.unchanged() for b in (x, dy, stats, gamma))
    assert dx.unchanged() if case.dx_null else _padding_kept(dx, C)
    got = {"y": y.t[:, :C].cpu(), "stats": stats.t.cpu(), "dx": dx.t[:, :C].cpu(), "dgamma": dgamma.t.cpu(), "dbeta": dbeta.t.cpu()}
    _report("ln", case.name, mode, T.compare(got, ref, gates), gates)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("case", T.LN2_CASES, ids=lambda c: c.name)
def test_dual_layer_norm(rts, mode, case):
    rt, td = rts[mode], rts[mode].tdtype
    R, C, ld = case.rows, case.C, case.ld
    d, ref, gates = T.ln_inputs(case, mode), T.ln_ref(case, mode), T.ln_gates(case, mode)
    x, dy1, dy2 = _inp(d["x"], td), _inp(d["dy"], td), _inp(d["dy2"], td)
    g1, b1, g2, b2 = (_inp(d[k], torch.float32) for k in ("gamma", "beta", "gamma2", "beta2"))
    add = _inp(d["dx_add"], td) if case.add else None
    y1, y2, dx, stats = Buf((R, ld), td), Buf((R, ld), td), Buf((R, ld), td), Buf((R, 2), torch.float32)
    acc = {k: Buf((C,), torch.float32, d[k + "0"]) for k in ("dgamma", "dbeta", "dgamma2", "dbeta2")}
    _call(rt, "jen1_ln2_forward", x.ptr, g1.ptr, b1.ptr, g2.ptr, b2.ptr, y1.ptr, y2.ptr, stats.ptr, R, C, ld, case.eps, rt.dt)
    _call(rt, "jen1_ln2_backward_add", dy1.ptr, dy2.ptr, x.ptr, stats.ptr, g1.ptr, g2.ptr, dx.ptr, add.ptr if add else None,
          acc["dgamma"].ptr, acc["dbeta"].ptr, acc["dgamma2"].ptr, acc["dbeta2"].ptr, R, C, ld, rt.dt)
    assert all(b.intact() for b in [y1, y2, dx, stats] + list(acc.values())) and all(b.unchanged() for b in (x, dy1, dy2, g1, g2))
    got = {"y": y1.t.cpu(), "y2": y2.t.cpu(), "stats": stats.t.cpu(), "dx": dx.t.cpu(), **{k: b.t.cpu() for k, b in acc.items()}}
    _report("ln2", case.name, mode, T.compare(got, ref, gates), gates)


# ---------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------
def _act(rt, mode, mode_id, n, off, form):
    from jen1_amd import lib as L
    td = rt.tdtype
    xh, dyh = T.act_inputs(n, mode)
    ref, gates = T.act_ref(mode_id, n, mode), T.act_gates(mode_id, mode)
    x, dy = Buf((n,), td, xh, off), Buf((n,), td, dyh, off)
    y, dx = Buf((n,), td, None, off), Buf((n,), td, None, off)
    assert T.FORM_NAMES[rt.lib.jen1_act_form(x.ptr, y.ptr, None, n)] == form
    assert T.FORM_NAMES[rt.lib.jen1_act_form(dy.ptr, x.ptr, dx.ptr, n)] == form
    _call(rt, "jen1_act_forward", x.ptr, y.ptr, n, mode_id, rt.dt)
    _call(rt, "jen1_act_backward", dy.ptr, x.ptr, dx.ptr, n, mode_id, rt.dt)
    assert y.intact() and dx.intact() and x.unchanged() and dy.unchanged()
    _report("act", f"{T.ACT_NAMES[mode_id]}.n{n}+{off}", mode, T.compare({"y": y.t.cpu(), "dx": dx.t.cpu()}, ref, gates), gates)


@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("mode_id", [0, 1, 2], ids=lambda m: T.ACT_NAMES[m])
@pytest.mark.parametrize("n,off,form", T.ACT_CASES, ids=lambda v: str(v))
def test_activation(rts, mode, mode_id, n, off, form):
    _act(rts[mode], mode, mode_id, n, off, form)


@pytest.mark.parametrize("mode", T.MODES)
def test_activation_vector_loop_wraps(rts, mode):
    """8 x (256 x 32 x 256 + 1) elements: the 8-wide kernels' grid-stride loop takes a second turn (SiLU: the loop is the same for
    every mode, and the float64 reference of 16.8 M elements is what the case costs)"""
    _act(rts[mode], mode, 1, T.ACT_WRAP_VECTOR, 0, "vector")


# ---------------------------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", T.MODES)
@pytest.mark.parametrize("case", T.SOFTMAX_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_softmax(rts, mode, case):
    rt, td = rts[mode], rts[mode].tdtype
    Z, Nq, Nk, ld_s, ld_p, causal = case
    rows = Z * Nq
    sh, dph = T.softmax_inputs(case, mode)
    ref, gates = T.softmax_ref(case, mode), T.softmax_gates(case, mode)
    s, dp = _inp(sh, torch.float32, ld_s), _inp(dph, torch.float32, ld_s)
    p, ds = Buf((rows, ld_p), td), Buf((rows, ld_p), td)
    p_in = _inp(ref["p_in"], td, ld_p, pad=0.0)
    _call(rt, "jen1_softmax_forward", s.ptr, p.ptr, rows, Nq, Nk, ld_s, ld_p, causal, rt.dt)
    _call(rt, "jen1_softmax_backward", p_in.ptr, dp.ptr, ds.ptr, rows, Nk, ld_s, ld_p, rt.dt)
    assert p.intact() and ds.intact() and all(b.unchanged() for b in (s, dp, p_in))
    zero = torch.zeros((rows, ld_p - Nk), dtype=td)
    assert _same_bits(p.t[:, Nk:].cpu(), zero) and _same_bits(ds.t[:, Nk:].cpu(), zero)          # padding columns: exactly 0
    got_p = p.t[:, :Nk].cpu()
    masked = ~T.softmax_keep(case)
    assert bool((got_p[masked] == 0).all()) and bool((ds.t[:, :Nk].cpu()[masked] == 0).all())      # masked keys: exactly 0
    _report("softmax", "-".join(str(v) for v in case), mode, T.compare({"p": got_p, "ds": ds.t[:, :Nk].cpu()}, ref, gates), gates)
