"""-m gpu: the one-launch conv GEMM ``jen1_conv_gemm`` form by form against float64, on its three kernel families (csrc/conv_gemm.hip
LDS-staged, csrc/stream_gemm.hip register-direct, csrc/tile_gemm.hip lean tiles) and every tile configuration of each.

A case is ONE ``OpBuilder.conv`` call on a ``KernelCtx`` (no model, no ``Engine``, no weights) with the tile configuration -- and where
the case says so the tile geometry, the LDS stage and the K split -- forced through ``force``.  Cases, inputs, references and wrong
variants live in tests/conv_gemm_common.py and are pinned on the CPU by tests/test_conv_gemm_refs_host.py.

Every run checks: the values against the float64 reference at the kernel tier's tolerance; every requested statistic against float64
sums of the REFERENCE output; that the sentinel y was filled with is bit-identical afterwards in the rows outside the output window, in
the padding columns [out_C, ld_y) and in one more batch element's worth of rows allocated behind y (likewise zeros behind the statistics);
split-K counters back at zero and a second run of the same prepared launch; the FiLM scalar changed on the device between two runs.  A
combination the entry point refuses is asserted as refused: a non-zero return, the text of ``jen1_last_error``, y untouched.
"""
import ctypes as C

import pytest
import torch

import conv_gemm_common as G
from conv_gemm_common import MODES, STAT_TOL, TOL
from helpers import record_parity
from jen1_amd import lib as L

pytestmark = pytest.mark.gpu

WORST = {}                      # (family[.stats], mode) -> (worst observed error, case): recorded by the last test of the file


@pytest.fixture(scope="module", params=MODES)
def ctx(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.engine import KernelCtx
    return KernelCtx(request.param, "cuda", target_wgs=256), request.param


def note(kind, mode, err, name):
    if err > WORST.get((kind, mode), (-1.0, ""))[0]:
        WORST[(kind, mode)] = (err, name)


def dev(t, kc=None):
    return None if t is None else (t.to(kc.tdtype) if kc is not None else t).cuda().contiguous()


def src_of(t, kc, C_real=None, gn=None, rs=None):
    from jen1_amd.engine import Act
    B, Ln, ld = t.shape
    flat = lambda s: None if s is None else s.reshape(-1).cuda().contiguous()
    return Act(dev(t, kc), B, Ln, C_real or ld, ld, flat(gn), flat(rs))


def pack_flat(W, kc):
    """[M][K] in K order (tap, channel, then the extra segments) -> the flat packed weight [K / 32][M / 16][64][8]"""
    from jen1_amd.packing import pack_gemm_weight
    return pack_gemm_weight(W[None].cuda(), kc.tdtype)[0].contiguous()


class Out:
    """y [B][out_L][ld_y] in front of one more batch element's worth of rows, all pre-filled with a finite sentinel; the statistics
    outputs likewise in front of one more element's, pre-filled with zeros"""

    def __init__(self, kc, c):
        from jen1_amd.engine import Act
        B, rows, ld = c["B"], c["out_L"], c["ld_y"]
        self.c = c
        self.big = torch.empty(((B + 1) * rows, ld), dtype=torch.float32 if c["y_f32"] else kc.tdtype, device="cuda")
        self.gn = torch.empty((B + 1) * 64, device="cuda")
        self.rs = torch.empty((B + 1) * rows * 2, device="cuda")
        self.reset()
        self.act = Act(self.big[: B * rows].view(B, rows, ld), B, rows, c["out_C"], ld, self.gn[: B * 64] if c["gn_out"] else None,
                       self.rs[: B * rows * 2] if c["rs_out"] else None)

    def reset(self):
        self.big.fill_(G.SENTINEL)
        self.gn.zero_()
        self.rs.zero_()

    def untouched(self, what):
        assert bool((self.big == G.SENTINEL).all()) and not bool(self.gn.any()) and not bool(self.rs.any()), f"{what}: a refused launch wrote"

    def check(self, written, what):
        """written: bool [B][out_L], the rows the launch writes.  Returns (y [B][out_L][out_C], out_gn_stats [B][32][2], out_rowstats
        [B][out_L][2]) as float64 on the CPU"""
        c = self.c
        B, rows, oc = c["B"], c["out_L"], c["out_C"]
        y = self.big.cpu().double()
        win = y[: B * rows].view(B, rows, -1)
        assert bool((y[B * rows:] == G.SENTINEL).all()), f"{what}: the memory behind the last batch element was written"
        assert bool((win[~written] == G.SENTINEL).all()), f"{what}: a row outside the output window was written"
        assert bool((win[written][:, oc:] == G.SENTINEL).all()), f"{what}: the padding columns [out_C, ld_y) were written"
        assert bool(torch.isfinite(win[written][:, :oc]).all()), f"{what}: non-finite output"
        gn, rs = self.gn.cpu().double(), self.rs.cpu().double()
        assert not bool(gn[B * 64:].any()) and not bool(rs[B * rows * 2:].any()), f"{what}: the memory behind the statistics was written"
        assert c["gn_out"] or not bool(gn.any()), f"{what}: out_gn_stats written though not requested"
        assert c["rs_out"] or not bool(rs.any()), f"{what}: out_rowstats written though not requested"
        return win[..., :oc], gn[: B * 64].view(B, 32, 2), rs[: B * rows * 2].view(B, rows, 2)


def record(kc, c, t, mode, out, name):
    """one OpBuilder with the case's launch prepared; returns (builder, the film_step scalar or None)"""
    from jen1_amd.engine import Act, OpBuilder
    st = G.producer_stats(c, t, mode)
    cm = c["c0"] + c["c1"]
    x0 = src_of(t["x0"], kc, C_real=c["creal"] or c["ln_C"] or None, gn=st.get("gn0"), rs=st.get("rs0"))
    x1 = src_of(t["x1"], kc, gn=st.get("gn1")) if c["c1"] else None
    kw, step = {}, None
    if c["groups"]:
        kw["gn"] = (c["groups"], c["creal"] or cm, t["gamma"].cuda(), t["beta"].cuda(), c["eps"])
        if c["film"]:
            film = (t["film"].cuda(), dev(t["film_row"]), G.FILM_OFF, cm)
            if c["film"] == "step":
                step = torch.tensor([G.FILM_STEPS[0]], dtype=torch.int32, device="cuda")
                film += (step,)
            kw["film"] = film
    if c["ln"]:
        kw["ln"] = (c["ln_C"], dev(t.get("ln_gamma")), dev(t.get("ln_beta")))
    if c["residual"]:
        # the residual's pitch differs from y's where the case says so; what lies between its rows is loud
        B, rows, ld = c["B"], c["out_L"], c["ld_y"] + c["res_pad"]
        res = torch.full((B, rows, ld), 100.0)
        res[..., : c["out_C"]] = t["residual"]
        kw["residual"] = Act(dev(res, kc), B, rows, c["out_C"], ld)
    if c["row_scale"]:
        kw["row_scale"] = t["row_scale"].reshape(-1).cuda().contiguous()
    ob = OpBuilder(kc)
    r = ob.conv(ob.ops, src0=x0, src1=x1, src1_scale=c["src1_scale"], w=pack_flat(t["W"], kc), bias=t["bias"].cuda() if c["bias"] else None,
                out=out.act, taps=c["taps"], stride=c["stride"], pad_left=c["pad_left"], L_out=c["L_out"], ps_f=c["ps_f"], ps_off=c["ps_off"],
                L_y=c["L_y"], y_row0=c["y_row0"], pro=c["pro"], act=c["act"], y_f32=c["y_f32"], out_C=c["out_C"], flat_w=True,
                extra_segs=[(src_of(t[f"e{i}"], kc), sh) for i, (_, sh) in enumerate(c["extras"])], force=G.force_of(c), label=name, **kw)
    assert r is out.act, f"{name}: OpBuilder.conv declined the launch"
    ob.finalize_workspace()
    a = ob._keep[-1][0]
    got = (a.cfg, a.tb, a.nb, a.splitk, a.direct)
    want = (c["cfg"], c["tb_eff"], c["nb_eff"], c["splitk"], int(c["direct"]))
    assert got == want, f"{name}: the launch runs (cfg, tb, nb, splitk, direct) = {got}, the case states {want}"
    if c["family"] == "lds" and c["kc_stage"]:
        assert a.kc_stage == c["kc_stage"]
    return ob, step, a


def compare(c, t, mode, out, name, step, what):
    ref = G.ref(c, t, mode, step=step)
    written = ~torch.isnan(ref).all(-1)
    y, gn, rs = out.check(written, what)
    e = G.written_rel(y, ref)
    errs = {"err": e}
    note(c["family"], mode, e, name)
    print(f"{what}: {e:.3e} (tol {TOL[mode]})")
    assert e < TOL[mode], f"{what}: {e:.3e} >= {TOL[mode]}"
    want_gn, want_rs = G.out_stats(c, ref)
    for key, on, got, want in (("gn", c["gn_out"], gn, want_gn), ("rs", c["rs_out"], rs, want_rs)):
        if on:
            es = G.stat_rel(got, want)
            errs[key] = es
            note(c["family"] + ".stats", mode, es, name)
            print(f"{what}: {key} statistics {es:.3e} (tol {STAT_TOL[mode]})")
            assert es < STAT_TOL[mode], f"{what}: {key} statistics {es:.3e} >= {STAT_TOL[mode]}"
    return errs


@pytest.mark.parametrize("name", list(G.CASES))
def test_conv_gemm_form(ctx, name):
    kc, mode = ctx
    c = G.CASES[name]
    t = G.inputs(name, c)
    what = f"{name} {mode}"
    out = Out(kc, c)
    ob, step, a = record(kc, c, t, mode, out, name)
    s = torch.cuda.current_stream().cuda_stream
    if c["reject"]:
        rc = kc.lib.jen1_conv_gemm(C.byref(a), s)
        msg = kc.lib.jen1_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and c["reject"] in msg, f"{what}: expected a refusal naming '{c['reject']}', got rc = {rc}, '{msg}'"
        with pytest.raises(L.Jen1HipError, match=c["reject"]):
            ob.run()
        torch.cuda.synchronize()
        out.untouched(what)
        return
    ob.run()
    torch.cuda.synchronize()
    errs = compare(c, t, mode, out, name, G.FILM_STEPS[0] if step is not None else None, what)
    record_parity("conv_gemm_forms", name, mode, **errs)
    if c["splitk"] > 1:
        assert int(ob.counters.abs().sum().item()) == 0, f"{what}: split-K counters must be left at zero"
        out.reset()
        ob.run()
        torch.cuda.synchronize()
        compare(c, t, mode, out, name, None, what + ", second run of the prepared launch")
        assert int(ob.counters.abs().sum().item()) == 0, f"{what}: split-K counters must be left at zero (second run)"
    if step is not None:
        # the device scalar changes between two runs of the same prepared launch
        step.fill_(G.FILM_STEPS[1])
        out.reset()
        ob.run()
        torch.cuda.synchronize()
        compare(c, t, mode, out, name, G.FILM_STEPS[1], what + ", after film_step changed on the device")


def test_zz_worst_errors(ctx):
    """records the worst error per family for this mode next to its tolerance (helpers.record_parity's log; pytest -s prints); asserts nothing new"""
    _, mode = ctx
    for (kind, m), (e, name) in sorted(WORST.items()):
        if m == mode:
            tol = STAT_TOL[m] if kind.endswith("stats") else TOL[m]
            print(f"worst {kind} [{m}]: {e:.3e} in {name} (tol {tol})")
            record_parity("conv_gemm_forms.worst", f"{kind}: {name}", m, err=e, tol=tol)
