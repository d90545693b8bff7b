"""-m gpu: the two persistent launches (csrc/deep_kernel.hip, csrc/long_kernel.hip) phase by phase against float64.

A case is a program of one phase -- plus a plain 1x1 conv phase in front of every operand the case wants live -- recorded through
``OpBuilder.conv`` / ``OpBuilder.attention`` exactly as a ``Plan`` records it (so ``_conv_deep`` / ``_conv_long`` / ``_conv_tile``,
``_live_mask``, the statistics hand-off and ``_deep_nb_cap`` are under test too), on a ``KernelCtx``: no model, no ``Engine``, no weights.
Cases, references, wrong variants and the restated unit geometry live in tests/persistent_phases_common.py and are pinned on the CPU by
tests/test_persistent_phases_host.py.

Every run checks, in this order: the error word (a set word fails the test there, with the phase's label, and nothing more is
launched); the descriptor fields against the restated geometry (the case reached the form it states); that the rows around and between
the written ones still hold the sentinel they were poisoned with; that no 8-byte word the program had to write still is the sentinel;
the values against the float64 reference at the kernel tier's tolerance; and that a second poison + launch gives the same bits.
A failure message names the kind, the case, its form and the phase label.
"""
import ctypes as C

import pytest
import torch

import persistent_phases_common as P
from jen1_amd import lib as L
from persistent_phases_common import MODES, STAT_TOL, TOL

pytestmark = pytest.mark.gpu

PAD_ROWS = 2                    # canary rows in front of and behind every output
WORST = {}                      # (kind, mode) -> (worst observed error, case): printed by the last test of the file


@pytest.fixture(scope="module", params=MODES)
def ctx(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.engine import KernelCtx
    kc = KernelCtx(request.param, "cuda", target_wgs=256)
    # what the deep path reads from an Engine beside KernelCtx's fields (Engine.__init__'s defaults)
    kc.deep_nb_max, kc.deep_unit_target, kc.deep_reread_cap = P.DEEP_NB_MAX, P.DEEP_UNIT_TARGET, P.DEEP_REREAD_CAP
    return kc, request.param


def note(kind, mode, err, name):
    if err > WORST.get((kind, mode), (-1.0, ""))[0]:
        WORST[(kind, mode)] = (err, name)


# ---------------------------------------------------------------------------------------------- harness
def _builder(kc):
    from jen1_amd.engine import DeepProgram, LongProgram, OpBuilder

    class PhaseBuilder(OpBuilder):
        """an OpBuilder that records phases into ONE stand-alone program and runs it"""

        def open_deep(self):
            self.deep = self._prog = DeepProgram(self.eng)
            self._deep_on = True

        def open_long(self, B):
            self._lprog = LongProgram(self.eng, B)
            self._long_on = True

        def open_tile(self, lens):
            self.tile_lens = frozenset(lens)

        def _prog_open(self):
            if self._prog is None:
                self.deep = self._prog = DeepProgram(self.eng)

        def close(self):
            assert not self.tile_errors, self.tile_errors
            prog = self._lprog if self._lprog is not None else self._prog
            self._sync = torch.zeros((prog.sync_words(),), dtype=torch.int32, device=self.eng.device)
            prog.finalize(self._sync)
            prog.exclusive = False
            self.prog = prog
            return prog

        def launch(self, static):
            """poison, launch in the given scheduling form, synchronise; the error word is read straight after"""
            prog = self.prog
            prog.exclusive = bool(static)
            s = torch.cuda.current_stream(self.eng.device).cuda_stream
            try:
                prog.poison(s)
                prog.launch(s)
                torch.cuda.synchronize(self.eng.device)
            finally:
                prog.exclusive = False
            return prog.take_error()

        def release(self):
            """give the device's static schedule back: later tests build plans that claim it"""
            key = str(self.eng.device)
            ref = DeepProgram._static_owner.get(key)
            if ref is not None and ref() is self.prog.leader:
                del DeepProgram._static_owner[key]

    return PhaseBuilder(kc)


class Out:
    """an output [B][rows][C] inside a larger allocation: PAD_ROWS canary rows before and after.  The program poisons whole storages, so
    the canaries -- and the rows of the window the phase does not write -- must still be the all-ones sentinel after the run"""

    def __init__(self, kc, B, rows, Cc, gn=False, dtype=None):
        from jen1_amd.engine import Act
        self.big = torch.zeros((B * rows + 2 * PAD_ROWS, Cc), dtype=dtype or kc.tdtype, device="cuda")
        self.t = self.big[PAD_ROWS: PAD_ROWS + B * rows].view(B, rows, Cc)
        assert self.t.data_ptr() % 16 == 0
        self.act = Act(self.t, B, rows, Cc, Cc, torch.zeros(B * 64, device="cuda") if gn else None, None)

    def words(self, t=None):
        return (self.big if t is None else t).contiguous().view(torch.int64)

    def check(self, written, what):
        """written: bool [B][rows] -- the rows the phase writes.  Returns the window as float64 on the CPU"""
        w = self.words().cpu()
        assert bool((w[:PAD_ROWS] == -1).all()) and bool((w[-PAD_ROWS:] == -1).all()), f"{what}: a canary row was written"
        win = self.words(self.t).cpu().view(self.t.shape[0], self.t.shape[1], -1)
        assert bool((win[~written] == -1).all()), f"{what}: a row outside the phase's output window was written"
        assert not bool((win[written] == -1).any()), f"{what}: {int((win[written] == -1).sum())} words of the output are still the sentinel"
        return self.t.detach().cpu().double()


def no_sentinel(t, what):
    w = t.contiguous().view(torch.int64)
    assert not bool((w == -1).any()), f"{what}: {int((w == -1).sum())} words are still the sentinel"


def dev(t, kc=None):
    return None if t is None else (t.to(kc.tdtype) if kc is not None else t).cuda().contiguous()


def act_of(t, kc, gn=None):
    from jen1_amd.engine import Act
    B, Ln, Cc = t.shape
    return Act(dev(t, kc), B, Ln, Cc, Cc, gn if gn is not None else torch.zeros(B * 64, device="cuda"), None)


def pack_flat(W, kc):
    """[M][K] in K order (tap, channel, then the extra segments) -> the flat packed weight [K / 32][M / 16][64][8]"""
    from jen1_amd.packing import pack_gemm_weight
    return pack_gemm_weight(W[None].cuda(), kc.tdtype)[0].contiguous()


def descriptors(prog, size):
    """the first eight int32 of every linked descriptor: kind, n_units, rot, dep, dep_units, lds_bytes, dtype, ntrips"""
    img = prog.dev.cpu().numpy().tobytes()
    return [list((C.c_int32 * 8).from_buffer_copy(img[i * size: i * size + 32])) for i in range(len(prog))]


def front(ob, kc, t, k, gn=False):
    """the plain 1x1 conv phase that produces operand ``k`` (tests/persistent_phases_common.py: front_ref); returns its Out"""
    z = t["z." + k]
    o = Out(kc, z.shape[0], z.shape[1], t["wf." + k].shape[0], gn=gn)
    ob.conv(ob.ops, src0=act_of(z, kc), w=pack_flat(t["wf." + k], kc), bias=t["bf." + k].cuda(), out=o.act, flat_w=True, label="front." + k)
    return o


# ---------------------------------------------------------------------------------------------- conv phases of all three kinds
def record_conv(ob, kc, c, t, mode, kind):
    """record the case's phases; returns (Out of the phase under test, {operand: Out of its front phase}, the film_step scalar)"""
    fronts, acts = {}, {}
    want_stats = kind != "deep"
    for k in ("x0", "x1", "residual") + tuple(f"e{i}" for i in range(len(c["extras"]))):
        if k not in t or t[k] is None:
            continue
        if k in c["live"]:
            fronts[k] = front(ob, kc, t, k, gn=k in ("x0", "x1"))          # (a normalised source carries a statistics pointer)
            acts[k] = fronts[k].act
        else:
            gn = None
            if want_stats and c["groups"] and k in ("x0", "x1"):
                # totals [B][32][2] as a producer's epilogue leaves them before the launch
                gn = P.fine_group_sums(P.rounded(t[k], mode)).float().reshape(-1).cuda()
            acts[k] = act_of(t[k], kc, gn)
    out = Out(kc, c["B"], c["out_L"], c["out_C"], gn=c["stats"])
    cm = c["c0"] + c["c1"]
    kw, step = {}, None
    if c["groups"]:
        kw["gn"] = (c["groups"], cm, t["gamma"].cuda(), t["beta"].cuda(), c["eps"])
        if c["film"]:
            ob.film2 = t["film2"].cuda()
            film = (ob.film2, dev(t["film_row"]), P.FILM_OFF, cm)
            if c["film"] == "step":
                step = torch.tensor([P.FILM_STEPS[0]], dtype=torch.int32, device="cuda")
                film += (step,)
            kw["film"] = film
    ob.conv(ob.ops, src0=acts["x0"], src1=acts.get("x1"), src1_scale=c["src1_scale"], w=pack_flat(t["W"], kc),
            bias=t["bias"].cuda() if c["bias"] else None, edge_bias=dev(t.get("edge_bias")), out=out.act, taps=c["taps"], stride=c["stride"],
            pad_left=c["pad_left"], L_out=c["L_out"], ps_f=c["ps_f"], ps_off=c["ps_off"], L_y=c["L_y"], y_row0=c["y_row0"], pro=c["pro"],
            act=c["act"], residual=acts.get("residual"), out_C=c["out_C"], m_split=c["m_split"], k_split=c["k_split"], flat_w=True,
            extra_segs=[(acts[f"e{i}"], sh) for i, (_, sh) in enumerate(c["extras"])], label="case", **kw)
    return out, fronts, step


def run_conv_case(ctx, kind, name, static=False, also=()):
    """record, run, check.  also: further scheduling forms ("static" / "ticket" / "local") that must give the same bits"""
    kc, mode = ctx
    table = {"deep": P.DEEP_CONV_CASES, "long": P.LONG_CASES, "tile": P.TILE_CASES}[kind]
    c = table[name]
    t = P.conv_inputs(f"{kind}.{name}", c)
    what = f"{kind} case {name} [{c['form']}] {mode}"
    ob = _builder(kc)
    kc.deep_nb_max, kc.deep_unit_target = c["nb_max"], c["unit_target"]
    try:
        if kind == "deep":
            ob.open_deep()
        elif kind == "long":
            ob.open_long(c["B"])
        else:
            ob.open_tile({c["L_in"]} | {t["z." + k].shape[1] for k in c["live"]})
        out, fronts, step = record_conv(ob, kc, c, t, mode, kind)
        prog = ob.close()
    finally:
        kc.deep_nb_max, kc.deep_unit_target = P.DEEP_NB_MAX, P.DEEP_UNIT_TARGET
    try:
        err = ob.launch(static)
        assert err == 0, f"{what}: the error word is {err:#x} (1 + phase: {prog.labels[(err & 0xffff) - 1] if 0 < (err & 0xffff) <= len(prog) else '?'})"
        # the form
        if kind == "deep":
            g = P.deep_conv_geometry(c, mode, nwg=prog.nwg)
            d = descriptors(prog, L.load().jen1_deep_blob_bytes())[-1]
            assert (d[0], d[1], d[5], d[7]) == (0, g["n_units"], g["lds_bytes"], g["ntrips"]), f"{what}: descriptor {d} against the restated geometry {g}"
            if prog.nwg == P.NWG:
                for k, v in P.case_reach(c, mode).items():
                    assert g[k] == v, f"{what}: {k} = {g[k]}, the case states {v}"
        elif kind == "long":
            geo = prog.geometry(c["M"], c["L_out"])
            assert geo == P.long_geometry(c["M"], c["L_out"], prog.G), f"{what}: geometry {geo}"
        else:
            assert prog.kinds[-1] == "tile" and f"tb={P.tile_geometry(c, prog.nwg)['tb']} bm={P.tile_geometry(c)['bm']}" in prog.labels[-1], prog.labels[-1]
        # sentinels, canaries, values
        for k, fo in fronts.items():
            y = fo.check(torch.ones(fo.t.shape[:2], dtype=torch.bool), f"{what}: front phase of {k}")
            e = P.rel(y, P.front_ref(t, k, mode))
            note(kind + ".front", mode, e, name)
            assert e < TOL[mode], f"{what}: front phase of {k}: {e:.3e}"
        ref = P.conv_ref(c, t, mode, step=P.FILM_STEPS[0] if step is not None else None)
        written = ~torch.isnan(ref).all(-1)
        y = out.check(written, what)
        e = P.written_rel(y, ref)
        note(kind, mode, e, name)
        print(f"{what}: {e:.3e} (tol {TOL[mode]})")
        assert e < TOL[mode], f"{what}: {e:.3e} >= {TOL[mode]} ({prog.labels[-1]})"
        parts = {}
        if c["stats"]:
            if kind == "long":
                part, _, mb, _ = out.act.lp
                tb, n = prog.geometry(c["M"], c["L_out"])[2], c["out_C"] // 16
                got = P.long_part_sums(part.cpu(), mb, c["out_C"])
            else:
                part, _, n = out.act.part
                tb = P.tile_geometry(c, prog.nwg)["tb"]
                got = P.tile_part_sums(part.cpu())
            no_sentinel(part, f"{what}: partial sums")
            parts["out"] = part
            es = P.stat_rel(got, P.part_stats_ref(c, t, mode, tb, n, step=P.FILM_STEPS[0] if step is not None else None))
            note(kind + ".stats", mode, es, name)
            print(f"{what}: partial sums {es:.3e} (tol {STAT_TOL[mode]})")
            assert es < STAT_TOL[mode], f"{what}: partial sums {es:.3e} >= {STAT_TOL[mode]}"
        for k, fo in fronts.items():
            p = fo.act.lp[0] if fo.act.lp is not None else (fo.act.part[0] if fo.act.part is not None else None)
            if p is not None:
                no_sentinel(p, f"{what}: partial sums of the front phase of {k}")
                parts[k] = p
        # replay, and the other scheduling forms: the same bits
        snap = lambda: [o.big.clone() for o in [out] + list(fronts.values())] + [p.clone() for p in parts.values()]
        first = snap()
        for form in ("same",) + tuple(also):
            if form == "local":
                prog.local = True
            try:
                err = ob.launch({"same": static, "static": True, "ticket": False, "local": True}[form])
            finally:
                if form == "local":
                    prog.local = False
            assert err == 0, f"{what}: {form} form: the error word is {err:#x}"
            again = snap()
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, again)), \
                f"{what}: a second run ({form} form) changed bits"
        if step is not None:
            # the device scalar changes between two runs of the same program
            step.fill_(P.FILM_STEPS[1])
            assert ob.launch(static) == 0
            e = P.written_rel(out.check(written, what), P.conv_ref(c, t, mode, step=P.FILM_STEPS[1]))
            assert e < TOL[mode], f"{what}: after film_step changed on the device: {e:.3e}"
    finally:
        ob.release()


@pytest.mark.parametrize("name", list(P.DEEP_CONV_CASES))
def test_deep_conv_phase(ctx, name):
    """JEN1_DEEP_GEMM units, by ticket; one case also on the static map, bit for bit"""
    run_conv_case(ctx, "deep", name, also=("static",) if name == "gn_8groups" else ())


@pytest.mark.parametrize("name", list(P.LONG_CASES))
def test_long_phase(ctx, name):
    """jen1_long_phase_conv units on the static map; one case also by ticket, bit for bit"""
    run_conv_case(ctx, "long", name, static=True, also=("ticket",) if name == "full_tiles" else ())


@pytest.mark.parametrize("name", list(P.TILE_CASES))
def test_tile_phase(ctx, name):
    """JEN1_DEEP_TILE units through OpBuilder._conv_tile"""
    run_conv_case(ctx, "tile", name)


# ---------------------------------------------------------------------------------------------- attention phases
@pytest.mark.parametrize("name", list(P.ATTN_CASES))
def test_deep_attention_phase(ctx, name):
    kc, mode = ctx
    c = P.ATTN_CASES[name]
    t = P.attn_inputs(f"attn.{name}", c)
    H, d, Nq, Nk, Cc, B = c["H"], c["d"], c["Nq"], c["Nk"], c["Cc"], c["B"]
    mid = H * d
    what = f"attention case {name} {mode}"
    ob = _builder(kc)
    ob.open_deep()
    out = Out(kc, B, Nq, mid)
    u, b = t["u"].cuda(), t["b"].cuda()
    step, qkv = None, None
    if c["kind"] == "self":
        qkv = Out(kc, B, Nq, t["ld"])
        ob.conv(ob.ops, src0=act_of(t["z"], kc), w=pack_flat(t["wf"], kc), bias=t["bf"].cuda(), out=qkv.act, flat_w=True, label="projection")
        ob.attention(ob.ops, q=qkv.act, q_off=Cc, kv_t=qkv.t, ldkv=t["ld"], k_off=Cc + mid, v_off=Cc + 2 * mid, out=out.act, H=H, d=d, Nk=Nk,
                     causal=c["causal"], fin=(None, u, b, Cc, 1e-5, 1, 1))
    else:
        kw = {}
        if c["kind"] != "cross":
            kw = dict(kv_extra=dev(t["kv_extra"], kc), extra_row=dev(t["extra_row"]), ld_extra=t["ld_extra"], kx_off=t["kx_off"], vx_off=t["vx_off"])
            if c["kind"] == "cross_step":
                step = torch.tensor([P.ATTN_STEPS[0]], dtype=torch.int32, device="cuda")
                kw["extra_step"] = step
        ob.attention(ob.ops, q=act_of(t["q"], kc), q_off=Cc, kv_t=dev(t["kv"], kc), ldkv=2 * mid, k_off=0, v_off=mid, out=out.act, H=H, d=d, Nk=Nk,
                     causal=c["causal"], kv_row=dev(t["kv_row"]), fin=(None, u, b, Cc, 1e-5, 1, 0), **kw)
    prog = ob.close()
    try:
        err = ob.launch(False)
        assert err == 0, f"{what}: the error word is {err:#x} ({prog.labels[err - 1] if 0 < err <= len(prog) else '?'})"
        g = P.attn_geometry(d, Nq, Nk, mode, self_attn=c["kind"] == "self", finish_kv=c["kind"] == "self")
        dsc = descriptors(prog, L.load().jen1_deep_blob_bytes())[-1]
        assert (dsc[0], dsc[1], dsc[5]) == (1, B * H * g["nqc"], g["lds_bytes"]), f"{what}: descriptor {dsc} against the restated geometry {g}"
        rows = torch.ones(B, Nq, dtype=torch.bool)
        if qkv is not None:
            e = P.rel(qkv.check(rows, what + ": projection"), P.attn_qkv(c, t, mode))
            assert e < TOL[mode], f"{what}: projection {e:.3e}"
        y = out.check(rows, what)
        e = P.rel(y, P.attn_ref(c, t, mode, step=P.ATTN_STEPS[0] if step is not None else None))
        note("attn", mode, e, name)
        print(f"{what}: {e:.3e} (tol {TOL[mode]})")
        assert e < TOL[mode], f"{what}: {e:.3e} >= {TOL[mode]} ({prog.labels[-1]}, vsep={g['vsep']})"
        first = [out.big.clone()] + ([qkv.big.clone()] if qkv is not None else [])
        assert ob.launch(False) == 0
        again = [out.big] + ([qkv.big] if qkv is not None else [])
        assert all(torch.equal(a.view(torch.uint8), b2.view(torch.uint8)) for a, b2 in zip(first, again)), f"{what}: a second run changed bits"
        if step is not None:
            step.fill_(P.ATTN_STEPS[1])
            assert ob.launch(False) == 0
            e = P.rel(out.check(rows, what), P.attn_ref(c, t, mode, step=P.ATTN_STEPS[1]))
            assert e < TOL[mode], f"{what}: after extra_step changed on the device: {e:.3e}"
    finally:
        ob.release()


# ---------------------------------------------------------------------------------------------- stats phase
@pytest.mark.parametrize("name", list(P.STATS_CASES))
def test_deep_stats_phase(ctx, name):
    """JEN1_DEEP_STATS on a tensor the phase in front produced"""
    kc, mode = ctx
    c = P.STATS_CASES[name]
    t = P.stats_inputs(f"stats.{name}", c)
    what = f"stats case {name} {mode}"
    ob = _builder(kc)
    ob.open_deep()
    x = Out(kc, c["B"], c["L"], c["ld"])
    ob.conv(ob.ops, src0=act_of(t["z"], kc), w=pack_flat(t["wf"], kc), bias=t["bf"].cuda(), out=x.act, flat_w=True, label="front")
    # (the totals are not a tensor of the protocol: they are written once, plainly; NaN canaries around and under them)
    big = torch.full((c["B"] * 64 + 2 * 64,), float("nan"), device="cuda")
    stats = big[64: 64 + c["B"] * 64]
    ob._prog.add_stats(x.act, stats, f"stats B={c['B']} L={c['L']} ld={c['ld']}")
    prog = ob.close()
    try:
        err = ob.launch(False)
        assert err == 0, f"{what}: the error word is {err:#x}"
        dsc = descriptors(prog, L.load().jen1_deep_blob_bytes())[-1]
        assert (dsc[0], dsc[1]) == (2, c["B"])
        x.check(torch.ones(c["B"], c["L"], dtype=torch.bool), what + ": front")
        assert bool(torch.isnan(big[:64]).all()) and bool(torch.isnan(big[-64:]).all()), f"{what}: a canary was written"
        got = stats.cpu().double().reshape(c["B"], 32, 2)
        assert bool(torch.isfinite(got).all()), f"{what}: totals left unwritten"
        e = P.stat_rel(got, P.stats_ref(c, t, mode))
        note("stats", mode, e, name)
        print(f"{what}: {e:.3e} (tol {STAT_TOL[mode]})")
        assert e < STAT_TOL[mode], f"{what}: {e:.3e} >= {STAT_TOL[mode]}"
        first = big.clone()
        big.fill_(float("nan"))
        assert ob.launch(False) == 0
        assert torch.equal(first.view(torch.int32), big.view(torch.int32)), f"{what}: a second run changed bits"
    finally:
        ob.release()


# ---------------------------------------------------------------------------------------------- the `local` form, and the summary
def test_long_phase_local_form(ctx):
    """one B = 8 case in the XCD-local form of jen1_long_run: the same bits as the static form"""
    run_conv_case(ctx, "long", "ragged_tile", static=True, also=("local",))


def test_zz_worst_errors(ctx):
    """prints the worst error per kind for this mode next to its tolerance (pytest -s); asserts nothing new"""
    _, mode = ctx
    for (kind, m), (e, name) in sorted(WORST.items()):
        if m == mode:
            tol = STAT_TOL[m] if kind.endswith("stats") else TOL[m]
            print(f"worst {kind} [{m}]: {e:.3e} in {name} (tol {tol})")
            assert e < tol
