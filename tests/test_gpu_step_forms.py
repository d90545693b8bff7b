"""-m gpu: the sampler step kernels of csrc/elementwise.hip (cfg_step_kernel, cfg_step_vec_body and the tail launches around it), form by
form through the nine C entry points, against the float64 model of tests/step_forms_common.py.

Every output lies inside a larger allocation with guard elements either side, pre-filled with NaN where the call writes and with a
recognisable pattern where it must not (the context columns [C, ld_rows) of the packed rows, the columns of ``parts`` at and beyond C);
afterwards what is written must be finite and inside the model's elementwise bound, and everything else bit-equal to what it held.  The
padding columns [C, ld) of the network output hold 3e4.  Coefficients, noise and the blend's levels are tables of 5 rows behind a step
counter that points at row 1; every row that must not be read is NaN.  In bf16 mode the network output is rounded to bf16 first and both
sides read those values, so a gate covers the kernel's arithmetic and the rounding of the packed rows only.

Where include/jen1_hip.h promises bits -- the blend and the kind-4 row "every product and sum rounded to float32 by itself", ``parts`` "in
the layout and summation order of jen1_pack_input_parts" -- the comparison is bit for bit: with the float32 restatement of
step_forms_common (where no reduction and no division is involved), between the forms, and with jen1_pack_input_parts itself.
jen1_pack_input_parts and jen1_gn_stats_from_parts take a row length that is a multiple of 32 only, which most ld_rows of the case table
are not: they are given the smallest such length >= C, and channel c of either ``parts`` is compared with channel c of the other.
"""
import ctypes

import numpy as np
import pytest
import torch

import step_forms_common as S
from helpers import record_parity

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16"]
GUARD = 64                      # elements either side of a buffer (64 bytes at least: 16-byte alignment survives for every dtype)
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import lib as L
    return L, L.load()


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _pattern(shape, dtype):
    """recognisable values that bf16 holds exactly, no two neighbours alike"""
    n = int(np.prod(shape))
    return (((torch.arange(n, device="cuda") % 251) - 80).float() * 0.25).to(dtype).view(*shape)


class Guarded:
    """a buffer of ``shape`` inside a larger allocation.  fill None: NaN (a buffer that is written); a number or a tensor: those values"""

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        self.gv = -7.25 if dtype.is_floating_point else (0xA5 if dtype == torch.uint8 else -7)
        self.whole = torch.full((n + 2 * GUARD,), self.gv, dtype=dtype, device="cuda")
        self.t = self.whole[GUARD:GUARD + n].view(*shape)
        if fill is None:
            self.t.fill_(NAN)
        elif isinstance(fill, (int, float)):
            self.t.fill_(fill)
        else:
            self.t.copy_(fill)

    def intact(self):
        g = torch.cat([self.whole[:GUARD], self.whole[-GUARD:]])
        return _same_bits(g, torch.full_like(g, self.gv))

    def ptr(self):
        return self.t.data_ptr()


class Run:
    """the buffers of one case and the call.  ``rows``: the (kind, variant) of the table rows from S_ROW on (default: the case's own row);
    ``fill``: an entry of S.TAIL_FILLS for the tail forms; ``sync``: pass the tail's sync word"""

    def __init__(self, hip, mode, c, rows=None, inplace=False, fill=None, sync=True):
        self.L, self.lib = hip
        self.c, self.mode, self.inplace = c, mode, inplace
        self.bf16 = mode == "bf16"
        self.tdt = torch.bfloat16 if self.bf16 else torch.float32
        self.dt = self.L.BF16 if self.bf16 else self.L.F32
        B, C, T, ld, ld_rows, nrep = self.dims = S.shape_fields(c.shape)
        self.vec = S.is_vector(c.shape, 2 if self.bf16 else 4)
        self.ms = c.entry.endswith("_ms")
        self.rows_spec = rows or [(c.row or "k1", 0)]
        self.d = d = S.case_inputs(c, bf16=self.bf16)
        self.noises = [S.case_inputs(c, bf16=self.bf16, variant=v)["noise"] if v else d["noise"] for _, v in self.rows_spec]
        self.net = _dev(d["net"], self.tdt)
        assert _same_bits(self.net.float().cpu(), torch.from_numpy(d["net"]))                 # both sides read the same values
        self.x = Guarded((B, C, T), torch.float32, _dev(d["x"]))
        self.x_out = self.x if inplace else Guarded((B, C, T), torch.float32)
        self.eps_out = Guarded((B, C, T), torch.float32) if c.outs else None
        self.x0_out = Guarded((B, C, T), torch.float32) if c.outs else None
        coef = torch.full((S.N_TABLE, 8), NAN)
        kb = torch.full((S.N_TABLE, 2), NAN)
        noise = torch.full((S.N_TABLE, B, C, T), NAN)
        for j, (name, v) in enumerate(self.rows_spec):
            coef[S.S_ROW + j] = torch.from_numpy(S.coef_row(name, v))
            kb[S.S_ROW + j] = torch.tensor([float(p) for p in S.blend_level(v)])
            if not (self.vec and float(coef[S.S_ROW + j, 4]) == 0.0):                         # the vector form reads no noise at sigma == 0
                noise[S.S_ROW + j] = torch.from_numpy(self.noises[j])
        self.coef, self.kb = coef.cuda(), kb.cuda()
        self.noise = None if (self.ms or c.row == "k3" or c.entry == "cfg_combine") else noise.cuda()
        self.step = Guarded((1,), torch.int32, S.S_ROW)
        self.ticket = Guarded((1,), torch.int32, 0)
        self.hist = None
        if self.ms:                                            # only a kind-4 row with b1 != 0 reads the history
            self.hist = Guarded((B, C, T), torch.float32, _dev(d["hist"]) if self.rows_spec[0][0] == "k4" else None)
        self.blend = None
        if c.blend:
            self.known, self.eps_k, self.keep = _dev(d["known"]), _dev(d["eps_k"]), _dev(d["keep"])
            self.blend = self.L.BlendArgs(self.known.data_ptr(), self.eps_k.data_ptr(), self.keep.data_ptr(), self.kb.data_ptr())
        self.rows = self.parts = None
        if c.entry in S.PACKING:
            nb = (T + S.TB - 1) // S.TB
            self.rows = Guarded((nrep * B, T, ld_rows), self.tdt, _pattern((nrep * B, T, ld_rows), self.tdt))
            self.rows.t[:, :, :C] = NAN
            self.parts = Guarded((B, nb, ld_rows, 2), torch.float32, _pattern((B, nb, ld_rows, 2), torch.float32))
            self.parts.t[:, :, :C, :] = NAN
            self.rows_before, self.parts_before = self.rows.t.clone(), self.parts.t.clone()
        self.tail = c.entry.startswith("step_tail")
        if self.tail:
            sizes, zbytes = fill or S.TAIL_FILLS[0]
            self.sent = [Guarded((n,), torch.uint8, 0x5A) for n in sizes]
            self.zero = Guarded((zbytes,), torch.uint8, 0x5A)
            self.table = torch.tensor([[g.ptr(), n] for g, n in zip(self.sent, sizes)], dtype=torch.int64, device="cuda")
            self.sync = Guarded((1,), torch.int32, 12345) if sync else None
        self.guarded = [g for g in (self.x, self.x_out, self.eps_out, self.x0_out, self.step, self.ticket, self.hist, self.rows, self.parts)
                        if g is not None]
        if self.tail:
            self.guarded += self.sent + [self.zero] + ([self.sync] if self.sync else [])

    def model_args(self, j=0, x=None, hist=None):
        name, v = self.rows_spec[j]
        d = dict(self.d, noise=self.noises[j])
        return S.model_args(self.c._replace(row=name if self.c.row else None), d, variant=v, bf16=self.bf16, x=x, hist=hist)

    def launch(self, x=None, hist=None, C_arg=None):
        """-> the entry point's return code, after the stream has drained.  x / hist / C_arg: other pointers or another channel count than
        the case's (the refusals)"""
        c, lib = self.c, self.lib
        B, C, T, ld, ld_rows, nrep = self.dims
        C = C if C_arg is None else C_arg
        stream = torch.cuda.current_stream().cuda_stream
        p = lambda g: None if g is None else g.ptr()
        net, xp = self.net.data_ptr(), (self.x.ptr() if x is None else x)
        hp = p(self.hist) if hist is None else hist
        noise = None if self.noise is None else self.noise.data_ptr()
        coef, step = self.coef.data_ptr(), self.step.ptr()
        if c.entry == "cfg_ddim_step" and not c.indexed:       # one row, handed over directly
            coef += 4 * 8 * S.S_ROW
            noise = None if noise is None else noise + 4 * B * C * T * S.S_ROW
            step = None
        cfg = (nrep, S.SCALE, c.scale_cfg, c.phi, S.OBJ_ID[c.objective or "noise"], c.clip, self.dt)
        bl = None if self.blend is None else ctypes.byref(self.blend)
        pack = (step, self.ticket.ptr(), p(self.rows), p(self.parts), ld_rows, B, C, T, ld) + cfg
        fill = (self.table.data_ptr(), self.table.shape[0], p(self.sync), self.zero.ptr(), self.zero.t.numel()) if self.tail else ()
        if c.entry == "cfg_combine":
            rc = lib.jen1_cfg_combine(net, self.x_out.ptr(), B, C, T, ld, S.SCALE, c.scale_cfg, c.phi, self.dt, stream)
        elif c.entry == "cfg_ddim_step":
            rc = lib.jen1_cfg_ddim_step(net, xp, noise, coef, self.x_out.ptr(), p(self.eps_out), p(self.x0_out), step, B, C, T, ld, *cfg, stream)
        elif c.entry == "cfg_ddim_step_adv":
            rc = lib.jen1_cfg_ddim_step_adv(net, xp, noise, coef, self.x_out.ptr(), p(self.eps_out), p(self.x0_out), step, self.ticket.ptr(),
                                            B, C, T, ld, *cfg, stream)
        elif c.entry == "cfg_ddim_step_pack":
            rc = lib.jen1_cfg_ddim_step_pack(net, xp, noise, coef, self.x_out.ptr(), *pack, stream)
        elif c.entry == "cfg_ddim_step_pack_blend":
            rc = lib.jen1_cfg_ddim_step_pack_blend(net, xp, noise, coef, self.x_out.ptr(), *pack, bl, stream)
        elif c.entry == "cfg_ddim_step_pack_ms":
            rc = lib.jen1_cfg_ddim_step_pack_ms(net, xp, hp, coef, self.x_out.ptr(), *pack, bl, stream)
        elif c.entry == "step_tail":
            rc = lib.jen1_step_tail(net, xp, noise, coef, self.x_out.ptr(), *pack, *fill, stream)
        elif c.entry == "step_tail_blend":
            rc = lib.jen1_step_tail_blend(net, xp, noise, coef, self.x_out.ptr(), *pack, *fill, bl, stream)
        elif c.entry == "step_tail_ms":
            rc = lib.jen1_step_tail_ms(net, xp, hp, coef, self.x_out.ptr(), *pack, *fill, bl, stream)
        else:
            raise KeyError(c.entry)
        torch.cuda.synchronize()
        return rc

    def run(self):
        rc = self.launch()
        self.L.check(rc, self.c.entry)
        return self

    def snapshot(self):
        return [g.whole.clone() for g in self.guarded]

    def unchanged(self, snap):
        return all(_same_bits(g.whole, s) for g, s in zip(self.guarded, snap))


def _within(got, val, err, what):
    """got (a tensor) is finite and inside val +- err elementwise -> the worst error / bound"""
    g = got.detach().float().cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all(), f"{what}: not finite"
    diff = np.abs(g - val)
    err = np.broadcast_to(err, diff.shape)
    bad = diff > err
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside the bound, worst error / bound {float((diff[bad] / np.maximum(err[bad], 1e-300)).max()):.3g}"
    return float((diff[err > 0] / err[err > 0]).max()) if (err > 0).any() else 0.0


def _check(r, m, advanced=1):
    """one finished launch of Run r against the float64 model m: every output, the survivors, the guards, the counter -> {output: ratio}"""
    c = r.c
    B, C, T, ld, ld_rows, nrep = r.dims
    cid = S.case_id(c) + "." + r.mode
    out = {}
    out["x_out"] = _within(r.x_out.t, m.val["o" if c.entry == "cfg_combine" else "x_next"], m.err["o" if c.entry == "cfg_combine" else "x_next"],
                           cid + " x_out")
    if c.outs:
        out["eps_out"] = _within(r.eps_out.t, m.val["eps"], m.err["eps"], cid + " eps_out")
        out["x0_out"] = _within(r.x0_out.t, m.val["x0"], m.err["x0"], cid + " x0_out")
    if r.ms:
        out["hist"] = _within(r.hist.t, m.val["hist"], m.err["hist"], cid + " hist")
    if r.rows is not None:
        rows, parts = r.rows.t, r.parts.t
        out["rows"] = _within(rows[:, :, :C], m.val["rows"], m.err["rows"], cid + " rows")
        want = r.x_out.t.transpose(1, 2).to(r.tdt)
        for rep in range(nrep):                                # every replica IS x_out in the compute type
            assert _same_bits(rows[rep * B:(rep + 1) * B, :, :C], want), f"{cid}: rows of replica {rep} are not x_out"
        assert _same_bits(rows[:, :, C:], r.rows_before[:, :, C:]), f"{cid}: the context columns behind the latents changed"
        out["parts"] = _within(parts[:, :, :C, :], m.val["parts"], m.err["parts"], cid + " parts")
        assert _same_bits(parts[:, :, C:, :], r.parts_before[:, :, C:, :]), f"{cid}: parts columns at and beyond C changed"
    if not r.inplace:
        assert _same_bits(r.x.t, _dev(r.d["x"])), f"{cid}: the input latents changed"
    if c.entry in S.ADVANCING:
        assert int(r.step.t.item()) == S.S_ROW + advanced and int(r.ticket.t.item()) == 0, (cid, r.step.t.item(), r.ticket.t.item())
    else:
        assert int(r.step.t.item()) == S.S_ROW and int(r.ticket.t.item()) == 0, cid
    for g in r.guarded:
        assert g.intact(), f"{cid}: a guard element changed"
    return out


def _record(c, mode, ratios):
    record_parity("step_forms", S.case_id(c), mode, **{k: v for k, v in ratios.items()})


def _model(r, j=0, x=None, hist=None):
    args, kw = r.model_args(j, x=x, hist=hist)
    return S.step_model(*args, **kw)


def _f32(r, j=0):
    args, kw = r.model_args(j)
    return S.step_f32(*args, **kw)


def _ids(cases):
    return [S.case_id(c) for c in cases]


def _pack_parts_twin(r):
    """the header's promise for ``parts``: what jen1_pack_input_parts writes for this x_out, bit for bit, and the same group statistics
    out of jen1_gn_stats_from_parts"""
    B, C, T, ld, ld_rows, nrep = r.dims
    nb = (T + S.TB - 1) // S.TB
    ld_p = (C + 31) // 32 * 32
    stream = torch.cuda.current_stream().cuda_stream
    y = torch.full((nrep * B, T, ld_p), NAN, dtype=r.tdt, device="cuda")
    parts_p = torch.full((B, nb, ld_p, 2), NAN, device="cuda")
    xo = r.x_out.t.clone()
    r.L.check(r.lib.jen1_pack_input_parts(xo.data_ptr(), None, y.data_ptr(), parts_p.data_ptr(), B, C, 0, T, ld_p, nrep, r.dt, stream),
              "pack_input_parts")
    torch.cuda.synchronize()
    cid = S.case_id(r.c) + "." + r.mode
    assert bool(torch.isfinite(parts_p).all())
    assert _same_bits(parts_p[:, :, :C, :], r.parts.t[:, :, :C, :]), f"{cid}: parts are not jen1_pack_input_parts' bits"
    assert _same_bits(y[:, :, :C], r.rows.t[:, :, :C]), f"{cid}: rows are not jen1_pack_input_parts' bits"
    parts_q = parts_p.clone()
    parts_q[:, :, :C, :] = r.parts.t[:, :, :C, :]
    g = [torch.full((nrep * B * 64,), NAN, device="cuda") for _ in range(2)]
    for parts, gn in zip((parts_p, parts_q), g):
        r.L.check(r.lib.jen1_gn_stats_from_parts(parts.data_ptr(), gn.data_ptr(), B, T, ld_p, nrep, stream), "gn_stats_from_parts")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g[0]).all()) and _same_bits(g[0], g[1]), f"{cid}: group statistics differ"


def _check_select(r, plain):
    """keep in {0, 1}: an exact select between kn = p known + q eps_k (two products and a sum, each rounded) and the unblended x_out"""
    d = r.d
    p, q = S.blend_level(r.rows_spec[0][1])
    kn = torch.from_numpy((p * d["known"]).astype(np.float32) + (q * d["eps_k"]).astype(np.float32))
    keep = torch.from_numpy(np.broadcast_to(d["keep"][:, None, :], kn.shape).copy())
    got, pl = r.x_out.t.cpu(), plain.x_out.t.cpu()
    cid = S.case_id(r.c) + "." + r.mode
    assert r.dims[2] < 3 or (bool((keep == 1).any()) and bool((keep == 0).any()))           # (keep_mask: both from T = 3 on)
    assert _same_bits(got[keep == 1], kn[keep == 1]), f"{cid}: keep == 1 is not the known latents at their level"
    assert _same_bits(got[keep == 0], pl[keep == 0]), f"{cid}: keep == 0 is not the unblended step"
    if r.hist is not None:
        assert _same_bits(r.hist.t, plain.hist.t), f"{cid}: the history must hold the unblended x0"


# ---------------------------------------------------------------------------------------------------------------------
# 1. the general kernel (what only it serves: C % 8 != 0, ld % 8 != 0)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", S.SCALAR_CASES, ids=_ids(S.SCALAR_CASES))
def test_general_kernel(hip, mode, c):
    """cfg_combine, cfg_ddim_step (with and without eps_out / x0_out, table-indexed and direct) and cfg_ddim_step_adv; row kinds 0-3"""
    r = Run(hip, mode, c)
    assert not r.vec
    _record(c, mode, _check(r.run(), _model(r)))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the vector kernel, unpacked
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", S.VEC_UNPACKED_CASES, ids=_ids(S.VEC_UNPACKED_CASES))
def test_vector_kernel_unpacked(hip, mode, c):
    """the same entry points on shapes the vector form serves; at sigma == 0 the whole noise table is NaN and every output finite"""
    r = Run(hip, mode, c)
    assert r.vec
    if c.row in ("k0_det", "k1"):
        assert r.noise is not None and bool(torch.isnan(r.noise).all())
    _record(c, mode, _check(r.run(), _model(r)))


# ---------------------------------------------------------------------------------------------------------------------
# 3. step + pack
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", S.PACK_CASES, ids=_ids(S.PACK_CASES))
def test_step_pack(hip, mode, c):
    """_pack, _pack_blend, _pack_ms without and with a blend: x_out, both replicas of rows, parts (against the model and against
    jen1_pack_input_parts), the history, the blend's exact select"""
    r = Run(hip, mode, c)
    if r.ms and c.row != "k4":
        assert bool(torch.isnan(r.hist.t).all())               # nothing to read: x_out must come out finite all the same
    _record(c, mode, _check(r.run(), _model(r)))
    _pack_parts_twin(r)
    if c.blend:
        plain = Run(hip, mode, c._replace(entry="cfg_ddim_step_pack_ms" if r.ms else "cfg_ddim_step_pack", blend=False)).run()
        _check_select(r, plain)


# ---------------------------------------------------------------------------------------------------------------------
# 4. bits where the header promises them
# ---------------------------------------------------------------------------------------------------------------------
# the cases of the tables that qualify, and -- the sparse crossing does not bring every row kind together with objective noise and no
# rescale -- every row kind once more with the CFG pair (no rescale) and without it, through the unpacked, the packed and the tail forms
_BIT_SHAPES = [(2, 72, 33, 80, 72, 2), (1, 136, 32, 136, 144, 1)]
BIT_CASES = [c for c in S.VEC_UNPACKED_CASES + S.PACK_CASES + S.TAIL_CASES if c.entry != "cfg_combine" and S.bit_exact(c)]
BIT_CASES += [S.Case(e, sh, row, "v" if row == "k3" else "noise", 0 if row == "k3" else clip, 0, 0.7, e.endswith("_blend"), e.endswith("_adv"), True)
              for clip, sh in enumerate(_BIT_SHAPES) for row in S.NOISE_ROWS
              for e in ("cfg_ddim_step_adv", "cfg_ddim_step_pack", "cfg_ddim_step_pack_blend", "step_tail_blend")]
BIT_CASES += [S.Case(e, sh, row, "noise", clip, 0, 0.7, bl, False, True)
              for clip, sh in enumerate(_BIT_SHAPES) for row in S.MS_ROWS for e, bl in (("cfg_ddim_step_pack_ms", False), ("cfg_ddim_step_pack_ms", True),
                                                                                      ("step_tail_ms", True))]
BIT_CASES = list(dict.fromkeys(BIT_CASES))
assert all(S.bit_exact(c) for c in BIT_CASES)


def test_bit_cases_cover_the_promises():
    rows = {c.row for c in BIT_CASES}
    assert rows == set(S.ROW_KINDS)
    assert any(c.blend for c in BIT_CASES) and any(c.blend and c.row == "k4" for c in BIT_CASES)
    assert any(c.shape[-1] == 2 for c in BIT_CASES) and any(c.shape[-1] == 1 for c in BIT_CASES)
    assert {c.entry for c in BIT_CASES} == set(S.ENTRY_POINTS) - {"cfg_combine"}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", BIT_CASES, ids=_ids(BIT_CASES))
def test_vector_forms_give_the_restatement_bits(hip, mode, c):
    """no reduction and no division: every product and sum rounded to float32 by itself, in the documented operand order, is one value"""
    r = Run(hip, mode, c, fill=S.TAIL_FILLS[0]).run()
    f = _f32(r)
    cid = S.case_id(c) + "." + mode
    assert _same_bits(r.x_out.t.cpu(), torch.from_numpy(f.val["x_next"])), f"{cid}: x_out"
    if c.outs:
        assert _same_bits(r.x0_out.t.cpu(), torch.from_numpy(f.val["x0"])), f"{cid}: x0_out"
        assert _same_bits(r.eps_out.t.cpu(), torch.from_numpy(f.val["eps"])), f"{cid}: eps_out"
    if r.ms:
        assert _same_bits(r.hist.t.cpu(), torch.from_numpy(f.val["hist"])), f"{cid}: hist"
    if r.rows is not None:
        C = r.dims[1]
        assert _same_bits(r.rows.t[:, :, :C].cpu(), torch.from_numpy(f.val["rows"]).to(r.tdt)), f"{cid}: rows"


FORM_CONFIGS = [("k0", "x0", 1, 1, 0.7), ("k2", "v", 0, 0, 1.0), ("k3", "v", 0, 1, 0.7)]     # row, objective, clip, scale_cfg, phi


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", S.VEC_SHAPES, ids=["x".join(str(v) for v in s) for s in S.VEC_SHAPES])
def test_vector_forms_agree_bit_for_bit(hip, mode, shape):
    """plain, _adv, _pack and the tail launch are one body: the same x_out bits (reductions and divisions included), rows and parts; a
    step in place (x_out == x, what the stepper does) gives what a step out of place gives"""
    for row, objective, clip, scale_cfg, phi in FORM_CONFIGS:
        runs = {}
        for entry in ("cfg_ddim_step", "cfg_ddim_step_adv", "cfg_ddim_step_pack", "step_tail"):
            for inplace in ((False, True) if entry in S.PACKING else (False,)):
                c = S.Case(entry, shape, row, objective, clip, scale_cfg, phi, False, False, True)
                runs[(entry, inplace)] = Run(hip, mode, c, inplace=inplace, fill=S.TAIL_FILLS[0]).run()
        ref = runs[("cfg_ddim_step", False)]
        assert bool(torch.isfinite(ref.x_out.t).all())
        for key, r in runs.items():
            assert _same_bits(r.x_out.t, ref.x_out.t), (shape, row, key)
            assert all(g.intact() for g in r.guarded), (shape, row, key)
        pk = runs[("cfg_ddim_step_pack", False)]
        for key, r in runs.items():
            if r.rows is not None:
                assert _same_bits(r.rows.t, pk.rows.t) and _same_bits(r.parts.t, pk.parts.t), (shape, row, key)


# ---------------------------------------------------------------------------------------------------------------------
# 5. two consecutive launches of every advancing form
# ---------------------------------------------------------------------------------------------------------------------
TWO_SHAPE, TWO_SCALAR_SHAPE = (2, 72, 33, 80, 72, 2), (2, 5, 33, 7, 2)
TWO_FORMS = [("cfg_ddim_step_adv", TWO_SCALAR_SHAPE, False)] + [(e, TWO_SHAPE, False) for e in S.ADVANCING] + \
            [(e, TWO_SHAPE, True) for e in ("cfg_ddim_step_pack_ms", "step_tail_ms")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", TWO_FORMS, ids=["%s-%s%s" % (e, "x".join(str(v) for v in s), "-blend" if b else "") for e, s, b in TWO_FORMS])
def test_two_consecutive_launches(hip, mode, form):
    """the counter goes s -> s + 1 -> s + 2 with the ticket back at 0 after each launch; the second launch reads row s + 1 of every table
    (the rows differ, all others are NaN) and, in the multistep forms, the x0 the first launch left in the history (NaN before it)"""
    entry, shape, blend = form
    ms = entry.endswith("_ms")
    blend = blend or entry.endswith("_blend")
    c = S.Case(entry, shape, "k4_first" if ms else "k0", "v", 1, 1, 0.7, blend, False, True)
    rows = [("k4_first", 0), ("k4", 1)] if ms else [("k0", 0), ("k0", 1)]
    r = Run(hip, mode, c, rows=rows, fill=S.TAIL_FILLS[1])
    ratios = _check(r.run(), _model(r, 0), advanced=1)
    x1 = r.x_out.t.clone()
    hist1 = None if not ms else r.hist.t.clone()
    # the second launch: its input is what the first one wrote; fresh outputs, the same counter, ticket and history
    r.x.t.copy_(x1)
    r.x_out.t.fill_(NAN)
    if r.rows is not None:
        r.rows.t.copy_(r.rows_before)
        r.parts.t.copy_(r.parts_before)
    r.L.check(r.launch(), entry)
    x1n = x1.cpu().numpy()
    m2 = _model(r, 1, x=x1n, hist=None if not ms else hist1.cpu().numpy())
    r.d = dict(r.d, x=x1n)                                     # (what _check compares the untouched input with)
    second = _check(r, m2, advanced=2)
    _record(c, mode, {k: max(v, second[k]) for k, v in ratios.items()})
    # with the first row's numbers the second result is outside the bound: the rows differ by far more than the bound
    wrong = _model(r, 0, x=x1n, hist=None if not ms else hist1.cpu().numpy())
    diff = np.abs(r.x_out.t.cpu().numpy().astype(np.float64) - wrong.val["x_next"])
    assert (diff > wrong.err["x_next"]).mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 6. the tail forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", range(len(S.TAIL_CASES)), ids=_ids(S.TAIL_CASES))
def test_tail_forms(hip, mode, i):
    """step_tail, _blend, _ms without and with a blend: the step as in test_step_pack and bit-equal to the matching _pack form; every
    byte of every sentinel entry 0xFF, every byte of the zeroed area 0, sync 0 (or NULL), not one byte outside"""
    c = S.TAIL_CASES[i]
    fill = S.TAIL_FILLS[i % len(S.TAIL_FILLS)]
    r = Run(hip, mode, c, fill=fill, sync=(i // len(S.TAIL_FILLS)) % 2 == 0)
    _record(c, mode, _check(r.run(), _model(r)))
    cid = S.case_id(c) + "." + mode
    for g in r.sent:
        assert bool((g.t == 0xFF).all()), f"{cid}: a sentinel entry of {g.t.numel()} bytes is not all ones"
    assert bool((r.zero.t == 0).all()), f"{cid}: the zeroed area of {r.zero.t.numel()} bytes is not all zero"
    assert r.sync is None or int(r.sync.t.item()) == 0, f"{cid}: sync"
    _pack_parts_twin(r)
    twin = Run(hip, mode, c._replace(entry={"step_tail": "cfg_ddim_step_pack", "step_tail_blend": "cfg_ddim_step_pack_blend",
                                            "step_tail_ms": "cfg_ddim_step_pack_ms"}[c.entry])).run()
    assert _same_bits(r.x_out.t, twin.x_out.t) and _same_bits(r.rows.t, twin.rows.t) and _same_bits(r.parts.t, twin.parts.t), cid
    if r.ms:
        assert _same_bits(r.hist.t, twin.hist.t), cid
    if c.blend:
        _check_select(r, Run(hip, mode, c._replace(entry="cfg_ddim_step_pack_ms" if r.ms else "cfg_ddim_step_pack", blend=False)).run())


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("entry", S.PACKING)
def test_refusals_launch_nothing(hip, mode, entry):
    """a pack or tail form without the vector form (C % 8 != 0), or with the history on the latents: a non-zero return, and every guarded
    buffer, the counter and the ticket bit-identical"""
    ms = entry.endswith("_ms")
    c = S.Case(entry, (2, 72, 33, 80, 72, 2), "k4" if ms else "k0", "noise", 1, 1, 0.7, entry.endswith("_blend"), False, True)
    r = Run(hip, mode, c, fill=S.TAIL_FILLS[1])
    snap = r.snapshot()
    assert r.launch(C_arg=70) != 0 and b"vector form" in r.lib.jen1_last_error()
    assert r.unchanged(snap)
    if ms:
        assert r.launch(hist=r.x.ptr()) != 0 and b"must not be the latents" in r.lib.jen1_last_error()
        assert r.unchanged(snap)
    assert r.launch() == 0                                     # and the same buffers are served once the arguments are right
    _check(r, _model(r))
