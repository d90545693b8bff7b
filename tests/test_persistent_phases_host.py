"""No GPU: pins tests/persistent_phases_common.py, the references and case tables of tests/test_gpu_persistent_phases.py.

  * every float64 reference agrees with an independent torch expression (F.conv1d, F.conv_transpose1d, F.group_norm,
    F.scaled_dot_product_attention) on cases of the table;
  * on the committed inputs, every wrong variant a case lists is at least POWER times the GPU tolerance away from the right answer in
    the metric the GPU test uses, in both modes;
  * the cases reach every value of every form parameter (persistent_phases_common.FORMS), as the restated geometry computes it;
  * the restated geometry agrees with the library's own host helpers, which fill host memory from plain pointers and need no device.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import persistent_phases_common as P
from jen1_amd import lib as L
from jen1_amd.packing import convT_weight_to_gemm
from persistent_phases_common import MODES, POWER, STAT_TOL, TOL

torch.set_num_threads(4)
_memo = {}


def inputs(kind, name):
    key = (kind, name)
    if key not in _memo:
        table, fn = {"deep": (P.DEEP_CONV_CASES, P.conv_inputs), "long": (P.LONG_CASES, P.conv_inputs), "tile": (P.TILE_CASES, P.conv_inputs),
                     "attn": (P.ATTN_CASES, P.attn_inputs), "stats": (P.STATS_CASES, P.stats_inputs)}[kind]
        _memo[key] = fn(f"{kind}.{name}", table[name])
    return _memo[key]


def step_of(c):
    return P.FILM_STEPS[0] if c["film"] == "step" else None


# ---------------------------------------------------------------------------------------------- references against torch
@pytest.mark.parametrize("name", ["taps3_halo", "taps3_causal", "stride2", "stride4", "plain"])
def test_conv_ref_is_conv1d(name):
    c, t = P.DEEP_CONV_CASES[name], inputs("deep", name)
    cm = c["c0"]
    w = t["W"].double().reshape(c["M"], c["taps"], cm).permute(0, 2, 1)            # K order (tap, channel) -> [M][C][k]
    x = t["x0"].double().permute(0, 2, 1)
    right = (c["L_out"] - 1) * c["stride"] + c["taps"] - c["pad_left"] - c["L_in"]
    want = F.conv1d(F.pad(x, (c["pad_left"], max(right, 0))), w, t["bias"].double(), stride=c["stride"])[:, :, : c["L_out"]].permute(0, 2, 1)
    got = P.conv_ref(c, {**t, "W": t["W"].double()}, "f32")
    assert got.shape == want.shape and P.rel(got, want) < 1e-6            # (operands rounded to float32: 6e-8 each)


@pytest.mark.parametrize("f,crop,y_row0", [(2, 0, 0), (2, 1, 0), (4, 3, 2), (4, 2, 0)])
def test_conv_ref_subpixel_is_conv_transpose1d(f, crop, y_row0):
    g = torch.Generator().manual_seed(f * 10 + crop)
    B, Ci, Co, Ln = 2, 32, 16, 5
    x = torch.randn(B, Ln, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(Ci, Co, 2 * f, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    p = f // 2 + f % 2
    full = F.conv_transpose1d(x.permute(0, 2, 1), w, b, stride=f, padding=p, output_padding=f % 2)
    assert full.shape[-1] == f * Ln
    want = full[:, :, crop // 2: crop // 2 + f * Ln - crop].permute(0, 2, 1)
    Wg = convT_weight_to_gemm(w, f)                                                # [2][f Co][Ci], tap 0 <-> x[q - 1]
    W = torch.cat([Wg[0], Wg[1]], 1)
    up = P._up(f, crop, Ln)
    got = P.conv_phase_ref(x, [], W, b, taps=2, pad_left=1, L_out=up["L_out"], out_C=Co, ps_f=f, ps_off=up["ps_off"], L_y=up["L_y"],
                           y_row0=y_row0, out_L=y_row0 + up["L_y"] + 1)
    assert torch.isnan(got[:, :y_row0]).all() and torch.isnan(got[:, y_row0 + up["L_y"]:]).all()
    win = got[:, y_row0: y_row0 + up["L_y"]]
    assert not torch.isnan(win).any() and P.rel(win, want) < 1e-12


@pytest.mark.parametrize("groups,silu", [(1, False), (8, True), (16, False)])
def test_prologue_ref_is_group_norm(groups, silu):
    g = torch.Generator().manual_seed(groups)
    x0, x1 = torch.randn(3, 5, 64, generator=g, dtype=torch.float64) + 0.5, torch.randn(3, 5, 64, generator=g, dtype=torch.float64) * 3
    gamma, beta = torch.rand(128, generator=g, dtype=torch.float64) + 0.5, torch.randn(128, generator=g, dtype=torch.float64)
    want = F.group_norm(torch.cat([x0, x1 * 2 ** -0.5], -1).permute(0, 2, 1), groups, gamma, beta, 1e-5).permute(0, 2, 1)
    want = F.silu(want) if silu else want
    got = P.prologue_ref(x0, x1, src1_scale=2 ** -0.5, groups=groups, p1=gamma, p2=beta, silu=silu)
    assert P.rel(got, want) < 1e-12
    # the fused GroupNorm-FiLM table: gamma (scale + 1) and beta (scale + 1) + shift, row by batch element
    scale, shift = torch.randn(6, 128, generator=g, dtype=torch.float64), torch.randn(6, 128, generator=g, dtype=torch.float64)
    rows = torch.tensor([4, 0, 2])
    got = P.prologue_ref(x0, x1, src1_scale=2 ** -0.5, groups=groups, p1=gamma * (scale + 1), p2=beta * (scale + 1) + shift, rows=rows)
    plain = F.group_norm(torch.cat([x0, x1 * 2 ** -0.5], -1).permute(0, 2, 1), groups, gamma, beta, 1e-5).permute(0, 2, 1)
    assert P.rel(got, plain * (scale[rows][:, None] + 1) + shift[rows][:, None]) < 1e-12


def test_conv_ref_composes_prologue_extras_dual_range_and_edges():
    """the parts F.conv1d does not have, each against a direct expression on one case of the table"""
    c, t = P.DEEP_CONV_CASES["extra_segs"], inputs("deep", "extra_segs")
    xh = F.silu(F.group_norm(t["x0"].double().permute(0, 2, 1), 8, t["gamma"].double(), t["beta"].double(), 1e-5))
    W = t["W"].double()
    y = F.conv1d(F.pad(xh, (1, 1)), W[:, :192].reshape(32, 3, 64).permute(0, 2, 1), t["bias"].double()).permute(0, 2, 1)
    y = y + t["e0"].double() @ W[:, 192:224].T
    e1 = F.pad(t["e1"].double(), (0, 0, 1, 0))[:, :-1]                           # row shift -1: column t reads row t - 1
    y = y + e1 @ W[:, 224:].T
    assert P.rel(P.conv_ref(c, t, "f32"), y) < 1e-6
    c, t = P.DEEP_CONV_CASES["dual_range"], inputs("deep", "dual_range")
    X, W = torch.cat([t["x0"], t["e0"]], -1).double(), t["W"].double()
    lo = X[..., :64] @ W[:32, :64].T + t["bias"].double()[:32] + t["residual"].double()
    hi = F.gelu(X @ W[32:].T + t["bias"].double()[32:])
    assert P.rel(P.conv_ref(c, t, "f32"), torch.cat([lo, hi], -1)) < 1e-6
    c, t = P.DEEP_CONV_CASES["edge_bias_L2"], inputs("deep", "edge_bias_L2")
    y = F.conv1d(F.pad(t["x0"].double().permute(0, 2, 1), (1, 1)), t["W"].double().reshape(32, 3, 32).permute(0, 2, 1)).permute(0, 2, 1)
    y[:, 0] += t["edge_bias"][0].double()
    y[:, 1] += t["edge_bias"][1].double()
    assert P.rel(P.conv_ref(c, t, "f32"), y) < 1e-6


@pytest.mark.parametrize("name", ["self_d32_q7_k7_h1", "self_d8_q24_k24_h1", "cross_d64_q12_k129_h1", "cross_step_d8_q5_k129_h1"])
def test_attn_ref_is_sdpa(name):
    c, t = P.ATTN_CASES[name], inputs("attn", name)
    H, d, Cc, B, Nq, Nk = c["H"], c["d"], c["Cc"], c["B"], c["Nq"], c["Nk"]
    mid = H * d
    step = P.ATTN_STEPS[0] if c["kind"] == "cross_step" else None
    got = P.attn_ref(c, t, "f32", step=step)
    q = P.attn_qkv(c, t, "f32") if c["kind"] == "self" else t["q"].double()
    x = q[..., :Cc]
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    fin = lambda raw, off: (raw - mean * t["u"].double()[off: off + mid]) / torch.sqrt(var + 1e-5) + t["b"].double()[off: off + mid]
    qq = fin(q[..., Cc: Cc + mid], Cc)
    if c["kind"] == "self":
        k, v = fin(q[..., Cc + mid: Cc + 2 * mid], Cc + mid), fin(q[..., Cc + 2 * mid: Cc + 3 * mid], Cc + 2 * mid)
    else:
        kv = t["kv"].double()[t["kv_row"].long()].clone()
        if c["kind"] != "cross":
            for b in range(B):
                if int(t["extra_row"][b]) >= 0:
                    kv[b, Nk - 1, :mid] = t["kv_extra"].double()[step, t["kx_off"]: t["kx_off"] + mid]
                    kv[b, Nk - 1, mid:] = t["kv_extra"].double()[step, t["vx_off"]: t["vx_off"] + mid]
        k, v = kv[..., :mid], kv[..., mid:]
    h = lambda a: a.reshape(B, -1, H, d).transpose(1, 2)
    want = F.scaled_dot_product_attention(h(qq), h(k), h(v), is_causal=c["causal"]).transpose(1, 2).reshape(B, Nq, mid)
    assert P.rel(got, want) < 1e-9


def test_stats_and_partial_sums_refs():
    g = torch.Generator().manual_seed(1)
    y = torch.randn(3, 7, 256, generator=g, dtype=torch.float64)
    want = torch.stack([y.reshape(3, 7, 16, 16).sum(dim=(1, 3)), (y ** 2).reshape(3, 7, 16, 16).sum(dim=(1, 3))], -1)
    assert torch.allclose(P.entry_sums(y), want)
    # a long phase's partial array, built the way the kernel fills it (unit e = tile e // mblocks, M block e % mblocks; wave s = 16 GEMM rows;
    # GEMM row m is output channel m % out_C), gives the same sums -- for a plain conv (out_C = M = 256) and a sub-pixel one (out_C = 128)
    for out_C, M in ((256, 256), (128, 256), (128, 128)):
        mb, tiles, tb = M // 128, 4, 2
        Y = torch.randn(3, tiles * tb, M, generator=g, dtype=torch.float64)             # GEMM output [B][column][row m]
        part = torch.zeros(3, 8, tiles * mb, 2, dtype=torch.float64)
        for e in range(tiles * mb):
            blk = Y[:, e // mb * tb: (e // mb + 1) * tb, (e % mb) * 128: (e % mb + 1) * 128].reshape(3, tb, 8, 16)
            part[:, :, e, 0], part[:, :, e, 1] = blk.sum(dim=(1, 3)), (blk ** 2).sum(dim=(1, 3))
        by_channel = torch.stack([Y[..., ph * out_C: (ph + 1) * out_C] for ph in range(M // out_C)], 0)      # [ph][B][col][out_C]
        want = torch.stack([by_channel.reshape(-1, 3, tiles * tb, out_C // 16, 16).sum(dim=(0, 2, 4)),
                            (by_channel ** 2).reshape(-1, 3, tiles * tb, out_C // 16, 16).sum(dim=(0, 2, 4))], -1)
        assert torch.allclose(P.long_part_sums(part, mb, out_C), want)
    c, t = P.STATS_CASES["ld256_L24"], inputs("stats", "ld256_L24")
    y = t["z"].double() @ t["wf"].double().T + t["bf"].double()
    y = y.float().double()
    want = torch.stack([y.reshape(3, 24, 32, 8).sum(dim=(1, 3)), (y ** 2).reshape(3, 24, 32, 8).sum(dim=(1, 3))], -1)
    assert P.stat_rel(P.stats_ref(c, t, "f32"), want) < 1e-6


# ---------------------------------------------------------------------------------------------- the wrong variants are far away
def _conv_wrong_cases():
    return [(kind, name, w) for kind, table in (("deep", P.DEEP_CONV_CASES), ("long", P.LONG_CASES), ("tile", P.TILE_CASES))
            for name, c in table.items() for w in c["wrong"] + c["wrong_f32"]]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,name,wrong", _conv_wrong_cases())
def test_conv_wrong_variants_are_far(kind, name, wrong, mode):
    c = {"deep": P.DEEP_CONV_CASES, "long": P.LONG_CASES, "tile": P.TILE_CASES}[kind][name]
    if mode != "f32" and wrong in c["wrong_f32"]:
        return          # (listed for float32 alone: the case table says why)
    t = inputs(kind, name)
    key = (kind, name, mode, "ref")
    if key not in _memo:
        _memo[key] = P.conv_ref(c, t, mode, step=step_of(c))
    ref = _memo[key]
    if wrong == P.TAIL:
        tb, n = (P.long_geometry(c["M"], c["L_out"], P.NWG // c["B"])[2], c["out_C"] // 16) if kind == "long" else (P.tile_geometry(c)["tb"], 8)
        d = P.stat_rel(P.part_stats_ref(c, t, mode, tb, n, step=step_of(c), wrong=wrong), P.part_stats_ref(c, t, mode, tb, n, step=step_of(c)))
        assert d >= POWER * STAT_TOL[mode], (name, wrong, mode, d)
        return
    bad = P.conv_ref(c, t, mode, step=step_of(c), wrong=wrong)
    m = ~torch.isnan(ref) & ~torch.isnan(bad)            # (a mistake that also writes other rows is judged on the rows both write)
    d = P.rel(bad[m], ref[m])
    assert d >= POWER * TOL[mode], (name, wrong, mode, d)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(P.ATTN_CASES))
def test_attn_wrong_variants_are_far(name, mode):
    c, t = P.ATTN_CASES[name], inputs("attn", name)
    step = P.ATTN_STEPS[0] if c["kind"] == "cross_step" else None
    ref = P.attn_ref(c, t, mode, step=step)
    for wrong in P.attn_wrong_kinds(c):
        d = P.rel(P.attn_ref(c, t, mode, step=step, wrong=wrong), ref)
        assert d >= POWER * TOL[mode], (name, wrong, mode, d)
    if c["kind"] == "cross_step":
        # ... and the two values of the device scalar give answers that far apart, as does reading extra_row as the row
        other = P.attn_ref(c, t, mode, step=P.ATTN_STEPS[1])
        assert P.rel(other, ref) >= POWER * TOL[mode]
        assert P.rel(P.attn_ref({**c, "kind": "cross_row"}, t, mode), ref) >= POWER * TOL[mode]


def test_film_steps_give_different_answers():
    for kind, table in (("deep", P.DEEP_CONV_CASES), ("long", P.LONG_CASES)):
        c, t = table["film_step"], inputs(kind, "film_step")
        for mode in MODES:
            a, b = (P.conv_ref(c, t, mode, step=s) for s in P.FILM_STEPS)
            assert P.rel(a, b) >= POWER * TOL[mode]


# ---------------------------------------------------------------------------------------------- forms
def test_cases_reach_every_form():
    got = P.forms_reached()
    missing = {k: sorted(set(v) - got[k], key=str) for k, v in P.FORMS.items() if set(v) - got[k]}
    assert not missing, missing


@pytest.mark.parametrize("mode", MODES)
def test_cases_reach_the_form_they_state(mode):
    for name, c in P.DEEP_CONV_CASES.items():
        g = P.deep_conv_geometry(c, mode)
        assert g is not None, name
        for k, v in P.case_reach(c, mode).items():
            assert g[k] == v, (name, mode, k, g[k], v)
    for name, c in P.LONG_CASES.items():
        r = P.long_reach(c)
        for k, v in c["reach"].items():
            assert r[k] == v, (name, k, r[k], v)
    for name, c in P.TILE_CASES.items():
        g = P.tile_geometry(c)
        for k, v in c["reach"].items():
            assert g[k] == v, (name, k, g[k], v)


# ---------------------------------------------------------------------------------------------- the library's own host helpers
# They only fill host memory from the pointers they are given (never dereferenced on the host), so they run here.  The first eight int32
# of a filled deep descriptor are kind, n_units, rot, dep, dep_units, lds_bytes, dtype, ntrips (include/jen1_deep.h: "field order is
# ABI"); jen1_deep_link's headers are {n_units, rot, kind, units before} per phase.
FAKE = 1 << 20          # a 16-byte aligned non-null "device pointer"


def _conv_args(c, mode, nb_only=False):
    a = L.ConvArgs()
    a.x0, a.c0, a.ld0 = FAKE, c["c0"], c["c0"]
    if c["c1"]:
        a.x1, a.c1, a.ld1 = FAKE, c["c1"], c["c1"]
    a.w, a.bias, a.y = FAKE, FAKE, FAKE
    a.dtype = L.F32 if mode == "f32" else L.BF16
    a.B, a.L_in, a.L_out = c["B"], c["L_in"], c["L_out"]
    a.taps, a.stride, a.pad_left = c["taps"], c["stride"], c["pad_left"]
    a.out_C, a.ps_f, a.ps_off, a.M = c["out_C"], c["ps_f"], c["ps_off"], c["M"]
    a.ld_y, a.L_y, a.y_brows, a.y_row0 = c["out_C"], c["L_y"], c["out_L"], c["y_row0"]
    if c["residual"]:
        a.residual, a.ld_res = FAKE, c["m_split"] or c["out_C"]
    if c["edge_bias"]:
        a.edge_bias = FAKE
    a.pro_mode, a.src1_scale, a.act = c["pro"], c["src1_scale"], c["act"]
    cm = c["c0"] + c["c1"]
    if c["groups"]:
        a.gn_groups, a.gn_cpg, a.gn_count, a.gn_eps = c["groups"], cm // c["groups"], cm // c["groups"] * c["L_in"], c["eps"]
        a.gn_gamma = a.gn_beta = a.gn_stats0 = a.gn_stats1 = FAKE
        if c["film"]:
            a.film, a.film_off, a.film_C, a.film_ld = FAKE, P.FILM_OFF, cm, 2 * cm + P.FILM_OFF + 3
            a.film_row = FAKE if c["film"] in ("row", "step") else None
            a.film_step = FAKE if c["film"] == "step" else None
    for i, (ce, sh) in enumerate(c["extras"]):
        s = a.seg[i]
        s.x, s.ld, s.shift, s.kch = FAKE, ce, sh, ce // 32
    a.nseg = len(c["extras"])
    a.m_split, a.k_split = c["m_split"], c["k_split"]
    return a


def _lib():
    try:
        return L.load()
    except OSError as e:          # the library is not built: the GPU file checks the same fields on the descriptors it records
        pytest.skip(f"libjen1_hip.so does not load here: {e}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(P.DEEP_CONV_CASES))
def test_deep_conv_geometry_is_the_librarys(name, mode):
    lib = _lib()
    c = P.DEEP_CONV_CASES[name]
    g = P.deep_conv_geometry(c, mode)
    buf = (C.c_char * lib.jen1_deep_phase_size())()
    rc = lib.jen1_deep_phase_conv(C.byref(_conv_args(c, mode)), P.deep_nb_cap(c, mode), C.cast(buf, C.c_void_p))
    assert rc == 0, lib.jen1_last_error()
    head = (C.c_int32 * 8).from_buffer(buf)
    assert (head[0], head[1], head[5], head[7]) == (0, g["n_units_unlinked"], g["lds_bytes"] if g["mrep"] == 1 else head[5], g["ntrips"]), \
        (name, mode, list(head), g)
    bb = lib.jen1_deep_blob_bytes()
    blobs, hdrs = (C.c_char * bb)(), (C.c_int32 * 4)()
    lds = lib.jen1_deep_link(C.cast(buf, C.c_void_p), 1, P.NWG, C.cast(blobs, C.c_void_p), C.cast(hdrs, C.c_void_p))
    assert lds > 0, lib.jen1_last_error()
    linked = (C.c_int32 * 8).from_buffer(blobs)
    assert hdrs[0] == linked[1] == g["n_units"] and linked[5] == g["lds_bytes"] and hdrs[2] == 0, (name, mode, list(hdrs), list(linked), g)


@pytest.mark.parametrize("mode", MODES)
def test_attn_geometry_is_the_librarys(mode):
    lib = _lib()
    dt = L.F32 if mode == "f32" else L.BF16
    for name, c in P.ATTN_CASES.items():
        self_attn = c["kind"] == "self"
        g = P.attn_geometry(c["d"], c["Nq"], c["Nk"], mode, self_attn=self_attn, finish_kv=self_attn)
        mid = c["H"] * c["d"]
        buf = (C.c_char * lib.jen1_deep_phase_size())()
        rc = lib.jen1_deep_phase_attention(FAKE, FAKE, FAKE, FAKE, None if self_attn else FAKE, None, None, None, 0, 0, 0, c["B"], c["H"], c["d"],
                                           c["Nq"], c["Nk"], 32 + 4 * mid, 32, 32 + 4 * mid, 32 + mid, 32 + 2 * mid, mid, int(c["causal"]),
                                           c["d"] ** -0.5, FAKE, FAKE, 32, 1e-5, 1, int(self_attn), 3 if self_attn else 2, dt,
                                           C.cast(buf, C.c_void_p))
        assert rc == 0, (name, lib.jen1_last_error())
        head = (C.c_int32 * 8).from_buffer(buf)
        assert (head[0], head[1], head[5]) == (1, c["B"] * c["H"] * g["nqc"], g["lds_bytes"]), (name, mode, list(head), g)
    # the shape the table leaves out is refused by the library too
    assert P.attn_geometry(128, 33, 33, mode, self_attn=True, finish_kv=True) is None
    buf = (C.c_char * lib.jen1_deep_phase_size())()
    assert lib.jen1_deep_phase_attention(FAKE, FAKE, FAKE, FAKE, None, None, None, None, 0, 0, 0, 3, 1, 128, 33, 33, 544, 32, 544, 160, 288, 128,
                                         0, 128 ** -0.5, FAKE, FAKE, 32, 1e-5, 1, 1, 3, dt, C.cast(buf, C.c_void_p)) != 0


def test_stats_and_long_geometry_are_the_librarys():
    lib = _lib()
    for c in P.STATS_CASES.values():
        buf = (C.c_char * lib.jen1_deep_phase_size())()
        assert lib.jen1_deep_phase_stats(FAKE, FAKE, c["B"], c["L"], c["ld"], L.F32, C.cast(buf, C.c_void_p)) == 0
        head = (C.c_int32 * 8).from_buffer(buf)
        assert (head[0], head[1]) == (2, c["B"])
    for name, c in P.LONG_CASES.items():
        G = P.NWG // c["B"]
        mb, tl, tb = C.c_int(0), C.c_int(0), C.c_int(0)
        assert lib.jen1_long_geometry(c["M"], c["L_out"], G, C.byref(mb), C.byref(tl), C.byref(tb)) == 0, name
        assert (mb.value, tl.value, tb.value) == P.long_geometry(c["M"], c["L_out"], G), name
        for mode in MODES:
            # the descriptor of the phase itself (statistics as totals: the partial forms need the phase in front)
            buf = (C.c_char * 512)()
            a = _conv_args(c, mode)
            rc = lib.jen1_long_phase_conv(C.byref(a), G, FAKE if c["groups"] else None, 0, 1, 32, FAKE if c["c1"] and c["groups"] else None,
                                          0, 1, 32, 0, FAKE if c["stats"] else None, C.cast(buf, C.c_void_p))
            assert rc == 0, (name, mode, lib.jen1_last_error())
            assert lib.jen1_long_phase_units(C.cast(buf, C.c_void_p)) == mb.value * tl.value
    assert P.long_geometry(128, 97 * 32, 32) is None and lib.jen1_long_geometry(128, 97 * 32, 32, None, None, None) != 0
    assert P.long_geometry(192, 10, 32) is None and lib.jen1_long_geometry(192, 10, 32, None, None, None) != 0
