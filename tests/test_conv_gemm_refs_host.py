"""No GPU: pins tests/conv_gemm_common.py, the references and case tables of tests/test_gpu_conv_gemm_forms.py.

  * the extended references (persistent_phases_common.prologue_ref / conv_phase_ref with the one-launch contract's keywords) agree with
    an independent float64 torch expression (F.conv1d, F.conv_transpose1d, F.group_norm, F.layer_norm, F.silu, F.gelu) on EVERY case;
  * on the committed inputs every wrong variant a case can show is at least POWER times the GPU tolerance away from the right answer in
    the metric the GPU test uses, in both modes, and every variant has a case in every family whose kernel can make that mistake;
  * every (family, tile configuration) is reached with every form its kernel accepts (conv_gemm_common.ACCEPTS);
  * the tile tables agree with the library and with OpBuilder, and OpBuilder._choose_tiles honours ``tb`` / ``nb`` / ``kc_stage`` in
    ``force`` -- and changes nothing without them.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_gemm_common as G
from conv_gemm_common import MODES, POWER, STAT_TOL, TOL
from jen1_amd import lib as L

torch.set_num_threads(4)
_memo = {}
LIVE = [n for n, c in G.CASES.items() if not c["reject"]]


def inputs(name):
    if name not in _memo:
        _memo[name] = G.inputs(name, G.CASES[name])
    return _memo[name]


def step_of(c):
    return G.FILM_STEPS[0] if c["film"] == "step" else None


# ---------------------------------------------------------------------------------------------- references against torch
def torch_expr(c, t, step=None):
    """the case the way the model writes it, on [B][C][L] float64 tensors with torch's own layers; [B][out_L][out_C], NaN = not written"""
    d = lambda k: t[k].double()
    B, Li, Lo, c0, cm = c["B"], c["L_in"], c["L_out"], c["c0"], c["c0"] + c["c1"]
    x = (d("x0") if not c["c1"] else torch.cat([d("x0"), d("x1") * c["src1_scale"]], -1)).permute(0, 2, 1)          # [B][C][L]
    if c["groups"]:
        real = c["creal"] or cm
        h = F.group_norm(x[:, :real], c["groups"], d("gamma")[:real], d("beta")[:real], c["eps"])
        h = F.pad(h, (0, 0, 0, cm - real))                 # (the padding channels meet zero weights: their value does not matter)
        if c["film"]:
            rows = torch.full((B,), step) if c["film"] == "step" else (torch.arange(B) if c["film"] == "b" else t["film_row"].long())
            f = d("film")[rows]
            h = h * (f[:, G.FILM_OFF: G.FILM_OFF + cm, None] + 1.0) + f[:, G.FILM_OFF + cm: G.FILM_OFF + 2 * cm, None]
        x = h
    elif c["ln"]:
        n = c["ln_C"]
        g_, b_ = (d("ln_gamma")[:n], d("ln_beta")[:n]) if c["ln"] == "affine" else (None, None)
        x = F.pad(F.layer_norm(x.permute(0, 2, 1)[..., :n], (n,), g_, b_, 1e-5), (0, c0 - n)).permute(0, 2, 1)
    if c["pro"] in (G.GNS, G.SILU):
        x = F.silu(x)
    W = d("W")
    bias = d("bias") if c["bias"] else None
    Kt = c["taps"] * cm
    if c["ps_f"] == 1:
        right = max((Lo - 1) * c["stride"] + c["taps"] - c["pad_left"] - Li, 0)
        w = W[:, :Kt].reshape(c["M"], c["taps"], cm).permute(0, 2, 1)                       # K order (tap, channel) -> [M][C][k]
        y = F.conv1d(F.pad(x, (c["pad_left"], right)), w, bias, stride=c["stride"])[:, :, :Lo]
        off = Kt
        for i, (ce, sh) in enumerate(c["extras"]):
            e = F.pad(d(f"e{i}").permute(0, 2, 1), (1, 1 + Lo * c["stride"]))[:, :, 1 + sh:]     # column t reads row t stride + shift
            y = y + F.conv1d(e[:, :, : (Lo - 1) * c["stride"] + 1], W[:, off: off + ce, None], stride=c["stride"])
            off += ce
        if c["act"] == G.GELU:
            y = F.gelu(y)
        out = torch.full((B, c["out_L"], c["out_C"]), float("nan"), dtype=torch.float64)
        out[:, c["y_row0"]: c["y_row0"] + Lo] = y.permute(0, 2, 1)
    else:
        # the 2-tap sub-pixel GEMM is ConvTranspose1d(k = 2 f, stride f, padding p) with the centre crop (packing.convT_weight_to_gemm):
        # tap 0 <-> x[q - 1] holds kernel entries f .. 2 f, tap 1 <-> x[q] entries 0 .. f; GEMM row m = r out_C + co
        f_, oc = c["ps_f"], c["out_C"]
        w_r = torch.cat([W[:, cm:].reshape(f_, oc, cm), W[:, :cm].reshape(f_, oc, cm)], 0)       # [j][co][ci]
        p = f_ // 2 + f_ % 2
        full = F.conv_transpose1d(x, w_r.permute(2, 1, 0), bias, stride=f_, padding=p, output_padding=f_ % 2)
        assert full.shape[-1] == f_ * Li
        st = c["ps_off"] - p
        out = torch.full((B, c["out_L"], oc), float("nan"), dtype=torch.float64)
        out[:, c["y_row0"]: c["y_row0"] + c["L_y"]] = full[:, :, st: st + c["L_y"]].permute(0, 2, 1)
    if c["residual"]:
        out = out + d("residual")
    if c["row_scale"]:
        out = out * d("row_scale")[..., None]
    return out


@pytest.mark.parametrize("name", LIVE)
def test_ref_is_the_torch_expression(name):
    """float32 operands are their own float64 values, so the "f32" reference and the expression see the same numbers"""
    c, t = G.CASES[name], inputs(name)
    want = torch_expr(c, t, step_of(c))
    got = G.ref(c, t, "f32", step=step_of(c))
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)), name
    assert not torch.isnan(got).all() and G.written_rel(got, want) < 1e-9, (name, G.written_rel(got, want))
    if c["film"] == "step":
        other = G.ref(c, t, "f32", step=G.FILM_STEPS[1])
        assert G.written_rel(other, torch_expr(c, t, G.FILM_STEPS[1])) < 1e-9
        for mode in MODES:
            assert G.written_rel(G.ref(c, t, mode, step=G.FILM_STEPS[1]), G.ref(c, t, mode, step=G.FILM_STEPS[0])) >= POWER * TOL[mode]


def test_statistics_refs():
    """out_stats: plain sums of the written rows, per fine group of ld_y / 32 columns and per row over the out_C columns; producer_stats:
    the sums of the rounded operands"""
    for name in ("lds.up2_crop3_stats.cfg0", "lds.stats_plain.cfg3", "tile.up2_crop3_row0_stats.cfg8", "direct.stats_plain.cfg4"):
        c, t = G.CASES[name], inputs(name)
        y = G.ref(c, t, "bf16")
        gn, rs = G.out_stats(c, y)
        w = ~torch.isnan(y).all(-1)
        cpf = c["ld_y"] // 32
        for b in range(c["B"]):
            rows = y[b][w[b]]
            for fg in (0, 5, 31):
                blk = rows[:, fg * cpf: (fg + 1) * cpf]
                blk = blk[:, : max(0, min(cpf, c["out_C"] - fg * cpf))]
                assert torch.allclose(gn[b, fg], torch.stack([blk.sum(), (blk * blk).sum()]), rtol=1e-12, atol=1e-12)
            assert torch.allclose(rs[b][w[b]][:, 0], rows.sum(-1)) and torch.allclose(rs[b][w[b]][:, 1], (rows * rows).sum(-1))
            assert not bool(rs[b][~w[b]].any())
    c, t = G.CASES["lds.gn_g4_two.cfg0"], inputs("lds.gn_g4_two.cfg0")
    st = G.producer_stats(c, t, "bf16")
    x1 = t["x1"].to(torch.bfloat16).double()
    assert st["gn1"].dtype == torch.float32 and torch.allclose(st["gn1"][1, 3, 0].double(), x1[1][:, 6:8].sum(), rtol=1e-6)
    c, t = G.CASES["lds.ln_plain.cfg0"], inputs("lds.ln_plain.cfg0")
    st = G.producer_stats(c, t, "f32")
    assert torch.allclose(st["rs0"][2, 4, 1].double(), (t["x0"][2, 4, :150].double() ** 2).sum(), rtol=1e-6)
    assert not bool(t["x0"][..., 150:].any()) and not bool(t["W"][:, 150:160].any())


# ---------------------------------------------------------------------------------------------- the wrong variants are far away
@pytest.mark.parametrize("name", LIVE)
def test_wrong_variants_are_far(name):
    c, t = G.CASES[name], inputs(name)
    for mode in MODES:
        ref = G.ref(c, t, mode, step=step_of(c))
        for wrong in G.wrong_kinds(c, mode):
            bad = G.ref(c, t, mode, step=step_of(c), wrong=wrong)
            if wrong in G.STAT_WRONG:
                d = G.stat_rel(G.out_stats(c, bad)[0], G.out_stats(c, ref)[0])
                assert d >= POWER * STAT_TOL[mode], (name, wrong, mode, d)
            else:
                m = ~torch.isnan(ref) & ~torch.isnan(bad)            # (a mistake that also writes other rows is judged on the rows both write)
                d = G.rel(bad[m], ref[m])
                assert d >= POWER * TOL[mode], (name, wrong, mode, d)


def test_every_variant_has_a_case_in_every_family_and_cfg():
    """... that can make the mistake, in both modes where the mistake shows in both (gelu_tanh: float32 alone)"""
    have = {}
    for name in LIVE:
        c = G.CASES[name]
        for mode in MODES:
            for w in G.wrong_kinds(c, mode):
                have.setdefault((w, c["family"], c["cfg"]), set()).add(mode)
    for w, fams in G.WRONG_FAMILIES.items():
        for fam in fams:
            for cfg in G.FAMILY_CFGS[fam]:
                modes = have.get((w, fam, cfg), set())
                assert "f32" in modes and (w == G.TANH or "bf16" in modes), (w, fam, cfg, modes)
    assert {w for w, _, _ in have} == set(G.WRONG_FAMILIES)
    for (w, fam, _) in have:
        assert fam in G.WRONG_FAMILIES[w], (w, fam)


def test_wrong_variants_need_the_keyword():
    """a wrong variant that a case cannot show is the right answer there (the applicability rules leave nothing out by accident):
    spot checks"""
    c, t = G.CASES["lds.up2_crop3.cfg0"], inputs("lds.up2_crop3.cfg0")
    assert G.HALO not in G.wrong_kinds(c, "f32")          # the crop takes both columns that read a halo row
    assert torch.equal(torch.nan_to_num(G.ref(c, t, "f32", wrong=G.HALO)), torch.nan_to_num(G.ref(c, t, "f32")))
    c, t = G.CASES["lds.k5s2p2_L2_tb1.cfg0"], inputs("lds.k5s2p2_L2_tb1.cfg0")
    assert G.EDGE not in G.wrong_kinds(c, "f32")          # one column per tile: its first column is all of it
    assert torch.equal(G.ref(c, t, "f32", wrong=G.EDGE), G.ref(c, t, "f32"))
    assert G.EDGE in G.wrong_kinds(G.CASES["lds.k5s2p2_L37_tb4.cfg0"], "bf16")


# ---------------------------------------------------------------------------------------------- forms
def test_cases_reach_every_form_on_every_cfg():
    got = G.forms_reached()
    missing = {k: [f for f in G.ACCEPTS[k[0]] if f not in v] for k, v in got.items()}
    assert not {k: v for k, v in missing.items() if v}, missing
    # what a family does not accept is in no accepted case of it, and is asserted as refused where the table has a refusal for it
    for name in LIVE:
        c = G.CASES[name]
        assert G.features(c) <= set(G.ACCEPTS[c["family"]]), (name, G.features(c) - set(G.ACCEPTS[c["family"]]))
    for cfg in G.FAMILY_CFGS["tile"]:
        assert G.CASES[f"tile.gelu_refused.cfg{cfg}"]["reject"] and G.CASES[f"tile.ln_refused.cfg{cfg}"]["reject"]


def test_cases_state_the_geometry_the_issue_names():
    for cfg in G.FAMILY_CFGS["lds"]:
        BM, BN = G.CFG_BM[cfg], G.CFG_BN[cfg]
        c = G.CASES[f"lds.tiles_partial.cfg{cfg}"]
        assert c["B"] % c["nb_eff"] and c["L_out"] % c["tb_eff"] and c["nb_eff"] * c["tb_eff"] < BN
        assert (c["M"] % BM != 0) == (BM > 16)               # a partial M tile for BM 64 and 128
        assert G.CASES[f"lds.tiles_full.cfg{cfg}"]["tb_eff"] == BN
        c = G.CASES[f"lds.sk3_5chunks.cfg{cfg}"]
        assert G.k_chunks(c) == 5 and G.k_stages(c) == 2 and G.k_tail(c).numel() == 3 * 32            # the last slice: one chunk of each tap
        assert G.k_stages(G.CASES[f"lds.st3_96_64.cfg{cfg}"]) == 2 and G.k_stages(G.CASES[f"lds.st1_96_64.cfg{cfg}"]) == 5
        # tb = 1 on the strided convs: the first tile drops leading taps, the last one trailing taps
        for form, taps, st, pad in (("k5s2p2_L37_tb1", 5, 2, 2), ("k9s4p4_L37_tb1", 9, 4, 4)):
            c = G.CASES[f"lds.{form}.cfg{cfg}"]
            assert 0 * st + 0 - pad < 0 and (c["L_out"] - 1) * st + taps - 1 - pad >= c["L_in"]
    for cfg in G.FAMILY_CFGS["direct"]:
        c = G.CASES[f"direct.flat_sk3.cfg{cfg}"]
        assert G.k_chunks(c) == 7 and G.k_tail(c).tolist() == list(range(6 * 32, 7 * 32))
        c = G.CASES[f"direct.nb2_partial.cfg{cfg}"]
        assert c["nb_eff"] == 2 and c["B"] % 2 == 1
    for cfg in G.FAMILY_CFGS["tile"]:
        BM, BN = G.CFG_BM[cfg], G.CFG_BN[cfg]
        assert [G.CASES[f"tile.{f}.cfg{cfg}"]["L_out"] for f in ("pos_short", "pos_over", "pos_two_tiles")] == [BN - 3, BN + 1, 2 * BN + 5]
        assert {G.CASES[f"tile.{f}.cfg{cfg}"]["M"] for f in ("pos_short", "pos_over")} == {BM, BM + 16}
        for f in ("up2_crop1", "up4_crop3", "up2_crop3_row0_stats"):
            assert G.CASES[f"tile.{f}.cfg{cfg}"]["out_C"] % BM == 0


# ---------------------------------------------------------------------------------------------- the library and OpBuilder
def test_tile_tables_are_the_librarys_and_opbuilders():
    from jen1_amd.engine import OpBuilder
    lib = L.load()
    for cfg in range(11):
        assert (lib.jen1_cfg_bm(cfg), lib.jen1_cfg_bn(cfg)) == (G.CFG_BM[cfg], G.CFG_BN[cfg])
    for B in (1, 3, 4):
        for Lo in (1, 2, 9, 13, 37, 61, 69, 133):
            for BN in (16, 32, 64):
                assert OpBuilder.tile_geometry(B, Lo, BN)[:2] == G.tile_geometry(B, Lo, BN)


class _Eng:
    """what OpBuilder._choose_tiles reads of an engine, without a device"""

    def __init__(self, mode):
        from jen1_amd.engine import KernelCtx
        self.__dict__.update(KernelCtx(mode, "cpu", target_wgs=256).__dict__)


def _args(c, mode):
    a = L.ConvArgs()
    a.dtype = L.F32 if mode == "f32" else L.BF16
    a.B, a.L_in, a.L_out, a.M, a.out_C, a.ps_f = c["B"], c["L_in"], c["L_out"], c["M"], c["out_C"], c["ps_f"]
    a.c0, a.c1, a.taps, a.stride, a.pad_left, a.pro_mode = c["c0"], c["c1"], c["taps"], c["stride"], c["pad_left"], c["pro"]
    return a


@pytest.mark.parametrize("mode", MODES)
def test_choose_tiles_honours_the_forced_geometry(mode):
    from jen1_amd.engine import OpBuilder
    eng = _Eng(mode)
    for name, c in G.CASES.items():
        ob, a = OpBuilder(eng), _args(c, mode)
        ob._choose_tiles(a, G.force_of(c), k_extra=sum(ce for ce, _ in c["extras"]) // 32, tile_ok=True)
        assert (a.cfg, a.tb, a.nb, a.splitk) == (c["cfg"], c["tb_eff"], c["nb_eff"], c["splitk"]), name
        if c["kc_stage"] and c["family"] == "lds":
            assert a.kc_stage == c["kc_stage"], name
        if c["splitk"] > 1:
            # the slab holds one BM x BN partial tile per (tile, slice) of the FORCED tile count
            tiles = -(-c["L_out"] // a.tb) * -(-c["B"] // a.nb) * -(-c["M"] // G.CFG_BM[c["cfg"]])
            assert ob._max_tiles == tiles and ob._slab_floats == tiles * c["splitk"] * G.CFG_BM[c["cfg"]] * G.CFG_BN[c["cfg"]], name
        # without the three keys the heuristics decide, as they did before the keys existed: the same as with no geometry forced at all
        f = {k: v for k, v in G.force_of(c).items() if k not in ("tb", "nb", "kc_stage")}
        b = _args(c, mode)
        OpBuilder(eng)._choose_tiles(b, f, k_extra=sum(ce for ce, _ in c["extras"]) // 32, tile_ok=True)
        tb, nb = G.tile_geometry(c["B"], c["L_out"], G.CFG_BN[c["cfg"]])
        assert (b.tb, b.nb) == (tb, 1 if c["family"] == "tile" else nb), name
        if c["family"] == "lds" and not c["c1"]:
            assert b.kc_stage == -(-(c["c0"] // 32) // c["splitk"]), name           # one stage: these cases are far below the LDS limit
