"""Float64 references of the one-launch conv GEMM ``jen1_conv_gemm`` (include/jen1_hip.h) form by form: the case tables the GPU test
drives its three kernel families with (csrc/conv_gemm.hip LDS-staged, csrc/stream_gemm.hip register-direct, csrc/tile_gemm.hip lean
tiles), their inputs, the references and the deliberately wrong variants of every reference; importable without a GPU
(tests/test_conv_gemm_refs_host.py pins all of it, tests/test_gpu_conv_gemm_forms.py runs it).

A case is ONE ``OpBuilder.conv`` call with the tile configuration -- and where the case says so the tile geometry, the LDS stage and the
K split -- forced through ``force``.  The reference is the contract of the header written the way the model writes the operation
(reference blocks.py:34-53, :69-95, :137-145, :148-165, :219-231, :427-446), on channel-last tensors, in float64, on operands rounded to
the launch dtype (``persistent_phases_common.prologue_ref`` / ``conv_phase_ref``: there is no second conv reference here).  Tables and
vectors stay float32.  The statistics a launch is HANDED (gn_stats*, ln_rowstats) are float64 sums of the rounded operands cast to
float32, the producer's contract; the statistics it LEAVES are compared with float64 sums of the reference output.

``wrong=`` selects one mistake such a kernel can plausibly make; ``wrong_kinds`` lists the ones a case can show, and the host test
requires each of them to be at least ``POWER`` times the GPU tolerance away from the right answer in the GPU test's own metric.
"""
import torch

from jen1_amd import lib as L
from persistent_phases_common import (HALO, NEXT, ROW0, SCALE, _up, ceil_div, ceil_to, conv_phase_ref, group_sums, prologue_ref, stat_rel,  # noqa: F401
                                      written_rel)
from transformer_forms_common import POWER, STAT_TOL, TDTYPE, TOL, _gen, fine_group_sums, rel, rounded, row_sums  # noqa: F401

MODES = ("f32", "bf16")
# BM x BN of every tile configuration (jen1_cfg_bm / jen1_cfg_bn; the host test compares)
CFG_BM = {0: 64, 1: 128, 2: 16, 3: 16, 4: 16, 5: 128, 6: 128, 7: 128, 8: 256, 9: 256, 10: 64}
CFG_BN = {0: 64, 1: 64, 2: 64, 3: 32, 4: 16, 5: 64, 6: 32, 7: 16, 8: 32, 9: 16, 10: 64}
FAMILY_CFGS = {"lds": (0, 1, 2, 3, 4), "direct": (2, 3, 4), "tile": (5, 6, 7, 8, 9, 10)}
FILM_ROWS, FILM_OFF = 6, 8
FILM_STEPS = (5, 1)                  # the device scalar's two values: neither is an entry of film_row
FILM_ROW = (4, 0, 2, 3)
SENTINEL = 7.5                       # what y holds before the launch: finite, exact in bfloat16

PAD, EDGE, KTAIL, MASKRES, CROPSTAT, PADCOUNT, TANH = ("pad_before_prologue", "edge_tap_dropped", "k_tail_dropped", "residual_after_mask",
                                                       "stats_with_cropped", "pad_group_count", "gelu_tanh")
STAT_WRONG = (CROPSTAT,)             # mistakes of the output statistics alone: judged with stat_rel against STAT_TOL
# the families whose kernel can make each mistake: the host test requires a case of each of them for it (the direct kernel has no
# prologue; the T* tiles no K split, stage, activation or row mask)
ALL3 = ("lds", "direct", "tile")
WRONG_FAMILIES = {"halo_read": ALL3, "ps_off_ignored": ALL3, EDGE: ALL3, CROPSTAT: ALL3,
                  "stats_next_element": ("lds", "tile"), "scale_after_norm": ("lds", "tile"), "film_row0": ("lds", "tile"),
                  "step_ignored": ("lds", "tile"), PAD: ("lds", "tile"), PADCOUNT: ("lds", "tile"),
                  KTAIL: ("lds", "direct"), MASKRES: ("lds", "direct"), TANH: ("lds", "direct")}


def tile_geometry(B, L_out, BN):
    """OpBuilder.tile_geometry: (positions per tile, balanced over the tiles of a row; batch elements per tile)"""
    nt = ceil_div(L_out, BN)
    tb = ceil_div(L_out, nt)
    return tb, max(1, min(B, BN // tb))


# ====================================================================================================== cases
def _case(family, form, cfg, **kw):
    c = dict(family=family, form=form, cfg=cfg, B=3, L_in=9, L_out=None, c0=64, c1=0, creal=None, M=64, out_C=None, taps=1, stride=1,
             pad_left=0, pro=L.PRO_NONE, groups=0, eps=1e-5, film=None, src1_scale=1.0, ln=None, ln_C=0, extras=(), act=L.ACT_NONE,
             residual=False, res_pad=0, row_scale=False, y_f32=False, bias=True, ps_f=1, ps_off=0, L_y=None, y_row0=0, out_L=None, gn_out=False,
             rs_out=False, tb=None, nb=None, kc_stage=None, splitk=1, reject=None, not_wrong=(), neg_pre=False)
    assert not set(kw) - set(c), set(kw) - set(c)
    c.update(kw)
    c["L_out"] = c["L_out"] if c["L_out"] is not None else c["L_in"]
    c["out_C"] = c["out_C"] or c["M"] // c["ps_f"]
    c["L_y"] = c["L_y"] if c["L_y"] is not None else c["L_out"] * c["ps_f"]
    c["out_L"] = c["out_L"] if c["out_L"] is not None else c["y_row0"] + c["L_y"]
    c["ld_y"] = ceil_to(c["out_C"], 32)
    c["direct"] = family == "direct"
    # the tile the launch runs with: forced, or OpBuilder.tile_geometry's (the T* tiles: one batch element per tile)
    tb, nb = tile_geometry(c["B"], c["L_out"], CFG_BN[cfg])
    c["tb_eff"] = c["tb"] or tb
    c["nb_eff"] = 1 if family == "tile" else (c["nb"] or (max(1, min(c["B"], CFG_BN[cfg] // c["tb_eff"])) if c["tb"] else nb))
    return c


K3 = dict(taps=3, pad_left=1)
TWO = dict(c1=64, src1_scale=2 ** -0.5)
GN, GNS, LN_, SILU, GELU = L.PRO_GN, L.PRO_GN_SILU, L.PRO_LN, L.PRO_SILU, L.ACT_GELU
STRADDLE = "straddles the source boundary"


def _lds_forms(cfg):
    """the LDS-staged kernel (csrc/conv_gemm.hip): W64x64, W128x64, and the S16x* tiles with direct = 0"""
    BN = CFG_BN[cfg]
    f = {
        # ---- tiles: partial batch tile, partial position tile, nb tb < BN, 80 GEMM rows (a partial M tile for BM 64 / 128)
        "tiles_partial": dict(L_in=37, M=80, tb=5, nb=2, **K3),
        "tiles_full": dict(L_in=37, M=80, tb=BN, nb=1, **K3),
        # ---- stages and split-K
        "sk3_5chunks": dict(c0=160, splitk=3, kc_stage=1, **K3),                      # slices of 2, 2, 1 chunks in stages of 1
        "sk2_two_src_st1": dict(**TWO, splitk=2, kc_stage=1, **K3),                   # the split lies on the x0 / x1 boundary
        "sk2_two_src_st2": dict(**TWO, splitk=2, kc_stage=2, **K3),
        "st1_96_64": dict(c0=96, c1=64, kc_stage=1, **K3),
        "st3_96_64": dict(c0=96, c1=64, kc_stage=3, **K3),                            # stages of 3 + 2 chunks: the boundary between them
        "st2_96_64_refused": dict(c0=96, c1=64, kc_stage=2, **K3, reject=STRADDLE),
        # ---- sub-pixel
        "up4_crop1_row0": dict(M=128, y_row0=3, out_L=4 * 11 - 1 + 5, **_up(4, 1, 11)),
        "up2_crop3_stats": dict(M=128, gn_out=True, rs_out=True, **_up(2, 3, 11)),
        # ---- prologues
        "gn_g1": dict(pro=GN, groups=1, **K3),
        "gn_g4_two": dict(pro=GN, groups=4, **TWO, **K3),
        "gn_g32": dict(pro=GN, groups=32, **K3),
        "gnsilu_g1_causal": dict(pro=GNS, groups=1, taps=3, pad_left=2),
        "gnsilu_g4": dict(pro=GNS, groups=4, **K3),
        "gnsilu_g32_two": dict(pro=GNS, groups=32, **TWO, **K3),                      # groups of 4 channels: a staged vector spans two
        "gnsilu_g8_two_quarter": dict(pro=GNS, groups=8, c1=64, src1_scale=0.25, **K3),
        "gn_g4": dict(pro=GN, groups=4, **K3),
        "gn_g32_two": dict(pro=GN, groups=32, **TWO, **K3),
        "gnsilu_g4_two": dict(pro=GNS, groups=4, **TWO, **K3),
        "gnsilu_g32": dict(pro=GNS, groups=32, **K3),
        # one group over two sources: its width is the concat's, which the source boundary cuts
        "gn_g1_two_refused": dict(pro=GN, groups=1, **TWO, **K3, reject=STRADDLE),
        "gnsilu_g1_two_refused": dict(pro=GNS, groups=1, **TWO, **K3, reject=STRADDLE),
        # 48 real channels in a 64-wide tensor, handed over as Plan.resblock does: gn = (groups, REAL channels, gamma / beta of the padded
        # width) -> gn_cpg = 12, gn_count = 12 L, and the last group takes the 16 padding columns.  The entry point accepts it
        "gnsilu_pad48": dict(pro=GNS, groups=4, creal=48, **K3),
        "film_b": dict(pro=GNS, groups=4, film="b", **K3),
        "film_row": dict(pro=GNS, groups=4, film="row", **TWO, **K3),
        "film_step": dict(pro=GNS, groups=4, film="step", **K3),
        "ln_affine_causal": dict(pro=LN_, ln="affine", c0=160, ln_C=150, taps=3, pad_left=2),
        "ln_plain": dict(pro=LN_, ln="plain", c0=160, ln_C=150),
        "silu_f32out": dict(pro=SILU, y_f32=True, **K3),
        # ---- epilogues
        "no_bias": dict(bias=False, **K3),
        "gelu": dict(act=GELU, **K3),
        "gelu_neg": dict(act=GELU, neg_pre=True, **K3),
        "residual_ld": dict(residual=True, res_pad=32, M=80, **K3),
        "row_scale_res": dict(residual=True, row_scale=True, **K3),
        "y_f32": dict(y_f32=True, **K3),
        "stats_plain": dict(gn_out=True, rs_out=True, **K3),
        "stats_sk2": dict(c0=128, splitk=2, gn_out=True, rs_out=True, **K3),
    }
    # ---- stride and edges: the live-tap skip is decided per tile; with tb = 1 the first and the last tiles drop different taps
    for taps, stride, pad in ((5, 2, 2), (9, 4, 4), (3, 1, 2)):
        for Ln, tb in ((37, 4), (37, 1), (1, 1), (2, 1)):
            f[f"k{taps}s{stride}p{pad}_L{Ln}_tb{tb}"] = dict(L_in=Ln, L_out=ceil_div(Ln, stride), taps=taps, stride=stride, pad_left=pad, tb=tb)
    for fct in (2, 4):
        for crop in (0, 1, 3):
            f[f"up{fct}_crop{crop}"] = dict(M=32 * fct, **_up(fct, crop, 11))
    return f


def _direct_forms(cfg):
    """the register-direct streaming kernel (csrc/stream_gemm.hip): S16x* with direct = 1, no prologue"""
    f = {
        "taps3_two_src": dict(c1=32, **K3),                                           # segments derived as (tap, source) pairs
        "explicit_3seg": dict(extras=((96, -1), (32, 1))),                            # shifts 0, -1, +1 with 2, 3 and 1 chunks
        "dead_L1": dict(L_in=1, extras=((32, -1),), **K3),
        "dead_L2": dict(L_in=2, extras=((32, -1),), **K3),
        "flat_sk3": dict(c0=32, taps=7, pad_left=3, splitk=3),                        # 7 chunks: slices of 3, 3, 1
        "nb2_partial": dict(L_in=5, tb=5, nb=2, **K3),
        "up2_crop1": dict(M=64, **_up(2, 1, 7)),
        "up4_crop3": dict(M=128, **_up(4, 3, 7)),
        "up8_crop3": dict(M=256, **_up(8, 3, 7)),
        "up2_crop3_stats": dict(M=128, gn_out=True, rs_out=True, **_up(2, 3, 7)),
        "no_bias": dict(bias=False, **K3),
        "gelu": dict(act=GELU, **K3),
        "gelu_neg": dict(act=GELU, neg_pre=True, **K3),
        "residual_ld": dict(residual=True, res_pad=32, M=80, **K3),
        # (a third of the rows are masked and the loud residual sets the scale: a tap lost to the whole tile is 0.27 of it in bf16)
        "row_scale_res": dict(residual=True, row_scale=True, not_wrong=(EDGE,), **K3),
        "y_f32": dict(y_f32=True, **K3),
        "stats_plain": dict(gn_out=True, rs_out=True, **K3),
    }
    return f


def _tile_forms(cfg):
    """the lean tile kernel (csrc/tile_gemm.hip): the six T* configurations"""
    BM, BN = CFG_BM[cfg], CFG_BN[cfg]
    g8 = dict(pro=GNS, groups=8)
    f = {
        "pos_short": dict(L_in=BN - 3, M=BM, **K3),
        "pos_over": dict(L_in=BN + 1, M=BM + 16, **K3),
        "pos_two_tiles": dict(L_in=2 * BN + 5, M=BM + 16, **K3),
        "silu": dict(pro=SILU, L_in=BN + 1, M=BM, **K3),
        "gn_g1": dict(pro=GN, groups=1, L_in=BN + 1, M=BM, **K3),
        "gnsilu_g1": dict(pro=GNS, groups=1, L_in=BN + 1, M=BM, taps=3, pad_left=2),
        "gnsilu_g4_two": dict(pro=GNS, groups=4, L_in=BN + 1, M=BM, **TWO, **K3),
        "gn_g8_two": dict(pro=GN, groups=8, L_in=BN + 1, M=BM, **TWO, **K3),
        "gnsilu_g8_two_quarter": dict(L_in=BN + 1, M=BM, c1=64, src1_scale=0.25, **g8, **K3),
        "gnsilu_pad48": dict(pro=GNS, groups=4, creal=48, L_in=BN + 1, M=BM, **K3),
        "film_b": dict(film="b", L_in=BN + 1, M=BM, **g8, **K3),
        "film_row": dict(film="row", L_in=BN + 1, M=BM, **g8, **TWO, **K3),
        "film_step": dict(film="step", L_in=BN + 1, M=BM, **g8, **K3),
        "extra1": dict(L_in=BN + 1, M=BM, extras=((64, 0),), **g8, **K3),
        "extra2": dict(L_in=BN + 1, M=BM, extras=((64, 0), (32, 0)), **g8, **K3),
        "up2_crop1": dict(M=2 * BM, **_up(2, 1, BN // 2 + 3)),
        "up4_crop3": dict(M=4 * BM, **_up(4, 3, BN // 2 + 3)),
        "up2_crop3_row0_stats": dict(M=2 * BM, gn_out=True, y_row0=2, out_L=2 * (BN // 2 + 3) - 3 + 5, **_up(2, 3, BN // 2 + 3)),
        "no_bias": dict(bias=False, L_in=BN + 1, M=BM, **K3),
        "residual_ld": dict(residual=True, res_pad=32, L_in=BN + 1, M=BM + 16, **K3),
        "y_f32": dict(y_f32=True, L_in=BN + 1, M=BM, **K3),
        "stats_plain": dict(gn_out=True, L_in=BN + 1, M=BM, **K3),
        "gelu_refused": dict(act=GELU, L_in=BN + 1, M=BM, **K3, reject="T* tile configurations take"),
        "ln_refused": dict(pro=LN_, ln="plain", c0=160, ln_C=150, L_in=BN + 1, M=BM, reject="T* tile configurations take"),
    }
    for taps, stride in ((3, 1), (5, 2), (9, 4)):
        kw = dict(L_in=2 * BN + 5, L_out=ceil_div(2 * BN + 5, stride), taps=taps, stride=stride, pad_left=(taps - 1) // 2, M=BM)
        f[f"k{taps}s{stride}"] = dict(**kw)
        f[f"k{taps}s{stride}_gnsilu"] = dict(**kw, **g8)
    return f


def _cases():
    out = {}
    for family, forms in (("lds", _lds_forms), ("direct", _direct_forms), ("tile", _tile_forms)):
        for cfg in FAMILY_CFGS[family]:
            for form, kw in forms(cfg).items():
                out[f"{family}.{form}.cfg{cfg}"] = _case(family, form, cfg, **kw)
    return out


CASES = _cases()


def force_of(c):
    """the ``force`` argument of OpBuilder.conv for a case"""
    f = {"cfg": c["cfg"]}
    if c["family"] != "tile":
        f["direct"] = c["direct"]
        f["splitk"] = c["splitk"]
    for k in ("tb", "nb", "kc_stage"):
        if c[k] is not None:
            f[k] = c[k]
    return f


# ====================================================================================================== geometry of a case
def k_chunks(c):
    """32-channel chunks the K split works on: per tap for the LDS-staged kernel, the flat (segment, chunk) list for the direct one"""
    kch = (c["c0"] + c["c1"]) // 32
    return kch * c["taps"] + sum(ce for ce, _ in c["extras"]) // 32 if c["direct"] else kch


def k_stages(c):
    """LDS stages per K slice of an LDS-staged case"""
    cps = ceil_div(k_chunks(c), c["splitk"])
    return ceil_div(cps, min(c["kc_stage"] or cps, cps))


def k_tail(c):
    """K columns (of W [M][K] in K order) of the chunks a kernel would lose with its last split-K slice -- or, without a split, with
    its last LDS stage; None when the slice / stage is all there is"""
    G, cm = k_chunks(c), c["c0"] + c["c1"]
    cps = ceil_div(G, c["splitk"])
    if c["splitk"] > 1:
        lo = (c["splitk"] - 1) * cps
    elif not c["direct"] and c["family"] == "lds" and k_stages(c) > 1:
        st = min(c["kc_stage"], cps)
        lo = (G - 1) // st * st
    else:
        return None
    chunks = torch.arange(lo, G)
    cols = (chunks[:, None] * 32 + torch.arange(32)[None, :]).reshape(-1)
    if c["direct"]:
        return cols
    return (torch.arange(c["taps"])[:, None] * cm + cols[None, :]).reshape(-1)


def _shifts(c):
    return [k - c["pad_left"] for k in range(c["taps"])] + [sh for _, sh in c["extras"]]


def stored_columns(c):
    """the GEMM columns of which at least one sub-pixel phase survives the crop"""
    t = torch.arange(c["L_out"])
    ty = t[:, None] * c["ps_f"] + torch.arange(c["ps_f"])[None, :] - c["ps_off"]
    return t[((ty >= 0) & (ty < c["L_y"])).any(1)]


def reads_padding(c):
    """a stored GEMM column reads a row outside [0, L_in)"""
    t = stored_columns(c) * c["stride"]
    return any(bool(((t + sh < 0) | (t + sh >= c["L_in"])).any()) for sh in _shifts(c))


def _edge_applies(c):
    """a tap is dead for the first column of some position tile and live for a later column of it"""
    tb, Lo, st = c["tb_eff"], c["L_out"], c["stride"]
    for sh in _shifts(c):
        for t0 in range(0, Lo, tb):
            if t0 * st + sh < 0 and any(0 <= t * st + sh < c["L_in"] for t in stored_columns(c).tolist() if t0 <= t < t0 + tb):
                return True
    return False


def _cropped(c):
    ty = torch.arange(c["L_out"] * c["ps_f"]) - c["ps_off"]
    return bool(((ty < 0) | (ty >= c["L_y"])).any())


def wrong_kinds(c, mode):
    """the mistakes a case can show in ``mode`` (``not_wrong``: the ones its table entry takes out, with the reason there)"""
    if c["reject"]:
        return []
    pad = reads_padding(c)
    w = [HALO] * (pad and c["B"] >= 3)
    w += ["ps_off_ignored"] * (c["ps_f"] > 1 and c["ps_off"] > 0)
    w += [NEXT] * bool(c["groups"])
    # src1_scale on the wrong side of the normalisation changes the x1 half by the factor itself: 1 - 2^-1/2 = 0.29 of the largest output
    # at most, below POWER x the bf16 tolerance whatever the inputs -- shown in float32, and in bf16 by the cases with a scale of 1 / 4
    w += [SCALE] * bool(c["groups"] and c["c1"] and (mode == "f32" or c["src1_scale"] <= 0.25))
    w += [ROW0] * (c["film"] in ("row", "b")) + ["step_ignored"] * (c["film"] == "step")
    w += [PAD] * (pad and (bool(c["groups"]) or c["ln"] == "affine"))
    w += [EDGE] * _edge_applies(c)
    w += [KTAIL] * (k_tail(c) is not None)
    w += [MASKRES] * (c["residual"] and c["row_scale"])
    w += [CROPSTAT] * (c["gn_out"] and _cropped(c) and not c["residual"] and not c["row_scale"])
    w += [PADCOUNT] * (c["creal"] is not None)
    # the two GELUs differ by 5e-4 at most: visible in float32 alone, and only where no output is large (``neg_pre``, see ``inputs``)
    w += [TANH] * (c["act"] == GELU and c["neg_pre"] and mode == "f32")
    return [k for k in w if k not in c["not_wrong"]]


# ====================================================================================================== inputs
def inputs(name, c):
    """float32 operands of one case, from a generator seeded by the case name.  Activations have a non-zero mean and differ in mean and
    spread from one batch element to the next (statistics over the wrong rows show; a neighbour's row in place of a zero shows); x1 is
    wide (src1_scale on the wrong side of the normalisation shows); beta and the FiLM shifts are of order 1 (a padding row that went
    through the prologue is silu(~1), not ~0); row_scale is zero on rows whose residual is loud; padding columns hold zeros, in the
    activations and in the weights, as the engine lays them out."""
    g = _gen("conv_gemm", c["family"], c["form"], c["L_in"], c["M"])            # (the same operands on every tile configuration they fit)
    r = lambda *s: torch.randn(*s, generator=g)
    B, Li, c0, c1 = c["B"], c["L_in"], c["c0"], c["c1"]
    cm = c0 + c1
    real = c["creal"] or (c["ln_C"] if c["ln"] else c0)            # real channels of x0
    amp = 4.0 ** (torch.arange(B) % 3).float() if c["groups"] or c["ln"] else 1.0 + 0.5 * (torch.arange(B) % 2).float()
    elem = amp[:, None, None]
    # a normalised source lies 2 sigma below zero: the image of a zero row is then far above every data row's
    t = dict(x0=(r(B, Li, c0) + (-2.0 if c["groups"] else 0.5)) * elem)
    t["x0"][..., real:] = 0.0
    if c1:
        t["x1"] = (r(B, Li, c1) * 3.0 - 0.7) * elem
    for i, (ce, sh) in enumerate(c["extras"]):
        # (an unshifted extra segment only adds to every output: quiet, so that it does not bury the mistakes of the taps beside it)
        t[f"e{i}"] = (r(B, Li, ce) + 0.3) * (1.0 if sh else 0.5)
    for k in ["x0"] * (not c["groups"] and not c["ln"]) + [f"e{i}" for i, (_, sh) in enumerate(c["extras"]) if sh]:
        # raw shifted sources: the first and the last row of a batch element are loud -- the rows a halo read takes from the neighbour
        t[k][:, 0] *= 3.0
        t[k][:, -1] *= 3.0
    K = c["taps"] * cm + sum(ce for ce, _ in c["extras"])
    t["W"] = r(c["M"], K) / K ** 0.5
    for k in range(c["taps"]):
        t["W"][:, k * cm + real: k * cm + c0] = 0.0
        if c["creal"]:
            # the real channels of the last GroupNorm group weigh three times the others: what its statistics do to them shows
            t["W"][:, k * cm + real - real // c["groups"]: k * cm + real] *= 3.0
    if c["bias"]:
        t["bias"] = r(c["out_C"]) * 0.5
    if c["neg_pre"]:
        # every pre-activation in about [-4, -1]: GELU's outputs stay within [-0.17, 0], where the 5e-4 between erf and tanh GELU shows
        t["W"] *= 0.25
        t["bias"] = r(c["out_C"]) * 0.2 - 2.5
    if c["row_scale"]:
        rs = torch.rand(B, c["out_L"], generator=g) + 0.5
        rs[:, 1::3] = 0.0
        t["row_scale"] = rs
    if c["residual"]:
        res = r(B, c["out_L"], c["out_C"]) * 0.25
        if c["row_scale"]:
            res[:, 1::3] *= 8.0
        t["residual"] = res
    if c["groups"]:
        t["gamma"], t["beta"] = torch.rand(cm, generator=g) + 0.5, r(cm) + 0.5
        t["gamma"][real:c0], t["beta"][real:c0] = 0.0, 0.0
        if c["film"]:
            tab = r(FILM_ROWS, 2 * cm + FILM_OFF + 3)
            # scale (the kernel adds 1) and shift differ from one table row to the next
            tab[:, FILM_OFF: FILM_OFF + cm] = tab[:, FILM_OFF: FILM_OFF + cm] * 0.5 + 0.4 * torch.arange(FILM_ROWS).float()[:, None]
            tab[:, FILM_OFF + cm: FILM_OFF + 2 * cm] += 0.5 * torch.arange(FILM_ROWS).float()[:, None] - 1.0
            t["film"] = tab
            t["film_row"] = torch.tensor(FILM_ROW[:B], dtype=torch.int32) if c["film"] in ("row", "step") else None
    if c["ln"] == "affine":
        t["ln_gamma"], t["ln_beta"] = torch.rand(c0, generator=g) + 0.5, r(c0) + 0.5
        t["ln_gamma"][real:], t["ln_beta"][real:] = 0.0, 0.0
    return t


def producer_stats(c, t, mode):
    """what the producers of the sources hand the launch: gn_stats0 / gn_stats1 [B][32][2] and ln_rowstats [B L_in][2], float64 sums of the
    rounded operands cast to float32"""
    out = {}
    if c["groups"]:
        out["gn0"] = fine_group_sums(rounded(t["x0"], mode)).float()
        if c["c1"]:
            out["gn1"] = fine_group_sums(rounded(t["x1"], mode)).float()
    if c["ln"]:
        out["rs0"] = row_sums(rounded(t["x0"], mode), c["ln_C"]).float()
    return out


# ====================================================================================================== references
def ref(c, t, mode, step=None, wrong=None):
    """[B][out_L][out_C] float64 reference of a case on operands rounded to ``mode``, NaN where the launch writes nothing (wrong
    "stats_with_cropped": [B][L_out ps_f][out_C], every GEMM column); step: the value of the film_step scalar of a ``film == "step"`` case"""
    op = lambda k: rounded(t.get(k), mode)
    cm = c["c0"] + c["c1"]
    kw = {}
    if c["groups"]:
        kw = dict(p1=t["gamma"].double(), p2=t["beta"].double())
        if c["film"]:
            by_step = c["film"] == "step" and wrong != "step_ignored"
            rows = torch.full((c["B"],), int(step)) if by_step else (torch.arange(c["B"]) if c["film"] == "b" else t["film_row"])
            # x (scale + 1) + shift on top of gamma / beta (blocks.py:140-143), as one affine per table row
            sc1 = t["film"][:, FILM_OFF: FILM_OFF + cm].double() + 1.0
            kw = dict(p1=kw["p1"] * sc1, p2=kw["p2"] * sc1 + t["film"][:, FILM_OFF + cm: FILM_OFF + 2 * cm].double(), rows=rows)
    ln = None
    if c["ln"]:
        ln = (c["ln_C"], t.get("ln_gamma"), t.get("ln_beta"), 1e-5)
    x = prologue_ref(op("x0"), op("x1"), src1_scale=c["src1_scale"], groups=c["groups"], eps=c["eps"], silu=c["pro"] in (GNS, SILU), wrong=wrong,
                     creal=c["creal"], ln=ln, pad_row=wrong == PAD, **kw)
    pad_row = None
    if wrong == PAD:
        x, pad_row = x[:, :-1], x[:, -1:]
    extras = [(op(f"e{i}"), sh) for i, (_, sh) in enumerate(c["extras"])]
    return conv_phase_ref(x, extras, rounded(t["W"], mode), t.get("bias"), taps=c["taps"], stride=c["stride"], pad_left=c["pad_left"],
                          L_out=c["L_out"], act=c["act"], residual=op("residual"), out_C=c["out_C"], ps_f=c["ps_f"], ps_off=c["ps_off"],
                          L_y=c["L_y"], y_row0=c["y_row0"], out_L=c["out_L"], wrong=wrong, pad_row=pad_row, row_scale=t.get("row_scale"),
                          tb=c["tb_eff"], k_tail=k_tail(c) if wrong == KTAIL else None)


def out_stats(c, y):
    """the statistics a launch leaves, from the reference output ``y`` (NaN = not written): out_gn_stats [B][32][2] over the written rows
    per fine group of ld_y / 32 columns (the padding columns hold nothing), out_rowstats [B][rows][2] over the out_C columns"""
    yz = torch.nan_to_num(y.double(), nan=0.0)
    full = torch.cat([yz, torch.zeros(*yz.shape[:2], c["ld_y"] - c["out_C"], dtype=torch.float64)], -1)
    return group_sums(full, 32), row_sums(yz)


# ====================================================================================================== form coverage
# what every tile configuration of a family must be reached with (the host test requires it): the prologues and epilogue options the
# family's kernel accepts, a K range staged in more than one LDS stage, split-K, the sub-pixel store, extra K segments
ACCEPTS = {
    "lds": [("pro", p) for p in (L.PRO_NONE, GN, GNS, LN_, SILU)] +
           [("epi", e) for e in ("no_bias", "gelu", "residual", "row_scale", "y_f32", "gn_out", "rs_out")] +
           [("multi_stage", True), ("splitk", True), ("subpixel", True), ("batch_tile", True)],
    "direct": [("pro", L.PRO_NONE)] + [("epi", e) for e in ("no_bias", "gelu", "residual", "row_scale", "y_f32", "gn_out", "rs_out")] +
              [("splitk", True), ("subpixel", True), ("extras", True), ("batch_tile", True)],
    "tile": [("pro", p) for p in (L.PRO_NONE, GN, GNS, SILU)] + [("epi", e) for e in ("no_bias", "residual", "y_f32", "gn_out")] +
            [("subpixel", True), ("extras", True)],
}


def features(c):
    """the forms a case reaches, in ACCEPTS' vocabulary (batch_tile: nb > 1 with a partial last batch tile)"""
    f = {("pro", c["pro"])}
    f |= {("epi", k) for k, on in (("no_bias", not c["bias"]), ("gelu", c["act"] == GELU), ("residual", c["residual"]),
                                   ("row_scale", c["row_scale"]), ("y_f32", c["y_f32"]), ("gn_out", c["gn_out"]), ("rs_out", c["rs_out"])) if on}
    f |= {(k, True) for k, on in (("multi_stage", c["family"] == "lds" and k_stages(c) > 1), ("splitk", c["splitk"] > 1),
                                  ("subpixel", c["ps_f"] > 1), ("extras", bool(c["extras"])),
                                  ("batch_tile", c["nb_eff"] > 1 and c["B"] % c["nb_eff"] != 0)) if on}
    return f


def forms_reached():
    """{(family, cfg): the set of forms its accepted cases reach}"""
    got = {(fam, cfg): set() for fam, cfgs in FAMILY_CFGS.items() for cfg in cfgs}
    for c in CASES.values():
        if not c["reject"]:
            got[(c["family"], c["cfg"])] |= features(c)
    return got
