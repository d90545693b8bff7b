"""Float64 references of single phases of the two persistent launches (csrc/deep_kernel.hip, csrc/long_kernel.hip), the case tables the
GPU tests drive them with, deliberately wrong variants of every reference and the host helpers' unit-geometry arithmetic restated in
Python; importable without a GPU (tests/test_persistent_phases_host.py pins all of it, tests/test_gpu_persistent_phases.py runs it).

A case is a program of ONE phase on operands that exist before the launch; an operand listed in the case's ``live`` is produced by a
plain 1x1 conv phase in front instead (from a 32-channel tensor ``z.<operand>``), so the phase under test polls it.  Every reference is
written the way the model writes the operation (reference blocks.py:34-53, :69-95, :137-145, :219-231, :355-380), on channel-last tensors,
in float64, on operands rounded to the launch dtype.  ``prologue_ref`` / ``conv_phase_ref`` are also the references of the one-launch
conv GEMM's suite (tests/conv_gemm_common.py): what that contract has more -- a LayerNorm or SiLU-only prologue, a padded last GroupNorm
group, ``row_scale`` -- are keywords whose defaults leave the phases' results as they were, bit for bit.

The ``wrong`` keyword of a reference selects one mistake these kernels can plausibly make; the host tests require that on the committed
inputs every applicable one is at least ``POWER`` times the GPU tolerance away from the right answer in the GPU test's own metric.
"""
import math

import torch
import torch.nn.functional as F

from jen1_amd import lib as L
from transformer_forms_common import (POWER, STAT_TOL, TDTYPE, TOL, _gen, attention_ref, fine_group_sums, gelu, rel, rounded,  # noqa: F401
                                      row_sums)

MODES = ("f32", "bf16")
NWG = 256                      # workgroups of the launch on an MI355X (one per CU): what the case tables were laid out for
# Engine.__init__'s defaults of the three knobs OpBuilder._deep_nb_cap reads
DEEP_NB_MAX, DEEP_UNIT_TARGET, DEEP_REREAD_CAP = 0, 128, 16 << 20


def ceil_div(a, b):
    return -(-a // b)


def ceil_to(a, b):
    return ceil_div(a, b) * b


# ====================================================================================================== conv / linear phase
def prologue_ref(x0, x1, *, src1_scale=1.0, groups=0, eps=1e-5, p1=None, p2=None, rows=None, silu=False, wrong=None, creal=None, ln=None,
                 pad_row=False):
    """[x0, x1 * src1_scale] -> GroupNorm over the concat (``groups`` > 0) with the affine  xhat * p1 + p2  -> SiLU.  p1 / p2: [C]
    (gamma / beta) or the fused GroupNorm-FiLM table's halves [rows][C] with ``rows`` [B] the table row of every batch element.
    creal: the real channels of a tensor padded to C columns (zeros) -- a group is creal / groups channels, the last one also takes the
    padding columns, every group counts creal / groups channels.  ln = (ln_C, gamma or None, beta or None, eps): LayerNorm of every row
    over its first ln_C columns instead (groups = 0; gamma = None: standardise only).  groups = 0 without ln: SiLU only, or nothing.
    pad_row: the image of an all-zero row under the same prologue is appended as row L (conv_phase_ref's ``pad_row``).
    wrong: "stats_next_element" (the statistics of element b also cover element b + 1), "scale_after_norm" (src1_scale applied to the
    normalised values instead of the raw ones), "film_row0" (everybody takes element 0's table row), "pad_group_count" (the last group
    of a padded tensor divides by the channels it covers, padding included)."""
    scale_first = wrong != "scale_after_norm"
    x = x0.double() if x1 is None else torch.cat([x0.double(), x1.double() * (src1_scale if scale_first else 1.0)], -1)
    xin = torch.cat([x, torch.zeros_like(x[:, :1])], 1) if pad_row else x           # the rows to transform (statistics: the real ones)
    if groups:
        B, Ln, C = x.shape
        if creal is not None and creal != C:
            cpg = creal // groups
            gi = (torch.arange(C) // cpg).clamp(max=groups - 1)
            oh = F.one_hot(gi, groups).double()
            n = torch.full((groups,), float(cpg * Ln), dtype=torch.float64)
            if wrong == "pad_group_count":
                n[-1] = float((C - (groups - 1) * cpg) * Ln)
            s1, s2 = x.sum(1) @ oh, (x * x).sum(1) @ oh
            if wrong == "stats_next_element":
                s1, s2, n = s1 + s1.roll(-1, 0), s2 + s2.roll(-1, 0), 2 * n
            mean = s1 / n
            var = s2 / n - mean * mean
            x = (xin - mean[:, None, gi]) / torch.sqrt(var[:, None, gi] + eps)
        else:
            xg = x.reshape(B, Ln, groups, C // groups)
            sg = torch.cat([xg, xg.roll(-1, 0)], 1) if wrong == "stats_next_element" else xg
            mean, var = sg.mean(dim=(1, 3), keepdim=True), sg.var(dim=(1, 3), unbiased=False, keepdim=True)
            x = ((xin.reshape(B, -1, groups, C // groups) - mean) / torch.sqrt(var + eps)).reshape(B, -1, C)
        if not scale_first and x1 is not None:
            x = torch.cat([x[..., : x0.shape[-1]], x[..., x0.shape[-1]:] * src1_scale], -1)
        if p1.dim() == 1:
            x = x * p1.double() + p2.double()
        else:
            r = rows.long() if wrong != "film_row0" else rows.long()[:1].expand(B)
            x = x * p1.double()[r][:, None, :] + p2.double()[r][:, None, :]
    elif ln is not None:
        ln_C, g_, b_, leps = ln
        xs = xin[..., :ln_C]
        x = (xin - xs.mean(-1, keepdim=True)) / torch.sqrt(xs.var(-1, unbiased=False, keepdim=True) + leps)
        if g_ is not None:
            x = x * g_.double() + b_.double()
    else:
        x = xin
    return F.silu(x) if silu else x


def _rows_at(x, idx, wrong, pad=None):
    """rows ``idx`` [L_out] of every batch element of x [B][L][C], zero outside [0, L) -- ``pad`` [B][1][C] there when given.
    wrong "halo_read": a row outside the batch element is whatever lies there in the flat [B L][C] tensor -- the neighbouring batch
    element's row"""
    B, Ln, C = x.shape
    if wrong == "halo_read":
        flat = (torch.arange(B)[:, None] * Ln + idx[None, :]) % (B * Ln)
        return x.reshape(B * Ln, C)[flat]
    ok = (idx >= 0) & (idx < Ln)
    v = x[:, idx.clamp(0, Ln - 1)] * ok[None, :, None]
    return v if pad is None else v + pad * (~ok)[None, :, None]


def conv_phase_ref(x, extras, W, bias, *, taps=1, stride=1, pad_left=0, L_out, edge_bias=None, m_split=0, k_split=0, act=L.ACT_NONE,
                   residual=None, out_C=None, ps_f=1, ps_off=0, L_y=None, y_row0=0, out_L=None, wrong=None, pad_row=None, row_scale=None,
                   tb=None, k_tail=None):
    """One GEMM phase behind its prologue.  x: [B][L_in][cmain] float64 (``prologue_ref``); extras: [(tensor [B][L_in][ce], row shift)] raw
    K segments behind the taps; W: [M][taps cmain + sum ce] in K order (tap, channel), then the extras; GEMM column t reads input row
    t stride + tap - pad_left (extras: t stride + shift), zeros outside [0, L_in).  GEMM row m = ph out_C + co lands on output row
    y_row0 + t ps_f + ph - ps_off (when that is in [0, L_y)), column co: the sub-pixel form of ConvTranspose1d.  bias: [out_C], or [M]
    beside edge_bias [2][M] that replaces it in column 0 / L_out - 1.  Rows < m_split sum only the first k_split 32-channel chunks and
    take the residual, rows >= m_split take ``act`` (m_split = 0: all rows take both).  row_scale [B][out_L] multiplies the finished
    row, after the residual.  Returns [B][out_L][out_C] float64, NaN where the phase writes nothing.
    wrong: "halo_read", "edge_swapped", "k_split_ignored", "ps_off_ignored"; "pad_before_prologue" (the rows outside [0, L_in) of the
    taps are ``pad_row`` [B][1][cmain], the prologue's image of a zero row, instead of zeros); "edge_tap_dropped" (a tap or extra segment
    is left out of a whole position tile of ``tb`` GEMM columns when it is dead for the tile's FIRST column); "k_tail_dropped" (the K
    columns ``k_tail`` are left out); "residual_after_mask" (row_scale * act(...) + residual); "gelu_tanh" (tanh GELU); "stats_with_cropped"
    (no crop: every GEMM column is kept, as [B][L_out ps_f][out_C] -- what statistics that ignore the crop would sum)."""
    B = x.shape[0]
    M = W.shape[0]
    out_C = out_C or M
    t = torch.arange(L_out)
    pad = pad_row if wrong == "pad_before_prologue" else None
    cols = [_rows_at(x, t * stride + k - pad_left, wrong, pad) for k in range(taps)]
    cols += [_rows_at(e.double(), t * stride + sh, wrong) for e, sh in extras]
    if wrong == "edge_tap_dropped":
        t0 = t // tb * tb
        shifts = [k - pad_left for k in range(taps)] + [sh for _, sh in extras]
        cols = [c_ * (t0 * stride + sh >= 0)[None, :, None] for c_, sh in zip(cols, shifts)]
    X = torch.cat(cols, -1)                                                    # [B][L_out][K]
    if wrong == "k_tail_dropped":
        X[..., k_tail] = 0.0
    W = W.double()
    y = X @ W.T
    if m_split and wrong != "k_split_ignored":
        y[..., :m_split] = X[..., : 32 * k_split] @ W[:m_split, : 32 * k_split].T
    co = torch.arange(M) % out_C
    if edge_bias is not None:
        bb = bias.double()[None, :].repeat(L_out, 1)
        first, last = (1, 0) if wrong == "edge_swapped" else (0, 1)
        bb[L_out - 1] = edge_bias.double()[last]
        bb[0] = edge_bias.double()[first]             # (the first column wins where both apply: L_out == 1 is refused by the helper)
        y = y + bb
    elif bias is not None:
        y = y + bias.double()[co]
    if act == L.ACT_GELU:
        hi = y[..., m_split:]
        hi = 0.5 * hi * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (hi + 0.044715 * hi ** 3))) if wrong == "gelu_tanh" else gelu(hi)
        y = torch.cat([y[..., :m_split], hi], -1)
    if wrong == "stats_with_cropped":
        assert residual is None and row_scale is None
        return y.reshape(B, L_out * ps_f, out_C)
    L_y = L_y if L_y is not None else L_out * ps_f
    out_L = out_L if out_L is not None else y_row0 + L_y
    out = torch.full((B, out_L, out_C), float("nan"), dtype=torch.float64)
    off = 0 if wrong == "ps_off_ignored" else ps_off
    for ph in range(ps_f):
        ty = t * ps_f + ph - off
        ok = (ty >= 0) & (ty < L_y)
        out[:, y_row0 + ty[ok]] = y[:, ok, ph * out_C: (ph + 1) * out_C]
    if row_scale is not None and wrong == "residual_after_mask":
        out = out * row_scale.double()[..., None]
    if residual is not None:
        r = residual.double()
        if m_split:
            out[..., :m_split] += r[..., :m_split]
        else:
            out = out + r
    if row_scale is not None and wrong != "residual_after_mask":
        out = out * row_scale.double()[..., None]
    return out


def entry_sums(y):
    """(sum, sumsq) of the written rows of a phase's output per batch element and 16-channel slot: [B][out_C / 16][2] float64 -- what
    a consumer forms from a long phase's per-unit partial sums"""
    return group_sums(y, y.shape[-1] // 16)


def long_part_sums(part, mblocks, out_C):
    """the sums a consumer forms from a long phase's partial array [B][8][entries][2] (include/jen1_long.h): wave s of unit e owns GEMM
    rows 128 (e % mblocks) + 16 s .. + 16, i.e. output channels (that row) % out_C -> [B][out_C / 16][2] float64"""
    B, _, ne, _ = part.shape
    out = torch.zeros(B, out_C // 16, 2, dtype=torch.float64)
    for e in range(ne):
        for s in range(8):
            out[:, ((e % mblocks) * 128 + 16 * s) % out_C // 16] += part[:, s, e].double()
    return out


def tile_part_sums(part):
    """the same from a tile phase's partial array [B][tiles][nfg][2] (include/jen1_deep.h), per statistics group of out_C / nfg channels:
    [B][nfg][2] float64"""
    return part.double().sum(1)


def group_sums(y, n):
    """(sum, sumsq) of a [B][L][C] tensor per batch element and group of C / n channels (NaN = not written): [B][n][2]"""
    B, Ln, C = y.shape
    g = torch.nan_to_num(y.double(), nan=0.0).reshape(B, Ln, n, C // n)
    return torch.stack([g.sum(dim=(1, 3)), (g * g).sum(dim=(1, 3))], -1)


def stat_rel(a, b) -> float:
    """the metric of every statistics comparison: sums and sums of squares each against their own largest reference value"""
    return max(rel(a[..., 0], b[..., 0]), rel(a[..., 1], b[..., 1]))


# ---------------------------------------------------------------------------------------------- cases
def _case(form, **kw):
    c = dict(form=form, B=2, L_in=5, L_out=None, c0=32, c1=0, M=32, out_C=None, taps=1, stride=1, pad_left=0, pro=L.PRO_NONE, groups=0,
             eps=1e-5, film=None, src1_scale=1.0, extras=(), m_split=0, k_split=0, act=L.ACT_NONE, residual=False, edge_bias=False,
             bias=True, ps_f=1, ps_off=0, L_y=None, y_row0=0, out_L=None, nb_max=0, unit_target=0, live=(), reach={}, stats=False, st=None,
             tail_gain=1.0, wrong=(), wrong_f32=())
    c.update(kw)
    c["L_out"] = c["L_out"] if c["L_out"] is not None else c["L_in"]
    c["out_C"] = c["out_C"] or c["M"] // c["ps_f"]
    c["L_y"] = c["L_y"] if c["L_y"] is not None else c["L_out"] * c["ps_f"]
    c["out_L"] = c["out_L"] if c["out_L"] is not None else c["y_row0"] + c["L_y"]
    return c


def _up(f, crop, L_in, **kw):
    """the sub-pixel form as Upsample1d sets it (engine Plan._build_unet): ConvTranspose1d(k = 2 f, stride f, padding p) as 2 taps
    over L_in + 1 GEMM columns, centre crop folded into the store"""
    p = f // 2 + f % 2
    return dict(taps=2, pad_left=1, L_in=L_in, L_out=L_in + 1, ps_f=f, ps_off=p + crop // 2, L_y=f * L_in - crop, **kw)


GN8 = dict(pro=L.PRO_GN_SILU, groups=8)
HALO, NEXT, SCALE, ROW0 = "halo_read", "stats_next_element", "scale_after_norm", "film_row0"

# name -> case.  ``reach``: the form the case is meant to reach, as fields of the restated unit geometry (``deep_conv_geometry``), per
# mode where the modes differ; ``wrong``: the mistakes the case can show
DEEP_CONV_CASES = {
    "plain":          _case("smallest unit", B=2, L_in=5, c0=32, M=16, reach=dict(nb=2, NF=1, groups_n=1, ntrips=1, Hb=0)),
    "taps3_halo":     _case("halo rows on both sides, short last batch group", B=3, L_in=7, c0=64, M=48, taps=3, pad_left=1, nb_max=2,
                            reach=dict(nb=2, groups_n=2, Hb=1, Lp=9), wrong=(HALO,)),
    "taps3_causal":   _case("causal pad: two halo rows in front, none behind", B=3, L_in=7, c0=64, M=48, taps=3, pad_left=2, nb_max=2,
                            reach=dict(nb=2, groups_n=2, Hb=2, Lp=9), wrong=(HALO,)),
    "stride2":        _case("strided down conv", B=3, L_in=24, L_out=12, c0=32, M=32, taps=4, stride=2, pad_left=1, reach=dict(Hb=1, Lp=26),
                            wrong=(HALO,)),
    "stride4":        _case("strided down conv", B=3, L_in=24, L_out=6, c0=32, M=32, taps=8, stride=4, pad_left=3, reach=dict(Hb=3, Lp=28),
                            wrong=(HALO,)),
    "gn_1group":      _case("GroupNorm, one group over both sources", B=3, c0=64, c1=64, src1_scale=2 ** -0.5, pro=L.PRO_GN, groups=1,
                            taps=3, pad_left=1, reach=dict(nb=2, lvpg=4), wrong=(HALO, NEXT), wrong_f32=(SCALE,)),
    "gn_8groups":     _case("GroupNorm + SiLU, 8 groups of 16, group boundary on the source boundary", B=3, c0=64, c1=64,
                            src1_scale=2 ** -0.5, taps=3, pad_left=1, **GN8, reach=dict(nb=2, lvpg=1), wrong=(HALO, NEXT), wrong_f32=(SCALE,)),
    "gn_16groups":    _case("GroupNorm, 16 groups of 8 (the minimum)", B=3, c0=64, c1=64, src1_scale=2 ** -0.5, pro=L.PRO_GN, groups=16,
                            taps=3, pad_left=1, reach=dict(nb=2, lvpg=0), wrong=(HALO, NEXT), wrong_f32=(SCALE,)),
    # src1_scale on the wrong side of the normalisation changes the x1 half of a group that lies inside x1 by exactly the factor
    # 2^-1/2, an error of at most 1 - 2^-1/2 = 0.29 of the largest output: below POWER x the bf16 tolerance (0.3) whatever the inputs.  The
    # cases above therefore list that mistake for float32 only, and this one repeats gn_8groups with a skip scale of 1 / 4
    "gn_scale_quarter": _case("GroupNorm + SiLU over two sources, src1_scale 1 / 4", B=3, c0=64, c1=64, src1_scale=0.25, taps=3, pad_left=1,
                            **GN8, reach=dict(nb=2, lvpg=1), wrong=(HALO, NEXT, SCALE)),
    "film_row":       _case("FiLM rows per element through film_row: nb = 1", B=4, c0=64, film="row", **GN8, reach=dict(nb=1, groups_n=4),
                            wrong=(ROW0,)),
    "film_b":         _case("FiLM row = batch element: nb = 1", B=4, c0=64, film="b", **GN8, reach=dict(nb=1, groups_n=4), wrong=(ROW0,)),
    "film_step":      _case("one FiLM row through the device scalar: nb stays > 1", B=4, c0=64, film="step", **GN8,
                            reach=dict(nb=4, groups_n=1), wrong=(NEXT, "step_ignored")),
    # the issue's 32 + 64 raw channels are refused behind a normalised source ("vectors per row must be a power of two": 96 / 8 = 12);
    # 32 + 96 = 128 keeps two segments of different width
    "extra_segs":     _case("fused shortcut: raw extra K segments at shifts 0 and -1 behind 3 normalised taps", B=2, c0=64, taps=3,
                            pad_left=1, extras=((32, 0), (96, -1)), **GN8, reach=dict(Hb=1, lvr=4), wrong=(HALO, NEXT)),
    "dual_range":     _case("dual range: residual on the low rows, GELU on the high rows", B=2, c0=64, extras=((64, 0),), M=64, m_split=32,
                            k_split=2, act=L.ACT_GELU, residual=True, wrong=("k_split_ignored",)),
    "edge_bias":      _case("edge bias", B=2, L_in=5, c0=32, taps=3, pad_left=1, M=32, edge_bias=True, wrong=(HALO, "edge_swapped")),
    "edge_bias_L2":   _case("edge bias, first and last column adjacent", B=3, L_in=2, c0=32, taps=3, pad_left=1, M=32, edge_bias=True,
                            wrong=(HALO, "edge_swapped")),
    "subpixel2":      _case("sub-pixel output mapping, factor 2", B=2, c0=32, M=64, **_up(2, 0, 5), wrong=(HALO, "ps_off_ignored")),
    "subpixel4_crop": _case("sub-pixel output mapping, factor 4, cropped last row, output window inside a longer tensor", B=3, c0=32, M=64,
                            y_row0=2, out_L=20, **_up(4, 3, 5), wrong=(HALO, "ps_off_ignored")),
    "subpixel2_edge": _case("sub-pixel mapping with the edge bias of the folded up conv and a residual", B=2, c0=32, M=64, edge_bias=True,
                            residual=True, **_up(2, 1, 6), wrong=(HALO, "edge_swapped", "ps_off_ignored")),
    "residual_live":  _case("residual and source produced by the phases in front: live_mask bits 0 and 8", B=3, c0=64, M=32, taps=3,
                            pad_left=1, residual=True, live=("x0", "residual"), **GN8, reach=dict(live_mask=257), wrong=(HALO, NEXT)),
    "nf4":            _case("four 16-column fragments", B=4, L_in=16, c0=32, M=16, reach=dict(nb=4, NF=4)),
    "nf3":            _case("three fragments, the last ragged, short last batch group", B=3, L_in=20, c0=32, M=16,
                            reach=dict(nb=2, NF=3, groups_n=2)),
    "nf_ragged":      _case("one ragged column fragment", B=1, L_in=17, c0=32, M=16, reach=dict(nb=1, NF=2)),
    # (32 positions, not the 36 of the helper's comment: two batch elements are then 64 columns, which lets bf16 keep nb = 2 in 3 trips)
    "long_rows":      _case("staging in several trips", B=2, L_in=32, c0=512, M=16, taps=3, pad_left=1, pro=L.PRO_GN_SILU, groups=32,
                            reach=dict(f32=dict(nb=1, ntrips=2), bf16=dict(nb=2, ntrips=3)), wrong=(HALO,)),
    "unit_target":    _case("the Engine's default unit target picks nb", B=4, L_in=3, c0=32, M=1024, unit_target=DEEP_UNIT_TARGET,
                            reach=dict(nb=2, groups_n=2, n_units=128)),
    "mrep2":          _case("a unit finishes 2 M tiles", B=8, L_in=1, c0=32, M=1024, nb_max=1, reach=dict(nb=1, mrep=2, n_units=256)),
    "mrep4":          _case("a unit finishes 4 M tiles", B=8, L_in=1, c0=32, M=2048, nb_max=1, reach=dict(nb=1, mrep=4, n_units=256)),
    "mrep8":          _case("a unit finishes 8 M tiles", B=16, L_in=1, c0=32, M=2048, nb_max=1, reach=dict(nb=1, mrep=8, n_units=256)),
}

FILM_ROWS, FILM_OFF = 6, 8
FILM_STEPS = (5, 1)                  # the device scalar's two values: neither is an entry of film_row
FILM_ROW = (4, 0, 2, 3, 1, 5, 0, 2)


def conv_inputs(name, c):
    """float32 operands of one conv case, from a generator seeded by the case name.  Activations have a non-zero mean and differ in
    mean and spread from one batch element to the next, so that statistics taken over the wrong rows show; x1 is wide, so that
    src1_scale on the wrong side of the normalisation shows."""
    g = _gen("persistent", name)
    r = lambda *s: torch.randn(*s, generator=g)
    B, Li, cm = c["B"], c["L_in"], c["c0"] + c["c1"]
    # (behind a GroupNorm the outputs of all batch elements are alike whatever the inputs' scale, so the contrast can be strong there: a
    # factor 4 from one element to the next; raw inputs keep to a factor 1.5, or the quiet elements would hide under the loud ones)
    amp = 4.0 ** (torch.arange(B) % 3).float() if c["groups"] else 1.0 + 0.5 * (torch.arange(B) % 2).float()
    elem = lambda: amp[:, None, None]
    t = dict(x0=(r(B, Li, c["c0"]) + 0.5) * elem())
    if c["tail_gain"] != 1.0:
        # the positions of the ragged last tile are few (less than one tile in 32): louder, so that leaving them out of the sums shows
        _, _, tb = long_geometry(c["M"], c["L_out"], NWG // B)
        t["x0"][:, c["L_out"] // tb * tb:] *= c["tail_gain"]
    if c["c1"]:
        t["x1"] = (r(B, Li, c["c1"]) * 3.0 - 0.7) * elem()
    for i, (ce, _) in enumerate(c["extras"]):
        t[f"e{i}"] = r(B, Li, ce) + 0.3
    K = c["taps"] * cm + sum(ce for ce, _ in c["extras"])
    t["W"] = r(c["M"], K) / K ** 0.5
    if c["m_split"]:
        t["W"][: c["m_split"], 32 * c["k_split"]:] *= 3.0          # the block the low rows must skip
    if c["bias"]:
        t["bias"] = r(c["M"] if c["edge_bias"] else c["out_C"]) * 0.5
    if c["edge_bias"]:
        t["edge_bias"] = torch.stack([t["bias"] + 2.0 + r(c["M"]) * 0.3, t["bias"] - 2.0 + r(c["M"]) * 0.3])
    if c["residual"]:
        t["residual"] = r(B, c["out_L"], c["m_split"] or c["out_C"]) * 0.25
    if c["groups"]:
        t["gamma"], t["beta"] = torch.rand(cm, generator=g) + 0.5, r(cm) * 0.3 + 0.4
        if c["film"]:
            tab = r(FILM_ROWS, 2 * cm + FILM_OFF + 3)
            tab[:, FILM_OFF: FILM_OFF + cm] = tab[:, FILM_OFF: FILM_OFF + cm] * 0.5 + 1.0 + 0.4 * torch.arange(FILM_ROWS).float()[:, None]
            t["film2"] = tab
            t["film_row"] = torch.tensor(FILM_ROW[:B], dtype=torch.int32) if c["film"] in ("row", "step") else None
    for k in c["live"]:
        # the operand comes out of a 1x1 conv phase in front: z [B][rows][32] -> W_f z + b_f, in place of the tensor drawn above
        shape = t[k].shape
        t["z." + k] = (r(shape[0], shape[1], 32) + 0.5) * (elem() if k != "residual" else 1.0)
        t["wf." + k], t["bf." + k] = r(shape[2], 32) / 32 ** 0.5, r(shape[2]) * 0.3
    return t


def front_ref(t, k, mode):
    """what the 1x1 conv phase in front of a live operand leaves in memory: rounded to the launch dtype, float64"""
    y = rounded(t["z." + k], mode) @ rounded(t["wf." + k], mode).T + t["bf." + k].double()
    return rounded(y.to(TDTYPE[mode]), mode)


def conv_ref(c, t, mode, step=None, wrong=None):
    """[B][out_L][out_C] float64 reference of a conv case on operands rounded to ``mode`` (tables and vectors stay float32); step: the
    value of the film_step scalar of a ``film == "step"`` case"""
    op = lambda k: None if k not in t or t[k] is None else (front_ref(t, k, mode) if k in c["live"] else rounded(t[k], mode))
    rows = None
    if c["film"]:
        B = c["B"]
        by_step = c["film"] == "step" and wrong != "step_ignored"
        rows = torch.full((B,), int(step)) if by_step else (torch.arange(B) if c["film"] == "b" else t["film_row"])
        cm = c["c0"] + c["c1"]
        p1, p2 = t["film2"][:, FILM_OFF: FILM_OFF + cm], t["film2"][:, FILM_OFF + cm: FILM_OFF + 2 * cm]
    else:
        p1, p2 = t.get("gamma"), t.get("beta")
    x = prologue_ref(op("x0"), op("x1"), src1_scale=c["src1_scale"], groups=c["groups"], eps=c["eps"], p1=p1, p2=p2, rows=rows,
                     silu=c["pro"] == L.PRO_GN_SILU, wrong=wrong)
    extras = [(op(f"e{i}"), sh) for i, (_, sh) in enumerate(c["extras"])]
    return conv_phase_ref(x, extras, rounded(t["W"], mode), t.get("bias"), taps=c["taps"], stride=c["stride"], pad_left=c["pad_left"],
                          L_out=c["L_out"], edge_bias=t.get("edge_bias"), m_split=c["m_split"], k_split=c["k_split"], act=c["act"],
                          residual=op("residual"), out_C=c["out_C"], ps_f=c["ps_f"], ps_off=c["ps_off"], L_y=c["L_y"], y_row0=c["y_row0"],
                          out_L=c["out_L"], wrong=wrong)


def written_rel(y, ref) -> float:
    """``rel`` over the elements the phase writes (the reference is NaN elsewhere)"""
    m = ~torch.isnan(ref)
    return rel(y.double()[m], ref[m])


# ---------------------------------------------------------------------------------------------- restated unit geometry
MAXV, MAX_TRIPS, THREADS = 3, 4, 512
LDS_BUDGET = 160 * 1024 - (256 * 16 + 2 * 4096 + 16 + 64)        # LDS_TOTAL - WS_OFF of csrc/deep_kernel.hip


def deep_nb_cap(c, mode):
    """OpBuilder._deep_nb_cap: the cap on the batch elements per unit the recorder hands to jen1_deep_phase_conv.  The Engine's default
    (deep_unit_target = 128 units per phase) makes every small layer nb = 1, so the cases run with ``unit_target`` = 0 ("as many as fit":
    the helper's own rule decides) and ``nb_max`` as deep_nb_max, except the one case that states the Engine's target"""
    es = 4 if mode == "f32" else 2
    cm = c["c0"] + c["c1"]
    cap = c["nb_max"] or DEEP_NB_MAX
    if c["unit_target"] > 0:
        wbytes = (c["taps"] * cm + sum(ce for ce, _ in c["extras"])) * c["M"] * es
        nb, B = 1, c["B"]
        while nb < B and ((c["M"] // 16) * ceil_div(B, nb) > c["unit_target"] or ceil_div(B, nb) * wbytes > DEEP_REREAD_CAP):
            nb *= 2
        cap = nb if cap == 0 else min(cap, nb)
    return cap


def deep_conv_geometry(c, mode, nb_max=None, nwg=NWG):
    """what jen1_deep_phase_conv derives for a case (nb, NF, groups_n, ntrips, Lp, Hb, lvpg, lvr, n_units, lds_bytes) and what
    jen1_deep_link makes of it on ``nwg`` workgroups (mrep, n_units); None when the helper refuses the layer"""
    es = 4 if mode == "f32" else 2
    B, Li, Lo, cm = c["B"], c["L_in"], c["L_out"], c["c0"] + c["c1"]
    nb_max = deep_nb_cap(c, mode) if nb_max is None else nb_max
    coff = cm + sum(ce for ce, _ in c["extras"])
    norm_C = cm if c["groups"] else 0
    vr = (coff - norm_C) // 8
    if vr & (vr - 1) or vr > THREADS:
        return None
    shifts = [k - c["pad_left"] for k in range(c["taps"])] + [sh for _, sh in c["extras"]]
    Hb = -min(0, min(shifts))
    Ha = max(0, (Lo - 1) * c["stride"] + max(0, max(shifts)) - (Li - 1))
    Lp = Hb + Li + Ha
    lvpg = 0
    if norm_C:
        cpg = cm // c["groups"]
        vpg = cpg // 8
        if cpg % 8 or vpg & (vpg - 1) or c["groups"] & (c["groups"] - 1) or vpg > 128:
            return None
        lvpg = int(math.log2(vpg))
    nb0 = 1
    while nb0 * 2 <= B:
        nb0 *= 2
    if nb_max > 0:
        while nb0 > nb_max:
            nb0 //= 2
    if c["film"] in ("row", "b"):
        nb0 = 1
    max_trips, nb = 1, nb0
    while True:
        if nb < 1 and max_trips == 1:
            max_trips, nb = MAX_TRIPS, nb0
        if nb < 1:
            return None
        NF = ceil_div(nb * Lo, 16)
        ok, ntrips = NF <= 4, 1
        if ok and norm_C:
            pairs = nb * c["groups"]
            ok = pairs <= THREADS // 2
            if ok:
                S = min(THREADS // pairs, 128 if (1 << lvpg) > 64 else 64)
                per_lane = ceil_div(Li << lvpg, S)
                ok = (1 << lvpg) <= S and per_lane <= MAXV * max_trips
                ntrips = ceil_div(per_lane, MAXV)
        if ok:
            Rtot = nb * Lp + (Hb + Ha + 1)
            tile_b = ceil_to(Rtot * (coff + 8) * es, 16)
            red_b = max((THREADS // 64) * NF * 1024, THREADS * 8 * es)
            ok = tile_b + red_b <= LDS_BUDGET
        if ok:
            break
        nb //= 2
    MT, groups_n = c["M"] // 16, ceil_div(B, nb)
    mrep, mts = 1, c["m_split"] // 16
    while mrep < 8 and (MT // mrep) * groups_n > nwg and MT % (2 * mrep) == 0 and mts % (2 * mrep) == 0:
        mrep *= 2
    if mrep > 1 and tile_b + 2 * red_b > LDS_BUDGET:
        mrep = 1
    live = sum(1 << i for i, k in enumerate(["x0"] + ["x1"] * bool(c["c1"]) + [f"e{i}" for i in range(len(c["extras"]))]) if k in c["live"])
    return dict(nb=nb, NF=NF, groups_n=groups_n, ntrips=ntrips, Lp=Lp, Hb=Hb, lvpg=lvpg, lvr=int(math.log2(vr)) if vr else 0, mrep=mrep,
                n_units_unlinked=MT * groups_n, n_units=(MT // mrep) * groups_n, lds_bytes=tile_b + red_b * (2 if mrep > 1 else 1),
                live_mask=live | (256 if "residual" in c["live"] else 0))


def case_reach(c, mode):
    r = dict(c["reach"])
    per_mode = r.pop(mode, None)
    for m in MODES:
        r.pop(m, None)
    r.update(per_mode or {})
    return r


# ====================================================================================================== attention phase
QCHUNK = 32


def attn_geometry(d, Nq, Nk, mode, *, self_attn, finish_kv):
    """what jen1_deep_phase_attention derives: (nqc, vsep, lds_bytes), or None when it refuses the shape"""
    es = 4 if mode == "f32" else 2
    if d not in (8, 16, 32, 64, 128) or Nk > 192 or Nk * (d // 8) > ceil_to(141 * 16, THREADS):
        return None
    if self_attn and Nk * (d // 8) > 2 * THREADS:
        return None
    if finish_kv and not (self_attn and Nk * (d // 8) <= THREADS and Nq == Nk):
        return None
    DP, DC = max(d, 32), max(d, 16)
    NKP = ceil_to(Nk, 32)
    dq, vt, sp = DP + 8, NKP + 8, NKP + 4
    st_rows = max(Nk, QCHUNK)

    def lds_of(vsep):
        kv = ceil_to(NKP * dq, 16) + DC * vt if vsep else max(NKP * dq, DC * vt)
        return es * QCHUNK * dq + es * ceil_to(kv, 16) + 4 * ceil_to(QCHUNK * sp, 4) + es * ceil_to(QCHUNK * vt, 8) + 8 * st_rows + 64
    vsep = lds_of(True) <= LDS_BUDGET
    if lds_of(vsep) > LDS_BUDGET:
        return None
    return dict(nqc=ceil_div(Nq, QCHUNK), vsep=int(vsep), lds_bytes=ceil_to(lds_of(vsep), 16))


ATTN_D = (8, 32, 64, 128)
# (kind, Nq, Nk, causal): 129 keys are four 32-key tiles and one key, so the tail of the last tile is masked; self = K / V live from the projection phase in front, finish of Q, K and V; cross = cached K / V rows picked by
# kv_row (shared by batch elements), finish of Q alone; cross_row / cross_step = the last key from kv_extra through extra_row / extra_step
ATTN_SHAPES = (("self", 1, 1, False), ("self", 7, 7, True), ("self", 24, 24, False), ("self", 33, 33, False), ("cross", 12, 129, False),
               ("cross_row", 5, 129, False), ("cross_step", 5, 129, False))
ATTN_STEPS = (5, 1)                  # the device scalar's two values: neither is an entry of extra_row


def _attn_cases():
    out = {}
    for i, d in enumerate(ATTN_D):
        for j, (kind, Nq, Nk, causal) in enumerate(ATTN_SHAPES):
            H = 3 if (i + j) % 2 else 1
            # (33, 33) at d = 128 is 528 K vectors: the K / V finish takes at most 512, so the model never builds it -- left out
            if attn_geometry(d, Nq, Nk, "f32", self_attn=kind == "self", finish_kv=kind == "self") is None:
                continue
            out[f"{kind}_d{d}_q{Nq}_k{Nk}_h{H}"] = dict(kind=kind, d=d, Nq=Nq, Nk=Nk, H=H, causal=causal, B=3 if kind == "self" else 5, Cc=32)
    return out


ATTN_CASES = _attn_cases()


def attn_inputs(name, c):
    """float32 operands of one attention case.  self: z [B][N][32] and the projection W_f [ld][32], b_f of the phase in front, whose
    output is [x | q_raw | k_raw | v_raw] (ld = Cc + 3 mid padded to 32); cross: that tensor's first Cc + mid columns given directly.
    x is wide (std 3), so that a finish that should not happen -- a factor rstd of about 1 / 3 -- is far outside the tolerance; u and b
    differ from Q's to V's columns."""
    g = _gen("persistent.attn", name)
    r = lambda *s: torch.randn(*s, generator=g)
    B, H, d, Nq, Nk, Cc = c["B"], c["H"], c["d"], c["Nq"], c["Nk"], c["Cc"]
    mid = H * d
    t = {}
    if c["kind"] == "self":
        ld = ceil_to(Cc + 3 * mid, 32)
        t["z"] = r(B, Nq, 32)
        wf, bf = r(ld, 32) / 32 ** 0.5, r(ld) * 0.3
        wf[:Cc] *= 3.0
        bf[:Cc] += 0.5
        t["wf"], t["bf"] = wf, bf
    else:
        ld = ceil_to(Cc + mid, 32)
        q = r(B, Nq, ld)
        q[:, :, :Cc] = q[:, :, :Cc] * 3.0 + 0.5
        q[:, :, Cc:] *= 3.0            # (the finish divides by about 3: finished queries of std 1 that differ from one another)
        t["q"] = q
        t["kv"] = r(2 * B, Nk, 2 * mid)
        t["kv_row"] = torch.tensor([4, 0, 4, 9, 2], dtype=torch.int32)      # elements 0 and 2 share a context row
        if c["kind"] != "cross":
            t["ld_extra"], t["kx_off"], t["vx_off"] = 2 * mid + 16, 8, 8 + mid
            # the extra row is loud (std 10 against 1): as a key it carries most of some query's softmax weight, and as a value it shows
            # even at the weight 1 / 129 of an ordinary key
            t["kv_extra"] = r(6, t["ld_extra"]) * 10.0
            t["extra_row"] = torch.tensor([-1, 2, 4, 0, 3], dtype=torch.int32)
    t["ld"] = ld
    t["u"] = torch.cat([torch.zeros(Cc), r(ld - Cc) * 0.7])
    t["b"] = torch.cat([torch.zeros(Cc), r(ld - Cc) * 0.3])
    return t


def attn_qkv(c, t, mode):
    """self-attention: the projection phase's output as it lies in memory, float64"""
    y = rounded(t["z"], mode) @ rounded(t["wf"], mode).T + t["bf"].double()
    return rounded(y.to(TDTYPE[mode]), mode)


ATTN_WRONG = ("causal_off_by_one", "extra_left_out", "finish_v_with_q_columns")


def attn_wrong_kinds(c):
    return ["causal_off_by_one"] * c["causal"] + ["extra_left_out"] * (c["kind"] in ("cross_row", "cross_step")) + \
           ["finish_v_with_q_columns"] * (c["kind"] == "self")


def attn_ref(c, t, mode, step=None, wrong=None):
    """[B][Nq][H d] float64.  The LayerNorm statistics are the consumer's own: row sums over the first Cc columns of q's tensor as it
    lies in memory.  step: the extra_step scalar of a cross_step case"""
    H, d, Nq, Nk, Cc = c["H"], c["d"], c["Nq"], c["Nk"], c["Cc"]
    mid = H * d
    if c["kind"] == "self":
        q = kv = attn_qkv(c, t, mode)
        kw = dict(k_off=Cc + mid, v_off=Cc + 2 * mid)
        fkv = 1
    else:
        q, kv = rounded(t["q"], mode), rounded(t["kv"], mode)
        kw = dict(k_off=0, v_off=mid, kv_row=t["kv_row"])
        fkv = 0
        if c["kind"] != "cross" and wrong != "extra_left_out":
            kw.update(kv_extra=rounded(t["kv_extra"], mode), extra_row=t["extra_row"], kx_off=t["kx_off"], vx_off=t["vx_off"],
                      extra_step=step if c["kind"] == "cross_step" else None)
    u, b = t["u"], t["b"]
    if wrong == "finish_v_with_q_columns":
        u, b = u.clone(), b.clone()
        u[Cc + 2 * mid: Cc + 3 * mid], b[Cc + 2 * mid: Cc + 3 * mid] = u[Cc: Cc + mid], b[Cc: Cc + mid]
    causal = c["causal"]
    if wrong == "causal_off_by_one":
        return _attn_causal_shifted(c, q, kv, u, b, kw)
    return attention_ref(q, kv, q_off=Cc, H=H, d=d, Nk=Nk, causal=causal, fin=(row_sums(q, Cc), u, b, Cc, 1e-5, 1, fkv), **kw)


def _attn_causal_shifted(c, q, kv, u, b, kw):
    """the causal mask one key short: query n sees keys < n (its own key only for n = 0) -- attention_ref has no such knob, so the mask
    is applied here on the finished heads it would form"""
    from transformer_forms_common import ln_finish
    H, d, Nq, Cc = c["H"], c["d"], c["Nq"], c["Cc"]
    mid = H * d
    B = q.shape[0]
    st = row_sums(q, Cc)
    fin = lambda off: ln_finish(q[..., off: off + mid], st, u[off: off + mid], b[off: off + mid], Cc, 1e-5)
    h = lambda x: x.reshape(B, -1, H, d).transpose(1, 2)
    qh, kh, vh = h(fin(Cc)), h(fin(kw["k_off"])), h(fin(kw["v_off"]))
    sim = torch.einsum("bhnd,bhmd->bhnm", qh, kh) * d ** -0.5
    mask = torch.ones(Nq, Nq, dtype=torch.bool).triu(0)
    mask[0, 0] = False
    out = torch.einsum("bhnm,bhmd->bhnd", sim.masked_fill(mask, -torch.finfo(sim.dtype).max).softmax(-1), vh)
    return out.transpose(1, 2).reshape(B, Nq, mid)


# ====================================================================================================== stats phase
STATS_CASES = {f"ld{ld}_L{Ln}": dict(ld=ld, L=Ln, B=3) for ld in (32, 256, 1024) for Ln in (1, 24)}


def stats_inputs(name, c):
    """the 1x1 conv phase in front of the stats phase: z [B][L][32], W_f [ld][32], b_f"""
    g = _gen("persistent.stats", name)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(z=r(c["B"], c["L"], 32) + 0.5, wf=r(c["ld"], 32) / 32 ** 0.5, bf=r(c["ld"]) * 0.3 + 0.5)


def stats_ref(c, t, mode):
    """fine-group sums [B][32][2] float64 of the tensor in front as it lies in memory"""
    return fine_group_sums(rounded((rounded(t["z"], mode) @ rounded(t["wf"], mode).T + t["bf"].double()).to(TDTYPE[mode]), mode))


# ====================================================================================================== long phases
def long_geometry(M, L_out, G):
    """jen1_long_geometry: (mblocks, tiles, tb), or None when refused"""
    if M < 128 or M % 128 or M // 128 > G:
        return None
    mb = M // 128
    tiles = G // mb
    tb = ceil_div(L_out, tiles)
    return None if tb > 96 else (mb, tiles, tb)


TAIL = "tail_dropped"
LGN = dict(pro=L.PRO_GN_SILU, groups=8)
# ``st``: where the GroupNorm statistics of the normalised sources come from -- "totals" ([B][32][2], written before the launch) or
# "live" (partials written by the 1x1 conv phase in front, which also produces the source); ``stats``: the phase writes partials of
# its own output, compared as sums per sample and 16-channel slot.  G = 256 / B workgroups per sample: 32 at B = 8, 85 at B = 3.
LONG_CASES = {
    "full_tiles":      _case("M 128: 32 full tiles of 16", B=8, L_in=512, c0=128, M=128, taps=3, pad_left=1, stats=True,
                             reach=dict(mblocks=1, tb=16, ragged=False), wrong=(HALO,)),
    "ragged_tile":     _case("ragged last tile; GroupNorm from totals, two sources, raw extra segment", B=8, L_in=500, c0=64, c1=64,
                             src1_scale=2 ** -0.5, M=128, taps=3, pad_left=1, extras=((32, 0),), st="totals", stats=True, tail_gain=6.0,
                             **LGN,
                             reach=dict(mblocks=1, tb=16, ragged=True), wrong=(HALO, NEXT, TAIL), wrong_f32=(SCALE,)),
    "short_tiles":     _case("tiles of fewer than 16 positions, M 256, one GroupNorm group from totals", B=8, L_in=100, c0=128, M=256,
                             taps=3, pad_left=1, pro=L.PRO_GN, groups=1, st="totals", stats=True,
                             reach=dict(mblocks=2, tb=7, ragged=True), wrong=(HALO, NEXT)),
    "b3_live":         _case("B = 3; both sources and their partials live", B=3, L_in=100, c0=128, c1=128, src1_scale=2 ** -0.5, M=256,
                             taps=3, pad_left=1, st="live", live=("x0", "x1"), stats=True, **LGN,
                             reach=dict(mblocks=2, tb=3, ragged=True), wrong=(HALO, NEXT), wrong_f32=(SCALE,)),
    "down2":           _case("stride 2 down conv, M 512", B=8, L_in=200, L_out=100, c0=128, M=512, taps=4, stride=2, pad_left=1,
                             reach=dict(mblocks=4, tb=13), wrong=(HALO,)),
    "down4":           _case("stride 4 down conv", B=3, L_in=200, L_out=50, c0=128, M=256, taps=8, stride=4, pad_left=3, stats=True,
                             reach=dict(mblocks=2, tb=2), wrong=(HALO,)),
    "up2":             _case("sub-pixel up conv, factor 2, residual live", B=8, c0=128, M=256, residual=True, live=("residual",), stats=True,
                             **_up(2, 1, 60), reach=dict(mblocks=2, tb=4), wrong=(HALO, "ps_off_ignored")),
    "up4":             _case("sub-pixel up conv, factor 4, M 512", B=3, c0=128, M=512, **_up(4, 2, 40), reach=dict(mblocks=4, tb=2),
                             wrong=(HALO, "ps_off_ignored")),
    "film_row":        _case("FiLM table by row, statistics live", B=8, L_in=64, c0=128, M=128, taps=3, pad_left=1, film="row", st="live",
                             live=("x0",), **LGN, reach=dict(mblocks=1, tb=2), wrong=(HALO, NEXT, ROW0)),
    "film_step":       _case("FiLM table by step, statistics from totals", B=8, L_in=64, c0=128, M=128, taps=3, pad_left=1, film="step",
                             st="totals", **LGN, reach=dict(mblocks=1, tb=2), wrong=(HALO, NEXT, "step_ignored")),
    "raw_two_src":     _case("no GroupNorm, scaled second source", B=8, L_in=32, c0=64, c1=64, src1_scale=0.25, M=128, taps=3, pad_left=1,
                             wrong=(HALO,)),
}


def long_reach(c):
    mb, tiles, tb = long_geometry(c["M"], c["L_out"], NWG // c["B"])
    return dict(mblocks=mb, tb=tb, ragged=c["L_out"] % tb != 0 or ceil_div(c["L_out"], tb) < tiles)


def part_stats_ref(c, t, mode, tb, n, step=None, wrong=None):
    """sums of the phase's own output per sample and group of out_C / n channels [B][n][2].  wrong "tail_dropped": the ragged last
    position tile (``tb`` GEMM columns per tile) is left out"""
    y = conv_ref(c, t, mode, step=step)
    if wrong == TAIL and c["L_out"] % tb:
        # a position tile covers tb GEMM columns = tb ps_f output rows before the crop
        y = y[:, : c["y_row0"] + c["L_out"] // tb * tb * c["ps_f"] - c["ps_off"]]
    return group_sums(y, n)


# ====================================================================================================== tile phases
# through OpBuilder._conv_tile (``tile_lens`` holds the case's input length): bm = 256 when M % 256 == 0 else 128; tb is the smallest of
# (16, 32, 48, 64) -- (16, 32) at bm = 256 -- that needs the fewest rounds of the 256 workgroups
def tile_geometry(c, nwg=NWG):
    bm = 256 if c["M"] % 256 == 0 else 128
    rounds = lambda tb: ceil_div((c["M"] // bm) * c["B"] * ceil_div(c["L_out"], tb), nwg)
    tb = min((16, 32, 48, 64) if bm == 128 else (16, 32), key=rounds)
    return dict(bm=bm, tb=tb, tiles=ceil_div(c["L_out"], tb), tail=c["L_out"] % tb != 0)


TILE_CASES = {
    "tb16_bm128":   _case("tb 16, bm 128, tail tile, totals", B=2, L_in=40, c0=64, M=128, taps=3, pad_left=1, st="totals", stats=True, **LGN,
                          reach=dict(tb=16, bm=128, tail=True), wrong=(HALO, NEXT, TAIL)),
    "tb64_bm128":   _case("tb 64, bm 128, tail tile, live partials", B=8, L_in=2000, c0=128, M=128, taps=3, pad_left=1, st="live",
                          live=("x0",), stats=True, **LGN, reach=dict(tb=64, bm=128, tail=True), wrong=(HALO, NEXT)),
    "tb16_bm256":   _case("tb 16, bm 256, strided", B=2, L_in=80, L_out=40, c0=64, M=256, taps=4, stride=2, pad_left=1,
                          reach=dict(tb=16, bm=256, tail=True), wrong=(HALO,)),
    "bm256_up2":    _case("bm 256, sub-pixel", B=2, c0=64, M=256, **_up(2, 1, 30), reach=dict(bm=256, tail=True),
                          wrong=(HALO, "ps_off_ignored")),
    "gn_two_src":   _case("GroupNorm + SiLU over two sources, groups inside the scaled second source", B=2, L_in=16, c0=64, c1=64,
                          src1_scale=0.25, M=128, taps=3, pad_left=1, st="totals", **LGN, wrong=(HALO, NEXT), wrong_f32=(SCALE,)),
    "raw_two_src":  _case("no GroupNorm, scaled second source", B=2, L_in=16, c0=64, c1=64, src1_scale=0.25, M=128, taps=3, pad_left=1,
                          wrong=(HALO,)),
}


# ====================================================================================================== form coverage
# every value of each form parameter the issue names, as the restated geometry computes it: the host test requires that the cases reach
# each of them
FORMS = {
    "deep.nb": (1, 2, 4), "deep.NF": (1, 2, 3, 4), "deep.short_last_group": (True,), "deep.ntrips": (1, 2, 3), "deep.mrep": (1, 2, 4, 8),
    "deep.Hb": (0, 1, 2, 3), "deep.lvpg": (0, 1, 4), "deep.film": ("row", "b", "step"), "deep.extras": (True,), "deep.dual": (True,),
    "deep.edge": (True,), "deep.ps_f": (1, 2, 4), "deep.live_mask": (0, 257),
    "attn.d": ATTN_D, "attn.nqc": (1, 2), "attn.vsep": (0, 1), "attn.H": (1, 3), "attn.kind": ("self", "cross", "cross_row", "cross_step"),
    "attn.causal": (False, True),
    "stats.ld": (32, 256, 1024), "stats.L": (1, 24),
    "long.mblocks": (1, 2, 4), "long.ragged": (False, True), "long.short_tile": (True,), "long.B": (3, 8), "long.M": (128, 256, 512),
    "long.stride": (1, 2, 4), "long.ps_f": (1, 2, 4), "long.st": (None, "totals", "live"), "long.groups": (0, 1, 8),
    "long.film": (None, "row", "step"), "long.residual_live": (True,), "long.extras": (True,),
    "tile.tb": (16, 64), "tile.bm": (128, 256), "tile.tail": (True,), "tile.st": ("totals", "live"), "tile.stride": (1, 2), "tile.ps_f": (1, 2),
}


def forms_reached():
    """{form parameter: the set of values the case tables reach}, by the restated geometry"""
    got = {k: set() for k in FORMS}

    def put(prefix, **kv):
        for k, v in kv.items():
            got[f"{prefix}.{k}"].add(v)

    for c in DEEP_CONV_CASES.values():
        for mode in MODES:
            g = deep_conv_geometry(c, mode)
            put("deep", nb=g["nb"], NF=g["NF"], ntrips=g["ntrips"], mrep=g["mrep"], Hb=g["Hb"], live_mask=g["live_mask"],
                short_last_group=g["nb"] > 1 and c["B"] % g["nb"] != 0)
            if c["groups"]:
                put("deep", lvpg=g["lvpg"])
        put("deep", film=c["film"], extras=bool(c["extras"]), dual=bool(c["m_split"]), edge=c["edge_bias"], ps_f=c["ps_f"])
    for c in ATTN_CASES.values():
        for mode in MODES:
            g = attn_geometry(c["d"], c["Nq"], c["Nk"], mode, self_attn=c["kind"] == "self", finish_kv=c["kind"] == "self")
            put("attn", nqc=g["nqc"], vsep=g["vsep"])
        put("attn", d=c["d"], H=c["H"], kind=c["kind"], causal=c["causal"])
    for c in STATS_CASES.values():
        put("stats", ld=c["ld"], L=c["L"])
    for c in LONG_CASES.values():
        r = long_reach(c)
        put("long", mblocks=r["mblocks"], ragged=r["ragged"], short_tile=r["tb"] < 16, B=c["B"], M=c["M"], stride=c["stride"], ps_f=c["ps_f"],
            st=c["st"], groups=c["groups"], film=c["film"], residual_live="residual" in c["live"], extras=bool(c["extras"]))
    for c in TILE_CASES.values():
        g = tile_geometry(c)
        put("tile", tb=g["tb"], bm=g["bm"], tail=g["tail"], st=c["st"], stride=c["stride"], ps_f=c["ps_f"])
    return got
