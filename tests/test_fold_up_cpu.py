"""The up-path fold of the persistent launch on the host (jen1_amd/packing.py: ff_out_matrix, fold_linear_into_upsample).

On the up path the transformer's output 1x1 conv feeds nothing but the level's ConvTranspose1d (reference blocks.py:754-758), so
the two linear maps run as ONE 2-tap sub-pixel GEMM whose bias differs in the first and the last GEMM column of a sample.  Here
the folded form -- evaluated column by column exactly as the GEMM unit evaluates it: zero halo rows, per-column bias, sub-pixel
scatter with the crop offset -- is compared in float64 with conv_transpose1d(conv1d(z)) at every output position.
"""
import pytest
import torch

from jen1_amd.packing import convT_weight_to_gemm, ff_out_matrix, fold_linear_into_upsample

C_, F_, CO = 32, 32, 16


def make_case(f, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    k, p = 2 * f, f // 2 + f % 2
    return dict(f=f, k=k, p=p, w_up=r(C_, CO, k) * 0.2, b_up=r(CO), wm=r(C_, C_ + F_) * 0.2, b_m=r(C_) + 0.5)


def reference(c, z, diff):
    """conv_transpose1d(conv1d(z)) cropped by ``diff`` positions the way the up path crops against the next level's skip
    (diff // 2 from the front, the rest from the back)"""
    y = torch.nn.functional.conv1d(z, c["wm"][:, :, None], c["b_m"])
    o = torch.nn.functional.conv_transpose1d(y, c["w_up"], c["b_up"], stride=c["f"], padding=c["p"])
    L_y = c["f"] * z.shape[-1] - diff
    return o[:, :, diff // 2: diff // 2 + L_y]


def subpixel(c, z, diff, wf, b_mid, b_first, b_last):
    """the folded conv as the GEMM unit runs it: column q in [0, L] = Wf[0] z[q-1] + Wf[1] z[q] + bias(q) with zero halo rows; row
    m = r * C_out + co of column q is output position q * f + r - ps_off, ps_off = p + diff // 2, kept when inside [0, L_y)"""
    f, p = c["f"], c["p"]
    B, _, L = z.shape
    L_y, ps_off = f * L - diff, p + diff // 2
    zp = torch.nn.functional.pad(z, (1, 1))
    out = torch.full((B, CO, L_y), float("nan"), dtype=torch.float64)
    for q in range(L + 1):
        bias = b_first if q == 0 else (b_last if q == L else b_mid)
        col = torch.einsum("mk,bk->bm", wf[0], zp[:, :, q]) + torch.einsum("mk,bk->bm", wf[1], zp[:, :, q + 1]) + bias
        for r in range(f):
            t = q * f + r - ps_off
            if 0 <= t < L_y:
                assert torch.isnan(out[:, :, t]).all(), "an output position written twice"
                out[:, :, t] = col[:, r * CO: (r + 1) * CO]
    assert not torch.isnan(out).any(), "an output position never written"
    return out


@pytest.mark.parametrize("diff", [0, 2])
@pytest.mark.parametrize("L_in", [1, 2, 3, 24])
@pytest.mark.parametrize("f", [2, 4])
def test_folded_upsample_equals_the_two_convs(f, L_in, diff):
    c = make_case(f, 100 * f + L_in)
    z = torch.randn(3, C_ + F_, L_in, generator=torch.Generator().manual_seed(7 + L_in), dtype=torch.float64)
    wf, b_mid, b_first, b_last = fold_linear_into_upsample(c["w_up"], c["b_up"], f, c["wm"], c["b_m"])
    assert wf.shape == (2, f * CO, C_ + F_) and b_mid.shape == b_first.shape == b_last.shape == (f * CO,)
    got, want = subpixel(c, z, diff, wf, b_mid, b_first, b_last), reference(c, z, diff)
    assert got.shape == want.shape == (3, CO, f * L_in - diff)
    if want.numel() == 0:
        return                                  # (factor 2, one position, cropped by two: nothing is left to compare)
    err = float((got - want).abs().max() / want.abs().max())
    assert err <= 1e-12, err


@pytest.mark.parametrize("f", [2, 4])
def test_interior_bias_everywhere_is_wrong_at_the_edges(f):
    """the check above can see what it is for: with the interior bias in every column the first and the last output positions are off
    by the inner bias seen through the tap that falls outside the sample, and every other position is still right"""
    c = make_case(f, 5)
    L_in = 3
    z = torch.randn(2, C_ + F_, L_in, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    wf, b_mid, _, _ = fold_linear_into_upsample(c["w_up"], c["b_up"], f, c["wm"], c["b_m"])
    got, want = subpixel(c, z, 0, wf, b_mid, b_mid, b_mid), reference(c, z, 0)
    rel = (got - want).abs().amax(dim=(0, 1)) / want.abs().max()
    assert float(rel[0]) > 1e-3 and float(rel[-1]) > 1e-3, rel
    assert float(rel[f: -f].max()) <= 1e-12, rel


def test_ff_out_matrix_is_the_transformer_tail():
    """[P | P W_ff2] [x ; f] + (b_P + P b_ff2) = conv1d(x + W_ff2 f + b_ff2) (reference blocks.py:446, :488, :536)"""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    wp, bp, w2, b2, x, fz = r(C_, C_, 1), r(C_), r(C_, F_), r(C_), r(2, C_, 5), r(2, F_, 5)
    wm, bm = ff_out_matrix(wp, bp, w2, b2)
    want = torch.nn.functional.conv1d(x + torch.einsum("cf,bfl->bcl", w2, fz) + b2[None, :, None], wp, bp)
    got = torch.einsum("ck,bkl->bcl", wm, torch.cat([x, fz], 1)) + bm[None, :, None]
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12


def test_folded_taps_follow_the_packed_tap_order():
    """tap 0 multiplies the row before the column, tap 1 the column's own row, as convT_weight_to_gemm packs the unfolded conv"""
    c = make_case(2, 9)
    wf, *_ = fold_linear_into_upsample(c["w_up"], c["b_up"], 2, c["wm"], c["b_m"])
    U = convT_weight_to_gemm(c["w_up"], 2)
    assert torch.equal(wf[0], U[0] @ c["wm"]) and torch.equal(wf[1], U[1] @ c["wm"])


def test_knob_parsing():
    from jen1_amd.engine import parse_fold_up
    assert parse_fold_up("1") is None and parse_fold_up("") is None
    assert parse_fold_up("0") == frozenset()
    assert parse_fold_up("8,7") == frozenset({7, 8}) and parse_fold_up("3,") == frozenset({3})


def test_edge_bias_contract_of_the_phase_descriptor():
    """include/jen1_deep.h: jen1_deep_phase_conv takes an edge bias only where the unit can honour it -- stride 1, no dual-range split,
    a [M] bias beside it, 16-byte aligned rows -- and every launch-per-layer / tile / long entry point refuses one (host side, no GPU)"""
    import ctypes as C

    from jen1_amd import lib as L
    L.build()
    lib = L.load()
    buf = (C.c_char * lib.jen1_deep_phase_size())()
    out = C.cast(buf, C.c_void_p)
    fake = 1 << 20                                         # (descriptors only store the pointers)

    def args():
        # the folded upsampling of the deepest level at B = 8: [x3 | f] of 2 x 1024 channels, one position, factor 2
        a = L.ConvArgs()
        a.x0, a.x1, a.w, a.bias, a.y = fake, fake + 2048, fake + 8192, fake + 12288, fake + 16384
        a.edge_bias = fake + 32768
        a.dtype, a.B, a.L_in, a.L_out = L.BF16, 8, 1, 2
        a.c0, a.c1, a.ld0, a.ld1, a.src1_scale = 1024, 1024, 2048, 2048, 1.0
        a.taps, a.stride, a.pad_left = 2, 1, 1
        a.M, a.out_C, a.ps_f, a.ps_off, a.L_y, a.y_brows, a.ld_y = 2048, 1024, 2, 1, 2, 2, 1024
        a.live_mask = 3
        return a

    a = args()
    assert lib.jen1_deep_phase_conv(C.byref(a), 0, out) == 0, lib.jen1_last_error()
    plain = bytes(buf)
    a.edge_bias = None
    assert lib.jen1_deep_phase_conv(C.byref(a), 0, out) == 0, lib.jen1_last_error()
    # the descriptor differs from the one without an edge bias in exactly one pointer: the same unit geometry either way
    delta = [i for i in range(len(plain)) if plain[i] != bytes(buf)[i]]
    assert delta and delta[-1] - delta[0] < 8, delta
    for change, what in ((dict(stride=2), b"stride"), (dict(L_out=1, L_in=1), b"two GEMM columns"), (dict(bias=None), b"bias"),
                         (dict(edge_bias=fake + 32768 + 4), b"aligned"), (dict(bias=fake + 12288 + 8), b"aligned"),
                         (dict(m_split=1024, k_split=32), b"dual-range")):
        a = args()
        for k, v in change.items():
            setattr(a, k, v)
        assert lib.jen1_deep_phase_conv(C.byref(a), 0, out) != 0, change
        assert what in lib.jen1_last_error(), (change, lib.jen1_last_error())
    a = args()
    a.cfg, a.tb, a.nb, a.kc_stage, a.splitk = L.CFG_S16x16, 16, 1, 1, 1
    assert lib.jen1_conv_gemm(C.byref(a), None) != 0 and b"edge bias" in lib.jen1_last_error()
    assert lib.jen1_deep_phase_tile(C.byref(a), 16, 128, None, 0, 0, None, 0, 0, 0, None, 0, out) != 0 and b"edge bias" in lib.jen1_last_error()
    lbuf = (C.c_char * 512)()
    assert lib.jen1_long_phase_conv(C.byref(a), 32, None, 0, 0, 0, None, 0, 0, 0, 0, None, C.cast(lbuf, C.c_void_p)) != 0
    assert b"edge bias" in lib.jen1_last_error()
