"""-m gpu: the kernels of csrc/encodec.hip form by form through the C ABI, and the SEANet building blocks of jen1_amd/encodec.py one by
one, each against a float64 reference (tests/encodec_common.py, pinned on the CPU by tests/test_encodec_refs_host.py).

LSTM (``jen1_lstm_layer``: lstm_layer_kernel<{float,bf16},{1,2,4}>; ``jen1_lstm_layer_multi``: lstm_multi_kernel<{float,bf16},{32,64,128}>
and lstm_multi_mfma_kernel): inputs gin ~ N(0,1), whh ~ U(-1,1)/sqrt(H), skip ~ N(0,1).  In bf16 mode the reference gets the same
bf16-rounded weights and skip the kernel reads, so only the kernel's arithmetic is under test.  Gates are per element and absolute:
float32 ``|y - ref| <= 8 e``, bf16 ``|y - ref| <= 2^-8 |ref| + 8 e`` (one bf16 ulp of the exact value for the rounding of y), where e is
the error of a float32 numpy restatement of the same recurrence on the same inputs (with h split into bf16 high + low for the
matrix-core kernel), computed in the test.  The factor 8 covers expf / tanhf that differ from numpy's by a few ulp and the different
summation order; it stays ~300x below the 5e-4 that bf16-rounded weights move the result by.  Measured: profiles/encodec_kernel_parity.txt.

Every y is [B + 1][T][ld_y] pre-filled with a sentinel: the extra sequence and the columns H..ld_y must come back bit-identical.  The
exchange buffer of the multi-workgroup kernels is pre-filled with NaN (a kernel may only read what it wrote), the barrier counters are
zeroed per launch, their time-out flag must stay 0 and every group's counter must end at T x workgroups.  No launch has more than 64
workgroups.
"""
import numpy as np
import pytest
import torch

from encodec_common import (bf16_round, dec_params, elu64, enc_params, group_norm64, lstm_inputs, lstm_layer_emul, lstm_layer_ref,
                            rvq_decode_ref, sconv1d64, sconv_transpose1d64)
from helpers import BF16_TOL, F32_TOL, record_parity, rel_err

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16"]
SENTINEL = -7.25                # exact in bf16
BIG = 3.0e4                     # padding columns of skip: finite in bf16, and no result may depend on them
U23, U8 = 2.0 ** -23, 2.0 ** -8
MARGIN = 8.0                    # x the float32 emulation's own error


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import lib as L
    return L.load()


def _sync_check(rc, what):
    from jen1_amd import lib as L
    L.check(rc, what)
    torch.cuda.synchronize()


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _is_sentinel(t: torch.Tensor) -> bool:
    return bool(torch.equal(_bits(t), _bits(torch.full_like(t, SENTINEL))))


# ---------------------------------------------------------------------------------------------------------------------
# LSTM
# ---------------------------------------------------------------------------------------------------------------------
def _lstm_case(lib, kind, mode, H, B, T, with_skip):
    """one launch of ``kind`` in ("single", "plain", "mfma"); returns (max |y - ref|, the largest excess over the rounding term, bound)"""
    from jen1_amd import lib as L
    bf = mode == "bf16"
    mfma_form = bf and H == 512 and B > 1
    assert (kind == "mfma") == (mfma_form and kind != "single"), "the case does not reach the kernel it names"
    tdt = torch.bfloat16 if bf else torch.float32
    ld_y = H + 8 if with_skip else H
    gin, whh, skip = lstm_inputs(B, T, H, 1000 * H + 10 * B + T)
    if bf:
        whh, skip = bf16_round(whh), bf16_round(skip)          # what the kernel reads
    sk = skip if with_skip else None
    ref = lstm_layer_ref(gin, whh, sk)
    emul_err = float(np.abs(lstm_layer_emul(gin, whh, sk, split_h=kind == "mfma") - ref).max())
    assert 0 < emul_err < 1e-5
    y = torch.full((B + 1, T, ld_y), SENTINEL, dtype=tdt, device="cuda")
    skip_d = None
    if with_skip:
        skip_d = torch.full((B, T, ld_y), BIG, dtype=tdt, device="cuda")
        skip_d[:, :, :H] = torch.from_numpy(skip).to(tdt)
    gin_d = torch.from_numpy(gin).cuda()
    s = torch.cuda.current_stream().cuda_stream
    dt = L.BF16 if bf else L.F32
    if kind == "single":
        assert B <= 64
        w = torch.from_numpy(whh).t().contiguous().to(tdt).cuda()                      # [H][4H]
        _sync_check(lib.jen1_lstm_layer(gin_d.data_ptr(), w.data_ptr(), None if skip_d is None else skip_d.data_ptr(), y.data_ptr(),
                                        B, T, H, ld_y, dt, s), "jen1_lstm_layer")
    else:
        groups8 = (B + 7) // 8
        used = (B + 15) // 16 if kind == "mfma" else groups8
        nw = H // 32
        assert used * nw <= 64
        w = torch.from_numpy(whh).to(tdt).cuda()                                       # [4H][H]
        hbuf = torch.full((groups8, 2, 16, H), float("nan"), dtype=torch.float32, device="cuda")
        cnt = torch.zeros((groups8, 32), dtype=torch.int32, device="cuda")
        _sync_check(lib.jen1_lstm_layer_multi(gin_d.data_ptr(), w.data_ptr(), None if skip_d is None else skip_d.data_ptr(), y.data_ptr(),
                                              hbuf.data_ptr(), cnt.data_ptr(), B, T, H, ld_y, dt, s), "jen1_lstm_layer_multi")
        c = cnt.cpu().numpy()
        assert (c[:, 1] == 0).all(), "grid barrier time-out"
        assert (c[:used, 0] == T * nw).all() and (c[used:, 0] == 0).all(), c[:, 0]
        assert (c[:, 2:] == 0).all()
    assert _is_sentinel(y[B]), "the sequence after the last one was written"
    assert ld_y == H or _is_sentinel(y[:B, :, H:]), "columns H..ld_y were written"
    got = y[:B, :, :H].float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    bound = MARGIN * emul_err
    excess = float((err - (U8 * np.abs(ref) if bf else 0.0)).max())
    name = f"{kind}.H{H}.B{B}.T{T}.{'skip' if with_skip else 'noskip'}"
    record_parity("encodec_lstm", name, mode, max_err=err.max(), excess=excess, emul_err=emul_err, bound=bound, max_ref=np.abs(ref).max())
    print(f"encodec_lstm {name} {mode}: max|y-ref| {err.max():.3e} beyond-rounding {excess:.3e} emulation {emul_err:.3e} bound {bound:.3e}")
    assert excess <= bound, (name, mode, excess, bound)


SKIP_FORMS = [False, True]      # (no skip, ld_y = H), (skip, ld_y = H + 8)


@pytest.mark.parametrize("with_skip", SKIP_FORMS)
@pytest.mark.parametrize("B,T", [(1, 1), (3, 17)])
@pytest.mark.parametrize("H", [256, 512, 1024])
@pytest.mark.parametrize("mode", MODES)
def test_lstm_layer_single_workgroup(lib, mode, H, B, T, with_skip):
    """lstm_layer_kernel<{float, bf16}, RPT = 1 / 2 / 4>"""
    _lstm_case(lib, "single", mode, H, B, T, with_skip)


# every H at (B, T) = (9, 19) (two groups, the second one with a single sequence); bf16 with more than one sequence only where the
# launcher keeps the plain kernel (H = 512 goes to the matrix cores); bf16 with one sequence at every H
PLAIN_H_CASES = ([("f32", H, 9, 19) for H in (256, 512, 1024)] + [("bf16", H, 9, 19) for H in (256, 1024)] +
                 [("bf16", H, 1, 19) for H in (256, 512, 1024)])
# every (B, T) pair at H = 512: float32, and bf16 for the single sequence
PLAIN_BT_CASES = ([("f32", 512, B, T) for B in (1, 7, 8, 9) for T in (1, 2, 19) if (B, T) != (9, 19)] +
                  [("bf16", 512, 1, T) for T in (1, 2)])


@pytest.mark.parametrize("with_skip", SKIP_FORMS)
@pytest.mark.parametrize("mode,H,B,T", PLAIN_H_CASES + PLAIN_BT_CASES)
def test_lstm_layer_multi_plain(lib, mode, H, B, T, with_skip):
    """lstm_multi_kernel<{float, bf16}, KS = 32 / 64 / 128>: groups of 8 sequences"""
    _lstm_case(lib, "plain", mode, H, B, T, with_skip)


@pytest.mark.parametrize("with_skip", SKIP_FORMS)
@pytest.mark.parametrize("T", [1, 2, 19])
@pytest.mark.parametrize("B", [2, 15, 16, 17, 33])
def test_lstm_layer_multi_mfma(lib, B, T, with_skip):
    """lstm_multi_mfma_kernel: bf16, H = 512, groups of 16 sequences"""
    _lstm_case(lib, "mfma", "bf16", 512, B, T, with_skip)


def test_lstm_layer_multi_mfma_long(lib):
    """300 steps: the error does not grow along the recurrence (with these inputs the recurrence contracts)"""
    _lstm_case(lib, "mfma", "bf16", 512, 3, 300, True)


# ---------------------------------------------------------------------------------------------------------------------
# RVQ decode
# ---------------------------------------------------------------------------------------------------------------------
RVQ_CASES = [
    # n_q, B, T, bins, D
    (1, 1, 1, 5, 8),                # minimum; one codebook: the table rows themselves
    (16, 2, 63, 1024, 128),         # the product's tables, one frame short of a tile
    (16, 2, 64, 1024, 128),         # exactly one tile
    (3, 3, 65, 33, 130),            # a second tile with one frame; a second d0 pass with two columns; out-of-range codes
    (2, 1, 130, 7, 257),            # three tiles, three d0 passes
    (4, 2, 37, 16, 64),             # D below the 128-column pass
]
RVQ_GUARD = 64


@pytest.mark.parametrize("case", RVQ_CASES, ids=lambda c: "x".join(map(str, c)))
def test_rvq_decode(lib, case):
    n_q, B, T, bins, D = case
    assert (T + 63) // 64 * B <= 64
    g = torch.Generator().manual_seed(sum((i + 2) * v for i, v in enumerate(case)))
    tables = torch.randn((n_q, bins, D), generator=g)
    codes = torch.randint(0, bins, (n_q, B, T), generator=g, dtype=torch.int64)
    if case == (3, 3, 65, 33, 130):
        codes[0, 0, 0], codes[1, 2, 64], codes[2, 1, 63] = -1, bins, bins + 1000
        codes[0, 2, 64], codes[2, 0, 1] = -(2 ** 40), 2 ** 40                        # beyond 32 bits either way
    ref = rvq_decode_ref(codes.numpy(), tables.numpy())
    mag = rvq_decode_ref(codes.numpy(), tables.numpy(), magnitude=True)
    whole = torch.full((B * D * T + RVQ_GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    t_d, c_d = tables.cuda(), codes.cuda()
    _sync_check(lib.jen1_rvq_decode(c_d.data_ptr(), t_d.data_ptr(), whole.data_ptr(), n_q, B, T, bins, D,
                                    torch.cuda.current_stream().cuda_stream), "jen1_rvq_decode")
    assert _is_sentinel(whole[B * D * T:]), "written past the end of out"
    got = whole[:B * D * T].view(B, D, T).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    record_parity("encodec_rvq", "x".join(map(str, case)), "f32", max_err=err.max(), worst_ratio=(err / np.maximum(n_q * U23 * mag, 1e-300)).max())
    if n_q == 1:
        assert np.array_equal(got, ref)
    else:
        assert (err <= n_q * U23 * mag).all(), float((err / (n_q * U23 * mag)).max())     # a sequential float32 sum of n_q terms


# ---------------------------------------------------------------------------------------------------------------------
# SEANet blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd.encodec import SEANetDecoderHIP, SEANetEncoderHIP
    dp, ep = dec_params(), enc_params()
    out = {"dec_p": dp, "enc_p": ep}
    for mode in MODES:
        out["dec", mode] = SEANetDecoderHIP({k: torch.from_numpy(v) for k, v in dp.items()}, compute_dtype=mode)
        out["enc", mode] = SEANetEncoderHIP({k: torch.from_numpy(v) for k, v in ep.items()}, compute_dtype=mode)
    return out


def _rows(net, B, C, L, seed):
    """random rows [B][L][pad8(C)] in the net's dtype (padding columns 0) and the float64 [B][C][L] array they hold"""
    g = torch.Generator().manual_seed(seed)
    x = net._to_rows(torch.randn((B, C, L), generator=g).to(net.device))
    return x, x[:, :, :C].float().cpu().numpy().astype(np.float64).transpose(0, 2, 1)


def _from_rows(y, C):
    y = y.float().cpu().numpy().astype(np.float64)
    assert y.shape[-1] == C or float(np.abs(y[:, :, C:]).max()) == 0.0, "padding columns must stay exactly 0"
    return y[:, :, :C].transpose(0, 2, 1)


def _edge_err(got, ref, k):
    """the max-norm error over the first and last k frames alone, relative to the largest reference entry among them"""
    n = ref.shape[-1]
    idx = sorted(set(range(min(k, n))) | set(range(max(0, n - k), n)))
    return rel_err(got[..., idx], ref[..., idx])


def _gate_conv(what, case, mode, got, ref, k):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    tol = F32_TOL if mode == "f32" else BF16_TOL
    e, edge = rel_err(got, ref), _edge_err(got, ref, k)
    record_parity(what, case, mode, rel_err=e, edge_err=edge)
    print(f"{what} {case} {mode}: rel_err {e:.3e} edge {edge:.3e}")
    assert e < tol, (what, case, mode, e)
    assert edge < 4 * tol, (what, case, mode, edge)


@pytest.mark.parametrize("L", [4, 5, 37])
@pytest.mark.parametrize("name", ["layers.0", "layers.15"])          # 128 -> 512 and the output convolution 32 -> 2 (ld 8)
@pytest.mark.parametrize("mode", MODES)
def test_seanet_conv_k7(nets, mode, name, L):
    """SConv1d k = 7, stride 1: reflect padding 3 + 3 through the index map; L = 4 is the shortest the guard allows"""
    dec, p = nets["dec", mode], nets["dec_p"]
    co, ci, k = p[f"{name}.conv.weight"].shape
    assert k == 7
    x, x64 = _rows(dec, 2, ci, L, 100 + L)
    got = _from_rows(dec._conv(x, name), co)
    torch.cuda.synchronize()
    _gate_conv("encodec_conv_k7", f"{name}.L{L}", mode, got, sconv1d64(x64, p, name, round_weight=mode == "bf16"), k)


@pytest.mark.parametrize("mode", MODES)
def test_seanet_conv_k7_too_short(nets, mode):
    dec, p = nets["dec", mode], nets["dec_p"]
    x, _ = _rows(dec, 1, p["layers.0.conv.weight"].shape[1], 3, 1)
    with pytest.raises(NotImplementedError):
        dec._conv(x, "layers.0")


# the encoder's down-sampling convolutions: (layer, stride) and a length that is a multiple of the stride / one that is not (the extra
# right padding that makes the frame count whole)
STRIDED = [("layers.3", 2, 16), ("layers.3", 2, 17), ("layers.6", 4, 24), ("layers.6", 4, 26), ("layers.9", 5, 25), ("layers.9", 5, 28),
           ("layers.12", 8, 32), ("layers.12", 8, 37)]


@pytest.mark.parametrize("name,stride,L", STRIDED)
@pytest.mark.parametrize("mode", MODES)
def test_seanet_conv_strided(nets, mode, name, stride, L):
    enc, p = nets["enc", mode], nets["enc_p"]
    co, ci, k = p[f"{name}.conv.weight"].shape
    assert k == 2 * stride
    x, x64 = _rows(enc, 2, ci, L, 200 + L)
    got = _from_rows(enc._conv(x, name, stride=stride), co)
    torch.cuda.synchronize()
    assert got.shape[-1] == -(-L // stride)
    _gate_conv("encodec_conv_strided", f"{name}.s{stride}.L{L}", mode, got, sconv1d64(x64, p, name, stride, round_weight=mode == "bf16"), k)


@pytest.mark.parametrize("L", [1, 2, 9])
@pytest.mark.parametrize("name,ratio", [("layers.3", 8), ("layers.6", 5), ("layers.9", 4), ("layers.12", 2)])
@pytest.mark.parametrize("mode", MODES)
def test_seanet_conv_transpose(nets, mode, name, ratio, L):
    """SConvTranspose1d: GroupNorm over the untrimmed length, then the trim"""
    dec, p = nets["dec", mode], nets["dec_p"]
    ci, co, k = p[f"{name}.conv.weight"].shape
    assert k == 2 * ratio
    x, x64 = _rows(dec, 2, ci, L, 300 + L)
    got = _from_rows(dec._conv_transpose(x, name, ratio), co)
    torch.cuda.synchronize()
    assert got.shape[-1] == L * ratio
    _gate_conv("encodec_conv_transpose", f"{name}.r{ratio}.L{L}", mode, got, sconv_transpose1d64(x64, p, name, ratio, round_weight=mode == "bf16"), k)


def _bf16_ulp(v):
    """one unit in the last place of bfloat16 (8 significant bits) at the magnitude of v"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -126))) - 7)


@pytest.mark.parametrize("n", [48, 43])          # a multiple of 8 (the vector kernel) and not (the scalar kernel)
@pytest.mark.parametrize("mode", MODES)
def test_seanet_elu(nets, mode, n):
    dec = nets["dec", mode]
    grid = [0.0, -0.0, 1e-7, -1e-7, -20.0, -100.0, 1.0, -1.0, 0.5, -0.5, 3.0, -3.0, 1e-3, -1e-3, 20.0, -0.1, -5.0, -10.0, 100.0, -88.0]
    v = np.concatenate([grid, np.linspace(-6.0, 6.0, n - len(grid))]).astype(np.float32)
    x = torch.from_numpy(v).to(dec.rt.tdtype).cuda().view(1, 1, n)
    got = dec._elu(x).float().cpu().numpy().reshape(-1).astype(np.float64)
    torch.cuda.synchronize()
    ref = elu64(x.float().cpu().numpy().reshape(-1))
    err = np.abs(got - ref)
    if mode == "f32":
        rel = err / np.maximum(np.abs(ref), 1e-6)
        record_parity("encodec_elu", f"n{n}", mode, worst_rel=rel.max())
        assert (rel <= 4 * U23).all(), (float(rel.max()), v[int(rel.argmax())])
    else:
        ulps = err / _bf16_ulp(ref)
        record_parity("encodec_elu", f"n{n}", mode, worst_ulps=ulps.max())
        assert (ulps <= 1.0).all(), (float(ulps.max()), v[int(ulps.argmax())])
    assert (got[ref > 0] == ref[ref > 0]).all() and got[0] == 0.0 and got[1] == 0.0


@pytest.mark.parametrize("name,C,L", [("layers.15", 2, 11), ("layers.12", 32, 37)])     # the output convolution's norm in ld = 8; C = ld
@pytest.mark.parametrize("mode", MODES)
def test_seanet_group_norm(nets, mode, name, C, L):
    """GroupNorm(1 group) over (C, L) of padded rows.  Bound per element, float32: 2^-23 (8 (|y| + |beta|) + 32 |gamma|) -- a few
    roundings of the affine, plus the mean's error (a tree sum of <= 2^11 entries of magnitude <= 4 sigma: ~ 11 x 4 x 2^-24 sigma) and
    the variance's through 1 / sigma, both scaled by |gamma|.  bf16: the same plus one rounding of the output, 2^-8 |y|."""
    dec, p = nets["dec", mode], nets["dec_p"]
    gamma, beta = p[f"{name}.norm.weight"].astype(np.float64), p[f"{name}.norm.bias"].astype(np.float64)
    assert gamma.shape == (C,)
    x, x64 = _rows(dec, 3, C, L, 400 + C)
    x64 = x64 * 1.0
    got = _from_rows(dec._norm(x, name, C), C)
    torch.cuda.synchronize()
    ref = group_norm64(x64, gamma, beta)
    bound = U23 * (8 * (np.abs(ref) + np.abs(beta)[None, :, None]) + 32 * np.abs(gamma)[None, :, None]) + (U8 * np.abs(ref) if mode == "bf16" else 0.0)
    err = np.abs(got - ref)
    record_parity("encodec_group_norm", f"{name}.C{C}.L{L}", mode, max_err=err.max(), worst_ratio=(err / bound).max())
    assert (err <= bound).all(), float((err / bound).max())
