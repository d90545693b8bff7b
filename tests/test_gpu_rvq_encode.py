"""-m gpu: ``jen1_rvq_encode`` (csrc/encodec.hip: rvq_encode_kernel) through the C ABI against the float64 search of
tests/rvq_encode_common.py (pinned on the CPU by tests/test_rvq_encode_host.py).

A float32 search cannot be asked to reproduce a float64 one code for code: where two entries score within rounding of each other either is
a correct answer, and from there on the residuals part.  So every launch is checked twice.  VALIDITY, along the kernel's own path and with
no exclusions: the residual is rebuilt from the kernel's codes with its float32 subtracts (exact), and the entry it chose must score within
``tol`` of the best one.  PREFIX AGREEMENT: a frame is compared with the float64 search layer by layer up to the first layer whose top-2
gap in the reference is below ``2 tol``; up to there the codes must be equal, and in the 16 x 1024 cases at least 95 % of all cells must
be compared.  ``tol = (128 + 4 + q) 2^-24 (mag_a + mag_b)`` is the dot-product bound of the score, nothing in it is measured.

Both outputs are pre-filled with a sentinel and followed by a 64-element guard; everything outside the addressed time slots must come
back bit-identical.  The latents must be bit-equal to ``jen1_rvq_decode`` of the kernel's codes.  No launch has more than 13 workgroups.
"""
import numpy as np
import pytest
import torch

import rvq_encode_common as RC
from helpers import golden, record_parity

pytestmark = pytest.mark.gpu

GUARD = 64
LAT_SENTINEL = -7.25
CODE_SENTINEL = -7777
D = 128

# name: (n_q, rows, B_out, T, bins), padding of the outputs' time axis, t0
CASES = {
    "a": ((1, 1, 1, 1, 64), 0, 0),
    "b": ((2, 1, 1, 17, 64), 0, 0),
    "c": ((4, 6, 3, 70, 128), 29, 11),
    "d": ((16, 2, 2, 31, 1024), 0, 0),
    "e": ((16, 1, 1, 150, 1024), 0, 0),
}
TIE_FRAMES = [(0, 0), (1, 33), (4, 69), (5, 31)]          # (row, t) of case c: first / last lanes, both tiles' halves


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from jen1_amd import lib as L
    return L.load()


def _inputs(name):
    (n_q, rows, B_out, T, bins), _, _ = CASES[name]
    if name == "d":
        emb, tab = golden("encodec")["encoder.y"], RC.golden_tables(16)
        assert emb.shape == (rows, D, T)
        return emb, tab
    tab = RC.tables(n_q, bins, key=f"rvq_encode.{name}")
    emb = RC.frames(rows, T, key=f"rvq_encode.{name}")
    if name == "c":                       # an exact tie in codebook 1: entry 100 is a copy of entry 5
        tab = tab.copy()
        emb = emb.copy()
        tab[1, 100] = tab[1, 5]
        for i, (r, t) in enumerate(TIE_FRAMES):
            emb[r, :, t] = tab[0, 3 + 17 * i] + tab[1, 5]
    return emb, tab


class Launch:
    """one jen1_rvq_encode call into guarded, sentinel-filled outputs; ``.codes`` [n_q, B_out, span], ``.latents`` [B_out, 128, span]"""

    def __init__(self, lib, emb, tab, n_q, B_out, pad=0, t0=0, want_codes=True, want_latents=True, bufs=None, D_arg=D, bins_arg=None,
                 expect_error=False):
        from jen1_amd import lib as L
        rows, _, T = emb.shape
        bins = tab.shape[1]
        self.span = (rows // B_out) * T if rows % B_out == 0 else rows * T
        self.T_out = self.span + pad
        self.t0, self.n_q, self.B_out = t0, n_q, B_out
        if bufs is None:
            codes = torch.full((n_q * B_out * self.T_out + GUARD,), CODE_SENTINEL, dtype=torch.int64, device="cuda")
            lat = torch.full((B_out * D * self.T_out + GUARD,), LAT_SENTINEL, dtype=torch.float32, device="cuda")
        else:
            codes, lat = bufs
        self.codes_buf, self.lat_buf = codes, lat
        emb_d = torch.from_numpy(np.ascontiguousarray(emb)).cuda()
        tab_d = torch.from_numpy(np.ascontiguousarray(tab)).cuda()
        esq_d = (tab_d ** 2).sum(-1).contiguous()
        self.tab_d = tab_d
        rc = lib.jen1_rvq_encode(emb_d.data_ptr(), tab_d.data_ptr(), esq_d.data_ptr(), codes.data_ptr() if want_codes else None,
                                 lat.data_ptr() if want_latents else None, n_q, rows, T, bins if bins_arg is None else bins_arg, D_arg, B_out,
                                 self.T_out, t0, self.T_out, t0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        self.rc = rc
        if expect_error:
            return
        L.check(rc, "jen1_rvq_encode")
        c = codes[:-GUARD].view(n_q, B_out, self.T_out)
        z = lat[:-GUARD].view(B_out, D, self.T_out)
        self.codes = c[:, :, t0:t0 + self.span].contiguous() if want_codes else None
        self.latents = z[:, :, t0:t0 + self.span].contiguous() if want_latents else None
        # untouched memory: the guard, the time axis outside the slot, and an output that was not asked for
        assert bool((codes[-GUARD:] == CODE_SENTINEL).all()) and _all_sentinel(lat[-GUARD:]), "written past the end"
        assert bool((c[:, :, :t0] == CODE_SENTINEL).all()) and bool((c[:, :, t0 + self.span:] == CODE_SENTINEL).all()), "codes outside the slot"
        assert _all_sentinel(z[:, :, :t0]) and _all_sentinel(z[:, :, t0 + self.span:]), "latents outside the slot"
        if want_codes:
            assert bool(((self.codes >= 0) & (self.codes < bins)).all()), "a slot of the codes was not written"
        else:
            assert bool((codes == CODE_SENTINEL).all())
        if not want_latents:
            assert _all_sentinel(lat)


def _all_sentinel(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.contiguous().view(torch.int32), torch.full_like(t, LAT_SENTINEL).contiguous().view(torch.int32)))


def _bit_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _rows_view(codes: np.ndarray, rows: int, B_out: int, T: int) -> np.ndarray:
    """codes [n_q, B_out, (rows / B_out) T] -> [n_q, rows, T] in the order of the input rows (row j B_out + b)"""
    n_q = codes.shape[0]
    return codes.reshape(n_q, B_out, rows // B_out, T).transpose(0, 2, 1, 3).reshape(n_q, rows, T)


_cache = {}


def _case(lib, name):
    if name not in _cache:
        (n_q, rows, B_out, T, bins), pad, t0 = CASES[name]
        emb, tab = _inputs(name)
        run = Launch(lib, emb, tab, n_q, B_out, pad, t0)
        _cache[name] = (emb, tab, run, RC.search_ref(emb, tab))
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_validity_prefix_agreement_and_latents(lib, name):
    (n_q, rows, B_out, T, bins), _, _ = CASES[name]
    emb, tab, run, (ref_codes, clear) = _case(lib, name)
    got = _rows_view(run.codes.cpu().numpy(), rows, B_out, T)
    # 1. validity along the kernel's own path: every frame, every layer
    ratio = RC.validity(emb, tab, got)
    mask = RC.prefix_mask(clear)
    record_parity("rvq_encode", name, "f32", worst_validity_ratio=ratio.max(), compared=mask.mean(), differ=(got != ref_codes).mean())
    print(f"rvq_encode {name}: worst validity ratio {ratio.max():.3e}, compared cells {mask.mean():.4f}, cells that differ {(got != ref_codes).mean():.4f}")
    assert (ratio <= 1.0).all(), (name, float(ratio.max()))
    # 2. prefix agreement with the float64 search
    assert np.array_equal(got[mask], ref_codes[mask]), (name, int((got[mask] != ref_codes[mask]).sum()))
    if name in ("d", "e"):
        assert mask.mean() >= 0.95, mask.mean()
    if name == "d":
        assert np.array_equal(got[mask], golden("encodec")["encoder.codes"][mask])
    # 4. the latents are the decode kernel's sum of the kernel's own codes, bit for bit
    span = run.span
    want = torch.empty((B_out, D, span), dtype=torch.float32, device="cuda")
    from jen1_amd import lib as L
    L.check(lib.jen1_rvq_decode(run.codes.data_ptr(), run.tab_d.data_ptr(), want.data_ptr(), n_q, B_out, span, bins, D,
                                torch.cuda.current_stream().cuda_stream), "jen1_rvq_decode")
    torch.cuda.synchronize()
    assert _bit_equal(run.latents, want)


@pytest.mark.parametrize("name", ["b", "c"])
def test_one_output_alone(lib, name):
    """codes only / latents only: the same bits as the call with both, the other buffer untouched (checked in Launch)"""
    (n_q, rows, B_out, T, bins), pad, t0 = CASES[name]
    emb, tab, run, _ = _case(lib, name)
    only_c = Launch(lib, emb, tab, n_q, B_out, pad, t0, want_latents=False)
    only_z = Launch(lib, emb, tab, n_q, B_out, pad, t0, want_codes=False)
    assert torch.equal(only_c.codes, run.codes)
    assert _bit_equal(only_z.latents, run.latents)


def test_exact_ties_take_the_lowest_index(lib):
    (n_q, rows, B_out, T, bins), _, _ = CASES["c"]
    emb, tab, run, _ = _case(lib, "c")
    got = _rows_view(run.codes.cpu().numpy(), rows, B_out, T)
    assert np.array_equal(tab[1, 5], tab[1, 100])
    for i, (r, t) in enumerate(TIE_FRAMES):
        assert got[0, r, t] == 3 + 17 * i, (r, t, got[:, r, t])
        assert got[1, r, t] == 5, (r, t, got[:, r, t])
    assert not (got[1] == 100).any()


def test_row_to_batch_and_segment_mapping(lib):
    """case c, rows = 6 as 2 segments of B_out = 3: one launch per segment into the same buffers gives the same bits everywhere"""
    (n_q, rows, B_out, T, bins), pad, t0 = CASES["c"]
    emb, tab, run, _ = _case(lib, "c")
    codes = torch.full_like(run.codes_buf, CODE_SENTINEL)
    lat = torch.full_like(run.lat_buf, LAT_SENTINEL)
    T_out = run.T_out
    from jen1_amd import lib as L
    tab_d = run.tab_d
    esq_d = (tab_d ** 2).sum(-1).contiguous()
    for j in range(rows // B_out):
        part = torch.from_numpy(np.ascontiguousarray(emb[j * B_out:(j + 1) * B_out])).cuda()
        L.check(lib.jen1_rvq_encode(part.data_ptr(), tab_d.data_ptr(), esq_d.data_ptr(), codes.data_ptr(), lat.data_ptr(), n_q, B_out, T, bins, D,
                                    B_out, T_out, t0 + j * T, T_out, t0 + j * T, torch.cuda.current_stream().cuda_stream), "jen1_rvq_encode")
    torch.cuda.synchronize()
    assert torch.equal(codes, run.codes_buf)
    assert _bit_equal(lat, run.lat_buf)


def test_codes_do_not_depend_on_the_launch_shape(lib):
    """the 150 frames of case e as one row of 150 and as 5 rows of 30"""
    (n_q, _, _, T, bins), _, _ = CASES["e"]
    emb, tab, run, _ = _case(lib, "e")
    split = np.ascontiguousarray(emb[0].reshape(D, 5, 30).transpose(1, 0, 2))
    again = Launch(lib, split, tab, n_q, 1)
    assert torch.equal(again.codes, run.codes)
    assert _bit_equal(again.latents, run.latents)


@pytest.mark.parametrize("what", ["D64", "bins100", "both_null", "t0_overflow"])
def test_bad_arguments_launch_nothing(lib, what):
    n_q, B_out = 2, 1
    emb, tab = RC.frames(1, 17, key="rvq_encode.b"), RC.tables(2, 64, key="rvq_encode.b")
    kw = {"D64": dict(D_arg=64), "bins100": dict(bins_arg=100), "both_null": dict(want_codes=False, want_latents=False),
          "t0_overflow": dict(t0=1)}[what]
    run = Launch(lib, emb, tab, n_q, B_out, expect_error=True, **kw)
    assert run.rc != 0
    assert lib.jen1_last_error()
    assert bool((run.codes_buf == CODE_SENTINEL).all()) and _all_sentinel(run.lat_buf)
