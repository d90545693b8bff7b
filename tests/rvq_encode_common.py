"""Float64 reference of the residual search ``jen1_rvq_encode`` runs (core_vq.py ResidualVectorQuantization.encode), its inputs and the
tolerance the GPU tests compare with; importable without a GPU (tests/test_rvq_encode_host.py pins it).

Score of entry j for residual r: ``s_j = 2 r.e_j - |e_j|^2`` (``|r|^2`` does not move the argmax).  A float32 evaluation of s_j -- a
128-term dot product, the sum of squares, one multiply-subtract, and a residual that is itself q float32 subtracts away from the exact one
-- is off by at most ``(D + 4 + q) 2^-24 mag_j`` with ``mag_j = 2 sum_i |r_i e_ji| + sum_i e_ji^2`` (the standard dot-product bound).  Two
entries a, b are therefore told apart reliably only when their scores differ by more than ``tol = (D + 4 + q) 2^-24 (mag_a + mag_b)``.
Nothing in the bound is measured.
"""
import numpy as np

from helpers import SEED
from jen1_amd.init_fill import fill_normal

D = 128
U24 = 2.0 ** -24


def tables(n_q: int, bins: int, key: str = "rvq_encode") -> np.ndarray:
    """float32 [n_q, bins, 128]: entries N(0, 1) * 0.8^q (every layer's codebook a little smaller, as a trained RVQ's are)"""
    return np.stack([fill_normal(f"{key}.tables.{q}", (bins, D), SEED) * np.float32(0.8 ** q) for q in range(n_q)]).astype(np.float32)


def golden_tables(n_q: int = 16) -> np.ndarray:
    """the codebooks tests/golden/encodec.npz was made with"""
    return np.stack([fill_normal(f"encodec.quantizer.layers.{i}.codebook.embed", (1024, D), SEED) for i in range(n_q)])


def frames(rows: int, T: int, key: str = "rvq_encode") -> np.ndarray:
    """float32 [rows, 128, T] ~ N(0, 1)"""
    return fill_normal(f"{key}.frames.{rows}x{T}", (rows, D, T), SEED)


def e_sq32(tab: np.ndarray) -> np.ndarray:
    return (tab.astype(np.float32) ** 2).sum(-1, dtype=np.float32)


def scores_and_mag(res: np.ndarray, table: np.ndarray):
    """res float64 [F, 128], table [bins, 128] -> (scores, magnitudes) float64 [F, bins]"""
    e = table.astype(np.float64)
    sq = (e ** 2).sum(1)
    return 2.0 * res @ e.T - sq[None], 2.0 * np.abs(res) @ np.abs(e).T + sq[None]


def tol_of(q: int, mag_a, mag_b):
    return (D + 4 + q) * U24 * (mag_a + mag_b)


def search_ref(emb: np.ndarray, tab: np.ndarray):
    """the search in float64 along its own path.  emb [rows, 128, T], tab [n_q, bins, 128] -> (codes int64 [n_q, rows, T], clear bool
    [n_q, rows, T]): ``clear[q]`` says the reference's top-2 gap at layer q is at least ``2 tol`` of those two entries"""
    rows, _, T = emb.shape
    res = emb.transpose(0, 2, 1).reshape(rows * T, D).astype(np.float64)
    ar = np.arange(rows * T)
    codes, clear = [], []
    for q in range(tab.shape[0]):
        s, mag = scores_and_mag(res, tab[q])
        order = np.argsort(-s, axis=1, kind="stable")[:, :2]
        first, second = order[:, 0], order[:, 1]
        assert (first == s.argmax(1)).all()
        gap = s[ar, first] - s[ar, second]
        clear.append(gap >= 2.0 * tol_of(q, mag[ar, first], mag[ar, second]))
        codes.append(first)
        res = res - tab[q].astype(np.float64)[first]
    return np.stack(codes).reshape(-1, rows, T), np.stack(clear).reshape(-1, rows, T)


def prefix_mask(clear: np.ndarray) -> np.ndarray:
    """the (layer, frame) cells a search is compared on: every layer of a frame before the first one that is not clear"""
    return np.cumprod(clear.astype(np.int64), axis=0).astype(bool)


def validity(emb: np.ndarray, tab: np.ndarray, codes: np.ndarray) -> np.ndarray:
    """how far the entries ``codes`` [n_q, rows, T] name are from the best ones ALONG THE PATH THE CODES THEMSELVES DEFINE, in units of
    tol: the residual is rebuilt with the float32 subtracts the kernel makes (exact: the same operands, one IEEE operation each), scored in
    float64; returns (s_best - s_chosen) / tol per cell, 0 where the chosen entry is the best one.  Valid means <= 1 everywhere."""
    rows, _, T = emb.shape
    res = emb.transpose(0, 2, 1).reshape(rows * T, D).astype(np.float32)
    ar = np.arange(rows * T)
    out = []
    for q in range(codes.shape[0]):
        s, mag = scores_and_mag(res.astype(np.float64), tab[q])
        c = codes[q].reshape(-1)
        assert ((c >= 0) & (c < tab.shape[1])).all(), "a code outside the codebook"
        b = s.argmax(1)
        out.append((s[ar, b] - s[ar, c]) / tol_of(q, mag[ar, b], mag[ar, c]))
        res = res - tab[q].astype(np.float32)[c]
        assert res.dtype == np.float32
    return np.stack(out).reshape(-1, rows, T)
