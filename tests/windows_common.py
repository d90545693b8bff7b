"""Shared by test_windows_host.py and test_gpu_windows.py: overlapping sampler windows on one canvas restated in numpy, independent of
the package.

    W          = 1 + ceil((L - T) / hop),  offsets[j] = min(j hop, L - T)
    k(p)       = min(p + 1, T - p, ramp)                                  integer weight of window position p
    m[s][c][l] = sum_j k(l - off_j) x[s W + j][c][l - off_j] / sum_j k(l - off_j)      over the windows j covering canvas frame l

in float64; a frame covered by one window keeps its value.  Rows are piece-major: row s W + j is window j of piece s.
``oracle_loop`` of known_blend_common.py takes the merge as its per-step ``edits``.
"""
import numpy as np

from known_blend_common import oracle_loop  # noqa: F401  (re-exported: the windowed oracle trajectory is oracle_loop + merge_edits)


def np_offsets(L, T, hop):
    W = 1 + -(-(L - T) // hop)
    return [min(j * hop, L - T) for j in range(W)]


def np_k(T, ramp):
    p = np.arange(T)
    return np.minimum(np.minimum(p + 1, T - p), ramp).astype(np.int64)


def np_cover(L, T, offsets):
    """how many windows cover every canvas frame, int [L]"""
    c = np.zeros(L, dtype=np.int64)
    for off in offsets:
        c[off:off + T] += 1
    return c


def np_gather(canvas, T, offsets):
    """canvas [..., n, C, L] -> rows [..., n W, C, T]"""
    canvas = np.asarray(canvas)
    *lead, n, C, L = canvas.shape
    rows = np.stack([canvas[..., off:off + T] for off in offsets], axis=-3)          # [..., n, W, C, T]
    return np.ascontiguousarray(rows.reshape(*lead, n * len(offsets), C, T))


def np_merge(rows, L, offsets, ramp):
    """rows [n W, C, T] -> (the merged canvas in float64 [n, C, L], the largest |x| among the values covering each frame [n, C, L])"""
    rows = np.asarray(rows)
    W = len(offsets)
    nW, C, T = rows.shape
    n = nW // W
    k = np_k(T, ramp).astype(np.float64)
    x = rows.reshape(n, W, C, T).astype(np.float64)
    num, den, big = np.zeros((n, C, L)), np.zeros(L), np.zeros((n, C, L))
    for j, off in enumerate(offsets):
        num[:, :, off:off + T] += k * x[:, j]
        den[off:off + T] += k
        big[:, :, off:off + T] = np.maximum(big[:, :, off:off + T], np.abs(x[:, j]))
    assert (den > 0).all(), "a canvas frame no window covers"
    return num / den, big


def np_merge_rows(rows, L, offsets, ramp):
    """the merge as the sampler sees it: float32 rows [n W, C, T] -> merged float32 rows (singly covered frames keep their bits)"""
    rows = np.asarray(rows, dtype=np.float32)
    T = rows.shape[-1]
    canvas, _ = np_merge(rows, L, offsets, ramp)
    out = np_gather(canvas.astype(np.float32), T, offsets)
    single = np_gather(np.broadcast_to(np_cover(L, T, offsets) == 1, canvas.shape), T, offsets)
    return np.where(single, rows, out).astype(np.float32)


def merge_edits(S, L, offsets, ramp):
    """the per-step merges as ``oracle_loop`` edits {i: x -> x'}"""
    return {i: (lambda x: np_merge_rows(x, L, offsets, ramp)) for i in range(S)}
