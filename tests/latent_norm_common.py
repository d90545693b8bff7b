"""A float64 numpy model of the latent whitening (csrc/latent_norm.hip, jen1_amd/normalizer.py) and the case lists of its tests:
the moments, ``finalize`` for the three kinds, the affine map, and the error bounds the GPU tests hold the kernels to.  Nothing here
imports the HIP library.

Bounds (derived, not measured; u53 = 2^-53, u24 = 2^-24):
  moments   every product of two float32 values is exact in float64, so a sum of n of them in ANY order is off by at most
            (n - 1) u53 sum |z_c z_d| (to first order); the partials-then-state order adds no more than that count of roundings, and
            the model's own float64 sum sits inside the same bound.  The tests use (n + 2) u53 sum |z_c z_d| elementwise, n = frames.
  affine    one rounding of z - pre, a chain of C fmaf from 0, one rounding of + post:
            (C + 3) u24 sum_k |A_ck| |z_k - pre_k|  +  2 u24 |y|.
"""
import numpy as np

U53 = 2.0 ** -53
U24 = 2.0 ** -24
KINDS = ("zca", "pca", "diag")

# (B, T, C): the run of a workgroup is 128 frames, the affine tile 64
MOMENT_CASES = [(1, 1, 128), (1, 63, 128), (2, 64, 128), (3, 65, 128), (2, 151, 128), (8, 1515, 128), (3, 65, 32)]
# (B, T, C, lengths): 0, 1, T - 1 and T, and run boundaries (127, 128, 129)
LENGTH_CASES = [(3, 65, 128, [0, 1, 64]), (3, 65, 128, [65, 64, 1]), (4, 151, 128, [151, 150, 0, 1]),
                (8, 1515, 128, [0, 1, 1514, 1515, 700, 128, 129, 127]), (3, 65, 32, [64, 0, 65])]
AFFINE_T = (1, 15, 64, 65, 150, 1515)
AFFINE_B = (1, 3)


def words(C):
    return 1 + C + C * C


def mixing(C, seed, lo=0.25, hi=4.0):
    """L with the eigenvalues of L L^T spread over [lo, hi]: a random rotation times the roots"""
    g = np.random.default_rng(seed)
    q, _ = np.linalg.qr(g.standard_normal((C, C)))
    return q * np.sqrt(np.geomspace(lo, hi, C))[None, :]


def latents(B, T, C, seed, mean_scale=1.0):
    """float32 [B, C, T]: z = L g + mu, mu of ``mean_scale`` standard deviations per channel"""
    g = np.random.default_rng(seed)
    L = mixing(C, seed + 1)
    std = np.sqrt(np.einsum("ck,ck->c", L, L))
    mu = mean_scale * std * g.choice([-1.0, 1.0], C)
    x = np.einsum("ck,bkt->bct", L, g.standard_normal((B, C, T))) + mu[None, :, None]
    return np.ascontiguousarray(x.astype(np.float32))


def frames_of(z, lengths=None):
    """the counted frames of z [B, C, T] as one float64 [C, n]"""
    B, C, T = z.shape
    lengths = [T] * B if lengths is None else lengths
    cols = [z[b, :, :int(lengths[b])].astype(np.float64) for b in range(B)]
    return np.concatenate(cols, axis=1) if cols else np.zeros((C, 0))


def moments(z, lengths=None):
    """(state [1 + C + C C], the same sums over absolute values: what the bound is made of)"""
    x = frames_of(z, lengths)
    C, n = x.shape
    a = np.abs(x)
    state = np.concatenate([[float(n)], x.sum(axis=1), (x @ x.T).reshape(-1)])
    mag = np.concatenate([[0.0], a.sum(axis=1), (a @ a.T).reshape(-1)])
    return state, mag


def moments_bound(n, mag):
    return (n + 2) * U53 * mag


def split(state):
    C = int(round((-1 + np.sqrt(1 + 4 * (state.size - 1))) / 2))
    assert words(C) == state.size
    return state[0], state[1:1 + C], state[1 + C:].reshape(C, C)


def finalize(state, kind="zca", eps=1e-6):
    """(mean, W, W^-1) in float64; W and W^-1 from the same floored spectrum"""
    n, s1, s2 = split(np.asarray(state, dtype=np.float64))
    C = s1.size
    if n < C + 1:
        raise ValueError("too few frames")
    mean = s1 / n
    cov = s2 / n - np.outer(mean, mean)
    cov = 0.5 * (cov + cov.T)
    if kind == "diag":
        var = np.diag(cov)
        std = np.sqrt(np.maximum(var, eps * var.max()))
        return mean, np.diag(1.0 / std), np.diag(std)
    lam, U = np.linalg.eigh(cov)
    root = np.sqrt(np.maximum(lam, eps * lam.max()))
    if kind == "zca":
        return mean, (U / root) @ U.T, (U * root) @ U.T
    if kind == "pca":
        return mean, U.T / root[:, None], U * root
    raise ValueError(kind)


def affine(z, A, pre=None, post=None):
    """(y, bound) in float64 for z [B, C, T]: y = A (z - pre) + post with the operands as given (float32 values, float64 arithmetic)"""
    z = np.asarray(z, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    C = A.shape[0]
    d = z if pre is None else z - np.asarray(pre, dtype=np.float64)[None, :, None]
    y = np.einsum("ck,bkt->bct", A, d)
    if post is not None:
        y = y + np.asarray(post, dtype=np.float64)[None, :, None]
    bound = (C + 3) * U24 * np.einsum("ck,bkt->bct", np.abs(A), np.abs(d)) + 2 * U24 * np.abs(y)
    return y, bound


def sample_cov(x):
    """x [C, n] -> covariance with the 1 / n rule of the fit"""
    m = x.mean(axis=1, keepdims=True)
    return (x - m) @ (x - m).T / x.shape[1]
