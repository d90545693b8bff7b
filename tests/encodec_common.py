"""Float64 references of the Encodec pieces, kernel by kernel; importable without a GPU (tests/test_encodec_refs_host.py pins them,
tests/test_gpu_encodec_kernels.py uses them).

``lstm_layer_ref`` is ONE layer of the recurrence with the input projection already applied (what ``jen1_lstm_layer`` and
``jen1_lstm_layer_multi`` compute); ``oracle.encodec_oracle.slstm`` is the float32, fused, two-layer form and stays as it is.
``lstm_layer_emul`` restates the same recurrence in float32 (optionally with h split into a bf16 high + low part, as the matrix-core
kernel stages it): its error against the float64 layer is the yardstick the GPU gates are multiples of.  The SEANet wrappers call the
oracle's own functions on float64 arrays (every one of them keeps the dtype it is given).
"""
import json

import numpy as np
import torch

from helpers import SEED, golden
from jen1_amd.init_fill import fill
from oracle import encodec_oracle as EO


def bf16_round(a) -> np.ndarray:
    """round-to-nearest-even to bfloat16 and back (float32 array)"""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# LSTM layer
# ---------------------------------------------------------------------------------------------------------------------
def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_layer_ref(gin, whh, skip=None) -> np.ndarray:
    """one LSTM layer in float64: gin [B, T, 4H] (input projection + both biases), whh [4H, H]; gate order i, f, g, o (torch.nn.LSTM);
    zero initial state; returns h_t (+ skip) as [B, T, H]"""
    gin = np.asarray(gin, dtype=np.float64)
    w_t = np.asarray(whh, dtype=np.float64).T.copy()
    B, T, G = gin.shape
    H = G // 4
    assert w_t.shape == (H, G)
    h = np.zeros((B, H))
    c = np.zeros((B, H))
    out = np.empty((B, T, H))
    for t in range(T):
        g = gin[:, t] + h @ w_t
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        out[:, t] = h
    return out if skip is None else out + np.asarray(skip, dtype=np.float64)


def lstm_layer_emul(gin, whh, skip=None, split_h: bool = False) -> np.ndarray:
    """the same layer with every operation in float32 (numpy); ``split_h``: the recurrent product sees h as a bf16 high part plus a
    bf16 low part (two float32 products), which is what the matrix-core kernel does.  Nothing is rounded to bf16 at the end."""
    f32 = np.float32
    gin = np.asarray(gin, dtype=f32)
    w_t = np.ascontiguousarray(np.asarray(whh, dtype=f32).T)
    B, T, G = gin.shape
    H = G // 4
    one = f32(1.0)
    sig = lambda v: one / (one + np.exp(-v))      # noqa: E731
    h = np.zeros((B, H), dtype=f32)
    c = np.zeros((B, H), dtype=f32)
    out = np.empty((B, T, H), dtype=f32)
    for t in range(T):
        if split_h:
            hi = bf16_round(h)
            lo = bf16_round(h - hi)
            g = gin[:, t] + (hi @ w_t + lo @ w_t)
        else:
            g = gin[:, t] + h @ w_t
        i, f, gg, o = sig(g[:, :H]), sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), sig(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
        out[:, t] = h
    assert out.dtype == f32
    return out if skip is None else out + np.asarray(skip, dtype=f32)


def lstm_inputs(B: int, T: int, H: int, seed: int):
    """gin ~ N(0, 1), whh ~ U(-1, 1) / sqrt(H), skip ~ N(0, 1) as float32 arrays"""
    g = torch.Generator().manual_seed(seed)
    gin = torch.randn((B, T, 4 * H), generator=g)
    whh = (torch.rand((4 * H, H), generator=g) * 2.0 - 1.0) * H ** -0.5
    skip = torch.randn((B, T, H), generator=g)
    return gin.numpy(), whh.numpy(), skip.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# residual vector quantizer decode
# ---------------------------------------------------------------------------------------------------------------------
def rvq_decode_ref(codes, tables, magnitude: bool = False) -> np.ndarray:
    """codes int [n_q', B, T], tables [n_q, bins, D] -> float64 [B, D, T]: the sum over the codebooks of the looked-up entries
    (``magnitude``: of their absolute values, the scale of a summation bound); codes are clamped to [0, bins - 1], which is what the
    kernel does with an out-of-range code"""
    codes = np.asarray(codes)
    tables = np.asarray(tables, dtype=np.float64)
    n_q, bins, D = tables.shape
    assert codes.shape[0] <= n_q
    idx = np.clip(codes, 0, bins - 1)
    out = np.zeros((codes.shape[1], codes.shape[2], D))
    for q in range(codes.shape[0]):
        e = tables[q][idx[q]]
        out += np.abs(e) if magnitude else e
    return out.transpose(0, 2, 1)


# ---------------------------------------------------------------------------------------------------------------------
# SEANet blocks on float64 arrays [B, C, L]
# ---------------------------------------------------------------------------------------------------------------------
def dec_params():
    g = golden("encodec")
    return {k: fill("encodec.decoder." + k, tuple(s), SEED) for k, s in json.loads(str(g["schema"]))}


def enc_params():
    g = golden("encodec")
    return {k: fill("encodec.encoder." + k, tuple(s), SEED) for k, s in json.loads(str(g["enc_schema"]))}


def _p64(p, name, round_weight):
    """the float64 parameters of block ``name``; ``round_weight``: the convolution weight as the bf16 mode sees it (bias and the
    norm's affine stay float32 in both modes)"""
    q = {k: np.asarray(v, dtype=np.float64) for k, v in p.items() if k.startswith(name + ".")}
    if round_weight:
        q[f"{name}.conv.weight"] = bf16_round(p[f"{name}.conv.weight"]).astype(np.float64)
    return q


def sconv1d64(x, p, name, stride: int = 1, round_weight: bool = False):
    x = np.asarray(x, dtype=np.float64)
    q = _p64(p, name, round_weight)
    y = EO.sconv1d(x, q, name) if stride == 1 else EO.sconv1d_strided(x, q, name, stride)
    assert y.dtype == np.float64
    return y


def sconv_transpose1d64(x, p, name, stride: int, round_weight: bool = False):
    y = EO.sconv_transpose1d(np.asarray(x, dtype=np.float64), _p64(p, name, round_weight), name, stride)
    assert y.dtype == np.float64
    return y


def elu64(x):
    y = EO.elu(np.asarray(x, dtype=np.float64))
    assert y.dtype == np.float64
    return y


def group_norm64(x, gamma, beta, eps: float = 1e-5):
    y = EO.group_norm(np.asarray(x, dtype=np.float64), 1, np.asarray(gamma, dtype=np.float64), np.asarray(beta, dtype=np.float64), eps)
    assert y.dtype == np.float64
    return y
