"""Checkers of the Frechet Audio Distance (jen1_amd/fad.py, csrc/vggish.hip), restated without the package from the description of
VGGish's published pipeline: the front end in numpy (frames cut by slicing, ``np.fft.rfft``, the mel matrix by a plain loop) and the
network as a ``torch.nn`` model on the CPU.  Each runs in float64 (the truth) and in float32, which serves only to size tolerances: a
kernel is allowed 8x the error that the float32 chain itself makes on the same input against float64."""
import math

import numpy as np
import torch
from torch import nn

TOL_FACTOR = 8.0
SR16 = 16000
WIN, HOP, N_FFT, FRAMES, BANDS = 400, 160, 512, 96, 64
NARROW = dict(channels=(16, 32, 48, 64), hidden=256, dim=128)
FULL = dict(channels=(64, 128, 256, 512), hidden=4096, dim=128)


# ------------------------------------------------------------------ front end
def mel_matrix_loop() -> np.ndarray:
    """[64, 257] float64, entry by entry"""
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    lo_m, hi_m = mel(125.0), mel(7500.0)
    edges = [lo_m + (hi_m - lo_m) * i / 65.0 for i in range(66)]
    out = np.zeros((BANDS, N_FFT // 2 + 1))
    for k in range(1, N_FFT // 2 + 1):
        m = mel(8000.0 * k / (N_FFT // 2))
        for i in range(BANDS):
            lo, c, hi = edges[i], edges[i + 1], edges[i + 2]
            out[i, k] = max(0.0, min((m - lo) / (c - lo), (hi - m) / (hi - c)))
    return out


def count(n: int) -> int:
    return (1 + (n - WIN) // HOP) // FRAMES if n >= WIN else 0


def examples(x: np.ndarray, dtype=np.float64) -> np.ndarray:
    """x [n] at 16 kHz -> log-mel examples [N, 96, 64] in ``dtype`` (the signal is the float32 one either way)"""
    x = np.asarray(x).astype(dtype)
    n = x.shape[0]
    if n < WIN:
        return np.zeros((0, FRAMES, BANDS), dtype=dtype)
    nf = 1 + (n - WIN) // HOP
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN, dtype=np.float64) / WIN)).astype(np.float32).astype(dtype)   # the float32 table
    frames = np.stack([x[HOP * k:HOP * k + WIN] for k in range(nf)]) * window
    spec = np.abs(np.fft.rfft(frames.astype(dtype), N_FFT, axis=1))
    if dtype == np.float32:
        spec = spec.astype(np.float32)             # (numpy's FFT of float32 input may run in float64: round where float32 would)
    fb = mel_matrix_loop().astype(np.float32).astype(dtype)         # the kernel's weights are the float32 roundings
    logmel = np.log(spec @ fb.T + dtype(0.01)).astype(dtype)
    N = nf // FRAMES
    return logmel[:N * FRAMES].reshape(N, FRAMES, BANDS)


def mix(n: int, seed: int, sr: int = SR16) -> np.ndarray:
    """float32 [n]: tones and noise over a -80 dB bed, seeded"""
    rng = np.random.default_rng([seed, n])
    t = np.arange(n, dtype=np.float64) / sr
    x = 1e-4 * rng.standard_normal(n)
    for f in rng.uniform(80.0, 7000.0, size=4):
        x += rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28))
    x += 0.05 * rng.standard_normal(n) * (0.5 + 0.5 * np.sin(2 * np.pi * 1.5 * t))
    return x.astype(np.float32)


# ------------------------------------------------------------------ network
class VGGishModel(nn.Module):
    """the layer list of the common PyTorch port: ``features`` (indices 0, 3, 6, 8, 11, 13 are the convolutions) and ``embeddings``"""

    def __init__(self, channels=(64, 128, 256, 512), hidden=4096, dim=128, final_relu=False, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        c1, c2, c3, c4 = channels
        conv = lambda i, o: nn.Conv2d(i, o, 3, padding=1)
        self.features = nn.Sequential(
            conv(1, c1), nn.ReLU(), nn.MaxPool2d(2, 2),
            conv(c1, c2), nn.ReLU(), nn.MaxPool2d(2, 2),
            conv(c2, c3), nn.ReLU(), conv(c3, c3), nn.ReLU(), nn.MaxPool2d(2, 2),
            conv(c3, c4), nn.ReLU(), conv(c4, c4), nn.ReLU(), nn.MaxPool2d(2, 2))
        layers = [nn.Linear(6 * 4 * c4, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, dim)]
        if final_relu:
            layers.append(nn.ReLU())
        self.embeddings = nn.Sequential(*layers)
        with torch.no_grad():                       # biases large enough to matter in every layer
            for m in self.modules():
                if isinstance(m, (nn.Conv2d, nn.Linear)):
                    m.bias.uniform_(-0.1, 0.1)

    def forward(self, x):
        """x [N, 96, 64] -> [N, dim]"""
        x = self.features(x[:, None])
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)          # (h, w, c)
        return self.embeddings(x)


def run_model(model: VGGishModel, ex: np.ndarray, dtype) -> np.ndarray:
    import copy
    m = copy.deepcopy(model).to(dtype)
    with torch.no_grad():
        return m(torch.from_numpy(np.ascontiguousarray(ex)).to(dtype)).numpy()


def conv_ref(x: np.ndarray, w: np.ndarray, b: np.ndarray, pool: bool, dtype=torch.float64):
    """x [N, H, W, Cin], w [Cout, Cin, 3, 3], b [Cout] -> (relu(conv) (+ pool) [N, H', W', Cout], the same sums on absolute values)"""
    F = torch.nn.functional
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).permute(0, 3, 1, 2)
    wt, bt = torch.from_numpy(w).to(dtype), torch.from_numpy(b).to(dtype)
    y = F.relu(F.conv2d(xt, wt, bt, padding=1))
    mag = F.conv2d(xt.abs(), wt.abs(), bt.abs(), padding=1)
    if pool:
        y, mag = F.max_pool2d(y, 2, 2), F.max_pool2d(mag, 2, 2)
    return y.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()


def rel_max(got: np.ndarray, want: np.ndarray) -> float:
    """max |got - want| over the largest |want|"""
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


# ------------------------------------------------------------------ distance
def frechet_np(ea: np.ndarray, eb: np.ndarray, sqrtm=None) -> float:
    """the distance from two sets of embeddings [n, d] by ``np.mean`` / ``np.cov``; the matrix root by ``sqrtm`` (scipy's) when given, else by
    the symmetric form"""
    mu_a, mu_b = ea.mean(0), eb.mean(0)
    Sa, Sb = np.cov(ea, rowvar=False), np.cov(eb, rowvar=False)
    d = mu_a - mu_b
    if sqrtm is not None:
        tr = np.trace(sqrtm(Sa @ Sb).real)
    else:
        lam, U = np.linalg.eigh(Sa)
        R = (U * np.sqrt(np.maximum(lam, 0))) @ U.T
        tr = np.sqrt(np.maximum(np.linalg.eigvalsh(R @ Sb @ R), 0)).sum()
    return float(d @ d + np.trace(Sa) + np.trace(Sb) - 2.0 * tr)
