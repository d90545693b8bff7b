"""The float64 oracle of the true-peak tests: ITU-R BS.1770-4 Annex 2 read as an F-fold interpolator, and the look-ahead limiter on
its envelope, restated in numpy and independent of jen1_amd/audio.py -- the filter from its formula (the Kaiser window through
``np.i0``), the oversampling as zero-stuffing and one convolution, the hold as a sliding window, the release as a literal loop over time
(vectorised across signals, not across time, as ``loudness_common.k_weight``), the attack as one convolution."""
import math

import numpy as np

TAPS = 16          # per phase
BETA = 8.0


def factor(sr):
    return 4 if sr < 80000 else 2 if sr < 160000 else 1


def prototype(F):
    """h[i] = sinc((i - F T / 2) / F) kaiser(F T + 1, beta)[i], i = 0 .. F T"""
    n = F * TAPS
    i = np.arange(n + 1, dtype=np.float64)
    t = (i - n / 2) / F
    tz = np.where(t == 0, 1.0, t)
    sinc = np.where(t == 0, 1.0, np.sin(np.pi * tz) / (np.pi * tz))
    alpha = n / 2.0
    kaiser = np.i0(BETA * np.sqrt(1.0 - ((i - alpha) / alpha) ** 2)) / np.i0(BETA)
    return sinc * kaiser


def phases(F):
    """[F - 1, T]: phase p = 1 .. F - 1, h_p[k] = h[p + k F]"""
    h = prototype(F)
    return np.array([[h[p + k * F] for k in range(TAPS)] for p in range(1, F)], dtype=np.float64).reshape(F - 1, TAPS)


def oversample(x, F):
    """x [S, L] -> o [S, L F] float64: zeros between the samples, one convolution with the prototype, the delay of F T / 2 taken off;
    o[n F] = x[n] exactly (phase 0 of the prototype is the identity up to sinc(integer) ~ 1e-17)"""
    x = np.asarray(x, dtype=np.float64)
    S, L = x.shape
    h = prototype(F)
    z = np.zeros((S, L * F))
    z[:, ::F] = x
    half = F * TAPS // 2
    o = np.stack([np.convolve(z[s], h)[half:half + L * F] for s in range(S)])
    o[:, ::F] = x
    return o


def envelope(x, sr):
    """x [C, L] -> env [L]: max over the channels and the F phases behind each sample of |o|"""
    F = factor(sr)
    x = np.asarray(x, dtype=np.float64)
    return np.abs(oversample(x, F)).reshape(x.shape[0], x.shape[1], F).max(axis=(0, 2))


def db(v):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(v)


def true_peak(x, sr):
    """x [C, L] -> dBTP (``-inf`` for silence)"""
    return float(db(envelope(x, sr).max()))


def lookahead(ms, sr):
    return int(round(ms * sr / 1000.0))


def rho_of(release_ms, sr):
    tau = release_ms * sr / 1000.0
    return math.exp(-1.0 / tau) if tau > 0 else 0.0


def hold(q, A):
    """q [S, L] -> Q [S, L + A]: Q[:, i + A] = max q[max(i, 0) .. min(i + A, L - 1)] for i = -A .. L - 1"""
    q = np.asarray(q, dtype=np.float64)
    S, L = q.shape
    qp = np.concatenate([np.zeros((S, A)), q, np.zeros((S, A))], axis=1)            # q >= 0: zeros never win
    return np.lib.stride_tricks.sliding_window_view(qp, A + 1, axis=1).max(axis=2)


def release(Q, rho):
    """d[i] = max(Q[i], rho d[i - 1]) from d = 0, one step per sample; rho: a float or one per signal [S]"""
    Qt = np.ascontiguousarray(np.asarray(Q, dtype=np.float64).T)
    out = np.empty_like(Qt)
    d = np.zeros(Qt.shape[1])
    for i in range(Qt.shape[0]):
        d = np.maximum(Qt[i], rho * d)
        out[i] = d
    return np.ascontiguousarray(out.T)


def window(A):
    j = np.arange(A + 1, dtype=np.float64)
    w = np.sin(np.pi * (j + 1.0) / (A + 2.0)) ** 2
    return w / w.sum()


def reduction(env, c, A, rho):
    """env [S, L] -> 1 - s [S, L], and d [S, L + A]"""
    env = np.asarray(env, dtype=np.float64)
    with np.errstate(divide="ignore"):
        q = 1.0 - np.minimum(1.0, c / env)
    d = release(hold(q, A), rho)
    w = window(A)
    L = env.shape[1]
    g = np.zeros_like(env)
    for j in range(A + 1):                                     # s[n] = 1 - sum_j w[j] d[n - j]; d of sample i sits at column i + A
        g += w[j] * d[:, A - j:A - j + L]
    return g, d


def limit(u, sr, ceiling_dbtp=-1.0, A=72, rho=None, release_ms=100.0):
    """u [C, L] float32 -> (y float32 [C, L], 1 - s float64 [L], env float64 [L])"""
    u = np.asarray(u, dtype=np.float32)
    rho = rho_of(release_ms, sr) if rho is None else rho
    env = envelope(u, sr)
    g, _ = reduction(env[None], 10.0 ** (ceiling_dbtp / 20.0), A, rho)
    y = ((1.0 - g) * u.astype(np.float64)).astype(np.float32)
    return y, g[0], env


# ------------------------------------------------------------------ known-answer tones
def faded_tone(freq, phase=0.0, n=9600, sr=48000, fade=480):
    """a full-scale tone with raised-cosine fades of ``fade`` samples at both ends (without them the onset rings above the tone)"""
    t = np.arange(n, dtype=np.float64)
    x = np.sin(2.0 * np.pi * freq * t / sr + phase)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(fade) + 0.5) / fade)
    x[:fade] *= ramp
    x[-fade:] *= ramp[::-1]
    return x


def loud_signals(n=12000, sr=48000):
    """[3, n] float32: uniform noise 12 dB over full scale, Gaussian noise (sigma 1), 50 Hz + 15 kHz at 1.5 each"""
    rng = np.random.default_rng(17702)
    t = np.arange(n, dtype=np.float64) / sr
    return np.stack([(rng.random(n) * 2.0 - 1.0) * 10.0 ** (12.0 / 20.0), rng.standard_normal(n),
                     1.5 * np.sin(2 * np.pi * 50.0 * t) + 1.5 * np.sin(2 * np.pi * 15000.0 * t + 0.3)]).astype(np.float32)
