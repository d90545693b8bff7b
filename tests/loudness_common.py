"""The float64 oracle of the loudness tests: ITU-R BS.1770-4 integrated loudness with every channel weight 1.0, restated in numpy and
independent of jen1_amd/audio.py -- the coefficient formulas, a literal sample-by-sample biquad cascade (vectorised across signals, not
across time), the gate as the standard writes it, and the gain rules of ``normalize_audio``."""
import math

import numpy as np

ABSOLUTE_GATE = -70.0
DEFAULT_HEADROOM_DB = {"loudness": 0.0, "peak": 1.0, "rms": 18.0, "clip": 0.0}


def coefficients(sr):
    """[2, 6] float64: (b0, b1, b2, 1, a1, a2) of the high shelf and of the high-pass"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K ** 2
    shelf = [(Vh + Vb * K / Q + K ** 2) / a0, 2.0 * (K ** 2 - Vh) / a0, (Vh - Vb * K / Q + K ** 2) / a0,
             1.0, 2.0 * (K ** 2 - 1.0) / a0, (1.0 - K / Q + K ** 2) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K ** 2
    return np.array([shelf, [1.0, -2.0, 1.0, 1.0, 2.0 * (K ** 2 - 1.0) / a0, (1.0 - K / Q + K ** 2) / a0]], dtype=np.float64)


def k_weight(x, sos):
    """x [S, L] float64 through the cascade, zero state at sample 0 -> y [S, L].  sos: [2, 6] for every signal or [S, 2, 6] per signal.
    Direct form I, one pass over the samples:  y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2] - a1 y[n-1] - a2 y[n-2]  for each section."""
    x = np.asarray(x, dtype=np.float64)
    S, L = x.shape
    sos = np.broadcast_to(np.asarray(sos, dtype=np.float64), (S, 2, 6))
    b0, b1, b2, a1, a2 = (np.ascontiguousarray(sos[:, 0, i]) for i in (0, 1, 2, 4, 5))
    c0, c1, c2, d1, d2 = (np.ascontiguousarray(sos[:, 1, i]) for i in (0, 1, 2, 4, 5))
    xt = np.ascontiguousarray(x.T)
    out = np.empty_like(xt)
    z = np.zeros(S)
    x1, x2, u1, u2, y1, y2 = z, z, z, z, z, z
    for n in range(L):
        x0 = xt[n]
        u0 = b0 * x0 + b1 * x1 + b2 * x2 - a1 * u1 - a2 * u2
        y0 = c0 * u0 + c1 * u1 + c2 * u2 - d1 * y1 - d2 * y2
        out[n] = y0
        x2, x1, u2, u1, y2, y1 = x1, x0, u1, u0, y1, y0
    return np.ascontiguousarray(out.T)


def hop_energies(y, hop):
    """y [..., L] -> [..., H]: the sum of y^2 over each complete hop"""
    H = y.shape[-1] // hop
    return (y[..., :H * hop].reshape(y.shape[:-1] + (H, hop)) ** 2).sum(axis=-1)


def block_powers(e, hop):
    """e [C, H] -> s [J]: the mean square of every 400 ms block (4 hops, 75 % overlap) summed over the channels"""
    C, H = e.shape
    J = max(0, H - 3)
    z = (e[:, 0:J] + e[:, 1:J + 1] + e[:, 2:J + 2] + e[:, 3:J + 3]) / (4.0 * hop)
    return z.sum(axis=0)


def lk(s):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(s)


def gate(e, hop, details=False):
    """e [C, H] -> integrated loudness; with ``details`` also (l [J], the relative threshold or None)"""
    s = block_powers(np.asarray(e, dtype=np.float64), hop)
    l = lk(s) if s.size else np.zeros(0)
    A = l > ABSOLUTE_GATE
    gamma, out = None, -math.inf
    if A.any():
        gamma = float(lk(s[A].mean())) - 10.0
        Gs = A & (l > gamma)
        if Gs.any():
            out = float(lk(s[Gs].mean()))
    return (out, l, gamma) if details else out


def gate_margin(e, hop):
    """the least distance in LU of any block from the two thresholds (inf when there is no block or no threshold)"""
    _, l, gamma = gate(e, hop, details=True)
    l = l[np.isfinite(l)]
    if l.size == 0:
        return math.inf
    m = float(np.abs(l - ABSOLUTE_GATE).min())
    if gamma is not None:
        m = min(m, float(np.abs(l - gamma).min()))
    return m


def ungated(e, hop):
    """the plain mean over all hops (no blocks, no gate)"""
    e = np.asarray(e, dtype=np.float64)
    return float(lk(e.sum() / (e.shape[1] * hop)))


def integrated(x, sr, details=False):
    """x [C, L] -> LUFS, through the literal filter (slow: one numpy step per sample)"""
    hop = sr // 10
    e = hop_energies(k_weight(np.asarray(x, dtype=np.float64), coefficients(sr)), hop)
    return (gate(e, hop), e) if details else gate(e, hop)


def gain(strategy, x, lufs=None, target=-14.0, headroom_db=None, energy_floor=2e-3):
    """the gain of one row x [C, L] in float64, not rounded"""
    x = np.asarray(x, dtype=np.float64)
    head = DEFAULT_HEADROOM_DB[strategy] if headroom_db is None else headroom_db
    rms = math.sqrt(float((x ** 2).sum()) / x.size)
    peak = float(np.abs(x).max())
    if strategy == "loudness":
        return 10.0 ** ((target - lufs) / 20.0) if (math.isfinite(lufs) and rms >= energy_floor) else 1.0
    if strategy == "peak":
        return 10.0 ** (-head / 20.0) / peak if peak > 0 else 1.0
    if strategy == "rms":
        return 10.0 ** (-head / 20.0) / rms if rms > 0 else 1.0
    if strategy == "clip":
        return 1.0
    raise ValueError(strategy)


# ------------------------------------------------------------------ known-answer signals (997 Hz at 48 kHz, 5 s)
KAT_SR = 48000


def tone(amplitude, seconds=5.0, sr=KAT_SR):
    return amplitude * np.sin(2.0 * np.pi * 997.0 * np.arange(int(round(seconds * sr))) / sr)


def gating_signal(sr=KAT_SR):
    """the tone at -60 dBFS for 1 s, -20 for 2 s, -40 for 1 s, then 1 s of zeros"""
    t = tone(1.0, 5.0, sr)
    env = np.concatenate([np.full(sr, 10 ** (-60 / 20)), np.full(2 * sr, 10 ** (-20 / 20)), np.full(sr, 10 ** (-40 / 20)), np.zeros(sr)])
    return t * env


_KAT = {}


def kat_energies():
    """hop energies [H] of one channel of: the tone at -23 dBFS, the tone at full scale, the gating signal -- one pass of the literal
    filter over the three, cached"""
    if not _KAT:
        x = np.stack([tone(10 ** (-23 / 20)), tone(1.0), gating_signal()])
        e = hop_energies(k_weight(x, coefficients(KAT_SR)), KAT_SR // 10)
        _KAT.update(tone23=e[0], tone0=e[1], gating=e[2])
    return _KAT


# ------------------------------------------------------------------ the signals of the kernel tests: one array, one pass, cached
_BANK = {}


def bank(lengths):
    """``lengths``: {sr: samples}.  Per rate, float32 base signals [12, n] -- 6 channels uniform in +-0.5 around a DC offset of 0.25, and
    6 more whose samples [2 hop, 3.5 hop) are 1000 x quieter -- and, at 48 kHz only, a unit impulse at sample 0 and a constant 0.5 of 2 s.
    Returns {name: (x float32 [S, n], y float64 [S, n])} with names ("base", sr) and "carry".  The filter is causal: the reference for
    a signal cut to its first L samples is the first L samples of y."""
    key = tuple(sorted(lengths.items()))
    if key in _BANK:
        return _BANK[key]
    rng = np.random.default_rng(1770)
    parts, sos, names = [], [], []
    for sr, n in sorted(lengths.items()):
        hop = sr // 10
        x = (rng.random((12, n)) - 0.5 + 0.25).astype(np.float32)
        x[6:, 2 * hop:3 * hop + hop // 2] *= np.float32(1e-3)
        parts.append(x)
        sos += [coefficients(sr)] * 12
        names.append((("base", sr), 12, n))
    carry = np.zeros((2, 2 * 48000), dtype=np.float32)
    carry[0, 0] = 1.0
    carry[1, :] = 0.5
    parts.append(carry)
    sos += [coefficients(48000)] * 2
    names.append(("carry", 2, carry.shape[1]))
    longest = max(p.shape[1] for p in parts)
    allx = np.zeros((sum(p.shape[0] for p in parts), longest), dtype=np.float64)
    r = 0
    for p in parts:
        allx[r:r + p.shape[0], :p.shape[1]] = p
        r += p.shape[0]
    ally = k_weight(allx, np.stack(sos))
    out, r = {}, 0
    for (name, S, n), p in zip(names, parts):
        y = ally[r:r + S, :n]
        y.setflags(write=False)
        out[name] = (p, y)
        r += S
    _BANK[key] = out
    return out
