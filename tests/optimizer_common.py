"""Float64 references, float32 restatements, gates and case tables of the optimiser kernels (csrc/optimizer.hip: jen1_grad_sqnorm,
jen1_grad_sqnorm_ws, jen1_adamw_step, jen1_adamw_step_counted, jen1_adamw_ema_step_counted); importable without a GPU.
tests/test_optimizer_refs_host.py pins the references against torch.optim.AdamW + clip_grad_norm_ in float64 and ema.ema_schedule and shows
that the gates reject wrong kernels; tests/test_gpu_optimizer_forms.py runs the same cases through the C ABI.

Reference of ONE call, in float64 on the operands as the kernel sees them (float32 p, g, m, v, ema; float32 lr, beta1, beta2, eps,
weight_decay, max_norm; double EMA settings; the float32 scalar S = gnorm_sq[0]), written from the reference project's lines
(nn.utils.clip_grad_norm_ then torch.optim.AdamW.step, trainer.py:144-149, train.py:56-60):

    skipped  = skip_nonfinite and S given and sqrt(S) not finite        -> p, m, v, ema, counter untouched
    coef     = min(1, max_norm / (sqrt(S) + 1e-6))                      (1 without S or with max_norm <= 0)
    g'       = coef g
    p1       = p (1 - lr wd)                                            decoupled decay, before the update
    m'       = beta1 m + (1 - beta1) g'
    v'       = beta2 v + (1 - beta2) g'^2
    denom    = sqrt(v') / sqrt(bc2) + eps,  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t,  t = the step being taken (1-based)
    p'       = p1 - (lr / bc1) m' / denom
    ema'     = ema | p' | ema + (1 - decay)(p' - ema)                   by the schedule of step t (ema.ema_schedule)

Every step is teacher-forced: the state a case starts from is data, so a gate measures one step and no drift.

Gates per element, with u = 2^-24 (half an ulp, the relative error of one rounded float32 operation) and the roundings counted along
adam1 of the kernel without contraction (a contracted multiply-add has one rounding fewer):

    coef : sqrtf 1 + the add of 1e-6 1 + the constant 1e-6f 0.5 + the division 1                      = 3.5 u     (relative)
    g'   : coef 3.5 + the product 1                                                                   = 4.5 u
    m'   : beta1 m: 1.  (1 - beta1) g': 1 (the difference) + 4.5 + 1 = 6.5.  The sum: 1 on |m'| <= S_m.
           |m' - ref| <= (6.5 + 1) u S_m                                                              -> C_M = 8
    v'   : beta2 v: 1.  ((1 - beta2) g') g': 1 + 2 x 4.5 + 2 = 12.  The sum: 1.  <= 13 u S_v           -> C_V = 13
    p'   : p1: lr wd 1, 1 - x 1, the product 1 = 3 on |p1|.
           m' / denom (lr / bc1): m' 7.5 u S_m;  relative to |m'| <= S_m: denom (v' 13 / 2 = 6.5, sqrtf 1, the float32 bias correction 1,
           the product 1, the add of eps 1 = 10.5), the quotient 1, lr / bc1 (bc1 to float32 1, the division 1 = 2), the product 1:
           (7.5 + 10.5 + 1 + 2 + 1) = 22 on T = (lr / bc1) S_m / denom.  The difference: 1 on |p'| <= S_p.
           |p' - ref| <= 3 u |p1| + 22 u T + 1 u S_p <= 23 u S_p                                      -> C_P = 24 (second-order terms)

with S_m = |beta1 m| + |(1 - beta1) g'|, S_v = |beta2 v| + (1 - beta2) g'^2, S_p = |p (1 - lr wd)| + (lr / bc1) S_m / denom: the
second term of S_p carries the cancellation in m through to the step.  The EMA: 4 ulp max(|e|, |p'|) as tests/test_gpu_ema.py (w to
float32, the difference, the fma: 3 roundings of at most that size).  Every gate carries the 2^-102 floor of train_ops_common (a result in
the denormal range may be flushed).

Sum of squares: the terms are non-negative, so every float32 addition on the way from a term to the result adds at most u x the result:
gate = (chain + 2) u ref, chain = the longest chain of additions the launch geometry allows (``norm_chain``), + 2 for the square and
the final sum's own rounding.  At the largest size tested (three trips of a full grid) chain + 2 = 54: 3.2e-6 < the 1e-5 that
test_gradient_norm_is_bit_reproducible asks.

Restatements (``adamw_emul``, ``ema_emul``, ``sqnorm_emul``): the same in float32 with every operation rounded, without and with the
multiply-adds contracted, and a ``fault`` that makes them wrong in one of the ways such a kernel goes wrong (ALL_WRONG).
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from train_ops_common import FLOOR, U23, U24

F = np.float32
POWER = 10.0                 # a wrong variant must lie this many gates from the right answer
C_M, C_V, C_P = 8.0, 13.0, 24.0
EMA_ULPS = 4.0
GUARD = 64                   # elements of pattern in front of and behind every buffer (the front keeps the 16-byte alignment)
PATTERN = 0x7FA5C3E1         # a NaN with a payload: survives only if nobody writes it
PASS = 16384 * 256 * 4       # elements one grid-stride pass of adamw_kernel / adamw_ema_kernel covers; the norm's full grid covers as many
NORM_MAX_BLOCKS = 4096
BIG_N = 2 * PASS + 4 * 4099 + 3          # three passes, the last one short, a tail of 3

SKIP, COPY, UPDATE = 0, 1, 2
SCHEDULES = [                # the five of tests/test_gpu_ema.py
    dict(beta=0.999, update_after_step=5, update_every=3, warmup=True, inv_gamma=1.0, power=2.0 / 3.0, min_decay=0.0),
    dict(beta=0.9, update_after_step=0, update_every=1, warmup=True, inv_gamma=1.0, power=0.75, min_decay=0.5),
    dict(beta=0.99, update_after_step=1, update_every=1, warmup=False, inv_gamma=1.0, power=2.0 / 3.0, min_decay=0.0),
    dict(beta=0.9999, update_after_step=100, update_every=10, warmup=True, inv_gamma=1.0, power=2.0 / 3.0, min_decay=0.0),
    dict(beta=0.95, update_after_step=12, update_every=2, warmup=True, inv_gamma=4.0, power=0.5, min_decay=0.1),
]

NORM_WRONG = ["tail_dropped", "last_vector_dropped"]
ADAM_WRONG = ["eps_in_bias_correction", "eps_under_root", "bc2_not_rooted", "step_minus_1", "step_plus_1", "l2_decay", "decay_after_update",
              "clip_without_1e-6", "coef_above_1", "clip_m_not_v", "tail_dropped", "last_vector_dropped", "nan_is_finite"]
EMA_WRONG = ["ema_copy_for_update", "ema_update_for_copy", "ema_k_from_0", "ema_clamps_swapped"]
ALL_WRONG = sorted(set(NORM_WRONG + ADAM_WRONG + ["skipped_step_counted"] + EMA_WRONG))
CAN_MAKE = {                 # entry -> the mistakes it could make (the host-step entry has no counter, the plain entries no EMA)
    "grad_sqnorm": NORM_WRONG,
    "grad_sqnorm_ws": NORM_WRONG,
    "adamw_step": ADAM_WRONG,
    "adamw_step_counted": ADAM_WRONG + ["skipped_step_counted"],
    "adamw_ema_step_counted": ADAM_WRONG + ["skipped_step_counted"] + EMA_WRONG,
}
UPDATE_ENTRIES = ["adamw_step", "adamw_step_counted", "adamw_ema_step_counted"]


# ---------------------------------------------------------------------------------------------------------------------
# the sum of squares
# ---------------------------------------------------------------------------------------------------------------------
def norm_blocks(n: int) -> int:
    """grid of grad_sqnorm_kernel: one block per 256 threads x 4 vectors of 4, at most 4096"""
    return min(max(((n >> 2) + 1023) // 1024, 1), NORM_MAX_BLOCKS)


def norm_chain(n: int) -> int:
    """the longest chain of float32 additions from one g^2 to out[0], read off the kernel: inside a vector (x^2 + y^2) + (z^2 + w^2): 2;
    s += once per vector, 4 vectors per trip of the grid-stride loop; the tail element of block 0: 1; the wave's butterfly: 6; the four
    waves: 4; the last block: one addition per 256 partials, the butterfly 6, the waves 4; out[0] +=: 1"""
    blocks = norm_blocks(n)
    trips = max(1, -(-(n >> 2) // (blocks * 256 * 4)))
    return 2 + 4 * trips + 1 + 6 + 4 + -(-blocks // 256) + 6 + 4 + 1


def sqnorm_ref(g, prior=0.0):
    """-> (float64 sum of squares + the float32 value ``out`` held before, which the call adds to)"""
    return float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) + float(prior)


def norm_gate(n: int, ref: float, extra: int = 0) -> float:
    """``extra``: additions outside the call's own chain (a second call into the same ``out`` puts one more addition, its ``out[0] +=``,
    behind the terms of the first; ``n`` is then the longer of the two)"""
    return (norm_chain(n) + 2 + extra) * U24 * (abs(ref) + FLOOR)


def sqnorm_emul(g, fma=False, fault=None):
    """float32 throughout (numpy's pairwise float32 sum: an order of its own; the kernel's order is gated, not restated)"""
    g = np.asarray(g, dtype=F)
    n = g.size
    nv = n >> 2
    if fault == "tail_dropped":
        g = g[:nv * 4]
    if fault == "last_vector_dropped" and nv:
        g = np.concatenate([g[:(nv - 1) * 4], g[nv * 4:]])
    if fma:                  # x x + y y with one rounding, pair by pair
        q = g.astype(np.float64) ** 2
        if q.size & 1:
            q = np.concatenate([q, [0.0]])
        sq = (q[0::2] + q[1::2]).astype(F)
    else:
        sq = g * g
    with np.errstate(over="ignore", invalid="ignore"):
        return F(np.sum(sq, dtype=F))


# ---------------------------------------------------------------------------------------------------------------------
# the EMA schedule and update
# ---------------------------------------------------------------------------------------------------------------------
def ema_mode_decay(t: int, s: dict, fault=None):
    """(SKIP | COPY | UPDATE, decay) of optimiser step t in float64, restated from ema.ema_schedule"""
    if t % s["update_every"] != 0:
        return SKIP, 0.0
    mode = COPY if t <= s["update_after_step"] else UPDATE
    if fault == "ema_copy_for_update" and mode == UPDATE:
        return COPY, 0.0
    if fault == "ema_update_for_copy" and mode == COPY:
        mode = UPDATE
    if mode == COPY:
        return COPY, 0.0
    decay = float(s["beta"])
    if s["warmup"]:
        k = float(t - s["update_after_step"]) - (1.0 if fault == "ema_k_from_0" else 0.0)
        with np.errstate(all="ignore"):
            decay = float(1.0 - np.power(np.float64(1.0 + k / s["inv_gamma"]), -s["power"]))
        if fault == "ema_clamps_swapped":
            decay = max(min(decay, float(s["min_decay"])), float(s["beta"]))
        else:
            decay = max(min(decay, float(s["beta"])), float(s["min_decay"]))
    return UPDATE, decay


def ema_ref(e, p_new, t, s):
    """-> (float64 expectation, gate) on the kernel's own previous EMA and new parameters; SKIP and COPY are exact"""
    mode, decay = ema_mode_decay(t, s)
    e64, p64 = np.asarray(e, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    if mode == SKIP:
        return e64, np.zeros_like(e64)
    if mode == COPY:
        return p64, np.zeros_like(e64)
    return e64 + (1.0 - decay) * (p64 - e64), EMA_ULPS * U23 * (np.maximum(np.abs(e64), np.abs(p64)) + FLOOR)


def ema_emul(e, p_new, t, s, fma=True, fault=None):
    mode, decay = ema_mode_decay(t, s, fault)
    e, p_new = np.asarray(e, dtype=F), np.asarray(p_new, dtype=F)
    if mode == SKIP:
        return e.copy()
    if mode == COPY:
        return p_new.copy()
    w = F(1.0 - decay)
    with np.errstate(all="ignore"):
        d = p_new - e
        if fma:              # the kernel writes this one as an explicit fma
            return (np.float64(w) * d.astype(np.float64) + e.astype(np.float64)).astype(F)
        return (w * d).astype(F) + e


# ---------------------------------------------------------------------------------------------------------------------
# clip + AdamW
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class HP:
    lr: float = 3e-5
    beta1: float = 0.9
    beta2: float = 0.95
    eps: float = 1e-8
    wd: float = 0.1
    max_norm: float = 0.7

    def f32(self):
        """the six values as the C ABI receives them"""
        return tuple(float(F(x)) for x in (self.lr, self.beta1, self.beta2, self.eps, self.wd, self.max_norm))


def coef_ref(S, max_norm, skip_nonfinite):
    """-> (skipped, coef) in float64.  ``S``: gnorm_sq[0] or None (no scalar given)"""
    if S is None:
        return False, 1.0
    with np.errstate(all="ignore"):
        nrm = float(np.sqrt(np.float64(S)))
    if skip_nonfinite and not math.isfinite(nrm):
        return True, 1.0
    if max_norm > 0.0:
        return False, min(1.0, max_norm / (nrm + 1e-6))
    return False, 1.0


def adamw_ref(p, g, m, v, hp: HP, t: int, S, skip_nonfinite=1):
    """one call in float64 -> dict(skipped, p, m, v, gate_p, gate_m, gate_v).  ``S``: the scalar the kernel reads (float32 value; the pin
    against torch passes the exact float64 sum), or None"""
    lr, b1, b2, eps, wd, max_norm = hp.f32()
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    skipped, coef = coef_ref(S, max_norm, skip_nonfinite)
    if skipped:
        z = np.zeros_like(p)
        return dict(skipped=True, p=p, m=m, v=v, gate_p=z, gate_m=z, gate_v=z)
    gc = g * coef
    p1 = p * (1.0 - lr * wd)
    m1 = b1 * m + (1.0 - b1) * gc
    v1 = b2 * v + (1.0 - b2) * gc * gc
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = np.sqrt(v1) / math.sqrt(bc2) + eps
    p2 = p1 - (lr / bc1) * (m1 / denom)
    S_m = np.abs(b1 * m) + np.abs((1.0 - b1) * gc)
    S_v = np.abs(b2 * v) + (1.0 - b2) * gc * gc
    S_p = np.abs(p1) + (lr / bc1) * S_m / denom
    return dict(skipped=False, p=p2, m=m1, v=v1, gate_p=C_P * U24 * (S_p + FLOOR), gate_m=C_M * U24 * (S_m + FLOOR),
                gate_v=C_V * U24 * (S_v + FLOOR))


def _fma(a, b, c):
    """a b + c with one rounding (the product of two float32 is exact in float64)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def adamw_emul(p, g, m, v, hp: HP, t: int, S, skip_nonfinite=1, fma=False, fault=None):
    """the kernel's adam1 in float32, operation by operation -> (p, m, v, taken).  ``fma``: the last product of every a b + c contracted"""
    lr, b1, b2, eps, wd, max_norm = (F(x) for x in hp.f32())
    p, g, m, v = (np.array(a, dtype=F) for a in (p, g, m, v))
    n = p.size
    with np.errstate(all="ignore"):
        coef = F(1.0)
        if S is not None:
            nrm = np.sqrt(F(S))
            finite = bool(nrm <= F(3.0e38)) or (fault == "nan_is_finite" and bool(np.isnan(nrm)))
            if skip_nonfinite and not finite:
                return p, m, v, (1 if fault == "skipped_step_counted" else 0)
            if max_norm > 0:
                c = max_norm / (nrm + (F(0.0) if fault == "clip_without_1e-6" else F(1e-6)))
                coef = c if (c < F(1.0) or fault == "coef_above_1") else F(1.0)
        tt = float(t + {"step_minus_1": -1, "step_plus_1": 1}.get(fault, 0))
        bc1 = F(1.0 - float(b1) ** tt)
        bc2d = 1.0 - float(b2) ** tt
        isb2 = F(1.0 / bc2d) if fault == "bc2_not_rooted" else F(1.0 / np.sqrt(np.float64(bc2d)))
        p0, m0, v0 = p.copy(), m.copy(), v.copy()
        gc = g * coef
        gv = g if fault == "clip_m_not_v" else gc
        if fault == "l2_decay":
            gc = gc + wd * p
            gv = gc
        elif fault != "decay_after_update":
            p = p * (F(1.0) - lr * wd)
        omb1, omb2 = F(1.0) - b1, F(1.0) - b2
        if fma:
            m = _fma(omb1, gc, b1 * m)
            v = _fma(omb2 * gv, gv, b2 * v)
        else:
            m = b1 * m + omb1 * gc
            v = b2 * v + (omb2 * gv) * gv
        if fault == "eps_in_bias_correction":
            denom = (np.sqrt(v) + eps) * isb2
        elif fault == "eps_under_root":
            denom = np.sqrt(v * isb2 * isb2 + eps)
        elif fma:
            denom = _fma(np.sqrt(v), isb2, eps)
        else:
            denom = np.sqrt(v) * isb2 + eps
        q = m / denom
        step = lr / bc1
        p = _fma(-step, q, p) if fma else p - step * q
        if fault == "decay_after_update":
            p = p * (F(1.0) - lr * wd)
    nv = n >> 2
    lo, hi = {"tail_dropped": (nv * 4, n), "last_vector_dropped": (max(nv - 1, 0) * 4, nv * 4)}.get(fault, (0, 0))
    p[lo:hi], m[lo:hi], v[lo:hi] = p0[lo:hi], m0[lo:hi], v0[lo:hi]
    return p, m, v, 1


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    n: int
    t: int = 3                       # the step being taken; the device counter holds t - 1
    p_kind: str = "normal"           # normal: N(0, 1); zero: exactly 0; lr: N(0, 1) lr
    g_scale: float = 1e-2
    clip: str = "above"              # below | above | edge_lo | edge_hi | tiny | off | off_neg | null
    lr: float = 1e-2
    wd: float = 0.1
    bad: Optional[str] = None        # inf_vec | nan_vec | inf_tail | nan_tail: one non-finite gradient element
    skip: int = 1
    sched: int = 1


SIZES = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1027, 4095, 4096, 4097, 8192 + 5, 257 * 4096 + 3]
STEPS = [1, 2, 3, 10, 5000, 10 ** 6]
G_SCALES = [1e-9, 1e-6, 1e-3, 1e-2, 1.0, 10.0]
CLIPS = ["below", "above", "edge_lo", "edge_hi", "tiny", "off", "off_neg", "null"]


def _cases():
    out = []
    for i, n in enumerate(SIZES):                                    # every size, one ordinary step each
        out.append(Case(f"n{n}", n, t=3, sched=i % 5, wd=(0.0, 0.1, 0.5)[i % 3], clip=("above", "below")[i % 2]))
    k = 0
    for t in STEPS:                                                  # optimiser state x parameter kind, the other axes cycling
        for pk in ("normal", "zero", "lr"):
            out.append(Case(f"t{t}.p-{pk}", 1027, t=t, p_kind=pk, g_scale=G_SCALES[k % 6], clip=CLIPS[k % 4], lr=(3e-5, 1e-2)[k % 2],
                            wd=(0.0, 0.1, 0.5)[k % 3], sched=k % 5))
            k += 1
    for j, gs in enumerate(G_SCALES):                                # the gradient's scale against eps, at p = 0 and p ~ lr
        out.append(Case(f"g{gs:g}.p-zero", 1027, t=3, p_kind="zero", g_scale=gs, clip="below", lr=1e-2, wd=0.5, sched=j % 5))
        out.append(Case(f"g{gs:g}.p-lr", 261, t=10, p_kind="lr", g_scale=gs, clip="null", lr=3e-5, wd=0.1, sched=(j + 2) % 5))
    for j, c in enumerate(CLIPS):                                    # every clip regime where the step is not swamped by p
        out.append(Case(f"clip-{c}.t2", 1027, t=2, p_kind="zero", g_scale=1e-2, clip=c, lr=1e-2, wd=0.5, sched=j % 5))
        out.append(Case(f"clip-{c}.t5000", 517, t=5000, p_kind="lr", g_scale=1.0, clip=c, lr=3e-5, wd=0.1, sched=(j + 3) % 5))
    for s in range(5):                                               # every schedule at a step of each kind it has
        for t in (1, 2, 10, 12, 13, 5000):
            out.append(Case(f"ema{s}.t{t}", 259, t=t, p_kind="lr", g_scale=1e-3, clip="above", lr=1e-2, wd=0.1, sched=s))
    for bad in ("inf_vec", "nan_vec", "inf_tail", "nan_tail"):       # a skipped step, clipping on and off
        out.append(Case(f"{bad}.clip", 1027, t=3, bad=bad, clip="above", sched=1))
        out.append(Case(f"{bad}.noclip", 7, t=10, bad=bad, clip="off", sched=2))
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
NORM_CASES = CASES[:len(SIZES)] +[Case(f"norm.g{gs:g}", 4097, g_scale=gs) for gs in G_SCALES]


class Built:
    """the operands of a case, its references and gates per entry, the restatement and the distance of any result from the reference"""

    def __init__(self, case: Case, index: int = 0):
        self.case = c = case
        rng = np.random.default_rng(9000 + index)
        n = c.n
        g = rng.standard_normal(n) * c.g_scale
        nrm = math.sqrt(float(np.sum(g * g)))
        target = {"tiny": 2e-6, "edge_lo": 0.7, "edge_hi": 0.7}.get(c.clip)
        if target is not None:
            g = g * (target / nrm)
        self.g = g.astype(F)
        self.p = {"normal": rng.standard_normal(n), "zero": np.zeros(n), "lr": rng.standard_normal(n) * c.lr}[c.p_kind].astype(F)
        if c.t > 1:                          # moments of a run at this gradient scale; m of either sign, so m' cancels in places
            scale = float(np.abs(self.g).mean()) * 1.25
            self.m = (rng.standard_normal(n) * scale * 0.5).astype(F)
            self.v = ((rng.standard_normal(n) * scale) ** 2 * 0.7).astype(F)
        else:
            self.m, self.v = np.zeros(n, dtype=F), np.zeros(n, dtype=F)
        self.ema = (self.p.astype(np.float64) + rng.standard_normal(n) * 3.0 * c.lr).astype(F)
        nv = n >> 2
        if c.bad:
            at = (nv // 2) * 4 + 1 if c.bad.endswith("vec") else nv * 4 + (n & 3) - 1
            assert 0 <= at < n and (c.bad.endswith("vec") or n & 3)
            self.g[at] = F(np.inf) if c.bad.startswith("inf") else F(np.nan)
        with np.errstate(all="ignore"):
            self.S = None if c.clip == "null" else F(np.sum(self.g.astype(np.float64) ** 2))
        nrm = 0.0 if self.S is None or not np.isfinite(self.S) else math.sqrt(float(self.S))
        max_norm = {"below": 10.0 * nrm, "above": nrm / 7.0, "edge_lo": nrm + 5e-7, "edge_hi": nrm - 5e-7, "tiny": 1e-6, "off": 0.0,
                    "off_neg": -1.0, "null": 0.7}[c.clip]
        if c.bad and c.clip == "above":      # no finite norm to scale from: clipping on means a fixed positive max_norm
            max_norm = 0.7
        self.hp = HP(lr=c.lr, wd=c.wd, max_norm=max_norm)
        self.sched = SCHEDULES[c.sched]
        self._ref = adamw_ref(self.p, self.g, self.m, self.v, self.hp, c.t, self.S, c.skip)
        self.skipped = self._ref["skipped"]

    def expected(self, entry: str) -> dict:
        """name -> (reference, gate) of every output of ``entry``; 'counter' is exact.  The EMA's reference is built on the new parameters
        the kernel itself produced (``p_new``, see ``distance``), so it is not part of this dict"""
        r = self._ref
        out = {"p": (r["p"], r["gate_p"]), "m": (r["m"], r["gate_m"]), "v": (r["v"], r["gate_v"])}
        if entry != "adamw_step":
            out["counter"] = self.case.t - 1 + (0 if self.skipped else 1)
        return out

    def emul(self, entry: str, fma=False, fault=None) -> dict:
        c = self.case
        p, m, v, taken = adamw_emul(self.p, self.g, self.m, self.v, self.hp, c.t, self.S, c.skip, fma, fault)
        out = {"p": p, "m": m, "v": v}
        if entry != "adamw_step":
            out["counter"] = c.t - 1 + taken
        if entry == "adamw_ema_step_counted":
            skipped = taken == 0 or (self.skipped and fault == "skipped_step_counted")
            out["ema"] = self.ema.copy() if skipped else ema_emul(self.ema, p, c.t, self.sched, True, fault)
        return out

    def ratios(self, entry: str, got: dict) -> dict:
        """name -> the largest |got - ref| / gate over the elements (a difference where the gate is 0, or a non-finite result: inf)"""
        exp = self.expected(entry)
        res = {}
        for k in ("p", "m", "v"):
            res[k] = _ratio(got[k], *exp[k])
        if "counter" in exp:
            res["counter"] = 0.0 if int(got["counter"]) == exp["counter"] else math.inf
        if entry == "adamw_ema_step_counted":
            if self.skipped:
                ref, gate = self.ema.astype(np.float64), np.zeros(self.case.n)
            else:
                ref, gate = ema_ref(self.ema, got["p"], self.case.t, self.sched)
            res["ema"] = _ratio(got["ema"], ref, gate)
        return res

    def distance(self, entry: str, fault, fma=False) -> float:
        return max(self.ratios(entry, self.emul(entry, fma, fault)).values())


def _ratio(got, ref, gate) -> float:
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return math.inf
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        r = np.where(err == 0.0, 0.0, np.where(gate > 0.0, err / np.where(gate > 0.0, gate, 1.0), np.inf))
    return float(r.max()) if r.size else 0.0


@functools.lru_cache(maxsize=None)
def built(index: int) -> Built:
    """the case's operands and references, computed once and shared (nobody writes into them)"""
    return Built(CASES[index], index)


@functools.lru_cache(maxsize=None)
def norm_operand(index: int):
    c = NORM_CASES[index]
    return (np.random.default_rng(7000 + index).standard_normal(c.n) * c.g_scale).astype(F)
