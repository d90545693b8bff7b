"""-m gpu: the optimiser kernels (csrc/optimizer.hip) and jen1_memset_zero entry by entry through the C ABI against the float64 references
of tests/optimizer_common.py (references, gates, case tables; tests/test_optimizer_refs_host.py pins them without a GPU).

Small forms: every case of the tables through jen1_grad_sqnorm / _ws, jen1_adamw_step (host step t), jen1_adamw_step_counted and
jen1_adamw_ema_step_counted (device counter t - 1), each output under its per-element gate, every buffer between guard bands that must come
back bit for bit, the gradient and the norm scalar unchanged.  The norm's contract (out accumulates, repeated calls give the same bits, the
scratch is left ready after any grid).  Skipped steps.  Multi-pass size (three grid-stride trips, generated and compared on the device):
needles whose squares are powers of 4 for the norm, an exact power-of-two decay for the updates, one call against the same call in slices
on random data.  Refusals that return before any launch.  FusedAdamW over several tensors.  What was measured goes to the parity log
(profiles/optimizer_forms_parity.txt is its summary).
"""
import math

import numpy as np
import pytest
import torch

import optimizer_common as OC
from helpers import record_parity
from jen1_amd import lib as L

pytestmark = pytest.mark.gpu
GUARD, PATTERN, PASS, BIG_N = OC.GUARD, OC.PATTERN, OC.PASS, OC.BIG_N
IDS = [c.id for c in OC.CASES]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """n 4-byte elements between two guard bands of PATTERN; the data starts on a 16-byte boundary, the rear band right behind element n - 1"""

    def __init__(self, data=None, n=None, dtype=torch.float32):
        n = int(n if data is None else len(data))
        self.n = n
        self.raw = torch.full((GUARD + n + GUARD + (-n % 4),), PATTERN, dtype=torch.int32, device="cuda")
        self.data = self.raw.view(dtype)[GUARD:GUARD + n]
        if data is not None:
            self.data.copy_(torch.as_tensor(data).to(dtype))
        assert self.data.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.data.data_ptr()

    def guards_ok(self):
        return bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[GUARD + self.n:] == PATTERN).all())

    def host(self):
        return self.data.cpu().numpy()


def _sched_args(s):
    return [s["beta"], s["update_after_step"], s["update_every"], int(s["warmup"]), s["inv_gamma"], s["power"], s["min_decay"]]


def _update(lib, entry, p, g, m, v, n, hp, t, gn, skip, counter=None, ema=None, sched=None):
    """one call of an update entry; pointers are integers (or None), ``t`` the host step of jen1_adamw_step"""
    head = [p, g, m, v, n, *hp.f32()[:5]]
    mx = hp.f32()[5]
    if entry == "adamw_step":
        return lib.jen1_adamw_step(*head, t, gn, mx, skip, _stream())
    if entry == "adamw_step_counted":
        return lib.jen1_adamw_step_counted(*head, counter, gn, mx, skip, _stream())
    return lib.jen1_adamw_ema_step_counted(*head, counter, gn, mx, skip, ema, *_sched_args(sched), _stream())


def _bits(t):
    return t.view(torch.int32) if t.dtype != torch.int32 else t


def _verdict(test, case_id, ratios):
    worst = max(ratios.values())
    print(f"{test} {case_id}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    record_parity("optimizer_forms." + test, case_id, "f32", **ratios)
    assert worst <= 1.0, f"{test} {case_id}: error / gate = {ratios}"


# ---------------------------------------------------------------------------------------------------------------------
# small forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scratch(lib):
    """caller-owned scratch of the norm, zeroed once here and shared by every test: each call has to leave it ready for the next"""
    return torch.zeros(int(lib.jen1_grad_sqnorm_scratch_bytes()) // 4, device="cuda")


def _sqnorm(lib, entry, g_ptr, n, out_ptr, scratch=None):
    if entry == "grad_sqnorm":
        return lib.jen1_grad_sqnorm(g_ptr, n, out_ptr, _stream())
    return lib.jen1_grad_sqnorm_ws(g_ptr, n, out_ptr, scratch.data_ptr(), _stream())


@pytest.mark.parametrize("i", range(len(OC.NORM_CASES)), ids=[c.id for c in OC.NORM_CASES])
def test_norm_entries_under_the_gate(lib, scratch, i):
    g_host = OC.norm_operand(i)
    n = g_host.size
    ref = OC.sqnorm_ref(g_host)
    g = Buf(g_host)
    before = g.raw.clone()
    for entry in ("grad_sqnorm", "grad_sqnorm_ws"):
        out = Buf(np.zeros(1, dtype=np.float32))
        L.check(_sqnorm(lib, entry, g.ptr, n, out.ptr, scratch), entry)
        torch.cuda.synchronize()
        assert torch.equal(g.raw, before) and out.guards_ok()
        _verdict(entry, OC.NORM_CASES[i].id, {"err_over_gate": abs(float(out.host()[0]) - ref) / OC.norm_gate(n, ref)})


@pytest.mark.parametrize("i", range(len(OC.CASES)), ids=IDS)
def test_update_entries_under_the_gates(lib, i):
    """the host-step entry at step t and the counted entries at counter t - 1 against the same float64 reference (not against each other:
    the host's and the device's pow may differ in a last bit)"""
    b = OC.built(i)
    c = b.case
    for entry in OC.UPDATE_ENTRIES:
        bufs = {k: Buf(getattr(b, k)) for k in ("p", "g", "m", "v", "ema")}
        gn = None if b.S is None else Buf(np.array([b.S], dtype=np.float32))
        counter = Buf(np.array([c.t - 1], dtype=np.int32), dtype=torch.int32)
        keep = {k: bufs[k].raw.clone() for k in ("g", "ema")}
        L.check(_update(lib, entry, bufs["p"].ptr, bufs["g"].ptr, bufs["m"].ptr, bufs["v"].ptr, c.n, b.hp, c.t, gn and gn.ptr, c.skip,
                        counter.ptr, bufs["ema"].ptr, b.sched), entry)
        torch.cuda.synchronize()
        got = {k: bufs[k].host() for k in ("p", "m", "v", "ema")}
        got["counter"] = int(counter.host()[0])
        ratios = b.ratios(entry, got)
        assert all(x.guards_ok() for x in bufs.values()) and counter.guards_ok(), (entry, c.id)
        assert torch.equal(bufs["g"].raw, keep["g"]), "the gradient is read-only"
        if gn is not None:
            assert gn.guards_ok() and gn.host().tobytes() == np.array([b.S], dtype=np.float32).tobytes()
        if entry != "adamw_ema_step_counted":
            assert torch.equal(bufs["ema"].raw, keep["ema"])
        if entry == "adamw_step":
            assert got["counter"] == c.t - 1             # never given to the entry
        if b.skipped:                                    # bit for bit, not merely equal
            for k in ("p", "m", "v", "ema"):
                assert got[k].tobytes() == getattr(b, k).tobytes(), (entry, k)
        _verdict(entry, c.id, ratios)


# ---------------------------------------------------------------------------------------------------------------------
# the norm's contract
# ---------------------------------------------------------------------------------------------------------------------
def _fresh_sq(lib, g):
    """the sum of squares of a device buffer with a scratch nobody used before -> float32 bits as a tensor"""
    out = torch.zeros(1, device="cuda")
    sc = torch.zeros(int(lib.jen1_grad_sqnorm_scratch_bytes()) // 4, device="cuda")
    L.check(lib.jen1_grad_sqnorm_ws(g.ptr, g.n, out.data_ptr(), sc.data_ptr(), _stream()), "ws")
    torch.cuda.synchronize()
    return out


def test_norm_accumulates_into_out_over_two_buffers(lib, scratch):
    rng = np.random.default_rng(11)
    a, b = Buf((rng.standard_normal(4097) * 0.3).astype(np.float32)), Buf((rng.standard_normal(1027) * 2.0).astype(np.float32))
    fa, fb = _fresh_sq(lib, a), _fresh_sq(lib, b)
    ref = OC.sqnorm_ref(a.host()) + OC.sqnorm_ref(b.host())
    for entry in ("grad_sqnorm", "grad_sqnorm_ws"):
        out = Buf(np.zeros(1, dtype=np.float32))
        L.check(_sqnorm(lib, entry, a.ptr, a.n, out.ptr, scratch), entry)
        L.check(_sqnorm(lib, entry, b.ptr, b.n, out.ptr, scratch), entry)
        torch.cuda.synchronize()
        assert torch.equal(out.data, fa + fb) and out.guards_ok()          # out[0] += tot: one float32 addition of the two fresh results
        # the first buffer's terms pass one more addition: the second call's out[0] +=
        _verdict(entry, "two-buffers", {"err_over_gate": abs(float(out.host()[0]) - ref) / OC.norm_gate(a.n, ref, extra=1)})


@pytest.mark.parametrize("entry", ["grad_sqnorm", "grad_sqnorm_ws"])
def test_norm_bits_do_not_depend_on_what_the_scratch_saw_before(lib, entry):
    """grids large -> small -> large -> small on one scratch (257 partials and the ticket of the large grid stay behind for the small one),
    repeated: every result is the fresh-scratch result bit for bit"""
    rng = np.random.default_rng(12)
    large = Buf((rng.standard_normal(257 * 4096 + 3) * 1e-2).astype(np.float32))
    mid = Buf((rng.standard_normal(8192 + 5) * 3.0).astype(np.float32))
    small = Buf((rng.standard_normal(5) * 100.0).astype(np.float32))
    fresh = {id(x): _fresh_sq(lib, x) for x in (large, mid, small)}
    sc = torch.zeros(int(lib.jen1_grad_sqnorm_scratch_bytes()) // 4, device="cuda")
    for x in (large, small, large, mid, small, small, mid, large, large):
        out = torch.zeros(1, device="cuda")
        L.check(_sqnorm(lib, entry, x.ptr, x.n, out.data_ptr(), sc), entry)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(fresh[id(x)])), (entry, x.n, float(out), float(fresh[id(x)]))
    if entry == "grad_sqnorm_ws":          # (the library's own scratch cannot be read from here: the bits above are its check)
        assert int(sc.view(torch.int32)[OC.NORM_MAX_BLOCKS]) == 0          # the ticket is back at 0


# ---------------------------------------------------------------------------------------------------------------------
# skipped steps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.0, -1.0, 0.7])
@pytest.mark.parametrize("bad", ["inf_vec", "nan_vec", "inf_tail", "nan_tail"])
def test_skip_leaves_everything_and_the_next_step_uses_the_uncounted_bias_correction(lib, scratch, bad, max_norm):
    """the norm comes from the norm kernel itself (the non-finite element in a vector or in the tail must reach it); with skip_nonfinite on
    the step is dropped whatever max_norm is, nothing changes by a bit, and the next good step is step counter + 1"""
    n, taken = 1027, 2
    rng = np.random.default_rng(13)
    hp = OC.HP(lr=1e-2, wd=0.5, max_norm=max_norm)
    sched = OC.SCHEDULES[1]
    good = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    g_bad = good.copy()
    g_bad[(n // 8) * 4 + 2 if bad.endswith("vec") else n - 1] = np.inf if bad.startswith("inf") else np.nan
    state = dict(p=np.zeros(n, dtype=np.float32), m=(rng.standard_normal(n) * 5e-3).astype(np.float32),
                 v=((rng.standard_normal(n) * 1e-2) ** 2).astype(np.float32), ema=(rng.standard_normal(n) * 3e-2).astype(np.float32))
    for entry in OC.UPDATE_ENTRIES:
        bufs = {k: Buf(a) for k, a in state.items()}
        g, gn = Buf(g_bad), Buf(np.zeros(1, dtype=np.float32))
        counter = Buf(np.array([taken], dtype=np.int32), dtype=torch.int32)
        before = {k: x.raw.clone() for k, x in bufs.items()}
        L.check(lib.jen1_grad_sqnorm_ws(g.ptr, n, gn.ptr, scratch.data_ptr(), _stream()), "ws")
        L.check(_update(lib, entry, bufs["p"].ptr, g.ptr, bufs["m"].ptr, bufs["v"].ptr, n, hp, taken + 1, gn.ptr, 1, counter.ptr,
                        bufs["ema"].ptr, sched), entry)
        torch.cuda.synchronize()
        assert not math.isfinite(float(gn.host()[0]))
        for k, x in bufs.items():
            assert torch.equal(x.raw, before[k]), (entry, k)
        assert int(counter.host()[0]) == taken and counter.guards_ok()
        # the good step behind it
        g.data.copy_(torch.from_numpy(good))
        gn.data.zero_()
        L.check(lib.jen1_grad_sqnorm_ws(g.ptr, n, gn.ptr, scratch.data_ptr(), _stream()), "ws")
        L.check(_update(lib, entry, bufs["p"].ptr, g.ptr, bufs["m"].ptr, bufs["v"].ptr, n, hp, taken + 1, gn.ptr, 1, counter.ptr,
                        bufs["ema"].ptr, sched), entry)
        torch.cuda.synchronize()
        S = gn.host()[0]
        r = OC.adamw_ref(state["p"], good, state["m"], state["v"], hp, taken + 1, S, 1)
        got = {k: x.host() for k, x in bufs.items()}
        ratios = {k: OC._ratio(got[k], r[k], r["gate_" + k]) for k in ("p", "m", "v")}
        ratios["norm"] = abs(float(S) - OC.sqnorm_ref(good)) / OC.norm_gate(n, OC.sqnorm_ref(good))
        if entry == "adamw_ema_step_counted":
            ratios["ema"] = OC._ratio(got["ema"], *OC.ema_ref(state["ema"], got["p"], taken + 1, sched))
        else:
            assert torch.equal(bufs["ema"].raw, before["ema"])
        assert int(counter.host()[0]) == (taken if entry == "adamw_step" else taken + 1)
        assert all(x.guards_ok() for x in bufs.values())
        _verdict(entry, f"after-skip.{bad}.max_norm{max_norm:g}", ratios)


# ---------------------------------------------------------------------------------------------------------------------
# every element exactly once, at multi-pass size
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(lib):
    """five buffers of BIG_N elements between guard bands (0.67 GB), reused by the tests below; each test fills what it needs"""
    return {k: Buf(n=BIG_N) for k in ("p", "g", "m", "v", "ema")}


def _randn_(t, seed, scale=1.0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t.normal_(0.0, scale, generator=gen)


NV4 = (BIG_N >> 2) << 2
NEEDLES = [0, 3, 4,                                              # the first vector's ends, the second vector
           1023, 1024,                                           # either side of block 0's 1024-element span
           4 * 4096 * 256 - 1, 4 * 4096 * 256,                   # either side of the 4 194 304-element offset of the second unrolled load
           PASS - 1, PASS, 2 * PASS - 1, 2 * PASS,               # either side of both pass boundaries
           NV4 - 4, NV4 - 1,                                     # the last full vector
           NV4, NV4 + 1, NV4 + 2]                                # the three tail elements


@pytest.mark.parametrize("entry", ["grad_sqnorm", "grad_sqnorm_ws"])
def test_norm_counts_every_needle_exactly_once_at_multi_pass_size(lib, scratch, big, entry):
    """the gradient is 0 except needles 2^k (k = 0 .. at most 11): squares 4^k sum below 2^24, so the float32 result is the exact integer in any
    order and each of its base-4 digits must be 1 (0: an element lost, 2: one counted twice)"""
    assert NEEDLES[-1] == BIG_N - 1 and BIG_N & 3 == 3 and len(set(NEEDLES)) == len(NEEDLES) == 16
    g = big["g"]
    g.data.zero_()
    for lo in (0, 8):
        at = NEEDLES[lo:lo + 8]
        idx = torch.tensor(at, device="cuda")
        g.data[idx] = torch.tensor([2.0 ** k for k in range(len(at))], device="cuda")
        out = Buf(np.zeros(1, dtype=np.float32))
        L.check(_sqnorm(lib, entry, g.ptr, BIG_N, out.ptr, scratch), entry)
        torch.cuda.synchronize()
        val = float(out.host()[0])
        g.data[idx] = 0.0
        assert val == int(val) and 0 <= val < 2 ** 24, val
        digits = [(int(val) >> (2 * k)) & 3 for k in range(12)]
        print(f"{entry} needles {at}: {int(val)} base-4 digits {digits}")
        assert digits == [1] * len(at) + [0] * (12 - len(at)), dict(zip(at, digits))
        assert out.guards_ok()
    assert g.guards_ok()


EXACT_SCHED = dict(beta=0.999, update_after_step=100, update_every=1, warmup=True, inv_gamma=1.0, power=2.0 / 3.0, min_decay=0.0)   # COPY


@pytest.mark.parametrize("entry", OC.UPDATE_ENTRIES)
def test_update_visits_every_element_exactly_once_at_multi_pass_size(lib, big, entry):
    """g = m = v = 0, lr = 2^-6, wd = 0.5: 1 - lr wd = 1 - 2^-7 exactly, the update term is 0, so a step is p <- fl(p (1 - 2^-7)) bit for
    bit; an element never visited keeps p0, one visited twice is decayed twice.  Two steps.  The fused entry copies: EMA == new p"""
    hp = OC.HP(lr=2.0 ** -6, wd=0.5, max_norm=0.7)
    p, g, m, v, ema = (big[k] for k in ("p", "g", "m", "v", "ema"))
    _randn_(p.data, 21)
    for x in (g, m, v):
        x.data.zero_()
    ema.data.fill_(-7.0)                                        # a sentinel no decayed N(0, 1) value equals by accident in 33 M draws
    want = p.data.clone()
    gn = Buf(np.zeros(1, dtype=np.float32))
    counter = Buf(np.zeros(1, dtype=np.int32), dtype=torch.int32)
    for t in (1, 2):
        L.check(_update(lib, entry, p.ptr, g.ptr, m.ptr, v.ptr, BIG_N, hp, t, gn.ptr, 1, counter.ptr, ema.ptr, EXACT_SCHED), entry)
        torch.cuda.synchronize()
        want.mul_(1.0 - 2.0 ** -7)
        differ = _bits(p.data) != _bits(want)
        wrong = int(differ.sum())
        first = int(differ.nonzero()[0]) if wrong else -1
        print(f"{entry} step {t}: {wrong} elements differ (first at {first})")
        assert wrong == 0, (entry, t, wrong, first)
        assert int(m.data.count_nonzero()) == 0 and int(v.data.count_nonzero()) == 0 and int(g.data.count_nonzero()) == 0
        if entry == "adamw_ema_step_counted":
            assert torch.equal(ema.data, p.data)
        else:
            assert bool((ema.data == -7.0).all())
        assert int(counter.host()[0]) == (0 if entry == "adamw_step" else t)
    assert all(x.guards_ok() for x in (p, g, m, v, ema, gn, counter))
    record_parity("optimizer_forms." + entry, "multi-pass.exact-decay", "f32", elements_wrong=0)


SLICES = [0, PASS, 30_000_000, BIG_N]          # at most one pass each, starts at multiples of 4: only the last slice has the tail


def _fill_random(big):
    _randn_(big["p"].data, 31)
    _randn_(big["g"].data, 32, 1e-2)
    _randn_(big["m"].data, 33, 5e-3)
    _randn_(big["v"].data, 34, 1e-2)
    big["v"].data.square_()
    _randn_(big["ema"].data, 35)


@pytest.mark.parametrize("entry", ["adamw_step", "adamw_ema_step_counted"])
def test_one_call_equals_the_same_call_in_slices_at_multi_pass_size(lib, scratch, big, entry):
    """random data: one call over three passes against the same call (same scalar, same step) over slices of at most one pass, bit for bit.
    The norm of the random gradient at this size is held to the float64 sum under its gate on the way"""
    hp = OC.HP(lr=1e-2, wd=0.1, max_norm=0.7)
    sched, taken = OC.SCHEDULES[2], 4                            # UPDATE at t = 5
    assert all(a % 4 == 0 for a in SLICES[:-1]) and all(b - a <= PASS for a, b in zip(SLICES, SLICES[1:]))
    _fill_random(big)
    gn = Buf(np.zeros(1, dtype=np.float32))
    L.check(lib.jen1_grad_sqnorm_ws(big["g"].ptr, BIG_N, gn.ptr, scratch.data_ptr(), _stream()), "ws")
    torch.cuda.synchronize()
    ref = float(big["g"].data.double().square().sum())
    _verdict("grad_sqnorm_ws", "multi-pass.random", {"err_over_gate": abs(float(gn.host()[0]) - ref) / OC.norm_gate(BIG_N, ref)})
    assert math.sqrt(ref) > hp.max_norm                          # the clip is on
    counter = Buf(np.array([taken], dtype=np.int32), dtype=torch.int32)
    ptr = {k: x.ptr for k, x in big.items()}
    L.check(_update(lib, entry, ptr["p"], ptr["g"], ptr["m"], ptr["v"], BIG_N, hp, taken + 1, gn.ptr, 1, counter.ptr, ptr["ema"], sched), entry)
    torch.cuda.synchronize()
    whole = {k: big[k].data.clone() for k in ("p", "m", "v", "ema")}
    g_bits = big["g"].raw.clone()
    _fill_random(big)
    assert torch.equal(big["g"].raw, g_bits)
    assert not torch.equal(whole["p"], big["p"].data)
    for a, b in zip(SLICES, SLICES[1:]):
        counter.data.fill_(taken)
        L.check(_update(lib, entry, ptr["p"] + 4 * a, ptr["g"] + 4 * a, ptr["m"] + 4 * a, ptr["v"] + 4 * a, b - a, hp, taken + 1, gn.ptr, 1,
                        counter.ptr, ptr["ema"] + 4 * a, sched), entry)
    torch.cuda.synchronize()
    for k in ("p", "m", "v", "ema"):
        differ = int((_bits(whole[k]) != _bits(big[k].data)).sum())
        print(f"{entry} {k}: {differ} elements differ between one call and slices")
        assert differ == 0, (entry, k, differ)
    assert all(x.guards_ok() for x in big.values())
    record_parity("optimizer_forms." + entry, "multi-pass.whole-vs-slices", "f32", elements_differ=0)


@pytest.mark.parametrize("nbytes", [4, 20, 2048 * 256 * 4 - 4, 2048 * 256 * 4 + 4, 3 * 2048 * 256 * 4 + 12])
def test_memset_zero_clears_exactly_its_bytes(lib, nbytes):
    """one word, five, either side of the capped grid's single pass (2048 blocks x 256 words), three passes and three words"""
    b = Buf(n=nbytes // 4, dtype=torch.int32)
    b.data.fill_(0x5A5A5A5A)
    L.check(lib.jen1_memset_zero(b.ptr, nbytes, _stream()), "memset")
    torch.cuda.synchronize()
    assert int(b.data.count_nonzero()) == 0 and b.guards_ok()
    L.check(lib.jen1_memset_zero(b.ptr, 0, _stream()), "memset of nothing")


# ---------------------------------------------------------------------------------------------------------------------
# refusals: every one returns on the host, before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_and_touch_nothing(lib, scratch):
    n = 8
    bufs = {k: Buf(np.arange(n, dtype=np.float32) + 1.0) for k in ("p", "g", "m", "v", "ema")}
    out = Buf(np.ones(1, dtype=np.float32))
    counter = Buf(np.array([3], dtype=np.int32), dtype=torch.int32)
    everything = list(bufs.values()) + [out, counter]
    before = [x.raw.clone() for x in everything]
    P = {k: x.ptr for k, x in bufs.items()}
    hp, bad_b1, bad_b2 = OC.HP(), OC.HP(beta1=1.0), OC.HP(beta2=-0.1)
    ok = OC.SCHEDULES[0]
    s = _stream()

    def upd(entry, hp=hp, t=4, n=n, counter_ptr=counter.ptr, sched=ok, **ptr):
        q = dict(P, **ptr)
        return _update(lib, entry, q["p"], q["g"], q["m"], q["v"], n, hp, t, out.ptr, 1, counter_ptr, q["ema"], sched)

    calls = {
        "sqnorm null g": lambda: lib.jen1_grad_sqnorm(None, n, out.ptr, s),
        "sqnorm null out": lambda: lib.jen1_grad_sqnorm(P["g"], n, None, s),
        "sqnorm unaligned g": lambda: lib.jen1_grad_sqnorm(P["g"] + 4, n - 1, out.ptr, s),
        "sqnorm n 0": lambda: lib.jen1_grad_sqnorm(P["g"], 0, out.ptr, s),
        "sqnorm n -4": lambda: lib.jen1_grad_sqnorm(P["g"], -4, out.ptr, s),
        "ws null scratch": lambda: lib.jen1_grad_sqnorm_ws(P["g"], n, out.ptr, None, s),
        "ws unaligned scratch": lambda: lib.jen1_grad_sqnorm_ws(P["g"], n, out.ptr, scratch.data_ptr() + 4, s),
        "ws unaligned g": lambda: lib.jen1_grad_sqnorm_ws(P["g"] + 8, n - 2, out.ptr, scratch.data_ptr(), s),
        "ws n 0": lambda: lib.jen1_grad_sqnorm_ws(P["g"], 0, out.ptr, scratch.data_ptr(), s),
        "memset null": lambda: lib.jen1_memset_zero(None, 16, s),
        "memset negative": lambda: lib.jen1_memset_zero(P["p"], -4, s),
        "memset ragged size": lambda: lib.jen1_memset_zero(P["p"], 6, s),
        "memset unaligned": lambda: lib.jen1_memset_zero(P["p"] + 2, 4, s),
        "step 0": lambda: upd("adamw_step", t=0),
        "step -1": lambda: upd("adamw_step", t=-1),
        "counted null counter": lambda: upd("adamw_step_counted", counter_ptr=None),
        "fused null counter": lambda: upd("adamw_ema_step_counted", counter_ptr=None),
        "fused null ema": lambda: upd("adamw_ema_step_counted", ema=None),
        "fused unaligned ema": lambda: upd("adamw_ema_step_counted", ema=P["ema"] + 4, n=n - 1),
    }
    for entry in OC.UPDATE_ENTRIES:
        for k in ("p", "g", "m", "v"):
            calls[f"{entry} null {k}"] = lambda entry=entry, k=k: upd(entry, **{k: None})
            calls[f"{entry} unaligned {k}"] = lambda entry=entry, k=k: upd(entry, n=n - 1, **{k: P[k] + 4})
        calls[f"{entry} n 0"] = lambda entry=entry: upd(entry, n=0)
        calls[f"{entry} n -1"] = lambda entry=entry: upd(entry, n=-1)
        calls[f"{entry} beta1 1"] = lambda entry=entry: upd(entry, hp=bad_b1)
        calls[f"{entry} beta2 < 0"] = lambda entry=entry: upd(entry, hp=bad_b2)
    for name, kw in (("beta 1", dict(beta=1.0)), ("min_decay above beta", dict(min_decay=0.9995)), ("min_decay < 0", dict(min_decay=-0.1)),
                     ("update_every 0", dict(update_every=0)), ("update_after_step -1", dict(update_after_step=-1)),
                     ("inv_gamma 0", dict(inv_gamma=0.0)), ("power 0", dict(power=0.0))):
        calls["fused " + name] = lambda kw=kw: upd("adamw_ema_step_counted", sched=dict(ok, **kw))
    for name, call in calls.items():
        assert call() != 0, f"{name}: accepted"
        assert lib.jen1_last_error(), name
    torch.cuda.synchronize()
    for x, b in zip(everything, before):
        assert torch.equal(x.raw, b)


# ---------------------------------------------------------------------------------------------------------------------
# FusedAdamW over several tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_adamw_keeps_the_padding_between_tensors_at_zero(lib):
    """tensors of 1, 3, 5 and 1027 elements start on 16-byte boundaries of the flat buffers; the elements between them stay exactly 0 in
    p, m, v and the EMA over 10 steps, and grad_norm() is the float64 norm under the norm's gate (halved by the root, + its rounding)"""
    from jen1_amd.ema import ParamEMA
    from jen1_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(5)
    sizes = [1, 3, 5, 1027]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in sizes]
    opt = FusedAdamW(ps, lr=1e-2, max_norm=0.7, skip_nonfinite=True)
    ema = ParamEMA(opt, beta=0.9, update_after_step=2, update_every=1, warmup=True)
    assert opt.offsets == [0, 4, 8, 16] and opt.numel == 16 + 1028
    pad = torch.ones(opt.numel, dtype=torch.bool)
    for o, s in zip(opt.offsets, sizes):
        pad[o:o + s] = False
    pad = pad.cuda()
    assert int(pad.sum()) == 3 + 1 + 3 + 1
    worst = 0.0
    for step in range(1, 11):
        gs = [torch.randn(s, generator=gen) * (0.02 * step) for s in sizes]
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        opt.step()
        torch.cuda.synchronize()
        for name, flat in (("p", opt.flat_param), ("m", opt.exp_avg), ("v", opt.exp_avg_sq), ("ema", ema.ema), ("g", opt.flat_grad)):
            assert int(flat[pad].count_nonzero()) == 0, (step, name)
        ref = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        gate = ((OC.norm_chain(opt.numel) + 2) / 2 + 1) * OC.U24 * ref
        worst = max(worst, abs(float(opt.grad_norm()) - ref) / gate)
        assert opt.step_count == step
    assert not torch.equal(ema.ema, opt.flat_param)
    _verdict("fused_adamw", "tensors-1-3-5-1027.grad_norm", {"err_over_gate": worst})
