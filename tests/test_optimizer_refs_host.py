"""CPU pins of tests/optimizer_common.py: the float64 reference of one optimiser call against torch.optim.AdamW + clip_grad_norm_ in
float64 and against ema.ema_schedule, the float32 restatements (with and without contracted multiply-adds) inside the gates over the whole
case table, and the power of every wrong variant in the GPU test's own metric."""
import math

import numpy as np
import pytest
import torch

import optimizer_common as OC
from jen1_amd.ema import ema_schedule

IDS = [c.id for c in OC.CASES]


def _torch_step(b: OC.Built):
    """clip_grad_norm_ + AdamW.step() in float64 from the case's state (trainer.py:145-147)"""
    c = b.case
    lr, b1, b2, eps, wd, max_norm = b.hp.f32()
    p = torch.nn.Parameter(torch.from_numpy(b.p.astype(np.float64)))
    p.grad = torch.from_numpy(b.g.astype(np.float64))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[p] = {"step": torch.tensor(float(c.t - 1)), "exp_avg": torch.from_numpy(b.m.astype(np.float64)),
                    "exp_avg_sq": torch.from_numpy(b.v.astype(np.float64))}
    if b.S is not None and max_norm > 0:
        torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt.step()
    st = opt.state[p]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("i", [i for i, c in enumerate(OC.CASES) if not c.bad], ids=[c.id for c in OC.CASES if not c.bad])
def test_reference_matches_torch_adamw_and_clip_in_float64(i):
    """the same step by torch; the scalar is the exact float64 sum here (torch computes its own norm), so the two agree to float64 rounding"""
    b = OC.built(i)
    S = None if b.S is None else OC.sqnorm_ref(b.g)
    r = OC.adamw_ref(b.p, b.g, b.m, b.v, b.hp, b.case.t, S, b.case.skip)
    p, m, v = _torch_step(b)
    r32 = b.expected("adamw_step")
    for got, want, name in ((r["p"], p, "p"), (r["m"], m, "m"), (r["v"], v, "v")):
        # float64 rounding only (torch's lerp_ and its own norm sum round differently): a millionth of the float32 gate of the element,
        # which scales with the terms that cancel in it
        worst = float((np.abs(got - want) / r32[name][1]).max())
        assert worst <= 1e-6, (name, worst)
    # ... and the float32 scalar the kernel reads moves the reference by less than a tenth of any gate
    for k in ("p", "m", "v"):
        assert (np.abs(r32[k][0] - r[k]) <= 0.1 * r32[k][1]).all(), k


@pytest.mark.parametrize("si", range(len(OC.SCHEDULES)))
def test_ema_schedule_restatement_matches_the_package(si):
    s = OC.SCHEDULES[si]
    for t in list(range(1, 3000)) + OC.STEPS + [4999, 5001, 99990, 100000]:
        mode, decay = OC.ema_mode_decay(t, s)
        want = ema_schedule(t, **s)
        assert mode == want[0] and abs(decay - want[1]) <= 1e-15, (t, mode, decay, want)


def test_skip_rule_of_the_reference():
    """a non-finite norm with skip_nonfinite on leaves everything untouched, whatever max_norm; without the scalar nothing is skipped"""
    for S in (np.float32(np.inf), np.float32(np.nan)):
        for mx in (0.7, 0.0, -1.0):
            assert OC.coef_ref(S, mx, 1) == (True, 1.0)
    assert OC.coef_ref(None, 0.7, 1) == (False, 1.0)
    assert OC.coef_ref(np.float32(4.0), 0.5, 1) == (False, 0.5 / (2.0 + 1e-6))
    assert OC.coef_ref(np.float32(4.0), 3.0, 1) == (False, 1.0) and OC.coef_ref(np.float32(4.0), 0.0, 1) == (False, 1.0)
    skipped = [i for i, c in enumerate(OC.CASES) if c.bad]
    assert len(skipped) == 8
    for i in skipped:
        b = OC.built(i)
        assert b.skipped and not np.isfinite(b.S)
        for e in OC.UPDATE_ENTRIES[1:]:
            assert b.expected(e)["counter"] == b.case.t - 1


@pytest.mark.parametrize("i", range(len(OC.CASES)), ids=IDS)
def test_both_restatements_stay_inside_the_gates(i):
    b = OC.built(i)
    for entry in OC.UPDATE_ENTRIES:
        for fma in (False, True):
            r = b.ratios(entry, b.emul(entry, fma))
            assert max(r.values()) <= 1.0, (entry, fma, r)


@pytest.mark.parametrize("i", range(len(OC.NORM_CASES)), ids=[c.id for c in OC.NORM_CASES])
def test_norm_restatements_stay_inside_the_gate(i):
    g = OC.norm_operand(i)
    ref = OC.sqnorm_ref(g)
    for fma in (False, True):
        assert abs(float(OC.sqnorm_emul(g, fma)) - ref) <= OC.norm_gate(g.size, ref)


def test_norm_chain_is_the_kernels_geometry():
    assert OC.norm_blocks(1) == 1 and OC.norm_blocks(4096) == 1 and OC.norm_blocks(4100) == 2 and OC.norm_blocks(257 * 4096 + 3) == 257
    assert OC.norm_blocks(OC.PASS) == 4096 == OC.norm_blocks(OC.BIG_N)
    assert OC.norm_chain(5) == 2 + 4 + 1 + 6 + 4 + 1 + 6 + 4 + 1
    assert OC.norm_chain(257 * 4096 + 3) == OC.norm_chain(5) + 1            # 257 partials: thread 0 of the last block adds two
    assert OC.norm_chain(OC.PASS) == OC.norm_chain(5) + 15
    assert OC.norm_chain(OC.BIG_N) + 2 == 54                                # three trips of a full grid
    assert OC.norm_gate(OC.BIG_N, 1.0) <= 1e-5                              # never looser than test_gradient_norm_is_bit_reproducible


def test_every_wrong_variant_lies_ten_gates_out_in_every_entry_that_could_make_it():
    far = {}
    for i in range(len(OC.CASES)):
        b = OC.built(i)
        for entry in OC.UPDATE_ENTRIES:
            for w in OC.CAN_MAKE[entry]:
                d = b.distance(entry, w)
                if d >= OC.POWER:
                    far.setdefault((entry, w), []).append((b.case.id, d))
    for i in range(len(OC.NORM_CASES)):
        g = OC.norm_operand(i)
        ref = OC.sqnorm_ref(g)
        for w in OC.NORM_WRONG:
            d = abs(float(OC.sqnorm_emul(g, False, w)) - ref) / OC.norm_gate(g.size, ref)
            if d >= OC.POWER:
                for entry in ("grad_sqnorm", "grad_sqnorm_ws"):
                    far.setdefault((entry, w), []).append((OC.NORM_CASES[i].id, d))
    missing = [(e, w) for e, ws in OC.CAN_MAKE.items() for w in ws if (e, w) not in far]
    assert not missing, missing
    assert {w for ws in OC.CAN_MAKE.values() for w in ws} == set(OC.ALL_WRONG)
    for (e, w), hits in sorted(far.items()):
        best = max(hits, key=lambda h: h[1])
        print(f"{e:<24} {w:<24} shown by {len(hits):>3} cases, most clearly by {best[0]} at {best[1]:.3g} gates")


def test_the_right_restatement_is_at_distance_zero_of_itself_and_unlisted_mistakes_do_not_show():
    b = OC.built(IDS.index("t1.p-normal"))
    assert b.distance("adamw_step", None) <= 1.0
    i4 = IDS.index("n4")                      # no tail at n = 4; one vector, so dropping it leaves everything unchanged
    assert OC.built(i4).distance("adamw_step", "tail_dropped") == OC.built(i4).distance("adamw_step", None)
    assert OC.built(i4).distance("adamw_step", "last_vector_dropped") >= OC.POWER
