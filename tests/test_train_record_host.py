"""The training path's host decisions against a committed record (tests/golden/train_record.json, written from the parent of the
change that introduced jen1_amd/gemm_host.py by ``python tools/train_record.py --write-fixture tests/golden/train_record.json``).

tools/train_record.py runs the host code on the CPU against a recording stand-in for the library: per case the launch list (function,
scalars, every field of the argument structs, pointers as null / not null) and ``rt.stats``.  Nothing runs on a GPU: a changed route,
argument mapping, split-K factor or accounting formula shows up as a difference, and is accepted by regenerating the fixture in the same
change.  The second test calls the route functions directly at the grid's shapes and checks them against the launches of the record.
"""
import importlib.util
import os
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("train_record", os.path.join(ROOT, "tools", "train_record.py"))
train_record = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(train_record)

SPLITK, SKINNY = 16, 22          # positions of ``splitk`` and ``reserved`` (the skinny form) in jen1_gemm_args
TAP_REV = 13                     # position of ``tap_rev`` among jen1_big_gemm_conv's arguments


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return train_record.load_fixture(os.path.join(golden_dir, "train_record.json"))


def test_record_matches_fixture(fixture):
    got = train_record.build_record()
    assert list(got) == list(fixture)
    diff = train_record.first_difference(fixture, got)
    assert diff is None, diff


def _gemm_form(block):
    if block[SKINNY] == 1:
        return ("skinny",)
    return ("splitk", block[SPLITK]) if block[SPLITK] > 1 else ("plain",)


def _products(case, kind):
    """the GEMM-shaped launches of a recorded operator case, in order, as (what launched, route)"""
    big = ("big_transposed",) if kind == "convT" else ("big",)
    out = []
    for name, args in case["launches"]:
        if name == "jen1_train_gemm":
            out.append(("gemm", _gemm_form(args[0])))
        elif name == "jen1_train_gemm_pair":
            out += [("pair", _gemm_form(args[0])), ("pair", _gemm_form(args[1]))]
        elif name in ("jen1_big_gemm_conv", "jen1_big_gemm_tn_conv"):
            out.append((name, big))
    return out


def _switches(**over):
    sw = dict(skinny_gemm=True, skinny_max_steps=64, target_wgs=256, min_steps=4, big_convs=True, big_conv_rows=4096, big_wgrads=True,
              big_wgrad_rows=4096, big_wgrad_unpair=False, pair_grads=True)
    return SimpleNamespace(**dict(sw, **over))


GRID = [(n, c, "bf16") for n, c in train_record.BF16_GRID.items() if c[0] in ("conv", "convT", "linear")] + \
       [(n, c, "f32") for n, c in train_record.F32_GRID.items()]


@pytest.mark.parametrize("paired", [True, False], ids=["default", "unpaired"])
@pytest.mark.parametrize("name,case,dtype", GRID, ids=[g[0] for g in GRID])
def test_route_functions_give_the_recorded_routes(fixture, name, case, dtype, paired):
    from jen1_amd import gemm_host as G
    from jen1_amd import lib as L
    kind, B, ci, co, Lx, k, stride, _ = case
    dt = L.BF16 if dtype == "bf16" else L.F32
    L_in = Lx
    L_out = (Lx - 1) // stride + 1 if kind == "conv" else Lx if kind == "linear" else (Lx - 1) * stride - 2 * (stride // 2 + stride % 2) + k + stride % 2
    cip, ldy = G.pad8(ci), G.pad8(co)
    sw = _switches(pair_grads=paired)
    prods = _products(fixture[name if paired else name + "/unpaired"], kind)
    assert len(prods) == 3, prods

    fwd = G.forward_route(sw, kind, B * L_out, ci, cip, co, k, dt, False)
    assert fwd == prods[0][1]
    assert (fwd[0] in ("big", "big_transposed")) == (prods[0][0] == "jen1_big_gemm_conv")
    # ConvFn.backward: the plan, then the weight gradient (deferred inside a pair) and the data gradient (with the transposed copy ``wd``)
    plan = G.backward_plan(sw, kind, B * L_in, ci, dt, True)
    assert plan == (("pair",) if prods[1][0] == "pair" else ("queue",))
    K = B * L_in if kind == "convT" else B * L_out
    wg = G.wgrad_route(sw, kind, K, co, ci, cip, ldy, k, dt, L_in, L_out, B * L_in, B * L_out, False, True, plan == ("pair",))
    assert wg == prods[1][1]
    assert (wg[0] in ("big", "big_transposed")) == (prods[1][0] == "jen1_big_gemm_tn_conv")
    dg = G.dgrad_route(sw, kind, B * L_in, ci, cip, ldy, ldy, k, dt, True, plan == ("pair",))
    assert dg == prods[2][1]
    assert (dg[0] in ("big", "big_transposed")) == (prods[2][0] == "jen1_big_gemm_conv")


def test_reflect_padding_takes_no_big_route(fixture):
    """the SEANet convolutions pad by reflection, which jen1_big_gemm_conv's row map does not do: 4096 rows in bf16 stay on jen1_train_gemm"""
    from jen1_amd import gemm_host as G
    from jen1_amd import lib as L
    prods = _products(fixture["conv_reflect_forward"], "conv")
    assert [p[0] for p in prods] == ["gemm"]
    assert G.forward_route(_switches(), "conv", 4096, 128, 128, 128, 7, L.BF16, True) == prods[0][1]
    assert G.forward_route(_switches(), "conv", 4096, 128, 128, 128, 7, L.BF16, False) == ("big",)


def test_route_functions_follow_the_switches():
    from jen1_amd import gemm_host as G
    from jen1_amd import lib as L
    args = ("conv", 4096, 128, 128, 128, 3, L.BF16, False)
    assert G.forward_route(_switches(), *args) == ("big",)
    assert G.forward_route(_switches(big_convs=False), *args) == ("plain",)
    assert G.forward_route(_switches(big_conv_rows=4097), *args) == ("plain",)
    assert G.pick_splitk(_switches(), 16, 512, 1728) > 1 and G.pick_splitk(_switches(target_wgs=2), 16, 512, 1728) == 1
    assert G.want_skinny(_switches(), 16, 512, 32) and not G.want_skinny(_switches(skinny_gemm=False), 16, 512, 32)
