"""-m gpu: what the host builder decides, against a committed record (tests/golden/plan_record.json, written by
``python tools/plan_record.py --no-run --out tests/golden/plan_record.json``).

For one plan per execution form (launch per layer with and without fixed-order statistics, GEMM / attention phases in bf16, float32 and
fp8, the sample-resident long-level launches, tile phases, the up-path fold on and off, table mode, per-sample tables) the launch ops
(kind, label, traffic / work accounting), the phase lists of the persistent programs, their LDS, workgroups and poison tables, and the
counts are compared entry by entry.  Nothing runs: a change of a tile or split-K heuristic, of an eligibility rule or of the accounting
shows up here as a difference, and is accepted by regenerating the fixture in the same change.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_record", os.path.join(ROOT, "tools", "plan_record.py"))
plan_record = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_record)


@pytest.fixture(scope="module")
def models():
    """built on first use: (configuration, dtype) -> UNetCFG1d"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    made = {}

    def get(cfg, dtype):
        if (cfg, dtype) not in made:
            made[(cfg, dtype)] = plan_record.make_model(cfg, dtype)
        return made[(cfg, dtype)]
    return get


@pytest.fixture(scope="module")
def golden(golden_dir):
    return plan_record.load_fixture(os.path.join(golden_dir, "plan_record.json"))


def test_fixture_covers_every_case_and_form(golden):
    assert list(golden) == list(plan_record.CASES)
    plan_record.check_forms(golden)


@pytest.mark.parametrize("name", list(plan_record.CASES))
def test_plan_matches_record(models, golden, name):
    case = plan_record.CASES[name]
    plan = plan_record.build_plan(models(case["cfg"], case["dtype"]), case)
    got = json.loads(json.dumps(plan_record.plan_record(plan)))
    diffs = plan_record.diff_structure(golden[name], got, name)
    assert not diffs, "\n".join(diffs[:20])
