"""The launch plan of one forward, held to a recorded golden (tests/golden/forward_plans.json, written by tools/record_forward_plans.py from
the case list below): for every case the COMPLETE ordered list of launch-group names (offk_set_profiling(h, 2), one forward,
offk_launch_times) equals the recorded one -- list equality, where test_gpu_switches.py asks for substrings that must or must not appear.

Cases: default handles at the project's smallest shapes on either side of every pair-count gate (7x7 at P = 12, 5x5 at 40, chains at 72),
every environment dict of forward.SWITCH_CASES at its own shape, the remaining switches of INTEGRATION.md section 7, consensus averaging,
a forward without the 28-head, the flow variant, an NHWC handle and the channels-last entry; in both arithmetic modes unless the switch or
the entry exists in one only.  The numbers are test_gpu_switches.py's business; here each case also repeats the forward with the trace off
and asserts the logits torch.equal to the traced run's: whether a launch name is built or not may not change what runs."""
import json
import os

import pytest
import torch

import offk_amd  # noqa: F401

from .featmaps import rt  # noqa: F401
from .forward import SWITCH_CASES
from .forward_plan import case_id, CASE_PARAMS, CASES, GOLDEN_FILE, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    """case id -> the recorded launch-group names"""
    with open(os.path.join(golden_dir, GOLDEN_FILE)) as f:
        g = json.load(f)
    return dict((cid, g["plans"][plan]) for cid, plan in g["cases"].items())


def test_golden_lists_the_cases(golden):
    assert sorted(golden) == sorted(case_id(k, p) for k, p in CASE_PARAMS)
    assert all(names and all(names) for names in golden.values())


def test_cases_cover_the_switch_module():
    """Every environment dict of forward.SWITCH_CASES is a case here, at its own shape and in its own arithmetic modes."""
    for name, case in SWITCH_CASES.items():
        assert CASES["switches-" + name][:3] == tuple(case[:3]), name


@pytest.mark.parametrize("case,prec", [pytest.param(k, p, id=case_id(k, p)) for k, p in CASE_PARAMS])
def test_forward_plan(rt, golden_dir, golden, case, prec):  # noqa: F811
    _h, names, traced, plain = run_case(rt, golden_dir, case, prec)
    assert names == golden[case_id(case, prec)], (names, golden[case_id(case, prec)])
    assert len(traced) == len(plain) == 3
    for a, b in zip(traced, plain):
        assert (a is None) == (b is None) == (a is None and not CASES[case][3].get("want28", True))
        if a is not None:
            assert torch.isfinite(a).all() and torch.equal(a, b)
