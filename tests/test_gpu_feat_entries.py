"""Every feature-map entry of include/offk.h -- the seven families forward, forward_parts, off_units_fused, off_units, off_units_train,
off_units_backward and pw_reduce, each in its plain, _typed and _cl form -- held to a recorded golden (tests/golden/feat_entry_refusals.json,
written by tools/record_feat_entries.py, which runs the case lists below):

  (a) what each entry refuses: the return code and the whole offk_last_error text of every refusable defect, alone and in the pairs
      that tell which check fires first, and nothing written to the workspace or to any buffer of the call;
  (b) the ordered launch names (offk_set_profiling(h, 2), offk_launch_times) of one good call per (entry, kind, dtype) and handle precision.

The calls go straight through ctypes: the Python wrapper's own checks would catch most defects first.  B = 1, L = 2 (one pair), RGB variant.
No case passes a misaligned or null pointer to a call that does not refuse it before its first launch."""
import json
import os

import pytest
import torch

import offk_amd  # noqa: F401

from .feat_entries import case_id, FAMILIES, GOLDEN_FILE, refusal_cases, trace_cases, World

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return World(runtime)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, GOLDEN_FILE)) as f:
        return json.load(f)


def test_golden_lists_the_cases(golden):
    assert sorted(golden["refusals"]) == sorted(case_id(*c) for c in refusal_cases())
    assert sorted(golden["traces"]) == sorted(case_id(*c) for c in trace_cases())
    assert all(rc != 0 and msg for rc, msg in golden["refusals"].values())


@pytest.mark.parametrize("family", FAMILIES)
def test_refused_calls(world, golden, family):
    """(a): code and message as recorded, and every byte of the workspace, the outputs, G / D and the gradient buffer still the sentinel."""
    for handle in world.handles:
        world.fill(world.handles[handle])
        for case in refusal_cases():
            if case[0] != handle or case[1] != family:
                continue
            got = world.refused(case)
            assert got[0] != 0, (case, got)                                           # (first: a call that ran is not asked to run again)
            assert got == golden["refusals"][case_id(*case)], (case, got, golden["refusals"][case_id(*case)])
        assert world.untouched(world.handles[handle]), (handle, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("handle", ["fp32", "split"])
def test_launch_names(world, golden, handle, family):
    """(b): the ordered launch names of one good call per (entry, kind, dtype)."""
    for case in trace_cases():
        if case[0] == handle and case[1] == family:
            assert world.traced(*case) == golden["traces"][case_id(*case)], case
