"""The conv backward entries of include/offk.h (K4b: stride 1 and 2, exact fp32 and split-fp32) held to a recorded golden,
tests/golden/conv_bwd_entries.json (tools/record_conv_bwd_entries.py wrote it from the library as it was before the entries were folded
onto one table, csrc/offk_api.hip's ConvBwdForm): for every rule of the six refusal tables of tests/conv_bwd_abi.py and tests/conv_bwd_s2_abi.py the return code
and the FULL offk_last_error text of the fp32 entry and of its split twin -- those tests look for the entry's name only; this pins the
wording and which check wins -- and the bytes and chunks of the six plan entries over a sweep of n_img.  No GPU: every refusal fires
before the first HIP call, the plans are host code."""
import json
import os

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

from . import conv_bwd_abi as s1_abi
from . import conv_bwd_s2_abi as s2_abi
from .conv_bwd_entries import GOLDEN_FILE, N_IMGS, plan_shapes, planned, refusal_cases, refused, SPLIT_TABLES, TABLES


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, GOLDEN_FILE)) as f:
        return json.load(f)


def test_golden_lists_the_cases(golden):
    want = sorted(cid for table in TABLES for cid, _e, _a in refusal_cases(table))
    assert len(want) == len(set(want)) and sorted(golden["refusals"]) == want
    assert all(rc == -1 and msg for rc, msg in golden["refusals"].values()), "every rule is a refusal with a text"
    assert sorted(golden["plans"]) == sorted("%s/%s" % (e, sid) for sid, _H, _ci, _co, _k, plans in plan_shapes() for e in plans)
    assert all(len(rows) == len(N_IMGS) and all(r[0] == 0 for r in rows) for rows in golden["plans"].values())
    # the six tables are all there: a rule added to one of them has to be recorded
    assert sum(len(t) for t in (s1_abi.REFUSALS, s2_abi.REFUSALS) + tuple(v[0] for v in SPLIT_TABLES.values())) == len(
        set(cid.rsplit("/", 1)[0] for cid in want))


@pytest.mark.parametrize("table", TABLES)
def test_refusals_keep_their_code_and_text(built, golden, table):
    cases = refusal_cases(table)
    assert cases
    for cid, entry, args in cases:
        got = refused(built, entry, args)
        assert got == golden["refusals"][cid], (cid, got, golden["refusals"][cid])
        assert (entry + ":") in got[1], "the text starts with the entry's own name"


@pytest.mark.parametrize("shape", plan_shapes(), ids=[s[0] for s in plan_shapes()])
def test_plans_keep_their_bytes_and_chunks(built, golden, shape):
    sid, H, ci, co, k, plans = shape
    for entry, (nsize, has_int) in sorted(plans.items()):
        want = golden["plans"]["%s/%s" % (entry, sid)]
        for n, row in zip(N_IMGS, want):
            assert planned(built, entry, nsize, has_int, n, H, ci, co, k) == row, (entry, sid, n)
