"""The conv backward entries of include/offk.h (K4b: stride 1 and 2, exact fp32 and split-fp32) held to a recorded golden,
tests/golden/conv_bwd_entries.json (tools/record_conv_bwd_entries.py wrote it from the library as it was before the entries were folded
onto one table, csrc/offk_api.hip's ConvBwdForm): for every rule of the six refusal tables of tests/test_conv_*_abi.py the return code
and the FULL offk_last_error text of the fp32 entry and of its split twin -- those tests look for the entry's name only; this pins the
wording and which check wins -- and the bytes and chunks of the six plan entries over a sweep of n_img.  No GPU: every refusal fires
before the first HIP call, the plans are host code."""
import ctypes
import json
import os

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

from .conv_bwd import S1 as cb
from .conv_bwd import S2 as s2
from . import test_conv_bwd_abi as s1_abi
from . import test_conv_bwd_s2_abi as s2_abi
from . import test_conv_dgrad_split_abi as s1_dgrad
from . import test_conv_s2_dgrad_split_abi as s2_dgrad
from . import test_conv_s2_wgrad_split_abi as s2_wgrad
from . import test_conv_wgrad_split_abi as s1_wgrad

GOLDEN_FILE = "conv_bwd_entries.json"

# fp32 compute entry -> its split twin (the same argument list)
TWINS = {"offk_conv2d_backward_data": "offk_conv2d_backward_data_split", "offk_conv2d_backward_weight": "offk_conv2d_backward_weight_split",
         "offk_conv2d_s2_backward_data": "offk_conv2d_s2_backward_data_split",
         "offk_conv2d_s2_backward_weight": "offk_conv2d_s2_backward_weight_split"}
# fp32 plan entry -> the split plan entries, which take the first 9 or 8 of its 10 arguments
PLAN_TWINS = {"offk_conv2d_backward_plan": (("offk_conv2d_backward_plan_split", 9), ("offk_conv2d_backward_data_plan_split", 8)),
              "offk_conv2d_s2_backward_plan": (("offk_conv2d_s2_backward_weight_plan_split", 9), ("offk_conv2d_s2_backward_plan_split", 8))}
# the four tables that hold overrides only: (module, the fp32 module whose argument list they override, the fp32 entry they were taken
# from, the argument list, is every rule a refusal of the fp32 entry too).  The data tables have rules of the split entry alone (its larger
# scratch, its alignment): those are asked of the split entry only, as their own tests do -- the fp32 entry would go on to launch
SPLIT_TABLES = {"conv_wgrad_split": (s1_wgrad, s1_abi, "offk_conv2d_backward_weight", "_weight_args", True),
                "conv_dgrad_split": (s1_dgrad, s1_abi, "offk_conv2d_backward_data", "_data_args", False),
                "conv_s2_wgrad_split": (s2_wgrad, s2_abi, "offk_conv2d_s2_backward_weight", "_weight_args", True),
                "conv_s2_dgrad_split": (s2_dgrad, s2_abi, "offk_conv2d_s2_backward_data", "_data_args", False)}
TABLES = ("conv_bwd", "conv_bwd_s2") + tuple(sorted(SPLIT_TABLES))

N_IMGS = tuple(range(1, 49)) + (96, 384)
# plan entry -> how many size_t outputs it has before the int (the chunks), has it the int
PLANS_S1 = {"offk_conv2d_backward_plan": (2, True), "offk_conv2d_backward_plan_split": (1, True), "offk_conv2d_backward_data_plan_split": (1, False)}
PLANS_S2 = {"offk_conv2d_s2_backward_plan": (2, True), "offk_conv2d_s2_backward_weight_plan_split": (1, True),
            "offk_conv2d_s2_backward_plan_split": (1, False)}


def refusal_cases(table):
    """[(id, entry, argument list)] of one refusal table: every rule, asked of the fp32 entry and of its split twin(s)"""
    out = []
    if table in SPLIT_TABLES:
        mod, fp32_mod, fp32, make, both = SPLIT_TABLES[table]
        for rule, over in sorted(mod._REFUSALS.items()):
            for entry in ((fp32, TWINS[fp32]) if both else (TWINS[fp32],)):
                out.append(("%s/%s/%s" % (table, rule, entry), entry, getattr(fp32_mod, make)(**over)))
        return out
    mod = s1_abi if table == "conv_bwd" else s2_abi
    for rule, (entry, make, over) in sorted(mod._REFUSALS.items()):
        args = make(**over)
        out.append(("%s/%s/%s" % (table, rule, entry), entry, args))
        if entry in TWINS:
            out.append(("%s/%s/%s" % (table, rule, TWINS[entry]), TWINS[entry], args))
        for twin, nargs in PLAN_TWINS.get(entry, ()):
            out.append(("%s/%s/%s" % (table, rule, twin), twin, args[:nargs]))
    return out


def refused(lib, entry, args):
    rc = getattr(lib, entry)(*args)
    return [rc, lib.offk_last_error(None).decode()]


def plan_shapes():
    """[(id, H, ci, co, k, the plan entries of its stride)]: tests/conv_bwd.S1.FUSION_SHAPES and tests/conv_bwd.S2.REAL"""
    out = [("%dx%d_%dto%d_k%d" % (H, H, ci, co, k), H, ci, co, k, PLANS_S1) for H, ci, co, k in cb.FUSION_SHAPES]
    return out + [(key, H, ci, co, k, PLANS_S2) for key, ci, co, k, H in s2.REAL]


def planned(lib, entry, nsize, has_int, n_img, H, ci, co, k):
    outs = [ctypes.c_size_t(0) for _ in range(nsize)] + ([ctypes.c_int(0)] if has_int else [])
    rc = getattr(lib, entry)(n_img, H, H, ci, co, k, k, *map(ctypes.byref, outs))
    return [rc] + [o.value for o in outs]


def record(lib):
    """what the golden file holds, from `lib`"""
    out = {"refusals": {}, "plans": {}}
    for table in TABLES:
        for cid, entry, args in refusal_cases(table):
            out["refusals"][cid] = refused(lib, entry, args)
    for sid, H, ci, co, k, plans in plan_shapes():
        for entry, (nsize, has_int) in sorted(plans.items()):
            out["plans"]["%s/%s" % (entry, sid)] = [planned(lib, entry, nsize, has_int, n, H, ci, co, k) for n in N_IMGS]
    return out


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
    assert sum(len(m._REFUSALS) for m in (s1_abi, s2_abi, s1_wgrad, s1_dgrad, s2_wgrad, s2_dgrad)) == len(
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
