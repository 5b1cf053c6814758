"""The case lists of tests/test_conv_bwd_entries.py and what it records of them (tools/record_conv_bwd_entries.py writes
tests/golden/conv_bwd_entries.json from the same lists): every refusal of the conv backward entries, fp32 entry and split twin, and what
the six plan entries return over a sweep of n_img.  A helper module: no tests of its own."""
import ctypes

from .conv_bwd import S1 as cb
from .conv_bwd import S2 as s2
from . import conv_bwd_abi as s1_abi
from . import conv_bwd_s2_abi as s2_abi

GOLDEN_FILE = "conv_bwd_entries.json"

# fp32 compute entry -> its split twin (the same argument list)
TWINS = {"offk_conv2d_backward_data": "offk_conv2d_backward_data_split", "offk_conv2d_backward_weight": "offk_conv2d_backward_weight_split",
         "offk_conv2d_s2_backward_data": "offk_conv2d_s2_backward_data_split",
         "offk_conv2d_s2_backward_weight": "offk_conv2d_s2_backward_weight_split"}
# fp32 plan entry -> the split plan entries, which take the first 9 or 8 of its 10 arguments
PLAN_TWINS = {"offk_conv2d_backward_plan": (("offk_conv2d_backward_plan_split", 9), ("offk_conv2d_backward_data_plan_split", 8)),
              "offk_conv2d_s2_backward_plan": (("offk_conv2d_s2_backward_weight_plan_split", 9), ("offk_conv2d_s2_backward_plan_split", 8))}
# the four tables that hold overrides only: (the table, the helper module whose argument list they override, the fp32 entry they were taken
# from, the argument list, is every rule a refusal of the fp32 entry too).  The data tables have rules of the split entry alone (its larger
# scratch, its alignment): those are asked of the split entry only, as their own tests do -- the fp32 entry would go on to launch
SPLIT_TABLES = {"conv_wgrad_split": (s1_abi.WGRAD_SPLIT_REFUSALS, s1_abi, "offk_conv2d_backward_weight", "weight_args", True),
                "conv_dgrad_split": (s1_abi.DGRAD_SPLIT_REFUSALS, s1_abi, "offk_conv2d_backward_data", "data_args", False),
                "conv_s2_wgrad_split": (s2_abi.WGRAD_SPLIT_REFUSALS, s2_abi, "offk_conv2d_s2_backward_weight", "weight_args", True),
                "conv_s2_dgrad_split": (s2_abi.DGRAD_SPLIT_REFUSALS, s2_abi, "offk_conv2d_s2_backward_data", "data_args", False)}
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
        rules, fp32_mod, fp32, make, both = SPLIT_TABLES[table]
        for rule, over in sorted(rules.items()):
            for entry in ((fp32, TWINS[fp32]) if both else (TWINS[fp32],)):
                out.append(("%s/%s/%s" % (table, rule, entry), entry, getattr(fp32_mod, make)(**over)))
        return out
    mod = s1_abi if table == "conv_bwd" else s2_abi
    for rule, (entry, make, over) in sorted(mod.REFUSALS.items()):
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
