"""The case list of tests/test_gpu_forward_plan.py and the run of one case (tools/record_forward_plans.py writes
tests/golden/forward_plans.json from the same list).  A helper module: no tests of its own."""
import json

import torch

import offk_amd  # noqa: F401
from offk_amd import spec

from .forward import HANDLE_PRECISIONS, SWITCH_CASES, dev, features, make_handle, shape_of

GOLDEN_FILE = "forward_plans.json"
BOTH, SPLIT = tuple(HANDLE_PRECISIONS), ("f32split",)
RGB, FLOW = spec.VARIANT_RGB, spec.VARIANT_FLOW
# workspace regions the recorder's digest mode hashes next to the three logit tensors: (name, channels)
REGIONS = (("fusion_28", 320), ("fusion_14", 1056), ("fusion_7", 832), ("xt_28", 128), ("sa_28", 256), ("sb_28", 256), ("xu_14", 256),
           ("sa_14", 512), ("xv_7", 512), ("sum_7", 1024))


def _cases():
    """id -> (switches, shape (a golden tag or (variant, B, L, feature config)), arithmetic modes, options).
    options: consensus (default False), want28 (default True), feat_layout (default 0), cl (channels_last maps: the _cl entry)."""
    out = {}
    # default handles: P = 1, 4, 18, 12, 40, 42, 72, and one pair below each gate (P = 11, 39, 71)
    for B, L in ((1, 2), (2, 3), (3, 7), (12, 2), (8, 6), (7, 7), (12, 7), (11, 2), (13, 4), (71, 2)):
        out["default-b%d-l%d" % (B, L)] = ({}, (RGB, B, L, 2), BOTH, {})
    for name, case in SWITCH_CASES.items():
        out["switches-" + name] = (case[0], case[1], case[2], {})
    p18, p42, p72, p4 = (RGB, 3, 7, 2), (RGB, 7, 7, 2), (RGB, 12, 7, 2), (RGB, 2, 3, 2)
    out["wino_mid0-p18"] = ({"OFFK_WINO_MID": "0"}, p18, BOTH, {})
    out["wino_mid0-p42"] = ({"OFFK_WINO_MID": "0"}, p42, BOTH, {})
    out["chain_wino0-p72"] = ({"OFFK_CHAIN_WINO": "0"}, p72, BOTH, {})
    out["wino_gemm0-p18"] = ({"OFFK_WINO_GEMM": "0"}, p18, BOTH, {})
    out["chain2-p18"] = ({"OFFK_CHAIN": "2"}, p18, BOTH, {})
    out["gates2-p4"] = ({"OFFK_WINOGRAD_5X5": "2", "OFFK_WINOGRAD_7X7": "2"}, p4, BOTH, {})
    out["consensus-p18"] = ({}, p18, BOTH, {"consensus": True})
    out["no28-p18"] = ({}, p18, BOTH, {"want28": False})
    out["flow-p18"] = ({}, (FLOW, 3, 7, 2), BOTH, {})
    out["nhwc-p4"] = ({}, p4, BOTH, {"feat_layout": 1})
    out["cl-p4"] = ({}, p4, SPLIT, {"cl": True})          # (channels_last maps reach the forward on split-fp32 handles only)
    return out


CASES = _cases()
CASE_PARAMS = [(k, p) for k, c in CASES.items() for p in c[2]]


def case_id(case, prec):
    return "%s|%s" % (case, prec)


def run_case(rt, golden_dir, case, prec):
    """(handle, launch-group names of one traced forward, its logits, the logits of the same forward with the trace off)."""
    env, shape, _precs, opt = CASES[case]
    variant, B, L, cfg, _g = shape_of(shape, golden_dir)
    h, _w = make_handle(rt, B, L, variant, consensus=opt.get("consensus", False), precision=prec, env=env, feat_layout=opt.get("feat_layout", 0))
    feats = [dev(f) for f in features(B, L, cfg)]
    if opt.get("feat_layout", 0) == 1:
        feats = [f.permute(0, 2, 3, 1).contiguous() for f in feats]
    if opt.get("cl"):
        feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
        assert h.takes_channels_last(feats)
    want28 = opt.get("want28", True)
    h.workspace.zero_()                                    # (the digest mode hashes whole regions)
    h.set_profiling(2)
    traced = h.forward(feats, want28=want28)
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    plain = h.forward(feats, want28=want28)
    torch.cuda.synchronize()
    return h, names, traced, plain


def dump_golden(plans_by_case, path):
    """{case id: names} as {"plans": {plan: names}, "cases": {case id: plan}}, one line per entry: many cases share a plan."""
    plans, cases = {}, {}
    for cid in sorted(plans_by_case):
        cases[cid] = plans.setdefault(tuple(plans_by_case[cid]), "plan%02d" % len(plans))
    with open(path, "w") as f:
        f.write('{"plans": {\n%s},\n"cases": {\n%s}}\n' % (",\n".join("%s: %s" % (json.dumps(v), json.dumps(list(k))) for k, v in plans.items()),
                                                          ",\n".join("%s: %s" % (json.dumps(c), json.dumps(v)) for c, v in cases.items())))
