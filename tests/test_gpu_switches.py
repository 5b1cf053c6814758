"""Every switch of INTEGRATION.md section 7 turned to its non-default value: the per-launch trace names the path that ran, and that path is
held to the goldens and to the oracle.

Until this module the GPU suite set OFFK_FUSED_UNITS, OFFK_SPLIT_GEMM, OFFK_WINO_MID, OFFK_CHAIN_WINO, OFFK_WINO_GEMM and the three
pair-count gates forced OPEN; nothing set OFFK_WINOGRAD=0, OFFK_CHAIN=0, OFFK_FOLD_POOL=0, OFFK_WINOGRAD_5X5=0, OFFK_WINOGRAD_7X7=0,
OFFK_SPLIT_CHAIN=0 or OFFK_SPLIT_MID=0, so the direct form of the seven Winograd convs inside the forward (residual / ReLU flags, channel
slices, pooling epilogue), pool_kernel + fc_kernel and the slab mode of the folded 14-head ran in no test.  Every case here asserts

  (a) the launches the setting must and must not produce (offk_launch_times),
  (b) the logits against the committed golden (where the shape has one) and against the oracle, < RTOL,
  (c) fusion_28 / fusion_14 / fusion_7 / sum_7 against the oracle's stage tensors, each < RTOL,
  (d) the row-to-row signal of all three logits, < RTOL_NORTH_STAR.

Also here: the pair-count gates at their boundaries, the documented accuracy of the direct path, and what INTEGRATION.md promises about
bit-identical results across batch sizes (test_pinned_paths_are_batch_invariant).
"""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from .featmaps import rt  # noqa: F401
from .forward import BOTH, CHAINS, FP32, HANDLE_PRECISIONS, P18, W5, W7, check_trace, check_whole_forward, dev, features, has, make_handle
from .forward import SWITCH_CASES as CASES
from .forward import oracle, shape_of, stage_errs, traced_forward

pytestmark = pytest.mark.gpu

# (the switch cases are a table of tests/forward.py: SWITCH_CASES, which tests/test_gpu_forward_plan.py reads too)
CASE_PARAMS = [pytest.param(k, p, id="%s-%s" % (k, p)) for k, c in CASES.items() for p in c[2]]


@pytest.mark.parametrize("case,prec", CASE_PARAMS)
def test_switch_off_path(rt, case, prec):
    env, shape, _precs, must, must_not, default_must, differs = CASES[case]
    if isinstance(must, dict):
        must, must_not = must[prec], must_not[prec]
    variant, B, L, cfg, _g = shape_of(shape)
    feats = [dev(f) for f in features(B, L, cfg)]
    h, w = make_handle(rt, B, L, variant, consensus=False, precision=prec, env=env)
    names, out = traced_forward(h, feats)
    check_trace(names, must, must_not)                                                   # (a)
    check_whole_forward(h, out, shape, w, "%s %s" % (case, prec))       # (b) (c) (d)
    if default_must is not None:
        h0, _ = make_handle(rt, B, L, variant, consensus=False, precision=prec)
        names0, _out0 = traced_forward(h0, feats)
        check_trace(names0, default_must, ())
        if differs is not None:     # the trace cannot tell the two kernels apart: the other one leaves other bits
            name, ch = differs
            assert not torch.equal(h.region(name, ch), h0.region(name, ch)), name


# ---- the pair-count gates at their boundaries ----------------------------------------------------------------------------------

GATES = {"7x7": ((11, 2), (12, 2), W7, BOTH), "5x5": ((13, 4), (8, 6), W5, BOTH), "chain": ((71, 2), (72, 2), "chain_28a", FP32)}


@pytest.mark.parametrize("gate,prec", [pytest.param(k, p, id="%s-%s" % (k, p)) for k, g in GATES.items() for p in g[3]])
def test_gate_boundary(rt, gate, prec):
    """Default handles one pair below each gate (P = 11 / 39 / 71: the gated launch is absent) and at it (P = 12 / 40 / 72: present, and
    the logits, stage tensors and signal against the oracle)."""
    below, at, sub, _precs = GATES[gate]
    for (B, L), present in ((below, False), (at, True)):
        feats = [dev(f) for f in features(B, L, 2)]
        h, w = make_handle(rt, B, L, spec.VARIANT_RGB, consensus=False, precision=prec)
        names, out = traced_forward(h, feats)
        assert has(names, sub) == present, (B * (L - 1), sub, names)
        if present:
            check_whole_forward(h, out, (spec.VARIANT_RGB, B, L, 2), w, "gate %s at P = %d %s" % (gate, B * (L - 1), prec))


def test_split_handles_chain_from_the_first_pair(rt):
    feats = [dev(f) for f in features(1, 2, 2)]
    h, _w = make_handle(rt, 1, 2, spec.VARIANT_RGB, consensus=False, precision="f32split")
    names, _out = traced_forward(h, feats)
    check_trace(names, CHAINS, ())
    h, _w = make_handle(rt, 1, 2, spec.VARIANT_RGB, consensus=False, precision="fp32")
    names, _out = traced_forward(h, feats)
    check_trace(names, (), ("chain_28",))


# ---- the documented accuracy of the direct path ----------------------------------------------------------------------------------

# worst stage-tensor error (fusion_28 / fusion_14 / fusion_7 / sum_7, max-normalised) against the oracle, fp32 handle, rgb_b3_l7, MI355X:
#   default (Winograd) paths 1.257e-05 (sum_7; fusion_14 5.67e-06), OFFK_WINOGRAD=0 1.346e-06 (fusion_7; sum_7 7.52e-07, fusion_14 1.14e-06)
DIRECT_MEASURED, WINOGRAD_MEASURED = 1.346e-06, 1.257e-05
DIRECT_BOUND = 4 * DIRECT_MEASURED     # run-to-run and box-to-box split-K differences


def test_direct_path_is_closer_to_the_oracle(rt):
    """INTEGRATION.md section 7, OFFK_WINOGRAD row: "≈ 1.3e-6 of the oracle instead of ≈ 1.3e-5".  Measured on an MI355X (fp32 handle,
    B = 3, L = 7, worst of the four stage tensors): direct 1.346e-06, Winograd 1.257e-05.  The direct path is held to 4 x its measured
    value, 5.4e-06 -- below what the Winograd path itself measures, or the sentence would say nothing."""
    variant, B, L, cfg, _g = shape_of(P18)
    feats = [dev(f) for f in features(B, L, cfg)]
    worst = {}
    for name, env in (("winograd", {}), ("direct", {"OFFK_WINOGRAD": "0"})):
        h, w = make_handle(rt, B, L, variant, consensus=False, precision="fp32", env=env)
        h.forward(feats)
        torch.cuda.synchronize()
        _want, st = oracle(variant, B, L, cfg, w)
        errs = stage_errs(h, st, B * (L - 1))
        worst[name] = max(errs.values())
        print("worst stage error vs oracle, %s path: %.3e (%s)" % (name, worst[name], " ".join("%s %.2e" % kv for kv in errs.items())))
    assert DIRECT_BOUND < WINOGRAD_MEASURED
    assert worst["direct"] < DIRECT_BOUND, worst
    assert worst["direct"] < worst["winograd"], worst


# ---- bit-identical results across batch sizes ------------------------------------------------------------------------------------

def set_same_plans(h):
    """One (tile, split-K depth) per fusion conv and merged conv, whatever the handle's size (offk_set_conv_plan): left alone,
    conv2d_auto_plan picks the depth from the grid -- motion_conv_trans_14: 48 slices at P = 3, 32 at P = 12."""
    for key, _co, _ci, k, _s, _p in spec.FUSION_CONVS:
        h.set_conv_plan(key, 3, 4 if k > 1 else 1)
    for key in ("merged_28a", "merged_14a", "merged_7"):
        h.set_conv_plan(key, 3, 1)


BATCH_PIN = {"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0", "OFFK_FOLD_POOL": "0"}


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("B", [4, 24])
def test_pinned_paths_are_batch_invariant(rt, B, prec):
    """per_clip slicing, OFFK_WINOGRAD=0 OFFK_CHAIN=0 OFFK_FOLD_POOL=0 and one conv plan for every handle give
    the logits of a clip BIT for bit, alone (P = 3) or inside a batch (P = 12; P = 72, where an unpinned fp32 handle would fuse the chains).

    Measured on an MI355X, B = 4 against B = 1, both arithmetic modes, with the stage regions compared clip by clip:
      * OFFK_WINOGRAD=0 OFFK_CHAIN=0 alone (what the document promised before): every fusion stage differs from xt_28 on (the split-K
        depths follow the grid), logits to 2.4e-7;
      * + OFFK_FOLD_POOL=0 alone: the same;
      * + the plans alone: every stage region identical, the 7- and 14-head logits of clips 1 .. 3 differ (1.9e-7 .. 2.2e-7): the folded
        average pool sums an image's 49 rows in per-slab pieces cut at img 49 mod 32 (clip 0 starts on a slab boundary in both handles);
      * + both: identical.  OFFK_FUSED_UNITS=0 is not needed; with the Winograd paths left on (the 7x7 gate at P = 12) xt_28 differs."""
    L = 4
    feats = synth.make_features(B, L, 6)
    hb, _w = make_handle(rt, B, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, precision=prec, env=BATCH_PIN)
    h1, _w = make_handle(rt, 1, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, precision=prec, env=BATCH_PIN)
    set_same_plans(hb)
    set_same_plans(h1)
    big = hb.forward([dev(f) for f in feats])
    for b in range(B):
        alone = h1.forward([dev(f) for f in synth.make_features(1, L, 6, clip_offset=b)])
        for x, y in zip(big, alone):
            assert torch.equal(x[b * (L - 1):(b + 1) * (L - 1)], y), b
