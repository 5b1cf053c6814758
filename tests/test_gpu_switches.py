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
import os

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

from .test_gpu_parity import GOLDEN, HANDLE_PRECISIONS, RTOL, RTOL_NORTH_STAR, dev, make_handle, rel_err, rt, signal_err  # noqa: F401
from .test_gpu_paths import STAGES, stage_errs

pytestmark = pytest.mark.gpu

# shapes: a golden tag (variant, B, L and the feature config come from its meta) or (variant, B, L, feature config)
P18, P18_FLOW, P4 = "rgb_b3_l7", "flow_b3_l7", "rgb_b2_l3"
P42 = (spec.VARIANT_RGB, 7, 7, 2)
P72 = (spec.VARIANT_RGB, 12, 7, 2)

WINO, CHAINS = "[winograd", ("chain_28a", "chain_28b", "chain_28c")
FC_FOLDED, POOL_ROWS_28 = "heads (fc on folded pools, one launch)", "head_28 (max pool rows)"
POOL_FC = ("head_7 (pool + fc)", "head_14 (pool + fc)", "head_28 (pool + fc)")
W5, W7, BETWEEN = "motion_conv_trans_14 [winograd", "motion_conv_trans_28 [winograd", "[winograd: between]"


def switched_handle(rt, monkeypatch, env, *args, **kw):
    """The pattern of test_gpu_paths.forced_handle: the switches are read once, at offk_create."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return make_handle(rt, *args, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def shape_of(shape, golden_dir):
    if isinstance(shape, str):
        g = np.load(os.path.join(golden_dir, shape + ".npz"))
        variant, B, L, cfg = (int(v) for v in g["meta"])
        return variant, B, L, cfg, g
    return shape + (None,)


_FEATS, _ORACLE = {}, {}


def features(B, L, cfg):
    """The nine maps of a shape; the last two shapes asked for are kept (the cases of one shape run one after the other)."""
    if (B, L, cfg) not in _FEATS:
        while len(_FEATS) >= 2:
            _FEATS.pop(next(iter(_FEATS)))
        _FEATS[(B, L, cfg)] = synth.make_features(B, L, cfg)
    return _FEATS[(B, L, cfg)]


def oracle(variant, B, L, cfg, w):
    """(logits, stage tensors) of the oracle, once per shape: shared by every case and both arithmetic modes, never written to."""
    key = (variant, B, L, cfg)
    if key not in _ORACLE:
        with torch.no_grad():
            want, st = orc.off_forward([torch.from_numpy(f) for f in features(B, L, cfg)], w, B, L, variant, orc.SLICE_FLAT,
                                       consensus=False, return_stages=True)
        _ORACLE[key] = (want, dict((name, st[name]) for name, _ch, _H in STAGES))
    return _ORACLE[key]


def traced_forward(h, feats):
    """One forward with the per-launch trace on: (names of its launch groups, logits)."""
    h.set_profiling(2)
    out = h.forward(feats)
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    return names, out


def has(names, sub):
    return any(sub in n for n in names)


def check_trace(names, must, must_not):
    for sub in must:
        assert has(names, sub), (sub, names)
    for sub in must_not:
        assert not has(names, sub), (sub, names)


def check_against_references(h, out, shape, golden_dir, w, what):
    """(b), (c), (d) of the module docstring."""
    variant, B, L, cfg, g = shape_of(shape, golden_dir)
    P = B * (L - 1)
    want, st = oracle(variant, B, L, cfg, w)
    lerr = [rel_err(a, b.reshape(a.shape)) for a, b in zip(out, want)]
    errs = stage_errs(h, st, P)
    sig = [signal_err(a, b) for a, b in zip(out, want)]
    gerr = [rel_err(a, g[k]) for a, k in zip(out, ("fc7", "fc14", "fc28"))] if g is not None else []
    gsig = [signal_err(a, g[k]) for a, k in zip(out, ("fc7", "fc14", "fc28"))] if g is not None else []
    print("%s: logits vs oracle %s, vs golden %s; stages %s; signal vs oracle %s, vs golden %s"
          % (what, " ".join("%.1e" % v for v in lerr), " ".join("%.1e" % v for v in gerr) or "-",
             " ".join("%s %.1e" % kv for kv in errs.items()), " ".join("%.1e" % v for v in sig), " ".join("%.1e" % v for v in gsig) or "-"))
    assert max(lerr + gerr) < RTOL, (lerr, gerr)
    assert max(errs.values()) < RTOL, errs
    assert max(sig + gsig) < RTOL_NORTH_STAR, (sig, gsig)
    return errs


# id -> (switches, shape, arithmetic modes, launches that must be there, launches that must not,
#        launches the DEFAULT handle of the same shape must show (None: not compared), region that must differ bitwise from the default handle's)
FP32, SPLIT, BOTH = ("fp32",), ("f32split",), tuple(HANDLE_PRECISIONS)
NO_WINO_CHAIN = {"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0"}


def winograd0(shape):
    """OFFK_WINOGRAD=0, per arithmetic mode: fp32 handles sit below their chain gate (72 pairs); split-fp32 handles keep theirs at the first
    pair and, with no plane images packed for chain_split.hip, run chain_fused.hip's direct 3x3 form (OFFK_WINOGRAD row)."""
    return ({"OFFK_WINOGRAD": "0"}, shape, BOTH, {"fp32": (FC_FOLDED,), "f32split": (FC_FOLDED,) + CHAINS},
            {"fp32": (WINO, "head_14 (pool + fc)", "chain_28"), "f32split": (WINO, "head_14 (pool + fc)")}, None, None)


CASES = {
    # direct implicit GEMMs everywhere, the 14-head's pool in conv_igemm's epilogue + fc_pooled in slab mode (winograd0 above)
    "winograd0": winograd0(P18), "winograd0-flow": winograd0(P18_FLOW), "winograd0-p4": winograd0(P4),
    # the documented pin of INTEGRATION.md section 7
    "winograd0-chain0-p18": (NO_WINO_CHAIN, P18, BOTH, ("motion_conv2_trans_28a",), (WINO, "chain_28"), None, None),
    "winograd0-chain0-p72": (NO_WINO_CHAIN, P72, BOTH, ("motion_conv2_trans_28a",), (WINO, "chain_28"), None, None),
    # pool_kernel + fc_kernel for all three heads
    "fold_pool0": ({"OFFK_FOLD_POOL": "0"}, P18, BOTH, POOL_FC, ("heads (fc on folded", POOL_ROWS_28), (FC_FOLDED, POOL_ROWS_28), None),
    "fold_pool0-winograd0": ({"OFFK_FOLD_POOL": "0", "OFFK_WINOGRAD": "0"}, P18, BOTH, POOL_FC, ("heads (fc on folded", POOL_ROWS_28, WINO), None, None),
    "chain0-p72": ({"OFFK_CHAIN": "0"}, P72, BOTH, ("motion_conv2_trans_28a", WINO), ("chain_28",), CHAINS, None),
    "winograd_5x5_0": ({"OFFK_WINOGRAD_5X5": "0"}, P42, BOTH, (W7, "motion_conv2_trans_14a [winograd", "motion_conv_trans [winograd"), (W5,), (W5, W7), None),
    "winograd_7x7_0": ({"OFFK_WINOGRAD_7X7": "0"}, P42, BOTH, (W5, "motion_conv2_trans_14a [winograd", "motion_conv_trans [winograd"), (W7,), (W5, W7), None),
    # split-fp32 handles: the chain gate back at 72 pairs; chain_fused.hip in place of chain_split.hip; wino_mid's 1x1 convs on the fp32 pipe
    "split_chain0": ({"OFFK_SPLIT_CHAIN": "0"}, P18, SPLIT, ("motion_conv2_trans_28a",), ("chain_28",), CHAINS, None),
    "chain2-split_chain0": ({"OFFK_CHAIN": "2", "OFFK_SPLIT_CHAIN": "0"}, P18, SPLIT, CHAINS, (), CHAINS, ("sa_28", 256)),
    "split_mid0": ({"OFFK_SPLIT_MID": "0"}, P18, SPLIT, (BETWEEN,), (), (BETWEEN,), ("xv_7", 512)),
    # switches other modules already turn, without saying which path ran: K1 + K2 apart; the Winograd GEMMs and the 1x1 convs on 7x7 maps
    # of a split-fp32 handle on the fp32 pipe.  (OFFK_WINO_GEMM=0 leaves the same launch names AND the same bits --
    # test_wino_gemm_persistent_matches_generic -- so nothing a test can read tells its two kernels apart.)
    "fused_units0": ({"OFFK_FUSED_UNITS": "0"}, P18, BOTH, ("units:pw_reduce (K1)", "units:sobel_tdiff (K2)"), ("units:pw_tdiff",), ("units:pw_tdiff (K1T)",), None),
    "split_gemm0": ({"OFFK_SPLIT_GEMM": "0"}, P18, SPLIT, (WINO,), (), (WINO,), ("sum_7", 1024)),
}
CASE_PARAMS = [pytest.param(k, p, id="%s-%s" % (k, p)) for k, c in CASES.items() for p in c[2]]


@pytest.mark.parametrize("case,prec", CASE_PARAMS)
def test_switch_off_path(rt, monkeypatch, golden_dir, case, prec):
    env, shape, _precs, must, must_not, default_must, differs = CASES[case]
    if isinstance(must, dict):
        must, must_not = must[prec], must_not[prec]
    variant, B, L, cfg, _g = shape_of(shape, golden_dir)
    feats = [dev(f) for f in features(B, L, cfg)]
    h, w = switched_handle(rt, monkeypatch, env, B, L, variant, consensus=False, precision=prec)
    names, out = traced_forward(h, feats)
    check_trace(names, must, must_not)                                                   # (a)
    check_against_references(h, out, shape, golden_dir, w, "%s %s" % (case, prec))       # (b) (c) (d)
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
def test_gate_boundary(rt, golden_dir, gate, prec):
    """Default handles one pair below each gate (P = 11 / 39 / 71: the gated launch is absent) and at it (P = 12 / 40 / 72: present, and
    the logits, stage tensors and signal against the oracle)."""
    below, at, sub, _precs = GATES[gate]
    for (B, L), present in ((below, False), (at, True)):
        feats = [dev(f) for f in features(B, L, 2)]
        h, w = make_handle(rt, B, L, spec.VARIANT_RGB, consensus=False, precision=prec)
        names, out = traced_forward(h, feats)
        assert has(names, sub) == present, (B * (L - 1), sub, names)
        if present:
            check_against_references(h, out, (spec.VARIANT_RGB, B, L, 2), golden_dir, w, "gate %s at P = %d %s" % (gate, B * (L - 1), prec))


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


def test_direct_path_is_closer_to_the_oracle(rt, monkeypatch, golden_dir):
    """INTEGRATION.md section 7, OFFK_WINOGRAD row: "≈ 1.3e-6 of the oracle instead of ≈ 1.3e-5".  Measured on an MI355X (fp32 handle,
    B = 3, L = 7, worst of the four stage tensors): direct 1.346e-06, Winograd 1.257e-05.  The direct path is held to 4 x its measured
    value, 5.4e-06 -- below what the Winograd path itself measures, or the sentence would say nothing."""
    variant, B, L, cfg, _g = shape_of(P18, golden_dir)
    feats = [dev(f) for f in features(B, L, cfg)]
    worst = {}
    for name, env in (("winograd", {}), ("direct", {"OFFK_WINOGRAD": "0"})):
        h, w = switched_handle(rt, monkeypatch, env, B, L, variant, consensus=False, precision="fp32")
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
def test_pinned_paths_are_batch_invariant(rt, monkeypatch, B, prec):
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
    hb, _w = switched_handle(rt, monkeypatch, BATCH_PIN, B, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, precision=prec)
    h1, _w = switched_handle(rt, monkeypatch, BATCH_PIN, 1, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, precision=prec)
    set_same_plans(hb)
    set_same_plans(h1)
    big = hb.forward([dev(f) for f in feats])
    for b in range(B):
        alone = h1.forward([dev(f) for f in synth.make_features(1, L, 6, clip_offset=b)])
        for x, y in zip(big, alone):
            assert torch.equal(x[b * (L - 1):(b + 1) * (L - 1)], y), b
