"""The case table of the weight-update tests (tests/test_weight_update_cases.py on the CPU, tests/test_gpu_weight_updates.py and its
siblings on the GPU): every state_dict key of the OFF sub-network, the group it is parametrised under, a deterministic perturbation
of its tensor, and the heads the key can change.

A handle keeps a weight up to four times over (the plain copy, the operand-order images of the fused units kernel, the merged
[main | branch] matrices, the derived images of offk_api.hip's kDerived), held together by three dirty flags; the tests built on
this table update ONE key after a first forward and ask whether every kernel that reads that weight saw it.

The dependency table (feeds) is derived from spec.FUSION, not typed in: a fusion stage reads its own units and carries the output
of the stage before it (spec.FUSION[..]["carry"]), so the 28x28 units and the fusion@28 convs reach all three heads, the 14x14
ones the 14- and the 7-head, the 7x7 ones the 7-head alone, and each FC its own head.  tests/test_weight_update_cases.py proves
the table against the fp64 oracle, key by key.
"""
import functools

import numpy as np
import torch

from offk_amd import spec, synth

from .arena import same_bits
from .forward import HANDLE_PRECISIONS, dev

VARIANTS = (spec.VARIANT_RGB, spec.VARIANT_FLOW)
VARIANT_TAGS = {spec.VARIANT_RGB: "rgb", spec.VARIANT_FLOW: "flow"}
B, L = 1, 3          # P = 2: the smallest shape at which a gate forced to "2" (from 2 pairs) still opens
HEAD_ORDER = ("7", "14", "28")         # the order every forward returns its logits in
GROUPS = ("gen_w", "gen_b", "down_w", "down_b", "dw_w", "dw_b", "sobel",
          "conv1x1_w", "conv3x3_w", "conv5x5_w", "conv7x7_w", "branch_w", "conv_b", "fc_w", "fc_b")
RGB_ONLY, FLOW_ONLY = ("dw_w", "dw_b"), ("sobel",)
# the branch 1x1 convs, the second halves of the merged [main | branch] matrices (RGB_OFF.py:665, :769, :840)
BRANCH_CONVS = ("motion_conv_branch_28a", "motion_conv_expand_trans_14a", "motion_conv_branch_trans")
# (main, branch) of each merged conv
MERGED_PAIRS = (("motion_conv3_trans_28a", "motion_conv_branch_28a"), ("motion_conv3_trans_14a", "motion_conv_expand_trans_14a"),
                ("motion_conv3_trans", "motion_conv_branch_trans"))
_UNIT_GROUPS = {"motion_conv_gen_": "gen", "motion_spatial_down_": "down", "motion_spatial_grad_": "dw"}
_CONV_K = dict((key, k) for key, _co, _ci, k, _s, _p in spec.FUSION_CONVS)
_HEAD_OF_FC = {"fc_action_motion": "7", "fc_action_motion_14": "14", "fc_action_motion_28": "28"}


def keys(variant):
    return list(spec.weight_shapes(variant))


def group(key):
    base, kind = key.rsplit(".", 1)
    sfx = "_w" if kind == "weight" else "_b"
    if key == spec.SOBEL_KEY:
        return "sobel"
    for prefix, g in _UNIT_GROUPS.items():
        if base.startswith(prefix):
            return g + sfx
    if base in _HEAD_OF_FC:
        return "fc" + sfx
    if base in _CONV_K:
        if kind == "bias":
            return "conv_b"
        if base in BRANCH_CONVS:
            return "branch_w"
        return "conv%dx%d_w" % (_CONV_K[base], _CONV_K[base])
    raise KeyError(key)


def groups(variant):
    """The groups the variant has, in GROUPS order."""
    skip = FLOW_ONLY if variant == spec.VARIANT_RGB else RGB_ONLY
    return [g for g in GROUPS if g not in skip]


def keys_of(variant, grp):
    return [k for k in keys(variant) if group(k) == grp]


# ---- the perturbation ------------------------------------------------------------------------------------------------------------
_D_EIGHTHS = np.array([1, -2, 2, -1, 3, -1, 1, -3], dtype=np.float32)      # never zero, sums to zero


def _d_scale(key):
    """d times this, for the keys whose farthest head moves by less than 1e-3 of its logits under the plain pattern (the fp64 oracle at
    B = 1, L = 3, d as it is: a unit bias of a 28x28 site moves the 7-head by 9e-5 .. 6e-4, one of a 14x14 site by 9e-4 .. 3e-3, a bias of a fusion@28
    conv by 9e-4 .. 3e-3).  tests/test_weight_update_cases.py holds every key to that 1e-3 with these factors in."""
    grp, stage = group(key), stage_of(key)
    if grp == "gen_b":
        return {"28": 8, "14": 4, "7": 1}[stage]
    if grp in ("down_b", "dw_w", "dw_b"):
        return {"28": 32, "14": 4, "7": 1}[stage]
    if grp == "conv_b" and stage == "28":
        return 4
    return 1


def delta(key, shape):
    """The fixed non-zero integer-over-8 pattern of a key's shape: element i holds _D_EIGHTHS[(i + i // 7) % 8] / 8 (the i // 7 keeps a
    period of 8 from lining up with the channel counts, all multiples of 8)."""
    n = int(np.prod(shape))
    i = np.arange(n)
    d = _D_EIGHTHS[(i + i // 7) % 8]
    if group(key) == "gen_b":
        # one sign: the temporal difference cancels a bias wherever the ReLU is open in both frames, so a gen bias acts only through the
        # ReLUs it opens or closes, and a pattern of both signs saturates at 1.0e-3 of the 7-head for the 28x28 sites, whatever its size
        d = np.abs(d)
    return (d * np.float32(0.125 * _d_scale(key))).reshape(shape)


def perturbed(key, w):
    """1.5 w + d, fp32: every element moves, zeros too (the four-tap Sobel weight becomes a dense nine-tap weight)."""
    w = np.asarray(w, dtype=np.float32)
    return (np.float32(1.5) * w + delta(key, w.shape)).astype(np.float32)


def with_key(w0, key, value=None):
    """A copy of the weight dict w0 (the arrays shared) with `key` perturbed, or set to `value`."""
    w1 = dict(w0)
    w1[key] = perturbed(key, w0[key]) if value is None else value
    return w1


# ---- which heads a key can change --------------------------------------------------------------------------------------------------
def _downstream():
    """fusion stage -> heads behind it: a stage with carry > 0 takes the output of the stage listed before it (spec.FUSION)."""
    order = list(spec.FUSION)
    out = {}
    for i, name in enumerate(order):
        heads = {name}
        for later in order[i + 1:]:
            if spec.FUSION[later]["carry"] == 0:
                break
            heads.add(later)
        out[name] = frozenset(heads)
    return out


_DOWNSTREAM = _downstream()
_STAGE_OF_SITE = dict((s, name) for name, f in spec.FUSION.items() for s in f["sites"])


def stage_of(key):
    """The fusion stage ("28", "14", "7") a unit or fusion-conv key belongs to; None for the Sobel weight (all nine sites) and the FCs."""
    base = key.rsplit(".", 1)[0]
    if key == spec.SOBEL_KEY or base in _HEAD_OF_FC:
        return None
    for prefix in _UNIT_GROUPS:
        if base.startswith(prefix):
            return _STAGE_OF_SITE[base[len(prefix):]]
    assert base in _CONV_K, key
    tail = base.rsplit("_", 1)[1]
    return "28" if tail.startswith("28") else "14" if tail.startswith("14") else "7"


def feeds(key):
    """The heads a key can change, a subset of {"7", "14", "28"}."""
    base = key.rsplit(".", 1)[0]
    if base in _HEAD_OF_FC:
        return frozenset((_HEAD_OF_FC[base],))
    if key == spec.SOBEL_KEY:
        return frozenset(HEAD_ORDER)
    return _DOWNSTREAM[stage_of(key)]


def site_of(key):
    """Index into spec.SITES of a unit key."""
    base = key.rsplit(".", 1)[0]
    for prefix in _UNIT_GROUPS:
        if base.startswith(prefix):
            return spec.SITE_NAMES.index(base[len(prefix):])
    raise KeyError(key)


# ---- the GPU side: the configurations, one forward and what it left (tests/test_gpu_weight_updates.py, test_gpu_bound_weights.py) ----
FEATURE_CONFIG = 2
GATES_OPEN = {"OFFK_CHAIN": "2", "OFFK_WINOGRAD_5X5": "2", "OFFK_WINOGRAD_7X7": "2", "OFFK_POOL_FIRST_7": "2"}
SPLIT = "f32split"
CONFIGS = {
    "default": ({}, HANDLE_PRECISIONS),
    "gates_open": (GATES_OPEN, HANDLE_PRECISIONS),
    "unfused_units": ({"OFFK_FUSED_UNITS": "0"}, HANDLE_PRECISIONS),
    "direct_convs": ({"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0"}, HANDLE_PRECISIONS),
    "split_on_fp32_pipe": (dict(GATES_OPEN, OFFK_SPLIT_GEMM="0", OFFK_SPLIT_CHAIN="0", OFFK_SPLIT_MID="0"), [SPLIT]),
}
REGIONS = [("fusion_28", 320), ("fusion_14", 1056), ("fusion_7", 832)] + [("D_" + s, spec.DOWN_CH) for s in spec.SITE_NAMES] + [("sum_7", 1024)]


@functools.lru_cache(maxsize=None)
def _feats():
    return tuple(dev(f) for f in synth.make_features(B, L, FEATURE_CONFIG))


def feats():
    return list(_feats())


def run(h):
    """One forward: name -> a copy of the three heads and of every stage region."""
    out = h.forward(feats())
    snap = dict((name, o.clone()) for name, o in zip(HEAD_ORDER, out))
    for name, ch in REGIONS:
        snap[name] = h.region(name, ch).clone()
    torch.cuda.synchronize()
    return snap


def differing(a, b):
    return sorted(name for name in a if not same_bits(a[name], b[name]))
