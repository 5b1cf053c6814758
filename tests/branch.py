"""The whole motion branch as INTEGRATION.md section 5 wires it -- ``OFFUnits``, the 24 ``FusionConv2d``, the three ``MotionHead`` -- and
the fp64 reference of one training step through it.  No tests of its own: tests/test_branch_reference.py (CPU) shows that the reference
can carry the comparison, tests/test_gpu_branch_step.py makes it.

Two statements of the topology meet here.  ``Branch`` is the device's, written from the recipe: it uses nothing of the oracle.
``reference_step`` runs the oracle's (oracle/off_oracle.py, pinned to the reference by the goldens).

Why the reference takes the device's activation pattern (DESIGN.md section 8.7 has the figures): the branch has about 3.6 M ReLU
elements at B = 2, L = 3, torch fp32 and fp64 decide two of them differently (|z| = 2.8e-8 at scale 2.2, 7.2e-8 at scale 0.5), and that
moves a weight gradient by 2.1e-2 of its max -- 100 x RTOL.  The 28-head's max-pool likewise: the two largest values of a window come
within 7.5e-7 of the map's max of each other.  So the fp64 side computes ``z * mask`` with the device's masks and gathers the pool at the device's
route, after ``check_pattern`` has shown that every decision that differs from fp64's own sits within rounding distance of its kink.
Then both sides differentiate the same piecewise-linear function and the reference alone stays below RTOL / 10.

The step is train_off.py:135-146 with one cross-entropy per head (the script's own :128-130 hand ``rst1`` to all three criteria; the
heads train only with their own logits, which is what its comments say and what is tested): loss7, loss14, loss28, and
``loss7.backward(retain_graph=True); loss14.backward(retain_graph=True); loss28.backward()`` -- or one backward of the sum.
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc        # reference_step and its helpers only; Branch and pattern_of use none of it

RTOL = 2e-4                     # of each tensor's max magnitude (tests/test_gpu_backward.py)
DROP_P = 0.8                    # nn.Dropout of the units (RGB_OFF.py:356) and of the heads (:785, :791, :845)
SLACK = {False: 1e-5, True: 1e-4}          # check_pattern's slack: default arithmetic / split switches on (tests/test_gpu_backward.py)
FEATURE_CONFIG = 2
TARGETS = (3, 77, 18, 50)       # one class per pair row
LR = 0.1                        # plain SGD of the two-step test; tests/test_branch_reference.py shows that it moves every gradient

#        name           variant B  L  seed  split   summed
CASES = {
    "rgb_b2_l3":       ("rgb",  2, 3, 7,    False,  False),     # P = 4: the flat slice (quirk Q1) takes a frame of the next clip
    "rgb_b1_l2":       ("rgb",  1, 2, 11,   False,  True),      # P = 1: one image everywhere, the squeeze edge
    "flow_b1_l4":      ("flow", 1, 4, 5,    False,  False),     # P = 3: odd count, frozen Sobel
    "rgb_b2_l3_split": ("rgb",  2, 3, 7,    True,   False),     # all five arithmetic switches, maps with a gradient
}
STEP2_SEED = 23                 # the two-step test's second step

# ---- the device side ------------------------------------------------------------------------------------------------------------------
# key -> (relu, relu_in, the conv whose output is this one's residual).  RGB_OFF.py:655-685, :759-780, :831-841.
WIRING = {
    "motion_conv_trans_28": (False, False, None),                       # x0: leaves pre-ReLU, the 28a branch reads it so (:665)
    "motion_conv1_trans_28a": (True, True, None),                       # reads max(x0, 0) (:658)
    "motion_conv2_trans_28a": (True, False, None),
    "motion_conv3_trans_28a": (True, False, "motion_conv_branch_28a"),
    "motion_conv_branch_28a": (False, False, None),
    "motion_conv_trans_14": (True, False, None),
    "motion_conv1_trans_14a": (True, False, None),
    "motion_conv2_trans_14a": (True, False, None),
    "motion_conv3_trans_14a": (True, False, "motion_conv_expand_trans_14a"),
    "motion_conv_expand_trans_14a": (False, False, None),
    "motion_conv1_trans_14b": (True, False, None),
    "motion_conv2_trans_14b": (True, False, None),
    "motion_conv3_trans_14b": (True, False, None),                      # 3x3 with its own ReLU; the join relu(s + .) is torch's (:779-780)
    "motion_conv_trans": (True, False, None),
    "motion_conv1_trans": (True, False, None),
    "motion_conv2_trans": (True, False, None),
    "motion_conv3_trans": (False, False, "motion_conv_branch_trans"),   # no ReLU behind the last join (:841)
    "motion_conv_branch_trans": (False, False, None),
}
for _blk in ("28b", "28c"):
    WIRING["motion_conv1_trans_" + _blk] = (True, False, None)
    WIRING["motion_conv2_trans_" + _blk] = (True, False, None)
    WIRING["motion_conv3_trans_" + _blk] = (True, False, "block input")
#          attribute              channels  maxpool  head_index
HEADS = (("fc_action_motion_28", 256, True, 0), ("fc_action_motion_14", 512, False, 1), ("fc_action_motion", 1024, False, 2))
FUSION_RELUS = ("x0", "c1_28a", "c2_28a", "s28a", "c1_28b", "c2_28b", "s28b", "c1_28c", "c2_28c", "s28c",
                "x1", "c1_14a", "c2_14a", "s14a", "c1_14b", "c2_14b", "c3_14b", "s14b", "x2", "c1_7", "c2_7")


class Branch(nn.Module):
    """The trainable motion branch of INTEGRATION.md section 5 under the reference's attribute names.  ``split``: every opt-in
    arithmetic switch at once (the units' three, wgrad_arith on the 22 stride-1 convs, dgrad_arith on the two openers)."""

    def __init__(self, batch, length, variant="rgb", split=False, feat_grad=False, num_classes=spec.NUM_CLASSES):
        super().__init__()
        from offk_amd import off_module as om
        ar = "f32split" if split else "fp32"
        self.off_units = om.OFFUnits(batch, length, variant=variant, precision="fp32", drop_p=DROP_P, feat_grad=feat_grad,
                                     feat_grad_arith=ar, wgrad_arith=ar, fwd_arith=ar)
        assert set(WIRING) == set(c[0] for c in spec.FUSION_CONVS)
        for key, co, ci, k, s, p in spec.FUSION_CONVS:
            relu, relu_in, _res = WIRING[key]
            sw = {"dgrad_arith": ar} if s == 2 else {"wgrad_arith": ar}
            setattr(self, key, om.FusionConv2d(ci, co, k, stride=s, padding=p, relu=relu, relu_in=relu_in, **sw))
        for key, cin, maxpool, index in HEADS:
            setattr(self, key, om.MotionHead(cin, num_classes, maxpool=maxpool, head_index=index, drop_p=DROP_P))
        self.acts = {}

    # the units' parameters sit one level down; checkpoints are flat (as off_module.BNInception_OFF does for 'off.')
    def state_dict(self, *a, **kw):
        sd = super().state_dict(*a, **kw)
        return type(sd)((k[len("off_units."):] if k.startswith("off_units.") else k, v) for k, v in sd.items())

    def load_state_dict(self, state_dict, strict=True, **kw):
        units = set(self.off_units.state_dict().keys())
        return super().load_state_dict(dict((("off_units." + k) if k in units else k, v) for k, v in state_dict.items()), strict=strict, **kw)

    def forward(self, feats, seed):
        """(fc7, fc14, fc28) as [P, classes] each.  Keeps every tensor a ReLU produced (x0: the tensor it reads) in ``self.acts``."""
        t = self.acts = {}
        m28, m14, m7 = self.off_units(feats, drop_seed=seed)
        # stage 28 (:655-685)
        x0 = t["x0"] = self.motion_conv_trans_28(m28)
        a = t["c1_28a"] = self.motion_conv1_trans_28a(x0)
        a = t["c2_28a"] = self.motion_conv2_trans_28a(a)
        s = t["s28a"] = self.motion_conv3_trans_28a(a, res=self.motion_conv_branch_28a(x0))
        for blk in ("28b", "28c"):
            a = t["c1_" + blk] = getattr(self, "motion_conv1_trans_" + blk)(s)
            a = t["c2_" + blk] = getattr(self, "motion_conv2_trans_" + blk)(a)
            s = t["s" + blk] = getattr(self, "motion_conv3_trans_" + blk)(a, res=s)
        motion_sum_28c = s
        fc28 = self.fc_action_motion_28(motion_sum_28c, drop_seed=seed)                          # :782-787
        # stage 14 (:759-780)
        x1 = t["x1"] = self.motion_conv_trans_14(torch.cat((m14, motion_sum_28c), 1))
        a = t["c1_14a"] = self.motion_conv1_trans_14a(x1)
        a = t["c2_14a"] = self.motion_conv2_trans_14a(a)
        s = t["s14a"] = self.motion_conv3_trans_14a(a, res=self.motion_conv_expand_trans_14a(x1))
        a = t["c1_14b"] = self.motion_conv1_trans_14b(s)
        a = t["c2_14b"] = self.motion_conv2_trans_14b(a)
        a = t["c3_14b"] = self.motion_conv3_trans_14b(a)
        motion_sum_14b = t["s14b"] = torch.relu(s + a)
        fc14 = self.fc_action_motion_14(motion_sum_14b, drop_seed=seed)                          # :789-793
        # stage 7 (:831-847)
        x2 = t["x2"] = self.motion_conv_trans(torch.cat((m7, motion_sum_14b), 1))
        a = t["c1_7"] = self.motion_conv1_trans(x2)
        a = t["c2_7"] = self.motion_conv2_trans(a)
        s7 = self.motion_conv3_trans(a, res=self.motion_conv_branch_trans(x2))
        fc7 = self.fc_action_motion(s7, drop_seed=seed)
        return fc7, fc14, fc28


def pattern_of(branch):
    """The decisions the device took in the forward that has just run: 21 fusion masks (y > 0 of the recorded tensors), nine gen masks
    (the handle's saved G > 0, as tests/test_gpu_backward.device_relu_masks reads them) and the 28-head's pool route -- the first
    maximum of the values the kernel saw (what tests/test_gpu_head_bwd_exact.py holds MotionHead to)."""
    u = branch.off_units
    n = u.batch * u.length
    masks = dict((k, (v.detach() > 0).cpu()) for k, v in branch.acts.items())
    assert set(masks) == set(FUSION_RELUS)
    gen = []
    for site, _c, H in spec.SITES:
        G = u._rt.region("G_" + site, 128).view(n, H * H, 128).permute(0, 2, 1).reshape(n, 128, H, H)
        gen.append((G > 0).cpu())
    s28 = branch.acts["s28c"].detach().cpu().double()
    _v, idx = F.max_pool2d(s28, 3, 2, ceil_mode=True, return_indices=True)
    return {"masks": masks, "gen": gen, "pool_idx": idx}


def check_pattern(pattern, free_run, slack):
    """tests/test_gpu_backward.device_relu_masks' two conditions on every mask of ``pattern`` against the free fp64 run: at most
    5 + slack * numel decisions differ, each at |z64| < slack * max(1, max |z64|).  The pool route: the same cap on the count, and the
    fp64 values at the two competing positions differ by less than slack * max.  Returns (ReLU flips, pool flips)."""
    named = list(pattern["masks"].items()) + [("gen_" + site, m) for (site, _c, _h), m in zip(spec.SITES, pattern["gen"])]
    assert len(named) == len(FUSION_RELUS) + spec.NUM_SITES
    flips = 0
    for name, mask in named:
        z = free_run["pre"][name]
        flip = mask.bool() != (z > 0)
        n = int(flip.sum())
        assert n <= 5 + slack * flip.numel(), (name, n)
        if n:
            worst = float(z[flip].abs().max())
            assert worst < slack * max(1.0, float(z.abs().max())), (name, n, worst)
        flips += n
    own, idx = free_run["pool_idx"], pattern["pool_idx"]
    diff = idx != own
    n = int(diff.sum())
    assert n <= 5 + slack * diff.numel(), ("pool", n)
    if n:
        s = free_run["pre"]["pool_in"].flatten(2)
        gap = (s.gather(2, own.flatten(2)) - s.gather(2, idx.flatten(2))).abs().view(idx.shape)[diff]
        assert float(gap.max()) < slack * float(s.abs().max()), ("pool", n, float(gap.max()))
    return flips, n


# ---- the reference side ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(variant, B, L):
    """(nine fp64 maps, fp64 weights) of a case: synth's, shared and never written."""
    v = spec.VARIANT_RGB if variant == "rgb" else spec.VARIANT_FLOW
    feats = tuple(torch.from_numpy(f).double() for f in synth.make_features(B, L, FEATURE_CONFIG))
    return feats, dict((k, t.double()) for k, t in orc.to_torch_weights(synth.make_weights(v)).items())


def targets(P):
    return torch.tensor(TARGETS[:P])


def dropout_multipliers(seed, P, dtype=torch.float64):
    """(units' nine [P,32,H,H], heads' three [P,C] in (fc7, fc14, fc28) order): keep / (1 - p) of the library's reproducible masks."""
    unit = [torch.from_numpy(synth.dropout_keep(seed, si, P, H, DROP_P)).to(dtype) / (1.0 - DROP_P) for si, (_n, _c, H) in enumerate(spec.SITES)]
    head = [torch.from_numpy(synth.head_dropout_keep(seed, index, P, cin, DROP_P)).to(dtype) / (1.0 - DROP_P)
            for index, cin in ((2, 1024), (1, 512), (0, 256))]
    return unit, head


def reference_step(variant, B, L, feats, w, seed, pattern=None, summed=False, feat_grad=False, train=True):
    """One step of the oracle in the dtype of ``feats`` / ``w`` under ``pattern`` (None: its own decisions, the free run).
    Returns a dict: "logits" (fc7, fc14, fc28 as [P, classes]), "grads" key -> tensor for every trainable parameter, "feat_grads"
    (nine, with feat_grad), and the run's own "pre" activations (the 21 fusion names, gen_<site>, pool_in) and "pool_idx"."""
    v = spec.VARIANT_RGB if variant == "rgb" else spec.VARIANT_FLOW
    P = B * (L - 1)
    dtype = feats[0].dtype
    wl = dict((k, t.detach().clone().requires_grad_(k != spec.SOBEL_KEY)) for k, t in w.items())
    fl = [f.detach().clone().requires_grad_(feat_grad) for f in feats]
    unit_drop, head_drop = dropout_multipliers(seed, P, dtype) if train else (None, None)
    pat = orc.Pattern(record=True)
    gen = None
    if pattern is not None:
        pat = orc.Pattern(dict((k, m.to(dtype)) for k, m in pattern["masks"].items()), pattern["pool_idx"], record=True)
        gen = [m.to(dtype) for m in pattern["gen"]]
    fcs = orc.off_forward(fl, wl, B, L, v, orc.SLICE_FLAT, consensus=False, unit_drop=unit_drop, unit_gen_mask=gen, pattern=pat,
                          head_drop=head_drop)
    logits = [t.reshape(P, -1) for t in fcs]                       # train_off.py:128-130 (squeeze dropped the pair axis at P == 1)
    losses = [F.cross_entropy(t, targets(P)) for t in logits]      # :135-142
    if summed:
        (losses[0] + losses[1] + losses[2]).backward()
    else:
        losses[0].backward(retain_graph=True)                      # :144
        losses[1].backward(retain_graph=True)                      # :145
        losses[2].backward()                                       # :146
    pre = dict((k, t.detach()) for k, t in pat.pre.items() if k != "pool")
    with torch.no_grad():
        for (site, _c, _h), x in zip(spec.SITES, fl):
            pre["gen_" + site] = F.conv2d(x, wl["motion_conv_gen_%s.weight" % site], wl["motion_conv_gen_%s.bias" % site])
        _v, own = F.max_pool2d(pre["pool_in"].double(), 3, 2, ceil_mode=True, return_indices=True)
    return {"logits": [t.detach() for t in logits], "grads": dict((k, t.grad) for k, t in wl.items() if t.requires_grad),
            "feat_grads": [f.grad for f in fl] if feat_grad else None, "pre": pre, "pool_idx": own}


def pattern_from_run(run):
    """An oracle run's own decisions in pattern_of's format."""
    return {"masks": dict((k, run["pre"][k] > 0) for k in FUSION_RELUS), "gen": [run["pre"]["gen_" + s] > 0 for s, _c, _h in spec.SITES],
            "pool_idx": run["pool_idx"]}


@functools.lru_cache(maxsize=None)
def free_run(name, seed=None, summed=None):
    """The free fp64 step of a case (its own seed and backward form unless given): computed once, shared, never written."""
    variant, B, L, case_seed, _split, case_summed = CASES[name]
    feats, w = inputs(variant, B, L)
    return reference_step(variant, B, L, feats, w, case_seed if seed is None else seed, summed=case_summed if summed is None else summed)


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def worst_error(got, ref):
    """(worst rel_err, its key) over logits (a list of three) / gradient dicts with equal key sets."""
    if isinstance(ref, dict):
        assert set(got) == set(ref), sorted(set(got) ^ set(ref))
        errs = [(rel_err(got[k], ref[k]), k) for k in ref]
    else:
        assert len(got) == len(ref)
        errs = [(rel_err(g, r), "#%d" % i) for i, (g, r) in enumerate(zip(got, ref))]
    return max(errs)
