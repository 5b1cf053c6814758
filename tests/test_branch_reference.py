"""The reference side of tests/test_gpu_branch_step.py on the CPU, at that file's shapes and seeds: the proof that the patterned fp64
oracle (tests/branch.py) can carry the comparison, and that ``Branch`` is the reference's branch by keys and shapes."""
import json
import os

import pytest
import torch

from . import branch as br

NAMES = sorted(br.CASES)


def same(a, b):
    return (all(torch.equal(x, y) for x, y in zip(a["logits"], b["logits"])) and set(a["grads"]) == set(b["grads"])
            and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"]))


@pytest.mark.parametrize("name", NAMES)
def test_own_pattern_changes_nothing(name):
    """The patterned oracle, fed the pattern of its own free fp64 run, is the free run: z * (z > 0) and the gather at the first maximum
    are relu and max_pool2d, forward and backward, to the bit."""
    variant, B, L, seed, _split, summed = br.CASES[name]
    free = br.free_run(name)
    feats, w = br.inputs(variant, B, L)
    again = br.reference_step(variant, B, L, feats, w, seed, pattern=br.pattern_from_run(free), summed=summed)
    assert same(free, again)
    assert br.check_pattern(br.pattern_from_run(free), free, 0.0) == (0, 0)


@pytest.mark.parametrize("name", NAMES)
def test_three_backwards_are_the_summed_loss(name):
    """train_off.py:144-146's three backward(retain_graph=True) calls against one backward of the summed loss, in fp64: 1e-12 of each
    tensor's max."""
    variant, B, L, seed, _split, summed = br.CASES[name]
    free = br.free_run(name)
    feats, w = br.inputs(variant, B, L)
    other = br.reference_step(variant, B, L, feats, w, seed, summed=not summed)
    assert all(torch.equal(a, b) for a, b in zip(free["logits"], other["logits"]))
    err, key = br.worst_error(other["grads"], free["grads"])
    assert err < 1e-12, (key, err)


@pytest.mark.parametrize("name", NAMES)
def test_reference_alone_margin(name):
    """torch fp32 on the CPU against fp64 under fp32's pattern: below RTOL / 10 on every tensor (measured <= 9.8e-6: rgb_b1_l2's
    motion_conv_gen_3a.bias), and fp32's pattern passes check_pattern.  A case that breaks either gets another seed, not another cap."""
    variant, B, L, seed, split, summed = br.CASES[name]
    feats, w = br.inputs(variant, B, L)
    r32 = br.reference_step(variant, B, L, [f.float() for f in feats], dict((k, v.float()) for k, v in w.items()), seed, summed=summed,
                            feat_grad=split)
    p32 = br.pattern_from_run(r32)
    flips = br.check_pattern(p32, br.free_run(name), br.SLACK[False])
    r64 = br.reference_step(variant, B, L, feats, w, seed, pattern=p32, summed=summed, feat_grad=split)
    worst = max(br.worst_error(r32["logits"], r64["logits"]), br.worst_error(r32["grads"], r64["grads"]))
    if split:
        worst = max(worst, br.worst_error(r32["feat_grads"], r64["feat_grads"]))
    print("%s: fp32 vs patterned fp64 worst %.2e (%s), flips %s" % (name, worst[0], worst[1], flips))
    assert worst[0] < br.RTOL / 10, worst


@pytest.mark.parametrize("name", NAMES)
def test_every_gradient_is_live_and_no_window_ties(name):
    """No parameter's reference gradient is all zero (a comparison of zeros against zeros proves nothing; smallest max |grad| measured:
    6.5e-4), and no window of the 28-head holds an exact tie of non-zero values (the route is then the fp64 side's to know)."""
    variant, _B, _L, _seed, _split, _summed = br.CASES[name]
    free = br.free_run(name)
    want = 54 + 48 + 6 if variant == "rgb" else 36 + 48 + 6
    assert len(free["grads"]) == want
    assert min(float(g.abs().max()) for g in free["grads"].values()) > 1e-4
    s = free["pre"]["pool_in"]
    assert tuple(s.shape[1:]) == (256, 14, 14)
    pad = torch.nn.functional.pad(s, (0, 1, 0, 1), value=float("-inf"))          # ceil_mode's overhang
    win = pad.unfold(2, 3, 2).unfold(3, 3, 2).reshape(s.shape[0], 256, 7, 7, 9)
    top = win.topk(2, dim=-1).values
    tie = top[..., 0] == top[..., 1]
    assert not bool((tie & (top[..., 0] != 0)).any())
    assert bool(tie.any())               # ties of zeros are there (3 - 9 % of the windows): the first-maximum rule is exercised


@pytest.mark.parametrize("variant", ["rgb", "flow"])
def test_branch_is_the_references_branch(variant, golden_dir):
    """Branch constructs without a GPU; its state_dict is the reference's motion*, fc_action_motion* and sobel_edge_diagonal* entries by
    key and shape, and a reference-format dict loads with strict=True."""
    with open(os.path.join(golden_dir, "state_dict_keys.json")) as f:
        ref = json.load(f)[variant]
    want = dict((k, tuple(v)) for k, v in ref.items() if k.startswith(("motion", "fc_action_motion", "sobel_edge_diagonal")))
    b = br.Branch(2, 3, variant)
    sd = b.state_dict()
    assert dict((k, tuple(v.shape)) for k, v in sd.items()) == want
    _feats, w = br.inputs(variant, 2, 3)
    loaded = b.load_state_dict(dict((k, v.float()) for k, v in w.items()), strict=True)
    assert not loaded.missing_keys and not loaded.unexpected_keys
    assert all(torch.equal(v, w[k].float()) for k, v in b.state_dict().items())
    trainable = set(k for k, p in b.state_dict(keep_vars=True).items() if p.requires_grad)
    assert trainable == set(want) - {"sobel_edge_diagonal.conv.weight"}
    # the wiring table against the module flags, and the switches of the split form
    s = br.Branch(2, 3, variant, split=True, feat_grad=True)
    assert (s.off_units.fwd_arith, s.off_units.wgrad_arith, s.off_units.feat_grad_arith, s.off_units.feat_grad) == ("f32split",) * 3 + (True,)
    convs = [getattr(s, c[0]) for c in br.spec.FUSION_CONVS]
    assert sum(c.wgrad_arith == "f32split" for c in convs) == 22 and sum(c.dgrad_arith == "f32split" for c in convs) == 2
    assert sum(c.relu for c in convs) == 19 and sum(c.relu_in for c in convs) == 1


def test_learning_rate_moves_every_gradient():
    """The two-step GPU test's learning rate: with the reference alone, step-2 gradients from the stale (step-1) weights differ from those
    from the updated weights by more than 10 RTOL of the tensor's max, for every parameter tensor -- a device that read a stale weight
    cannot pass that test by accident."""
    name = "rgb_b2_l3"
    variant, B, L, _seed, _split, summed = br.CASES[name]
    feats, w = br.inputs(variant, B, L)
    g1 = br.free_run(name)["grads"]
    w2 = dict((k, v - br.LR * g1[k] if k in g1 else v) for k, v in w.items())
    stale = br.reference_step(variant, B, L, feats, w, br.STEP2_SEED, summed=summed)
    fresh = br.reference_step(variant, B, L, feats, w2, br.STEP2_SEED, summed=summed)
    moved = dict((k, br.rel_err(stale["grads"][k], fresh["grads"][k])) for k in fresh["grads"])
    least = min(moved, key=moved.get)
    print("least moved: %s by %.2e" % (least, moved[least]))
    assert moved[least] > 10 * br.RTOL, (least, moved[least])
