"""One whole training step of the motion branch on liboffk -- the nine units, the 24 fusion convs and the three heads wired as
INTEGRATION.md section 5 says (tests/branch.Branch) -- against the fp64 oracle under the device's own activation pattern
(tests/branch.reference_step; tests/test_branch_reference.py shows on the CPU that this reference alone stays below RTOL / 10).

Every comparison: logits and all parameter gradients within RTOL = 2e-4 of each tensor's max magnitude, and check_pattern on the
pattern (at most 5 + slack numel decisions differ from fp64's own, each within slack of its kink).  Each case prints its worst error
and its flip count; DESIGN.md section 8.7 quotes them.  The step is train_off.py:135-146: three cross-entropies, three backward calls,
two of them with retain_graph=True, so every autograd node is entered up to three times and .grad accumulates."""
import pytest
import torch
import torch.nn.functional as F

from . import branch as br

pytestmark = pytest.mark.gpu
MAIN = "rgb_b2_l3"


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import off_module
    return off_module


_BRANCHES = {}


def fresh(name):
    """(the case's Branch with synth's weights, everything trainable and in train mode; its nine maps on the device).  One Branch per
    case for the whole module -- each test starts from the same parameters, reloaded in place."""
    variant, B, L, _seed, split, _summed = br.CASES[name]
    feats, w = br.inputs(variant, B, L)
    if name not in _BRANCHES:
        _BRANCHES[name] = br.Branch(B, L, variant, split=split, feat_grad=split).cuda()
    b = _BRANCHES[name]
    b.load_state_dict(dict((k, v.float()) for k, v in w.items()), strict=True)
    for k, p in b.state_dict(keep_vars=True).items():
        p.requires_grad_(k != br.spec.SOBEL_KEY)
        p.grad = None
    b.train()
    return b, [f.float().cuda().requires_grad_(split) for f in feats]


def losses_of(logits, P):
    t = br.targets(P).cuda()
    return [F.cross_entropy(x, t) for x in logits]


def backward(losses, summed):
    if summed:
        (losses[0] + losses[1] + losses[2]).backward()
    else:
        losses[0].backward(retain_graph=True)          # train_off.py:144-146
        losses[1].backward(retain_graph=True)
        losses[2].backward()


def grads_of(b):
    return dict((k, p.grad.clone()) for k, p in b.state_dict(keep_vars=True).items() if p.requires_grad and p.grad is not None)


def device_step(b, feats, seed, summed, between=None):
    """One train step; returns the run in reference_step's format plus the device's pattern, read right behind the forward."""
    for p in b.parameters():
        p.grad = None
    for f in feats:
        f.grad = None
    logits = b(feats, seed)
    pattern = br.pattern_of(b)
    if between is not None:
        between()
    backward(losses_of(logits, logits[0].shape[0]), summed)
    torch.cuda.synchronize()
    return {"logits": [x.detach().clone() for x in logits], "grads": grads_of(b), "pattern": pattern,
            "feat_grads": [f.grad.clone() for f in feats] if feats[0].requires_grad else None}


def compare(label, run, variant, B, L, w64, seed, summed, split, free=None):
    """check_pattern, then logits and every gradient against the patterned fp64 step within RTOL; prints the figures."""
    feats, _w = br.inputs(variant, B, L)
    if free is None:
        free = br.reference_step(variant, B, L, feats, w64, seed, summed=summed)
    flips = br.check_pattern(run["pattern"], free, br.SLACK[split])
    ref = br.reference_step(variant, B, L, feats, w64, seed, pattern=run["pattern"], summed=summed, feat_grad=split)
    n_unit = 54 if variant == "rgb" else 36
    assert len(ref["grads"]) == n_unit + 48 + 6
    worst = [("logits",) + br.worst_error(run["logits"], ref["logits"]), ("grads",) + br.worst_error(run["grads"], ref["grads"])]
    if split:
        worst.append(("feat_grads",) + br.worst_error(run["feat_grads"], ref["feat_grads"]))
    print("%s: " % label + ", ".join("%s worst %.2e (%s)" % x for x in worst) + ", ReLU flips %d, pool flips %d" % flips)
    bad = [x for x in worst if not x[1] < br.RTOL]
    assert not bad, bad


def same_run(a, b, keys=None):
    keys = sorted(a["grads"]) if keys is None else keys
    assert keys and set(keys) <= set(a["grads"]) and set(keys) <= set(b["grads"])
    assert all(torch.equal(x, y) for x, y in zip(a["logits"], b["logits"]))
    diff = [k for k in keys if not torch.equal(a["grads"][k], b["grads"][k])]
    assert not diff, diff


@pytest.mark.parametrize("name", sorted(br.CASES))
def test_step_vs_patterned_oracle(mods, name):
    """rgb_b2_l3: P = 4, the flat-slice quirk is live, three backward(retain_graph=True) calls.  rgb_b1_l2: P = 1, one image everywhere (one
    weight-gradient chunk, 49-row 7x7 maps, the squeeze edge), summed loss.  flow_b1_l4: P = 3, frozen Sobel without a gradient.
    rgb_b2_l3_split: all five arithmetic switches on, the maps require grad and their nine gradients are compared too."""
    variant, B, L, seed, split, summed = br.CASES[name]
    b, feats = fresh(name)
    run = device_step(b, feats, seed, summed)
    if variant == "flow":
        assert br.spec.SOBEL_KEY not in run["grads"] and b.off_units.sobel_edge_diagonal.conv.weight.grad is None
    compare(name, run, variant, B, L, br.inputs(variant, B, L)[1], seed, summed, split, free=br.free_run(name))


@pytest.mark.parametrize("summed", [False, True])
def test_step_is_reproducible(mods, summed):
    """The same step twice from the same seeds, .grad cleared in between: the same bits in every logit and every gradient."""
    seed = br.CASES[MAIN][3]
    b, feats = fresh(MAIN)
    first = device_step(b, feats, seed, summed)
    second = device_step(b, feats, seed, summed)
    assert len(first["grads"]) == 108
    same_run(first, second)


def test_two_steps(mods):
    """Step 1, p.data.add_(p.grad, alpha=-lr) on the device, step 2 under a new seed against the reference built from the device's
    updated parameters: within RTOL, with no re-bind and no new handle.  tests/test_branch_reference.py shows that a stale weight
    moves every step-2 gradient by more than 10 RTOL."""
    variant, B, L, seed, split, summed = br.CASES[MAIN]
    b, feats = fresh(MAIN)
    device_step(b, feats, seed, summed)
    rt = b.off_units._rt
    binds = []
    bind = rt.bind_weight
    rt.bind_weight = lambda key, tensor: (binds.append(key), bind(key, tensor))[1]
    try:
        with torch.no_grad():
            for p in b.parameters():
                if p.grad is not None:
                    p.data.add_(p.grad, alpha=-br.LR)
        w2 = dict((k, v.detach().cpu().double()) for k, v in b.state_dict().items())
        run = device_step(b, feats, br.STEP2_SEED, summed)
    finally:
        del rt.bind_weight
    assert b.off_units._rt is rt and binds == []
    compare("two steps, step 2", run, variant, B, L, w2, br.STEP2_SEED, summed, split)


def test_overtaken_forward(mods):
    """A train forward, an eval forward through the same Branch under no_grad, then the backward of the first: the gradients of the
    undisturbed step, to the bit (OFFUnits recomputes its generation; the convs and heads keep what they saved)."""
    _variant, _B, _L, seed, _split, summed = br.CASES[MAIN]
    b, feats = fresh(MAIN)
    plain = device_step(b, feats, seed, summed)

    def overtake():
        b.eval()
        with torch.no_grad():
            b(feats, seed)
        b.train()

    gen = b.off_units._generation
    disturbed = device_step(b, feats, seed, summed, between=overtake)
    assert b.off_units._generation == gen + 3          # the train forward, the eval forward, one recompute in the first backward
    same_run(plain, disturbed)


@pytest.mark.parametrize("name", [MAIN, "rgb_b1_l2"])
def test_train_then_deploy(mods, name):
    """After a step and its update: branch.eval() logits against the fp64 oracle (eval, its own pattern) within RTOL, and against
    OFFSubNetwork -- the deployed forward -- loaded from branch.state_dict(), in both precisions, within 2 RTOL of the max (both are
    within RTOL of the same reference).  want28=True; P = 4 and P = 1."""
    variant, B, L, seed, _split, summed = br.CASES[name]
    P = B * (L - 1)
    b, feats = fresh(name)
    device_step(b, feats, seed, summed)
    with torch.no_grad():
        for p in b.parameters():
            if p.grad is not None:
                p.data.add_(p.grad, alpha=-br.LR)
    b.eval()
    with torch.no_grad():
        got = [x.clone() for x in b(feats, seed)]
    assert all(tuple(x.shape) == (P, br.spec.NUM_CLASSES) for x in got)
    feats64, _w = br.inputs(variant, B, L)
    w2 = dict((k, v.detach().cpu().double()) for k, v in b.state_dict().items())
    v = br.spec.VARIANT_RGB if variant == "rgb" else br.spec.VARIANT_FLOW
    with torch.no_grad():
        ref = [x.reshape(P, -1) for x in br.orc.off_forward(list(feats64), w2, B, L, v, br.orc.SLICE_FLAT, consensus=False)]
    err = br.worst_error(got, ref)
    line = "%s deploy: branch.eval() vs fp64 %.2e" % (name, err[0])
    assert err[0] < br.RTOL, err
    for precision in ("fp32", "f32split"):
        net = mods.OFFSubNetwork(batch=B, length=L, variant=variant, consensus=False, precision=precision).cuda()
        net.load_state_dict(b.state_dict())
        dep = [x.reshape(P, -1) for x in net([f.detach() for f in feats], want28=True)]
        torch.cuda.synchronize()
        e_ref, e_dep = br.worst_error(dep, ref), br.worst_error(dep, got)
        line += ", OFFSubNetwork(%s) vs fp64 %.2e, vs branch %.2e" % (precision, e_ref[0], e_dep[0])
        assert e_ref[0] < br.RTOL, (precision, e_ref)
        assert e_dep[0] < 2 * br.RTOL, (precision, e_dep)
    print(line)


def test_frozen_units_and_launch_counts(mods):
    """The weight-gradient launches the recipe implies -- each conv and each head once per backward that reaches it: loss7 reaches all 24
    convs, loss14 the 19 of stages 28 and 14, loss28 the 11 of stage 28, one head each; the summed loss 24 and 3.  With the units'
    parameters frozen the fusion and head gradients are the unfrozen step's, to the bit, and the units get none."""
    _variant, _B, _L, seed, _split, _summed = br.CASES[MAIN]
    b, feats = fresh(MAIN)
    conv, head = mods.FusionConv2d, mods.MotionHead

    def counted(summed):
        c0, h0 = conv.weight_grad_launches, head.weight_grad_launches
        run = device_step(b, feats, seed, summed)
        return run, conv.weight_grad_launches - c0, head.weight_grad_launches - h0

    three, nc, nh = counted(False)
    assert (nc, nh) == (24 + 19 + 11, 3)
    _one, nc, nh = counted(True)
    assert (nc, nh) == (24, 3)
    unit_keys = set(b.off_units.state_dict().keys())
    for p in b.off_units.parameters():
        p.requires_grad_(False)
    frozen, nc, nh = counted(False)
    assert (nc, nh) == (24 + 19 + 11, 3)
    assert set(frozen["grads"]) == set(three["grads"]) - unit_keys and len(frozen["grads"]) == 48 + 6
    same_run(three, frozen, keys=sorted(frozen["grads"]))
