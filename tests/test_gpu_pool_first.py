"""The pool-first 7-head (OFFK_POOL_FIRST_7): on handles at or above its gate the forward skips merged_7, takes the
7-head from per-tile sums of xv_7 = [t2 | x2] with the composed weights W' = Wfc Wm, b' = Wfc bm + bfc, and leaves sum_7 to
offk_stage_tensors (runtime.OffForward.region("sum_7") calls it).

Shapes: P = 2 (B = 1, L = 3), P = 18 (3 x 7: two 16-image FC blocks), P = 33 (3 x 12: a third block holding one image), the gate forced
with OFFK_POOL_FIRST_7=2; both arithmetic modes.

* trace: the launch list of the new path lacks merged_7; the default gate sits between P = 95 and P = 96; OFFK_POOL_FIRST_7=0,
  OFFK_FOLD_POOL=0, OFFK_WINOGRAD=0 and OFFK_WINO_MID=0 each bring merged_7 back.
* the 7-head against fp64 from the device's own xv_7:  |got - ref64| <= c 2^-24 mag  with
  mag = mean49|xv| (|Wfc| |Wm|)^T + |Wfc| |bm| + |bfc|  and  c = 512 + 64 + 1 -- the a-priori count of an fp32 sum of 512 products, the 49
  cells and the combines of the partial sums, and the one rounding of W' (derived, not fitted).
  Measured worst |err| / (2^-24 mag) on an MI355X over all cases of test_head7_vs_fp64_from_device_xv: see MEASURED below (printed per
  case, not asserted).
* against the old path (a second handle with the gate closed, same inputs): logits_14 / logits_28 equal bit for bit, logits_7 to 2e-5 of
  max and 1e-3 of the row-to-row signal (the limits of tests/test_gpu_split.py across paths), region("sum_7") equal bit for bit.
* on-demand semantics of sum_7, weight updates through offk_set_weight for each of the six sources of W' / b', the 16-bit and
  channels-last entries, and one forward under the arena checker of tests/arena.py."""
import ctypes

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from .featmaps import rt  # noqa: F401
from .forward import HANDLE_PRECISIONS, check_trace, dev, head_handle, head_weights, make_handle, rel_err, traced_forward
from .guarded import forward_body, np_feats, two_runs

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
C_BOUND = 512 + 64 + 1
MEASURED = None      # worst |err| / (2^-24 mag) seen on an MI355X: filled in from the first GPU run of this module
GATE = {"OFFK_POOL_FIRST_7": "2"}
SHAPES = {"p2": (1, 3), "p18": (3, 7), "p33": (3, 12)}
FC_LAUNCH = "heads (fc on folded pools, one launch)"
SOURCES = ("motion_conv3_trans.weight", "motion_conv3_trans.bias", "motion_conv_branch_trans.weight", "motion_conv_branch_trans.bias",
           "fc_action_motion.weight", "fc_action_motion.bias")

_FEATS = {}


def feats_of(shape):
    if shape not in _FEATS:
        _FEATS[shape] = [dev(f) for f in synth.make_features(*SHAPES[shape], 5)]
    return _FEATS[shape]


def random_feats(B, L):
    """Nine maps of the right shapes for a launch list alone (the values are nobody's business there)."""
    g = torch.Generator(device="cuda").manual_seed(7)
    return [torch.randn(s, device="cuda", generator=g) for s in spec.feature_shapes(B, L)]


# ---- trace ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forced_gate_drops_merged_7(rt, shape, prec):
    B, L = SHAPES[shape]
    h, _ = head_handle(rt, GATE, B, L, prec)
    names, _out = traced_forward(h, feats_of(shape))
    check_trace(names, (FC_LAUNCH, "motion_conv2_trans [winograd: output transform]", "merged_14a"), ("merged_7", "head_7"))


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("B,L,new", [(16, 7, True), (19, 6, False)])
def test_default_gate_is_96_pairs(rt, B, L, new, prec):
    assert B * (L - 1) == (96 if new else 95)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, precision=prec)
    assert h.load_state_dict(head_weights(spec.NUM_CLASSES)) == []
    names, _out = traced_forward(h, random_feats(B, L))
    check_trace(names, (FC_LAUNCH,) + (() if new else ("merged_7",)), ("merged_7",) if new else ())


OFF = {"pool_first0": {"OFFK_POOL_FIRST_7": "0"}, "fold_pool0": dict(GATE, OFFK_FOLD_POOL="0"), "winograd0": dict(GATE, OFFK_WINOGRAD="0"),
       "wino_mid0": dict(GATE, OFFK_WINO_MID="0")}


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("switch", list(OFF))
def test_each_switch_restores_merged_7(rt, switch, prec):
    B, L = SHAPES["p18"]
    h, _ = head_handle(rt, OFF[switch], B, L, prec)
    names, _out = traced_forward(h, feats_of("p18"))
    check_trace(names, ("merged_7",), ())


# ---- the 7-head against fp64 from the device's own xv_7 -------------------------------------------------------------------------
def head7_ratio(got, xv, w):
    """max |got - ref64| / (2^-24 mag) of the 7-head on xv [P, 49, 512] (fp64, host) with the state dict w."""
    t = lambda k: torch.from_numpy(np.asarray(w[k])).double()      # noqa: E731
    Wm = torch.cat((t("motion_conv3_trans.weight")[:, :, 0, 0], t("motion_conv_branch_trans.weight")[:, :, 0, 0]), 1)
    bm = t("motion_conv3_trans.bias") + t("motion_conv_branch_trans.bias")
    Wfc, bfc = t("fc_action_motion.weight"), t("fc_action_motion.bias")
    assert Wm.shape == (1024, 512) and xv.shape[1:] == (49, 512)
    ref = xv.mean(1) @ (Wfc @ Wm).t() + (Wfc @ bm + bfc)
    mag = xv.abs().mean(1) @ (Wfc.abs() @ Wm.abs()).t() + Wfc.abs() @ bm.abs() + bfc.abs()
    got = got.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return ((got - ref).abs() / (EPS * mag)).max().item()


CONFIGS = {"ncls101": (101, False, True), "ncls51": (51, False, True), "consensus": (101, True, True), "no28": (101, False, False)}


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("config", list(CONFIGS))
def test_head7_vs_fp64_from_device_xv(rt, config, shape, prec):
    ncls, consensus, want28 = CONFIGS[config]
    B, L = SHAPES[shape]
    P = B * (L - 1)
    h, w = head_handle(rt, GATE, B, L, prec, ncls=ncls, consensus=consensus)
    h.region("poolpart_7t", 512)                      # (the region exists on handles that take the path only)
    o7, _o14, o28 = h.forward(feats_of(shape), want28=want28)
    torch.cuda.synchronize()
    assert (o28 is None) == (not want28)
    got = h.region("logit_7", ncls) if consensus else o7
    xv = h.region("xv_7", 512).view(P, 49, 512).double().cpu()
    ratio = head7_ratio(got, xv, w)
    print("pool-first 7-head %s %s %s: max |err| / (2^-24 mag) = %.2f (bound %d)" % (config, shape, prec, ratio, C_BOUND))
    assert ratio <= C_BOUND
    if consensus:
        assert o7.shape == (B, ncls)
        assert rel_err(o7, got.double().view(B, L - 1, -1).mean(1)) < 1e-6


# ---- against the old path; sum_7 on demand -----------------------------------------------------------------------------------------
def raw_region(h, name, channels):
    """OffForward.region without its call of offk_stage_tensors"""
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    assert h.lib.offk_workspace_region(h._h, name.encode(), ctypes.byref(off), ctypes.byref(nb)) == 0
    return h.workspace[off.value:off.value + nb.value].view(torch.float32).view(-1, channels)


def pair_of_handles(rt, shape, prec):
    B, L = SHAPES[shape]
    h1, _ = head_handle(rt, GATE, B, L, prec)
    h0, _ = head_handle(rt, {"OFFK_POOL_FIRST_7": "0"}, B, L, prec)
    return h1, h0


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_old_path(rt, shape, prec):
    h1, h0 = pair_of_handles(rt, shape, prec)
    a, b = h1.forward(feats_of(shape)), h0.forward(feats_of(shape))
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    x, y = a[0], b[0]
    sig = (y - y.mean(dim=0, keepdim=True)).abs().max().item()
    d = (x - y).abs().max().item()
    print("pool-first vs merged_7 %s %s: logits_7 differ by %.2e of max, %.2e of the row-to-row signal" % (shape, prec, d / y.abs().max().item(), d / sig))
    assert d / y.abs().max().item() < 2e-5
    assert d < 1e-3 * sig
    s1, s0 = h1.region("sum_7", 1024), h0.region("sum_7", 1024)
    assert torch.isfinite(s1).all() and torch.equal(s1, s0)
    assert torch.equal(h1.region("xv_7", 512), h0.region("xv_7", 512))


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
def test_sum_7_on_demand(rt, prec):
    h1, h0 = pair_of_handles(rt, "p18", prec)
    fa = feats_of("p18")
    fb = [f.flip(0).contiguous() for f in fa]
    h1.workspace.zero_()
    h0.workspace.zero_()
    # a handle below the gate never has anything pending: region() leaves whatever sits in sum_7
    h0.forward(fb)
    want_b = h0.region("sum_7", 1024).clone()
    h0.region("sum_7", 1024).zero_()
    assert not h0.region("sum_7", 1024).any()
    h0.forward(fa)
    want_a = h0.region("sum_7", 1024).clone()
    assert not torch.equal(want_a, want_b)
    # the new path: the forward itself does not write sum_7 ...
    h1.forward(fa)
    assert h1.region("xv_7", 512).any() and not raw_region(h1, "sum_7", 1024).any()
    # ... region() fills it, once
    first = h1.region("sum_7", 1024).clone()
    assert torch.equal(first, want_a)
    assert torch.equal(h1.region("sum_7", 1024), first)
    h1.region("sum_7", 1024).zero_()
    assert not h1.region("sum_7", 1024).any()          # nothing pending any more: no launch
    # forward(A), forward(B), then region: B's
    h1.forward(fa)
    h1.forward(fb)
    assert torch.equal(h1.region("sum_7", 1024), want_b)


# ---- weight updates ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("key", SOURCES)
def test_set_weight_remakes_the_composed_head(rt, key, prec):
    B, L = SHAPES["p18"]
    w = head_weights(spec.NUM_CLASSES)
    h, _ = head_handle(rt, GATE, B, L, prec)
    before = h.forward(feats_of("p18"))[0].clone()
    g = np.random.default_rng(SOURCES.index(key))
    new = (w[key] * 0.5 + 0.05 * g.standard_normal(w[key].shape) * (np.abs(w[key]).max() + 0.1)).astype(np.float32)
    h.set_weight(key, new)
    got = h.forward(feats_of("p18"))
    fresh, _ = make_handle(rt, B, L, spec.VARIANT_RGB, weights=dict(w, **{key: new}), precision=prec, env=GATE)
    want = fresh.forward(feats_of("p18"))
    torch.cuda.synchronize()
    assert not torch.equal(got[0], before), key
    for a, b in zip(got, want):
        assert torch.equal(a, b), key
    assert torch.equal(h.region("sum_7", 1024), fresh.region("sum_7", 1024))


# ---- the other forward entries -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bf16", "f32cl", "f16cl", "parts"])
def test_typed_and_channels_last_entries(rt, form):
    """offk_forward_typed / _cl / _parts share the forward behind the units: same logits as the plain entry on the widened, contiguous maps."""
    B, L = SHAPES["p18"]
    h, _ = head_handle(rt, GATE, B, L, "f32split")
    dt = {"bf16": torch.bfloat16, "f16cl": torch.float16}.get(form, torch.float32)
    base = [f.to(dt) for f in feats_of("p18")]
    if form.endswith("cl"):
        fs = [f.contiguous(memory_format=torch.channels_last) for f in base]
        assert h.takes_channels_last(fs)
    elif form == "parts":
        fs = [list(torch.split(f, [32, f.shape[1] - 32], dim=1)) for f in base]
        fs = [[p.contiguous() for p in ps] for ps in fs]
    else:
        fs = base
    names, got = traced_forward(h, fs)
    check_trace(names, (FC_LAUNCH,), ("merged_7",))
    want = h.forward([f.float().contiguous() for f in base])
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("B,L", [(1, 3), (3, 3)])
def test_forced_gate_forward_in_the_arena(rt, B, L, prec):
    """One forward on the new path with every buffer between guard bands and full of NaN beforehand (tests/guarded.two_runs):
    the per-tile sums poolpart_7t and, after offk_stage_tensors, sum_7 stay inside their regions, are written completely and do not
    depend on what the workspace held."""
    h = make_handle(rt, B, L, spec.VARIANT_RGB, precision=prec, env=GATE)[0]
    inner = forward_body(h, np_feats(B, L))

    def body(r):
        res = inner(r)
        res["poolpart_7t"] = h.region("poolpart_7t", 512)
        res["xv_7"] = h.region("xv_7", 512)
        return res

    a, _b = two_runs(body)
    assert a["poolpart_7t"].shape == (4 * B * (L - 1), 512)
    # the four tile sums of an image add up to the sum of its 49 cells of xv_7
    P = B * (L - 1)
    tiles = a["poolpart_7t"].double().view(P, 4, 512).sum(1)
    cells = a["xv_7"].double().view(P, 49, 512)
    assert ((tiles - cells.sum(1)).abs() <= 64 * EPS * cells.abs().sum(1)).all()
