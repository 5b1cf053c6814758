"""torch.channels_last feature maps on the training side of the OFF units (offk_pw_reduce_cl, offk_off_units_cl,
offk_off_units_train_cl, offk_off_units_backward_cl; the channels-last loaders of K1 in csrc/pw_reduce.hip and of K1b in
csrc/units_bwd.hip).  The contract is equality, not a tolerance: everything a _cl call writes -- G, D, the unit channels of the
fusion buffers, the flat gradient buffer -- is torch.equal to what the NCHW call of the same dtype writes from the contiguous
copies of the same logical tensors (include/offk.h).  All inputs here are finite, so no case is left out of the equality."""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth
from oracle import off_oracle as orc

from . import featmaps as fm
from .featmaps import (  # noqa: F401
    DROP_P, DROP_SEED, STEMS, ToyBackbone, _units_node, cotangents, device_relu_masks, grad_views, maps_of_kind, oracle_dm, rel_err,
    relu_maps, rt, run_units, to_cl, unit_drop, make_train_handle as make_handle)
from .units_grad import RTOL          # the fp32 path's bound against the oracle

pytestmark = pytest.mark.gpu

KIND = fm.KINDS["cl"]
DTYPES = KIND.dtypes
VARIANTS = {"rgb": spec.VARIANT_RGB, "flow": spec.VARIANT_FLOW}
SHAPES = [(1, 2), (2, 3), (3, 4), (5, 7), (2, 9)]
CLAST = torch.channels_last


def assert_forward_equal(h, x):
    """x: contiguous maps."""
    fm.assert_forward_equal(h, KIND, x)


def assert_backward_equal(h, x, views):
    fm.assert_backward_equal(h, KIND, x, views)


def _assert_refused(h, rt, fdt, ptrs, views, needle, stems=STEMS, kind=KIND):
    fm.assert_refused(h, rt, kind, fdt, ptrs, views, needle, stems)


# ---- 1. forward equality ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("slice_mode", [spec.SLICE_FLAT, spec.SLICE_PER_CLIP])
@pytest.mark.parametrize("precision", ["fp32", "f32split"])
@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_equals_contiguous_maps(rt, name, variant, slice_mode, precision, B, L):
    """off_units and off_units_train (seed 7, p 0.8) on channels_last maps: G, D and the unit regions finite and equal to the run on
    the contiguous copies; pw_reduce alone on every site."""
    h = make_handle(rt, B, L, VARIANTS[variant], slice_mode, precision)
    x = relu_maps(B, L, DTYPES[name], 11 * B + L)
    assert_forward_equal(h, x)
    xcl = to_cl(x)
    for site in range(spec.NUM_SITES):
        Gc, Dc = h.pw_reduce(site, xcl[site])
        Gn, Dn = h.pw_reduce(site, x[site])
        torch.cuda.synchronize()
        assert torch.isfinite(Gc).all() and torch.equal(Gc, Gn) and torch.equal(Dc, Dn), site


# ---- 2. backward equality ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("slice_mode", [spec.SLICE_FLAT, spec.SLICE_PER_CLIP])
@pytest.mark.parametrize("precision", ["fp32", "f32split"])
@pytest.mark.parametrize("B,L", SHAPES)
def test_backward_equals_contiguous_maps(rt, name, variant, slice_mode, precision, B, L):
    h = make_handle(rt, B, L, VARIANTS[variant], slice_mode, precision)
    x = relu_maps(B, L, DTYPES[name], 13 * B + L)
    assert_backward_equal(h, x, grad_views(oracle_dm(VARIANTS[variant], B, L, slice_mode)))


# ---- 3. input kinds ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("kind", ["relu", "random_bits", "full_mantissa", "heavy_tail"])
def test_input_kinds(rt, name, kind):
    """ReLU maps, random finite bit patterns (negative values, subnormals), every mantissa bit set, a heavy tail."""
    B, L = 3, 4
    h = make_handle(rt, B, L)
    x = maps_of_kind(kind, B, L, DTYPES[name], 4)
    assert all(bool(torch.isfinite(t.float()).all()) for t in x)
    assert_forward_equal(h, x)
    assert_backward_equal(h, x, grad_views(oracle_dm(spec.VARIANT_RGB, B, L, spec.SLICE_FLAT)))


# ---- 4. an anchor that does not pass through the NCHW kernels ----

@pytest.mark.parametrize("name", ["bf16", "f16"])
@pytest.mark.parametrize("variant,seed", [("rgb", DROP_SEED), ("flow", None)])
def test_backward_channels_last_maps_vs_oracle(rt, name, variant, seed):
    """Gradients from channels_last 16-bit maps against oracle.unit_backward on the same values, within the fp32 path's own RTOL."""
    B, L = 2, 3
    P = B * (L - 1)
    v = VARIANTS[variant]
    h = make_handle(rt, B, L, v)
    w = orc.to_torch_weights(synth.make_weights(v))
    xcl = to_cl([torch.from_numpy(f).cuda().to(DTYPES[name]).contiguous() for f in synth.make_features(B, L, 2)])
    tf = [x.float().cpu().contiguous() for x in xcl]
    drops = None if seed is None else unit_drop(seed, P)
    if seed is None:
        h.off_units(xcl)
    else:
        h.off_units_train(xcl, seed, DROP_P)
    ref, dm = orc.unit_backward(tf, w, B, L, v, spec.SLICE_FLAT, cotangents(P), drops, device_relu_masks(h, tf, w, B, L))
    _flat, got = h.off_units_backward(xcl, grad_views(dm), 0 if seed is None else seed, 0.0 if seed is None else DROP_P)
    torch.cuda.synchronize()
    assert set(got) == set(ref)
    errs = dict((k, rel_err(got[k], ref[k])) for k in ref)
    bad = dict((k, "%.2e" % e) for k, e in errs.items() if not e < RTOL or got[k].shape != ref[k].shape)
    assert not bad, bad


# ---- 5. OFFUnits behind a channels_last backbone ----

@pytest.mark.parametrize("name", ["none", "bf16", "f16"])
def test_off_units_behind_channels_last_backbone(rt, name):
    from offk_amd.off_module import OFFUnits
    import contextlib
    B, L = 2, 3
    P = B * (L - 1)
    dt = torch.float32 if name == "none" else DTYPES[name]
    autocast = (lambda: contextlib.nullcontext()) if name == "none" else (lambda: torch.autocast("cuda", dtype=dt))
    torch.manual_seed(0)
    bb = ToyBackbone(CLAST).cuda().requires_grad_(False)            # the frozen backbone
    wnp = synth.make_weights(spec.VARIANT_RGB)
    wg = {k: t.cuda() for k, t in orc.to_torch_weights(wnp).items()}
    cot = [c.cuda() for c in cotangents(P)]
    x = torch.randn(B * L, 3, 28, 28, device="cuda")
    with torch.no_grad(), autocast():
        other = [f * 0.5 for f in bb(x.flip(0))]                    # a second set of maps for the interleaved forward
        feats_cl = bb(x)
    assert all(f.dtype == dt and not f.is_contiguous() and f.is_contiguous(memory_format=CLAST) for f in feats_cl + other)

    def new_units():
        u = OFFUnits(B, L, "rgb").cuda()
        u.load_state_dict({k: torch.from_numpy(a) for k, a in wnp.items() if k in u.state_dict()}, strict=True)
        return u.train()

    def loss_of(m28, m14, m7):
        # the reference's fusion stages and heads as ordinary torch ops (the oracle's functions are plain torch)
        s28 = orc.fusion_28(m28, wg)
        s14 = orc.fusion_14(torch.cat((m14, s28), 1), wg)
        s7 = orc.fusion_7(torch.cat((m7, s14), 1), wg)
        return (orc.head(s7, wg, "fc_action_motion", False) * cot[0]).sum() + (orc.head(s14, wg, "fc_action_motion_14", False) * cot[1]).sum() \
            + (orc.head(s28, wg, "fc_action_motion_28", True) * cot[2]).sum()

    def step(units, layout, interleave):
        """One training step: units on the backbone's maps (as handed over, their contiguous copies, or a mix), torch fusion
        stages, loss.backward().  Returns the maps given, the maps the autograd node holds, the outputs and the parameter gradients."""
        for p in units.parameters():
            p.grad = None
        feats = list(feats_cl)
        if layout == "nchw":
            feats = [f.contiguous() for f in feats]
        elif layout == "mix":
            feats = [f.contiguous() if i % 2 else f for i, f in enumerate(feats)]
        with autocast():
            outs = units(feats, drop_seed=DROP_SEED)
        saved = list(_units_node(outs[0]).feats)
        if interleave:                                              # an eval forward between the forward and its backward
            units.eval()
            with torch.no_grad():
                units([f.contiguous() for f in other] if layout == "nchw" else other)
            units.train()
        loss = loss_of(*outs)
        loss.backward()
        return feats, saved, [o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in units.named_parameters() if p.grad is not None}

    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                       # the torch stages between the units and the loss, run twice
    try:
        ucl, unc = new_units(), new_units()
        given, saved_cl, out_cl, g_cl = step(ucl, "cl", False)
        _f, saved_nc, out_nc, g_nc = step(unc, "nchw", False)
        # no copy was made: the node holds the very tensors the backbone handed over
        assert [s.data_ptr() for s in saved_cl] == [f.data_ptr() for f in given] == [f.data_ptr() for f in feats_cl]
        assert all(s.dtype == dt and s.is_contiguous(memory_format=CLAST) and not s.is_contiguous() for s in saved_cl)
        assert all(s.is_contiguous() for s in saved_nc)
        assert all(o.dtype == torch.float32 for o in out_cl)
        assert all(torch.equal(a, b) for a, b in zip(out_cl, out_nc))
        assert g_cl.keys() == g_nc.keys() and len(g_cl) == 54
        for k in g_cl:
            assert g_cl[k].dtype == torch.float32 and torch.equal(g_cl[k], g_nc[k]), k
        # the interleaved forward: the backward finds a foreign generation and recomputes K1 + K2 from the saved channels_last maps
        _f, _s, _o, g_cli = step(ucl, "cl", True)
        _f, _s, _o, g_nci = step(unc, "nchw", True)
        for k in g_cl:
            assert torch.equal(g_cli[k], g_cl[k]) and torch.equal(g_cli[k], g_nci[k]), k
        # a mix of layouts still works, through contiguous copies
        _f, saved_mix, out_mix, g_mix = step(ucl, "mix", False)
        assert all(s.is_contiguous() for s in saved_mix)
        assert all(torch.equal(a, b) for a, b in zip(out_mix, out_nc))
        for k in g_cl:
            assert torch.equal(g_mix[k], g_nc[k]), k
    finally:
        torch.backends.cudnn.deterministic = det


# ---- 6. stream capture ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_train_and_backward_capture(rt, name):
    """off_units_train followed by off_units_backward on channels_last maps, captured in a torch.cuda.graph on one stream and
    replayed twice: bit-identical to the eager run."""
    fm.train_and_backward_capture(rt, KIND, name)


# ---- 7. what is refused, before any launch; and which handles are not ----

def test_refusals(rt):
    B, L = 2, 3
    x = relu_maps(B, L, torch.float32, 1)
    xcl = to_cl(x)
    ptrs = [t.data_ptr() for t in xcl]
    views = grad_views(oracle_dm(spec.VARIANT_RGB, B, L, spec.SLICE_FLAT))
    h = make_handle(rt, B, L)
    # an unknown dtype
    _assert_refused(h, rt, 7, ptrs, views, "unknown feat_dtype")
    # a null map: site 3a for pw_reduce (its own wording), the last site for the nine-map entries
    _assert_refused(h, rt, _lib.FEAT_F32, [None] + ptrs[1:], views, "bad argument", STEMS[:1])
    _assert_refused(h, rt, _lib.FEAT_BF16, ptrs[:8] + [None], views, "null feature map", STEMS[1:])
    # a map whose pointer is 4 mod 16: site 3a for pw_reduce, and another site for the nine-map entries
    for site in (0, 4):
        s = x[site]
        N, C, H, _ = s.shape
        buf = torch.empty(s.numel() + 8, dtype=s.dtype, device="cuda")
        off = buf[1:1 + s.numel()].view(N, H, H, C).permute(0, 3, 1, 2)
        off.copy_(s)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous(memory_format=CLAST) and not off.is_contiguous()
        bad = list(xcl)
        bad[site] = off
        for fdt in (_lib.FEAT_F32, _lib.FEAT_F16):
            _assert_refused(h, rt, fdt, [t.data_ptr() for t in bad], views, "16-byte aligned (site %s)" % spec.SITES[site][0],
                            STEMS if site == 0 else STEMS[1:])
        with pytest.raises(_lib.OffkError, match="16-byte aligned"):
            h.off_units_train(bad, DROP_SEED, DROP_P)
        if site == 0:
            with pytest.raises(_lib.OffkError, match="16-byte aligned"):
                h.pw_reduce(0, off)
    # mixed layouts (Python), on every entry that takes nine maps
    h.workspace.fill_(0x5a)
    mixed = xcl[:8] + [x[8]]
    for call in (lambda: h.off_units(mixed), lambda: h.off_units_train(mixed, DROP_SEED, DROP_P),
                 lambda: h.off_units_backward(mixed, views, DROP_SEED, DROP_P)):
        with pytest.raises(ValueError, match="one layout"):
            call()
    # a channels_last tensor of the wrong logical shape: another batch; H and C swapped
    wrong = list(xcl)
    wrong[3] = torch.zeros((B * L + 1,) + tuple(x[3].shape[1:]), device="cuda").contiguous(memory_format=CLAST)
    for call in (lambda: h.off_units(wrong), lambda: h.off_units_train(wrong, DROP_SEED, DROP_P),
                 lambda: h.off_units_backward(wrong, views, DROP_SEED, DROP_P)):
        with pytest.raises(ValueError, match=r"feats\[3\].*logical shape"):
            call()
    with pytest.raises(ValueError, match="logical shape"):
        h.pw_reduce(3, wrong[3])
    with pytest.raises(ValueError, match="logical shape"):
        h.pw_reduce(3, torch.zeros(B * L, 14, 14, 576, device="cuda").contiguous(memory_format=CLAST))
    torch.cuda.synchronize()
    assert bool((h.workspace == 0x5a).all())
    # an NHWC handle's _typed calls are refused as before, and so is its untyped backward
    hn = make_handle(rt, B, L, feat_layout=1)
    x16 = [t.to(torch.bfloat16) for t in x]
    _assert_refused(hn, rt, _lib.FEAT_BF16, [t.data_ptr() for t in x16], views, "NCHW", kind=fm.KINDS["typed"])
    nhwc = [t.permute(0, 2, 3, 1).contiguous() for t in x]
    with pytest.raises(_lib.OffkError, match="NCHW feature maps only"):
        hn.off_units_backward(nhwc, views, DROP_SEED, DROP_P)
    # and none of this disturbed the handles: the next call runs
    assert_forward_equal(h, x)


@pytest.mark.parametrize("name", list(DTYPES))
def test_layout_belongs_to_the_call_not_the_handle(rt, name):
    """The _cl entries on an NHWC handle (cfg.feat_layout is not looked at): forward and backward equal those of an NCHW handle
    with the same weights; and the NHWC handle's own untyped forward on the same memory still runs mode 2 as before."""
    B, L = 2, 3
    x = relu_maps(B, L, DTYPES[name], 5)
    xcl = to_cl(x)
    views = grad_views(oracle_dm(spec.VARIANT_RGB, B, L, spec.SLICE_FLAT))
    res = []
    for layout in (0, 1):
        h = make_handle(rt, B, L, feat_layout=layout)
        w = run_units(h, xcl, True)
        grads = torch.full((h.new_unit_grads().numel(),), float("nan"), device="cuda")
        h.off_units_backward(xcl, views, DROP_SEED, DROP_P, grads=grads)
        if layout == 1 and name == "f32":
            nhwc = [t.permute(0, 2, 3, 1) for t in xcl]
            assert all(t.is_contiguous() and t.data_ptr() == c.data_ptr() for t, c in zip(nhwc, xcl))
            for (n, a), (_n, b) in zip(run_units(h, nhwc, True), w):
                assert torch.equal(a, b), n
        torch.cuda.synchronize()
        res.append((w, grads))
    for (n, a), (_n, b) in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b), n
    assert torch.isfinite(res[0][1]).all() and torch.equal(res[0][1], res[1][1])
