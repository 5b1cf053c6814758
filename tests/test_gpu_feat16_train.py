"""bf16 / fp16 feature maps on the training side of the OFF units (offk_pw_reduce_typed, offk_off_units_typed,
offk_off_units_train_typed, offk_off_units_backward_typed; the 16-bit map forms of K1 in csrc/pw_reduce.hip and of K1b in
csrc/units_bwd.hip).  The contract is equality, not a tolerance: everything a typed call writes -- G, D, the unit channels of the
fusion buffers, the flat gradient buffer -- is torch.equal to what the untyped call writes from the maps upcast to fp32
(include/offk.h).  All inputs here are finite, so no case is left out of the equality."""
import ctypes

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth
from oracle import off_oracle as orc

from . import featmaps as fm
from .featmaps import (  # noqa: F401
    DROP_P, DROP_SEED, STEMS, ToyBackbone, _units_node, cotangents, device_relu_masks, grad_views, maps_of_kind, oracle_dm, rel_err,
    relu_maps, rt, unit_drop, make_train_handle as make_handle)
from .units_grad import RTOL          # the fp32 path's bound against the oracle

pytestmark = pytest.mark.gpu

KIND = fm.KINDS["typed"]
DTYPES = KIND.dtypes
VARIANTS = {"rgb": spec.VARIANT_RGB, "flow": spec.VARIANT_FLOW}
SHAPES = [(1, 2), (2, 3), (3, 4), (5, 7), (2, 9)]


def assert_forward_equal(h, x16):
    fm.assert_forward_equal(h, KIND, x16)


def assert_backward_equal(h, x16, views):
    fm.assert_backward_equal(h, KIND, x16, views)


def _assert_refused(h, rt, fdt, x16, views, needle, stems=STEMS):
    fm.assert_refused(h, rt, KIND, fdt, [x.data_ptr() for x in x16], views, needle, stems)


# ---- 1. forward equality ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("slice_mode", [spec.SLICE_FLAT, spec.SLICE_PER_CLIP])
@pytest.mark.parametrize("precision", ["fp32", "f32split"])
@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_equals_fp32_maps(rt, name, variant, slice_mode, precision, B, L):
    """off_units and off_units_train (seed 7, p 0.8) on 16-bit maps: G, D and the unit regions finite and equal to the run on
    x.float(); pw_reduce alone on sites 3a (28 x 28), 4a (14 x 14) and 5b (7 x 7, the 98-byte rows)."""
    h = make_handle(rt, B, L, VARIANTS[variant], slice_mode, precision)
    x16 = relu_maps(B, L, DTYPES[name], 11 * B + L)
    assert_forward_equal(h, x16)
    for site in (0, 3, 8):
        assert spec.SITES[site][0] in ("3a", "4a", "5b")
        G16, D16 = h.pw_reduce(site, x16[site])
        G32, D32 = h.pw_reduce(site, x16[site].float())
        torch.cuda.synchronize()
        assert torch.isfinite(G16).all() and torch.equal(G16, G32) and torch.equal(D16, D32)


# ---- 2. backward equality ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("slice_mode", [spec.SLICE_FLAT, spec.SLICE_PER_CLIP])
@pytest.mark.parametrize("precision", ["fp32", "f32split"])
@pytest.mark.parametrize("B,L", SHAPES)
def test_backward_equals_fp32_maps(rt, name, variant, slice_mode, precision, B, L):
    h = make_handle(rt, B, L, VARIANTS[variant], slice_mode, precision)
    x16 = relu_maps(B, L, DTYPES[name], 13 * B + L)
    assert_backward_equal(h, x16, grad_views(oracle_dm(VARIANTS[variant], B, L, slice_mode)))


# ---- 3. input kinds ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("kind", ["relu", "random_bits", "full_mantissa", "heavy_tail"])
def test_input_kinds(rt, name, kind):
    """ReLU maps, random finite bit patterns (negative values, the 16-bit type's subnormals), every mantissa bit set, a heavy tail."""
    B, L = 3, 4
    h = make_handle(rt, B, L)
    x16 = maps_of_kind(kind, B, L, DTYPES[name], 4)
    assert all(bool(torch.isfinite(x.float()).all()) for x in x16)
    assert_forward_equal(h, x16)
    assert_backward_equal(h, x16, grad_views(oracle_dm(spec.VARIANT_RGB, B, L, spec.SLICE_FLAT)))


# ---- 4. the oracle: the equal pair is also right ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("variant,seed", [("rgb", DROP_SEED), ("flow", None)])
def test_backward_16bit_maps_vs_oracle(rt, name, variant, seed):
    """Gradients from 16-bit maps against oracle.unit_backward on the upcast maps, within the fp32 path's own RTOL."""
    B, L = 2, 3
    P = B * (L - 1)
    v = VARIANTS[variant]
    h = make_handle(rt, B, L, v)
    w = orc.to_torch_weights(synth.make_weights(v))
    x16 = [torch.from_numpy(f).cuda().to(DTYPES[name]).contiguous() for f in synth.make_features(B, L, 2)]
    tf = [x.float().cpu() for x in x16]
    drops = None if seed is None else unit_drop(seed, P)
    if seed is None:
        h.off_units(x16)
    else:
        h.off_units_train(x16, seed, DROP_P)
    ref, dm = orc.unit_backward(tf, w, B, L, v, spec.SLICE_FLAT, cotangents(P), drops, device_relu_masks(h, tf, w, B, L))
    _flat, got = h.off_units_backward(x16, grad_views(dm), 0 if seed is None else seed, 0.0 if seed is None else DROP_P)
    torch.cuda.synchronize()
    assert set(got) == set(ref)
    errs = dict((k, rel_err(got[k], ref[k])) for k in ref)
    bad = dict((k, "%.2e" % e) for k, e in errs.items() if not e < RTOL or got[k].shape != ref[k].shape)
    assert not bad, bad


# ---- 5. OFFUnits behind an autocast backbone ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_off_units_under_autocast(rt, name):
    from offk_amd.off_module import OFFUnits
    B, L = 2, 3
    P = B * (L - 1)
    dt = DTYPES[name]
    torch.manual_seed(0)
    bb = ToyBackbone().cuda().requires_grad_(False)                 # the frozen backbone
    wnp = synth.make_weights(spec.VARIANT_RGB)
    wg = {k: t.cuda() for k, t in orc.to_torch_weights(wnp).items()}
    cot = [c.cuda() for c in cotangents(P)]
    x = torch.randn(B * L, 3, 28, 28, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        other = [f * 0.5 for f in bb(x.flip(0))]                    # a second set of maps for the interleaved forward

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

    def step(units, upcast, interleave):
        """One training step: backbone under autocast, units, torch fusion stages, loss.backward().  Returns the saved maps' dtypes,
        the outputs and the parameter gradients."""
        for p in units.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=dt):
            with torch.no_grad():
                feats = bb(x)
            assert all(f.dtype == dt for f in feats)
            if upcast:
                feats = [f.float() for f in feats]
            outs = units(feats, drop_seed=DROP_SEED)
        saved = [f.dtype for f in _units_node(outs[0]).feats]
        if interleave:                                              # an eval forward between the forward and its backward
            units.eval()
            with torch.no_grad():
                units([f.float() for f in other] if upcast else other)
            units.train()
        loss = loss_of(*outs)
        loss.backward()
        return saved, [o.detach().clone() for o in outs], {k: p.grad.clone() for k, p in units.named_parameters() if p.grad is not None}

    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                       # the torch stages between the units and the loss, run twice
    try:
        u16, u32 = new_units(), new_units()
        saved16, out16, g16 = step(u16, False, False)
        saved32, out32, g32 = step(u32, True, False)
        assert saved16 == [dt] * 9 and saved32 == [torch.float32] * 9          # ctx keeps the maps as they came
        assert all(o.dtype == torch.float32 for o in out16)
        assert all(torch.equal(a, b) for a, b in zip(out16, out32))
        assert g16.keys() == g32.keys() and len(g16) == 54
        for k in g16:
            assert g16[k].dtype == torch.float32 and torch.equal(g16[k], g32[k]), k
        # the interleaved forward: the backward finds a foreign generation and recomputes K1 + K2 from the saved 16-bit maps
        _s, _o, g16i = step(u16, False, True)
        _s, _o, g32i = step(u32, True, True)
        for k in g16:
            assert torch.equal(g16i[k], g16[k]) and torch.equal(g16i[k], g32i[k]), k
        # an optimizer step is seen by the next forward: the weights are bound, not copied
        for u in (u16, u32):
            with torch.no_grad():
                for p in u.parameters():
                    if p.grad is not None:
                        p -= 10.0 * p.grad
        _s, out16b, _g = step(u16, False, False)
        _s, out32b, _g = step(u32, True, False)
        assert all(torch.equal(a, b) for a, b in zip(out16b, out32b))
        assert not torch.equal(out16b[2], out16[2])
    finally:
        torch.backends.cudnn.deterministic = det


# ---- 6. stream capture ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_train_and_backward_capture(rt, name):
    """off_units_train followed by off_units_backward on 16-bit maps, captured in a torch.cuda.graph and replayed twice:
    bit-identical to the eager run."""
    fm.train_and_backward_capture(rt, KIND, name)


# ---- 7. what is refused, before any launch ----

def test_refusals(rt):
    B, L = 2, 3
    x16 = relu_maps(B, L, torch.bfloat16, 1)
    views = grad_views(oracle_dm(spec.VARIANT_RGB, B, L, spec.SLICE_FLAT))
    h = make_handle(rt, B, L)
    # an unknown dtype
    _assert_refused(h, rt, 7, x16, views, "unknown feat_dtype")
    # an NHWC handle
    _assert_refused(make_handle(rt, B, L, feat_layout=1), rt, _lib.FEAT_BF16, x16, views, "NCHW")
    # a pointer one element off alignment: site 3a for pw_reduce, and another site for the nine-map entries
    for site in (0, 4):
        bad = list(x16)
        s = x16[site]
        buf = torch.empty(s.numel() + 4, dtype=s.dtype, device="cuda")
        bad[site] = buf[1:1 + s.numel()].view(s.shape)
        bad[site].copy_(s)
        assert bad[site].data_ptr() % 8 == 2
        _assert_refused(h, rt, _lib.FEAT_BF16, bad, views, "8-byte aligned",
                        STEMS if site == 0 else STEMS[1:])
        with pytest.raises(_lib.OffkError, match="8-byte aligned"):
            h.off_units_train(bad, DROP_SEED, DROP_P)
    # null maps
    h.workspace.fill_(0x5a)
    arr = (ctypes.c_void_p * spec.NUM_SITES)(*[x.data_ptr() for x in x16[:8]] + [None])
    assert h.lib.offk_off_units_typed(h._h, rt._stream(h.device), _lib.FEAT_F16, arr, ctypes.c_void_p(h.workspace.data_ptr())) == -1
    assert "null feature map" in h.lib.offk_last_error(h._h).decode()
    torch.cuda.synchronize()
    assert bool((h.workspace == 0x5a).all())
    # mixed dtypes (Python), on every entry that takes nine maps
    mixed = x16[:8] + [x16[8].half()]
    for call in (lambda: h.off_units(mixed), lambda: h.off_units_train(mixed, DROP_SEED, DROP_P),
                 lambda: h.off_units_backward(mixed, views, DROP_SEED, DROP_P)):
        with pytest.raises(ValueError, match="one dtype"):
            call()
    # the inference forward keeps its own condition: 16-bit maps need a split-fp32 handle
    with pytest.raises(ValueError, match="f32split"):
        h.forward(x16)
    # and none of this disturbed the handle: the next call runs
    assert_forward_equal(h, x16)
