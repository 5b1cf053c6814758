"""The nine-tap, no-bias form of K2 (csrc/sobel_tdiff.hip, sobel_tdiff_kernel<.., T4 = 0, ..> with db == nullptr): what the Flow variant
runs whenever a checkpoint's sobel_edge_diagonal.conv.weight is not exactly the four-tap kernel of util.py:61 (offk_set_weight reads
the values and sets the handle's sobel_taps4 switch).  Every other test loads spec.DIAG_SOBEL, so that instantiation ran nowhere.

  * one-hot taps: channel c holds a single 1.0 at tap c % 9, so S must be the handle's own D shifted by that tap, zeros outside the
    map -- exact for any data, equal bits; this pins the tap order of repack_dw and of every K2 form;
  * integer taps (exact.dense_sobel): the exact forward and backward checks of tests/test_gpu_exact.py on the Flow sites;
  * a dense real-valued weight (weight_updates.perturbed of the fixed kernel) against the oracle: K2 alone, the units stage, the
    parameter gradients and the feature-map gradient, at the tolerances the four-tap tests use;
  * four-tap -> dense -> four-tap on one handle: the same launch groups three times, the first bits again at the end.

Wall time of this module on an MI355X (first run): 6.1 s for its 18 items.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

from . import exact
from . import exact_units as ge
from . import units_grad as ug
from . import weight_updates as wu
from .arena import same_bits
from .featmaps import rt  # noqa: F401
from .forward import HANDLE_PRECISIONS, check_sobel_tdiff, dev, make_handle, traced_forward

pytestmark = pytest.mark.gpu
FLOW = spec.VARIANT_FLOW


def one_hot_sobel():
    w = np.zeros((spec.DOWN_CH, 1, 3, 3), dtype=np.float32)
    for c in range(spec.DOWN_CH):
        w[c, 0, (c % 9) // 3, (c % 9) % 3] = 1.0
    return w


def dense_weights():
    w0 = synth.make_weights(FLOW)
    return wu.with_key(w0, spec.SOBEL_KEY)


# ---- one-hot taps -----------------------------------------------------------------------------------------------------------------
def check_shifted(h, P, what):
    """S of every site == that site's D_<site> moved by its channel's tap (cross-correlation: S[y, x] = D[y + dy - 1, x + dx - 1])."""
    torch.cuda.synchronize()
    for (name, _C, H), (reg, cs, coff) in zip(spec.SITES, ge.UNIT_SLOTS):
        D = h.region("D_" + name, spec.DOWN_CH).view(P, H, H, spec.DOWN_CH)
        Dp = F.pad(D, (0, 0, 1, 1, 1, 1))
        want = torch.stack([Dp[:, (c % 9) // 3:(c % 9) // 3 + H, (c % 9) % 3:(c % 9) % 3 + H, c] for c in range(spec.DOWN_CH)], dim=-1)
        got = h.region(reg, cs).view(P, H, H, cs)[..., coff:coff + spec.DOWN_CH]
        assert bool((D != 0).any()) and same_bits(got.contiguous(), want.contiguous()), (what, name)


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
def test_one_hot_taps_shift_d(rt, prec):
    B, L = 2, 3
    P = B * (L - 1)
    h = rt.OffForward(B, L, FLOW, precision=prec, training=True)
    assert h.load_state_dict(wu.with_key(synth.make_weights(FLOW), spec.SOBEL_KEY, one_hot_sobel())) == []
    feats = [dev(f) for f in synth.make_features(B, L, 4)]
    fusion = [("fusion_28", 320), ("fusion_14", 1056), ("fusion_7", 832)]
    ge.poison(h, fusion)
    h.off_units(feats)
    check_shifted(h, P, "off_units")
    for algo in (0, 1, 4):
        ge.poison(h, fusion)
        h.sobel_tdiff_all(algo)
        check_shifted(h, P, "sobel_tdiff_all(algo %d)" % algo)
    ge.poison(h, fusion + [("D_" + s, spec.DOWN_CH) for s in spec.SITE_NAMES])
    h.off_units_fused(feats)
    check_shifted(h, P, "off_units_fused")


# ---- integer taps -----------------------------------------------------------------------------------------------------------------
class DenseSobelCase(ge.Case):
    """tests/exact_units.py's Case with exact.dense_sobel at all nine sites."""

    def __init__(self, B, L, variant, slice_mode):
        sob = exact.dense_sobel()
        self.B, self.L, self.variant, self.slice_mode = B, L, variant, slice_mode
        self.N, self.P = B * L, B * (L - 1)
        self.sites = [exact.SiteInputs(si, B, L, variant, drop_seed=ge.DROP_SEED, sobel=sob) for si in range(spec.NUM_SITES)]
        self.worst, self.ref = 0.0, []
        for s in self.sites:
            out, cap = exact.unit_reference(s, B, L, variant, slice_mode)
            self.worst = max(self.worst, exact.check_caps(cap, s.name))
            self.ref.append(dict((k, v.cuda()) for k, v in out.items()))
        self.weights = exact.weights(variant, self.sites)
        assert np.array_equal(self.weights[spec.SOBEL_KEY], sob.numpy())
        self.feats = [s.x.cuda() for s in self.sites]


@pytest.fixture(scope="module", params=exact.SOBEL_SHAPES, ids=exact.SOBEL_IDS)
def sobel_case(request):
    return DenseSobelCase(*request.param)


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
def test_units_forward_exact_with_integer_taps(rt, sobel_case, prec):
    ge.units_forward_exact(rt, sobel_case, prec)


def test_units_backward_exact_with_integer_taps(rt, sobel_case):
    ge.units_backward_exact(rt, sobel_case)


# ---- a dense weight against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [0, 1, 4])
def test_sobel_tdiff_vs_oracle_with_a_dense_weight(rt, algo):
    B, L = 2, 4
    h, w = make_handle(rt, B, L, FLOW, weights=dense_weights())
    assert bool((w[spec.SOBEL_KEY] != 0).all())
    for site in range(spec.NUM_SITES):
        check_sobel_tdiff(h, w, B, L, site, FLOW, algo)


class DenseCase(ug.Case):
    """tests/units_grad.py's Case (a training handle after forward + backward on random dM) on the dense Sobel weight."""

    def __init__(self, rt, B, L, slice_mode, seed):
        self.B, self.L, self.variant, self.slice_mode, self.seed = B, L, FLOW, slice_mode, seed
        self.N, self.P = B * L, B * (L - 1)
        self.h = rt.OffForward(B, L, FLOW, slice_mode, training=True)
        self.wnp = dense_weights()
        assert self.h.load_state_dict(self.wnp) == []
        self.w = orc.to_torch_weights(self.wnp)
        self.feats_np = synth.make_features(B, L, 2 if B == 2 else 3)
        self.feats = [dev(f) for f in self.feats_np]
        self.bufs, self.views = ug.random_views(self.P)
        self.drop = (0, 0.0) if seed is None else (seed, ug.DROP_P)


@pytest.mark.parametrize("B,L,slice_mode,seed", [(2, 3, spec.SLICE_FLAT, None), (3, 4, spec.SLICE_PER_CLIP, 7)], ids=["b2l3_eval", "b3l4_clip_drop"])
def test_units_and_backward_vs_oracle_with_a_dense_weight(rt, B, L, slice_mode, seed):
    """The units stage (all nine sites), the parameter gradients (test_units_backward_vs_oracle's check) and the feature-map gradient
    (test_against_oracle_autograd's), each below the RTOL = 2e-4 of those tests."""
    c = DenseCase(rt, B, L, slice_mode, seed)
    c.forward()
    _flat, got = c.backward()
    dx = c.h.off_units_backward_feats(layout="nchw")
    torch.cuda.synchronize()
    tf = [torch.from_numpy(f) for f in c.feats_np]
    drops = None if seed is None else ug.unit_drop(seed, c.P)
    with torch.no_grad():
        m_ref = [orc.off_unit(x, c.w, site, B, L, FLOW, slice_mode, None if drops is None else drops[si])
                 for si, ((site, _c, _h), x) in enumerate(zip(spec.SITES, tf))]
    for (site, _C, H), (reg, cs, coff), ref in zip(spec.SITES, ge.UNIT_SLOTS, m_ref):
        m = c.h.region(reg, cs).view(c.P, H, H, cs)[..., coff:coff + spec.UNIT_CH].permute(0, 3, 1, 2)
        assert ug.rel_err(m[:, :spec.DOWN_CH], ref[:, :spec.DOWN_CH]) < ug.RTOL, site
        assert ug.rel_err(m, ref) < ug.RTOL, site
    masks = ug.device_relu_masks(c.h, tf, c.w, B, L)
    dm = [buf[..., coff:coff + spec.UNIT_CH].permute(0, 3, 1, 2).cpu() for buf, coff in c.views]
    ref = orc.unit_param_grads_from_dm(tf, c.w, B, L, FLOW, slice_mode, dm, drops, masks)
    assert set(got) == set(ref)
    bad = dict((k, "%.2e" % ug.rel_err(got[k], ref[k])) for k in ref if not ug.rel_err(got[k], ref[k]) < ug.RTOL or got[k].shape != ref[k].shape)
    assert not bad, bad
    for si, g, r in zip(range(spec.NUM_SITES), dx, ug.oracle_dx(c)):
        assert ug.rel_err(g, r) < ug.RTOL, (spec.SITES[si][0], ug.rel_err(g, r))


# ---- four-tap -> dense -> four-tap ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
def test_four_tap_dense_four_tap(rt, prec):
    w0 = synth.make_weights(FLOW)
    h, _w = make_handle(rt, wu.B, wu.L, FLOW, consensus=False, weights=w0, precision=prec)
    feats = [dev(f) for f in synth.make_features(wu.B, wu.L, 2)]

    def run():
        names, out = traced_forward(h, feats)
        return names, [o.clone() for o in out] + [h.region(n, ch).clone() for n, ch in (("fusion_28", 320), ("fusion_14", 1056), ("fusion_7", 832))]

    names0, first = run()
    h.set_weight(spec.SOBEL_KEY, wu.perturbed(spec.SOBEL_KEY, w0[spec.SOBEL_KEY]))
    names1, dense = run()
    h.set_weight(spec.SOBEL_KEY, w0[spec.SOBEL_KEY])
    names2, last = run()
    assert names0 == names1 == names2                      # the same launch groups: only values changed
    assert all(same_bits(a, b) for a, b in zip(first, last))
    assert not any(same_bits(a, b) for a, b in zip(first, dense))
    # the dense run against a handle that never held the four-tap kernel (a four-tap switch that sticks shows here)
    h, _w = make_handle(rt, wu.B, wu.L, FLOW, consensus=False, weights=wu.with_key(w0, spec.SOBEL_KEY), precision=prec)
    _names, fresh = run()
    assert all(same_bits(a, b) for a, b in zip(dense, fresh))
