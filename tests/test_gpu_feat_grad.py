"""The gradient w.r.t. the nine feature maps (offk_off_units_backward_feats, csrc/units_dx.hip; OFFUnits(feat_grad=True)):

    dX[frame n, pixel, c] = sum_o dGpre[n, pixel, o] Wg[o, c] + sum_j dD[r(n), pixel, j] Wd[j, c]

1. the kernel alone against an fp64 product of its own inputs, per element within 160 * 2^-23 * (|dG| |Wg| + |dD| |Wd|): the
   bound of a 160-term fp32 sum in any order, the unit roundoff taken at 2^-23 because nothing here has measured the matrix
   pipe's accumulate rounding;  2. against the oracle's autograd with the device's ReLU decisions, RTOL = 2e-4 of each tensor's
   max magnitude (the project's gradient constant);  3. equal bits: NHWC == NCHW, run to run, accumulate == 2 * first, graph
   replay, after the _typed and _cl backward forms;  4. memory discipline in a guarded arena;  5. bound weights after an in-place
   update;  6. refusals;  7. the module;  8. one full-size case.

Shapes: the smallest at which the row mapping and the tiling can go wrong, the ones tests/test_gpu_backward.py uses -- (1, 2):
P = 1 and 98 rows at the 7x7 sites, less than one 128-row tile; (2, 3) flat: frames 4 and 5 outside the slice; (3, 4) flat and
per-clip; (3, 2): one pair per clip; (5, 9) per-clip, Flow: L > 7.  All nine sites always: 320 and 608 channels end in half a
64-channel tile, HW = 49 puts image boundaries inside the tiles."""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import units_dx_checks as checks
from .units_grad import DX_FP32 as FORM
from .units_grad import (  # noqa: F401
    DOWN_W, GEN_W, RTOL, U, Case, as_rows, assert_module_dx_matches_the_oracle, case, dev, down_rows, make_units, module_cots, oracle_dx,
    rel_err, rt)

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_FLAT),
          (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP), (3, 2, spec.VARIANT_RGB, spec.SLICE_FLAT),
          (5, 9, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP)]
IDS = ["b1l2", "b2l3_flat", "b3l4_flat", "b3l4_clip", "b3l2", "b5l9_clip_flow"]


# ---- 1. the kernel alone ----

@pytest.mark.parametrize("seed", [None, 7], ids=["eval", "drop"])
@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_kernel_against_fp64_product(rt, B, L, variant, slice_mode, seed):
    c = case(rt, B, L, variant, slice_mode, seed)
    c.run()
    got = {lay: c.h.off_units_backward_feats(layout=lay) for lay in ("nchw", "cl")}
    torch.cuda.synchronize()
    worst = 0.0
    for si in range(spec.NUM_SITES):
        ref, bound, gen, inside = c.reference(si)
        assert float(ref.abs().max()) > 0
        for lay in ("nchw", "cl"):
            g = as_rows(got[lay][si], lay).double()
            assert tuple(g.shape) == tuple(ref.shape)
            err = (g - ref).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (spec.SITES[si][0], lay, float((err - bound).max()))
            # frames outside the slice: the gen part alone
            if not bool(inside.all()):
                out = ~inside
                assert bool(((g[out] - gen[out]).abs() <= bound[out]).all()), (spec.SITES[si][0], lay)
    print("worst |got - ref| / bound = %.3f" % worst)


# ---- 2. against the oracle's autograd ----

@pytest.mark.parametrize("seed", [None, 7], ids=["eval", "drop"])
@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_against_oracle_autograd(rt, B, L, variant, slice_mode, seed):
    c = case(rt, B, L, variant, slice_mode, seed)
    c.run()
    got = c.h.off_units_backward_feats(layout="nchw")
    torch.cuda.synchronize()
    for si, g, r in zip(range(spec.NUM_SITES), got, oracle_dx(c)):
        assert rel_err(g, r) < RTOL, (spec.SITES[si][0], rel_err(g, r))


# ---- 3. equal bits ----

def test_equal_bits_properties(rt):
    checks.equal_bits(FORM, case(rt, 3, 4, spec.VARIANT_RGB, spec.SLICE_FLAT, 7))


@pytest.mark.parametrize("kind", ["typed_bf16", "cl_f32", "cl_f16"])
def test_same_bits_after_the_typed_and_cl_backward(rt, kind):
    """offk_off_units_backward_typed / _cl on the same logical maps leave the same dG / dD, so dX is the plain form's."""
    checks.same_bits_after_the_other_backwards(FORM, Case(rt, 2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT, 7), kind, torch.float32)


# ---- 4. memory discipline ----

@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("B,L,slice_mode", [(1, 2, spec.SLICE_FLAT), (3, 4, spec.SLICE_PER_CLIP)])
def test_memory_discipline(rt, layout, B, L, slice_mode):
    for accumulate in (False, True):
        checks.memory_discipline(FORM, case(rt, B, L, spec.VARIANT_RGB, slice_mode, 7), layout, torch.float32, accumulate)


# ---- 5. bound weights ----

def test_bound_weights_after_an_in_place_update(rt):
    c = Case(rt, 2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    bound = c.bind_unit_weights()
    gen = torch.Generator(device="cuda").manual_seed(11)
    for k, t in bound.items():                     # the "optimizer step", on the stream the calls go to
        t.mul_(1.25).add_(0.01 * torch.randn(t.shape, device="cuda", generator=gen))
    c.run()
    got = c.h.off_units_backward_feats(layout="nchw")
    torch.cuda.synchronize()
    for si, (site, _c, _h) in enumerate(spec.SITES):
        wg, wd = bound[GEN_W % site].cpu().reshape(128, -1), bound[DOWN_W % site].cpu().reshape(32, -1)
        assert not torch.equal(wg, c.weights(si)[0])
        ref, bnd, _gen, _in = c.reference(si, wg, wd)
        assert bool(((as_rows(got[si], "nchw").double() - ref).abs() <= bnd).all()), site


# ---- 6. refusals ----

def test_refusals_leave_the_outputs_untouched(rt):
    checks.refusals(rt, FORM, torch.float32)


# ---- 7. the module ----

def test_module_feat_grad_matches_the_oracle(rt):
    B, L = 2, 3
    u, wnp = make_units(B, L, True)
    feats_np = synth.make_features(B, L, 2)
    feats = [dev(f).requires_grad_(True) for f in feats_np]
    cots = module_cots(B * (L - 1))
    torch.autograd.backward(u(feats, drop_seed=7), cots)
    torch.cuda.synchronize()
    assert_module_dx_matches_the_oracle(u, wnp, feats_np, feats, cots, B, L)


def test_module_partial_fine_tune_bf16_and_channels_last(rt):
    B, L = 2, 3
    P = B * (L - 1)
    cots = module_cots(P)
    feats_np = synth.make_features(B, L, 2)
    # only 5a and 5b require grad: the other seven get none, and the trace shows the new launch once
    u, _w = make_units(B, L, True)
    feats = [dev(f).requires_grad_(i >= 7) for i, f in enumerate(feats_np)]
    out = u(feats, drop_seed=7)
    u._rt.set_profiling(2)
    torch.autograd.backward(out, cots)
    tr = u._rt.launch_times()
    u._rt.set_profiling(0)
    new = [(k, v) for k, v in tr.items() if "feature-map gradient" in k]
    assert len(new) == 1 and new[0][1][1] == 1, tr
    assert all(f.grad is None for f in feats[:7]) and all(f.grad is not None and float(f.grad.abs().max()) > 0 for f in feats[7:])
    pgrads = {k: p.grad.clone() for k, p in u.named_parameters() if p.grad is not None}
    full = [f.grad.clone() for f in feats[7:]]
    # none requires grad: no launch
    out = u([f.detach() for f in feats], drop_seed=7)
    u._rt.set_profiling(2)
    torch.autograd.backward(out, cots)
    assert not [k for k in u._rt.launch_times() if "feature-map gradient" in k]
    u._rt.set_profiling(0)
    # feat_grad=False: the maps get nothing, the parameter gradients are the same bits
    u0, _w = make_units(B, L, False)
    f0 = [dev(f).requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u0(f0, drop_seed=7), cots)
    assert all(f.grad is None for f in f0)
    p0 = {k: p.grad for k, p in u0.named_parameters() if p.grad is not None}
    assert p0.keys() == pgrads.keys() and len(p0) == 54 and all(torch.equal(p0[k], pgrads[k]) for k in p0)
    # bf16 maps get bf16 gradients: the fp32 result of the same (bf16-valued) maps, cast
    fb = [dev(f).bfloat16().requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u(fb, drop_seed=7), cots)
    ff = [f.detach().float().requires_grad_(True) for f in fb]
    torch.autograd.backward(u(ff, drop_seed=7), cots)
    for a, b in zip(fb, ff):
        assert a.grad.dtype == torch.bfloat16 and torch.equal(a.grad, b.grad.bfloat16())
    # channels_last maps get channels_last gradients, the same values
    fc = [dev(f).contiguous(memory_format=torch.channels_last).requires_grad_(i >= 7) for i, f in enumerate(feats_np)]
    torch.autograd.backward(u(fc, drop_seed=7), cots)
    for f, want in zip(fc[7:], full):
        assert f.grad.is_contiguous(memory_format=torch.channels_last) and not f.grad.is_contiguous()
        assert torch.equal(f.grad, want)


# ---- 8. full size ----

def test_full_size(rt):
    """B = 64, L = 7: zero dM gives exactly zero, doubling dM doubles dX to 1e-6, and 4096 sampled rows per site lie within test
    1's bound against an fp64 matmul done on the device."""
    B, L = 64, 7
    rows = torch.tensor(down_rows(B, L, spec.SLICE_FLAT), device="cuda")

    def check_rows(si, h, wnp, idx, got):
        site, C, H = spec.SITES[si]
        HW = H * H
        f, px = idx // HW, idx % HW
        r = rows[f]
        a = torch.zeros(4096, 160, dtype=torch.float64, device="cuda")
        a[:, :128] = h.region("dG_" + site, 128)[idx].double()
        ins = r >= 0
        a[ins, 128:] = h.region("dD_" + site, 32)[(r * HW + px)[ins]].double()
        wcat = torch.cat((dev(wnp[GEN_W % site]).reshape(128, C), dev(wnp[DOWN_W % site]).reshape(32, C))).double()
        ref = torch.matmul(a, wcat)
        bound = 160 * U * torch.matmul(a.abs(), wcat.abs())
        assert bool(((got.double() - ref).abs() <= bound).all()), site
        assert float(ref.abs().max()) > 0

    checks.full_size(rt, FORM, check_rows)
