"""The units' feature-map gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_off_units_backward_feats_split,
csrc/units_dx_split.hip; OffForward.off_units_backward_feats(arith="f32split"), OFFUnits(feat_grad_arith="f32split")):

    dX[n, q, c] = sum_{k < 160} a[n HW + q, k] w[c, k],  a = [dGpre | dD at row r(n), zeros outside the slice],  w[c] = [Wg[:, c] ; Wd[:, c]]

 5. exact integer inputs (tests/exact.py): value for value the fp64 reference, both layouts, accumulate twice = 2 x, 16-bit = ref.to(dtype);
 6. worst-case mantissas (synth.make_adversarial) written into dG_<site> / dD_<site> and the weights; per element, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|a w| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    ref64 / dropped64 / sum|a w| from synth.split_terms, c_acc the CPU EMULATION's accumulation error on the same operands
    (synth.emulate_split_dot, form "units", K = 160; synth.split_c_acc) -- never the kernel's output: the formula of tests/test_gpu_split.py.
    tests/test_feat_grad_split_abi.py shows on the CPU that losing any one of the six kept products breaks it;
 7. the same inequality on what a real backward of random cotangents leaves, the fp32 entry's error printed beside (not asserted);
 8. equal bits: NCHW == NHWC, run to run, graph replay, after the _typed and _cl backward forms, a subset of sites == all nine,
    bf16 / fp16 == dx32s.to(dtype), accumulate == (old.float() + dx32s).to(dtype);
 9. guard bands, skipped sites, refusals;  10. the module;  11. one full-size case (the grouped launch's block -> site map at
    thousands of blocks).

Shapes: (1, 2) flat -- a 7x7 site smaller than one 128-row block, P = 1; (2, 3) flat -- quirk Q1, frames >= P get the gen term only;
(3, 4) per-clip -- frames with no spatial-slice row; (2, 3) flat, Flow.  All nine sites always: C % 64 == 32 (320, 608 channels) and
the 49-pixel sites are in every case."""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from . import arena as arena_mod
from . import exact
from . import exact_units as gx
from . import units_dx_checks as checks
from . import units_grad as ug
from .units_grad import DX_SPLIT as FORM
from .units_grad import dx_check_inequality as check_inequality
from .units_grad import dx_operands as operands
from .units_grad import exact_case, rows_of, rt  # noqa: F401

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP),
          (2, 3, spec.VARIANT_FLOW, spec.SLICE_FLAT)]
IDS = ["b1l2_flat", "b2l3_flat", "b3l4_clip", "b2l3_flat_flow"]


def split(h, **kw):
    return FORM.call(h, **kw)


# ---- 5. exact integers ----

@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_exact_integers(rt, B, L, variant, slice_mode):
    c = exact_case(B, L, variant, slice_mode)
    assert c.worst < 1.0                                  # largest sum of |terms| over its limit (2^24 for dX): measured on this data
    h = c.handle(rt)
    h.off_units_train(c.feats, gx.DROP_SEED, exact.DROP_P)
    h.off_units_backward(c.feats, c.views(), gx.DROP_SEED, exact.DROP_P)
    mm = exact.Mismatches()
    for layout in ("nchw", "cl"):
        dx = split(h, layout=layout)
        acc = [t.clone(memory_format=torch.preserve_format) for t in dx]
        split(h, layout=layout, out=acc, accumulate=True)
        d16 = dict((dt, split(h, layout=layout, dtype=dt)) for dt in (torch.bfloat16, torch.float16))
        torch.cuda.synchronize()
        for si, (s, ref) in enumerate(zip(c.sites, c.ref)):
            what = "split dX %s (%s)" % (s.name, layout)
            assert dx[si].is_contiguous() if layout == "nchw" else dx[si].permute(0, 2, 3, 1).is_contiguous()
            mm.check(rows_of(dx[si]), ref["dX"], what)
            mm.check(rows_of(acc[si]), 2.0 * ref["dX"], what + " accumulated")
            for dt, res in d16.items():
                want = ref["dX"].to(dt)
                assert res[si].dtype == dt
                if not torch.equal(rows_of(res[si]), want):
                    mm.found.append("%s %s: %d elements differ from ref.to(dtype)" % (what, dt, int((rows_of(res[si]) != want).sum())))
    mm.raise_if_any()


# ---- 6. worst-case mantissas ----

ADV = [(p, s) for p in (0x00FFFF, 0x7FFFFF, 0x7F7F7F) for s in ("same", "alternating")]


@pytest.mark.parametrize("pattern,signs", ADV, ids=["0x%06X_%s" % ps for ps in ADV])
def test_worst_case_mantissas(rt, pattern, signs):
    """Emulated c_acc, A and the measured GPU accumulation constant (maximum over the nine sites), first MI355X run (also DESIGN.md 8):

        pattern   signs        dG relu   c_acc (emulation)   A        gpu accumulation max
        0x00FFFF  same         no        1.092               2.184    1.092
        0x00FFFF  alternating  yes       0.802               1.604    0.802
        0x7FFFFF  same         yes       6.169               12.338   6.169
        0x7FFFFF  alternating  no        2.752               5.504    2.752
        0x7F7F7F  same         no        6.509               13.019   6.509
        0x7F7F7F  alternating  yes       4.204               8.408    4.204
    """
    B, L, slice_mode = 2, 3, spec.SLICE_FLAT
    N, P = B * L, B * (L - 1)
    relu = (ADV.index((pattern, signs)) // 2 + ADV.index((pattern, signs))) % 2 == 1        # dG post-ReLU-like for half the cases
    w = synth.make_weights(spec.VARIANT_RGB)
    for si, (name, C, _H) in enumerate(spec.SITES):
        for j, key in enumerate(("motion_conv_gen_%s.weight" % name, "motion_spatial_down_%s.weight" % name)):
            # contraction index k = the weight's output channel (axis 0): the signs alternate along it
            w[key] = synth.make_adversarial(w[key].shape, pattern, signs, seed=300 + 2 * si + j, k_axis=0) * np.float32(2.0 ** -4)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(w) == []
    feats = [ug.dev(f) for f in synth.make_features(B, L, 2)]
    h.off_units(feats)
    h.off_units_backward(feats, ug.random_views(P)[1])                # sets the backward-has-run flag; its dG / dD are replaced below
    for si, (name, _C, H) in enumerate(spec.SITES):
        h.region("dG_" + name, 128).copy_(ug.dev(synth.make_adversarial((N * H * H, 128), pattern, "same", seed=400 + si, relu=relu)))
        h.region("dD_" + name, 32).copy_(ug.dev(synth.make_adversarial((P * H * H, 32), pattern, "same", seed=500 + si)))
    got = split(h, layout="nchw")
    got_cl = split(h, layout="cl")
    torch.cuda.synchronize()
    worst = [0.0, 0.0]
    for si, (name, _C, _H) in enumerate(spec.SITES):
        a, wk = operands(h, B, L, slice_mode, si, w["motion_conv_gen_%s.weight" % name], w["motion_spatial_down_%s.weight" % name])
        assert arena_mod.same_bits(got[si], got_cl[si].contiguous())
        ce, cg = check_inequality("worst case 0x%06X %-11s relu %d site %s" % (pattern, signs, relu, name), rows_of(got[si]), a, wk)
        worst = [max(worst[0], ce), max(worst[1], cg)]
    print("worst case 0x%06X %-11s relu %d: emulated c_acc %.3f, A %.3f, gpu accumulation max %.3f" % (pattern, signs, relu, worst[0],
                                                                                                   max(1.0, 2 * worst[0]), worst[1]))


# ---- 7. random inputs from a real backward ----

@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_random_backward_within_the_bound(rt, B, L, variant, slice_mode):
    c = ug.case(rt, B, L, variant, slice_mode, 7)
    c.run()
    got = split(c.h, layout="nchw")
    got32 = c.h.off_units_backward_feats(layout="nchw")
    torch.cuda.synchronize()
    for si, (name, _C, _H) in enumerate(spec.SITES):
        wg, wd = c.weights(si)
        a, wk = operands(c.h, B, L, slice_mode, si, wg, wd)
        check_inequality("random %s site %s" % (IDS[SHAPES.index((B, L, variant, slice_mode))], name), rows_of(got[si]), a, wk, rows_of(got32[si]))
        assert float(got[si].abs().max()) > 0


# ---- 8. equal bits ----

def test_equal_bits_properties(rt):
    c = ug.case(rt, 2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    first, _per_dtype = checks.equal_bits(FORM, c)
    fp32 = c.h.off_units_backward_feats(layout="nchw")
    torch.cuda.synchronize()
    assert any(not arena_mod.same_bits(a, b) for a, b in zip(first, fp32))          # its own bits, not the fp32 entry's


@pytest.mark.parametrize("kind", ["typed_bf16", "cl_f32", "cl_f16"])
def test_same_bits_after_the_typed_and_cl_backward(rt, kind):
    checks.same_bits_after_the_other_backwards(FORM, ug.Case(rt, 2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT, 7), kind, torch.float32)


def test_bound_weights_are_read_at_launch_time(rt):
    """The pre-pass cuts the weights as they are when the call is enqueued: after an in-place update the result follows the new ones."""
    B, L = 1, 2
    c = ug.Case(rt, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    bound = c.bind_unit_weights()
    c.run()
    before = split(c.h, layout="nchw")
    for t in bound.values():
        t.mul_(1.25)
    got = split(c.h, layout="nchw")
    torch.cuda.synchronize()
    for si, (name, _C, _H) in enumerate(spec.SITES):
        a, wk = operands(c.h, B, L, spec.SLICE_FLAT, si, bound["motion_conv_gen_%s.weight" % name], bound["motion_spatial_down_%s.weight" % name])
        check_inequality("bound weights site %s" % name, rows_of(got[si]), a, wk)
        assert not torch.equal(got[si], before[si])


# ---- 9. memory discipline and refusals ----

@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("B,L,slice_mode", [(1, 2, spec.SLICE_FLAT), (3, 4, spec.SLICE_PER_CLIP)])
def test_memory_discipline(rt, layout, B, L, slice_mode, dt):
    for accumulate in (False, True):
        checks.memory_discipline(FORM, ug.case(rt, B, L, spec.VARIANT_RGB, slice_mode, 7), layout, dt, accumulate)


def test_refusals_leave_the_outputs_untouched(rt):
    checks.refusals(rt, FORM, torch.float32)


def test_trace_names(rt):
    c = ug.case(rt, 1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    c.run()
    c.h.set_profiling(2)
    split(c.h, layout="nchw")
    split(c.h, layout="cl", dtype=torch.bfloat16)
    split(c.h, layout="nchw", dtype=torch.float16)
    names = [k for k in c.h.launch_times() if "feature-map gradient" in k]
    c.h.set_profiling(0)
    assert sorted(names) == sorted(["units:feature-map gradient (dX, NCHW, split)", "units:feature-map gradient (dX, NHWC, split, bf16)",
                                    "units:feature-map gradient (dX, NCHW, split, fp16)"])


# ---- 10. the module ----

def test_module_split_feat_grad(rt, monkeypatch):
    B, L = 2, 3
    P = B * (L - 1)
    lib = _lib.load()
    calls = []
    for name in ("offk_off_units_backward_feats", "offk_off_units_backward_feats_typed", "offk_off_units_backward_feats_split"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append(name), real(*a))[1])(real, name))
    u, wnp = ug.make_units(B, L, True, feat_grad_arith="f32split")
    feats_np = synth.make_features(B, L, 2)
    feats = [ug.dev(f).requires_grad_(True) for f in feats_np]
    cots = ug.module_cots(P)
    torch.autograd.backward(u(feats, drop_seed=7), cots)
    torch.cuda.synchronize()
    assert calls == ["offk_off_units_backward_feats_split"]
    ug.assert_module_dx_matches_the_oracle(u, wnp, feats_np, feats, cots, B, L)
    pgrads = {k: p.grad.clone() for k, p in u.named_parameters() if p.grad is not None}
    split32 = [f.grad.clone() for f in feats]

    # the default module: the fp32 entry as before, the same parameter gradients bit for bit
    del calls[:]
    u0, _w = ug.make_units(B, L, True)
    assert u0.feat_grad_arith == "fp32"
    f0 = [ug.dev(f).requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u0(f0, drop_seed=7), cots)
    assert calls == ["offk_off_units_backward_feats"]
    p0 = {k: p.grad for k, p in u0.named_parameters() if p.grad is not None}
    assert p0.keys() == pgrads.keys() and len(p0) == 54 and all(torch.equal(p0[k], pgrads[k]) for k in p0)
    assert all(ug.rel_err(a, b.grad) < ug.RTOL for a, b in zip(split32, f0))

    # bf16 maps: bf16 gradients, the split fp32 result of the same (bf16-valued) maps rounded once
    del calls[:]
    fb = [ug.dev(f).bfloat16().requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u(fb, drop_seed=7), cots)
    ff = [f.detach().float().requires_grad_(True) for f in fb]
    torch.autograd.backward(u(ff, drop_seed=7), cots)
    assert calls == ["offk_off_units_backward_feats_split"] * 2
    for a, b in zip(fb, ff):
        assert a.grad.dtype == torch.bfloat16 and torch.equal(a.grad, b.grad.bfloat16())
    # channels_last maps: channels_last gradients, the same bits
    fc = [ug.dev(f).contiguous(memory_format=torch.channels_last).requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u(fc, drop_seed=7), cots)
    for f, want in zip(fc, split32):
        assert f.grad.is_contiguous(memory_format=torch.channels_last) and not f.grad.is_contiguous()
        assert torch.equal(f.grad, want)


# ---- 11. full size ----

def test_full_size(rt):
    """B = 64, L = 7: 4096 sampled rows per site (the first and the last among them) under test 6's inequality, both the fp32 NHWC
    and the bf16 NCHW form of the launch (9262 blocks); doubling dM doubles dX; zero dM gives exactly zero."""
    dxb = []

    def check_rows(si, h, wnp, idx, got):
        site = spec.SITES[si][0]
        if not dxb:
            dxb.extend(split(h, layout="nchw", dtype=torch.bfloat16))
        a, wk = operands(h, 64, 7, spec.SLICE_FLAT, si, wnp[ug.GEN_W % site], wnp[ug.DOWN_W % site], rows=idx)
        check_inequality("full size site %s" % site, got, a, wk)
        assert torch.equal(rows_of(dxb[si])[idx], got.bfloat16())

    checks.full_size(rt, FORM, check_rows)
