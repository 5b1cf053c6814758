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
import ctypes
import functools

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth
from oracle import off_oracle as orc

from . import arena as arena_mod

pytestmark = pytest.mark.gpu
RTOL = 2e-4
DROP_P = 0.8
U = 2.0 ** -23
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_FLAT),
          (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP), (3, 2, spec.VARIANT_RGB, spec.SLICE_FLAT),
          (5, 9, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP)]
IDS = ["b1l2", "b2l3_flat", "b3l4_flat", "b3l4_clip", "b3l2", "b5l9_clip_flow"]


@pytest.fixture(scope="module")
def rt():
    from offk_amd import runtime
    return runtime


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.cuda().contiguous()


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def unit_drop(seed, P, p=DROP_P):
    return [torch.from_numpy(synth.dropout_keep(seed, si, P, H, p)).float() / (1.0 - p) for si, (_n, _c, H) in enumerate(spec.SITES)]


def device_relu_masks(h, feats_cpu, w, B, L, slack=1e-5):
    """The ReLU decisions the device took (saved G > 0) as nine [N,128,H,H] 0/1 tensors, after checking that they differ from the
    oracle's own only for pre-activations within rounding distance of zero (as in tests/test_gpu_backward.py)."""
    masks = []
    for (site, _c, H), x in zip(spec.SITES, feats_cpu):
        G = h.region("G_" + site, 128).view(B * L, H * H, 128).permute(0, 2, 1).reshape(B * L, 128, H, H).cpu()
        with torch.no_grad():
            pre = torch.nn.functional.conv2d(x, w["motion_conv_gen_%s.weight" % site], w["motion_conv_gen_%s.bias" % site])
        mask = (G > 0)
        flip = mask != (pre > 0)
        assert int(flip.sum()) <= 5 + slack * flip.numel(), site
        if flip.any():
            assert float(pre[flip].abs().max()) < slack * max(1.0, float(pre.abs().max())), site
        masks.append(mask.float())
    return masks


def random_views(P, seed=5, scale=1.0):
    """Random gradients w.r.t. the three fusion buffers (channels-last) and the nine (tensor, coff) views of the units in them."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bufs = [scale * torch.randn(P, H, H, C, device="cuda", generator=gen) for H, C in ((28, 320), (14, 1056), (7, 832))]
    return bufs, [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]


def down_rows(B, L, slice_mode):
    """r(n) of every frame n, -1 outside the spatial slice."""
    N, P = B * L, B * (L - 1)
    if slice_mode == spec.SLICE_FLAT:
        return [n if n < P else -1 for n in range(N)]
    return [(n // L) * (L - 1) + n % L if n % L < L - 1 else -1 for n in range(N)]


class Case:
    """One handle after forward + backward on random dM, with everything the checks share."""

    def __init__(self, rt, B, L, variant, slice_mode, seed):
        self.B, self.L, self.variant, self.slice_mode, self.seed = B, L, variant, slice_mode, seed
        self.N, self.P = B * L, B * (L - 1)
        self.h = rt.OffForward(B, L, variant, slice_mode, training=True)
        self.wnp = synth.make_weights(variant)
        assert self.h.load_state_dict(self.wnp) == []
        self.w = orc.to_torch_weights(self.wnp)
        self.feats_np = synth.make_features(B, L, 2 if B == 2 else 3)
        self.feats = [dev(f) for f in self.feats_np]
        self.bufs, self.views = random_views(self.P)
        self.drop = (0, 0.0) if seed is None else (seed, DROP_P)
        self.run()

    def forward(self, feats=None):
        feats = self.feats if feats is None else feats
        if self.seed is None:
            self.h.off_units(feats)
        else:
            self.h.off_units_train(feats, self.seed, DROP_P)

    def backward(self, feats=None, views=None, grads=None):
        return self.h.off_units_backward(self.feats if feats is None else feats, self.views if views is None else views,
                                         self.drop[0], self.drop[1], grads=grads)

    def run(self):
        self.forward()
        self.backward()

    def weights(self, si):
        site = spec.SITES[si][0]
        return (self.w["motion_conv_gen_%s.weight" % site].reshape(128, -1), self.w["motion_spatial_down_%s.weight" % site].reshape(32, -1))

    def reference(self, si, wg=None, wd=None):
        """fp64 product of the kernel's own inputs on the host, as [N, HW, C], its bound, and the gen part alone."""
        site, C, H = spec.SITES[si]
        HW = H * H
        dG = self.h.region("dG_" + site, 128).cpu().double().view(self.N, HW, 128)
        dD = self.h.region("dD_" + site, 32).cpu().double().view(self.P, HW, 32)
        if wg is None:
            wg, wd = self.weights(si)
        wg, wd = wg.double(), wd.double()
        rows = down_rows(self.B, self.L, self.slice_mode)
        inside = torch.tensor([r >= 0 for r in rows])
        dDn = torch.zeros(self.N, HW, 32, dtype=torch.float64)
        dDn[inside] = dD[torch.tensor([r for r in rows if r >= 0], dtype=torch.long)]
        gen = dG @ wg
        ref = gen + dDn @ wd
        bound = 160 * U * (dG.abs() @ wg.abs() + dDn.abs() @ wd.abs())
        return ref, bound, gen, inside


@functools.lru_cache(maxsize=None)
def case(rt, B, L, variant, slice_mode, seed):
    return Case(rt, B, L, variant, slice_mode, seed)


def as_rows(t, layout):
    """[N, C, H, H] result of either layout -> [N, HW, C] on the host."""
    assert t.dtype == torch.float32 and t.dim() == 4
    if layout == "cl":
        assert t.permute(0, 2, 3, 1).is_contiguous()
    else:
        assert t.is_contiguous()
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).cpu()


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


def oracle_dx(c):
    """x.grad of every site from the oracle's unit, the device's ReLU decisions on both sides."""
    tf = [torch.from_numpy(f) for f in c.feats_np]
    masks = device_relu_masks(c.h, tf, c.w, c.B, c.L)
    drops = None if c.seed is None else unit_drop(c.seed, c.P)
    out = []
    for si, ((site, _c, _h), x) in enumerate(zip(spec.SITES, tf)):
        buf, coff = c.views[si]
        dm = buf[..., coff:coff + 160].permute(0, 3, 1, 2).cpu()
        x = x.clone().requires_grad_(True)
        orc.off_unit(x, c.w, site, c.B, c.L, c.variant, c.slice_mode, None if drops is None else drops[si], masks[si]).backward(dm)
        out.append(x.grad)
    return out


# ---- 3. equal bits ----

def test_equal_bits_properties(rt):
    B, L = 3, 4
    c = case(rt, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    c.run()
    first = c.h.off_units_backward_feats(layout="nchw")
    cl = c.h.off_units_backward_feats(layout="cl")
    again = c.h.off_units_backward_feats(layout="nchw")
    acc = [t.clone() for t in first]
    c.h.off_units_backward_feats(layout="nchw", out=acc, accumulate=True)
    acc_cl = [t.clone(memory_format=torch.preserve_format) for t in cl]
    c.h.off_units_backward_feats(layout="cl", out=acc_cl, accumulate=True)
    torch.cuda.synchronize()
    for a, b, d, e, f in zip(first, cl, again, acc, acc_cl):
        assert float(a.abs().max()) > 0
        assert not b.is_contiguous() and torch.equal(a, b) and arena_mod.same_bits(a, b.contiguous())
        assert arena_mod.same_bits(a, d)
        assert arena_mod.same_bits(e, 2 * a) and arena_mod.same_bits(f.contiguous(), 2 * a)

    # backward + the new call in one graph, one replay
    grads = c.h.new_unit_grads()
    outs = [torch.empty_like(t) for t in first]

    def launch():
        c.backward(grads=grads)
        c.h.off_units_backward_feats(layout="nchw", out=outs)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for t in outs:
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert all(arena_mod.same_bits(a, b) for a, b in zip(first, outs))


@pytest.mark.parametrize("kind", ["typed_bf16", "cl_f32", "cl_f16"])
def test_same_bits_after_the_typed_and_cl_backward(rt, kind):
    """offk_off_units_backward_typed / _cl on the same logical maps leave the same dG / dD, so dX is the plain form's."""
    B, L = 2, 3
    c = Case(rt, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    dt = {"typed_bf16": torch.bfloat16, "cl_f32": torch.float32, "cl_f16": torch.float16}[kind]
    x = [f.to(dt) for f in c.feats]
    plain = [t.float() for t in x]
    other = [t.contiguous(memory_format=torch.channels_last) for t in x] if kind.startswith("cl") else x
    res = []
    for feats in (plain, other):
        c.forward(feats)
        c.backward(feats)
        res.append(c.h.off_units_backward_feats(layout="nchw"))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert float(a.abs().max()) > 0 and arena_mod.same_bits(a, b)


# ---- 4. memory discipline ----

@pytest.mark.parametrize("layout", ["nchw", "cl"])
@pytest.mark.parametrize("B,L,slice_mode", [(1, 2, spec.SLICE_FLAT), (3, 4, spec.SLICE_PER_CLIP)])
def test_memory_discipline(rt, layout, B, L, slice_mode):
    c = case(rt, B, L, spec.VARIANT_RGB, slice_mode, 7)
    c.run()
    shapes = spec.feature_shapes(B, L)
    ar = arena_mod.Arena.for_sizes([4 * int(np.prod(s)) for s in shapes])
    skipped = (1, 6)

    def carve(i):
        n, ch, hh, _ = shapes[i]
        t = ar.empty("dx_%d" % i, (n, ch, hh, hh) if layout == "nchw" else (n, hh, hh, ch))
        return t if layout == "nchw" else t.permute(0, 3, 1, 2)

    bufs = [carve(i) for i in range(9)]           # full of the sentinel, a NaN
    want = c.h.off_units_backward_feats(layout=layout)
    got = c.h.off_units_backward_feats(sites=[i for i in range(9) if i not in skipped], layout=layout,
                                       out=[None if i in skipped else b for i, b in enumerate(bufs)])
    torch.cuda.synchronize()
    ar.check()
    for i in range(9):
        if i in skipped:
            assert got[i] is None and ar.untouched(bufs[i] if layout == "nchw" else bufs[i].permute(0, 2, 3, 1))
        else:
            assert not bool(torch.isnan(got[i]).any()) and torch.equal(got[i], want[i])


# ---- 5. bound weights ----

def test_bound_weights_after_an_in_place_update(rt):
    B, L = 2, 3
    c = Case(rt, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    bound = {}
    for k, v in c.wnp.items():
        if k.startswith(spec.UNIT_PARAM_PREFIXES):
            bound[k] = dev(v)
            c.h.bind_weight(k, bound[k])
    gen = torch.Generator(device="cuda").manual_seed(11)
    for k, t in bound.items():                     # the "optimizer step", on the stream the calls go to
        t.mul_(1.25).add_(0.01 * torch.randn(t.shape, device="cuda", generator=gen))
    c.run()
    got = c.h.off_units_backward_feats(layout="nchw")
    torch.cuda.synchronize()
    for si, (site, _c, _h) in enumerate(spec.SITES):
        wg = bound["motion_conv_gen_%s.weight" % site].cpu().reshape(128, -1)
        wd = bound["motion_spatial_down_%s.weight" % site].cpu().reshape(32, -1)
        assert not torch.equal(wg, c.weights(si)[0])
        ref, bnd, _gen, _in = c.reference(si, wg, wd)
        assert bool(((as_rows(got[si], "nchw").double() - ref).abs() <= bnd).all()), site


# ---- 6. refusals ----

def test_refusals_leave_the_outputs_untouched(rt):
    B, L = 1, 2
    shapes = spec.feature_shapes(B, L)
    outs = [torch.full(tuple(s), float("nan"), device="cuda") for s in shapes]
    keep = [arena_mod.bits(t).clone() for t in outs]
    arr = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def refused(h, ws, a, layout, needle):
        rc = lib.offk_off_units_backward_feats(h._h if h is not None else None, stream, ws, a, layout, 0)
        assert rc == -1 and needle in lib.offk_last_error(h._h if h is not None else None), lib.offk_last_error(h._h if h is not None else None)

    # a handle without the training workspace: the wrapper's refusal, in the words off_units_backward uses
    plain = rt.OffForward(B, L, spec.VARIANT_RGB)
    with pytest.raises(_lib.OffkError, match="create the handle with training=True for the units' backward"):
        plain.off_units_backward_feats(out=outs)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    ws = ctypes.c_void_p(h.workspace.data_ptr())
    # no backward has run on this handle yet
    refused(h, ws, arr, _lib.FEAT_NCHW, b"no offk_off_units_backward has run")
    feats = [dev(f) for f in synth.make_features(B, L, 3)]
    h.off_units(feats)
    h.off_units_backward(feats, random_views(B * (L - 1))[1])
    refused(None, ws, arr, _lib.FEAT_NCHW, b"null argument")
    refused(h, None, arr, _lib.FEAT_NCHW, b"null argument")
    refused(h, ws, None, _lib.FEAT_NCHW, b"null argument")
    refused(h, ws, arr, 2, b"layout must be")
    refused(h, ws, arr, -1, b"layout must be")
    mis = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    mis[4] = outs[4].data_ptr() + 4
    refused(h, ws, mis, _lib.FEAT_NHWC, b"16-byte aligned")
    over = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    over[8] = h.workspace.data_ptr() + 256
    refused(h, ws, over, _lib.FEAT_NCHW, b"overlaps the workspace")
    # the wrapper's own checks
    with pytest.raises(ValueError, match="layout"):
        h.off_units_backward_feats(layout="nhwc", out=outs)
    with pytest.raises(ValueError, match="channels_last"):
        h.off_units_backward_feats(layout="cl", out=outs)
    with pytest.raises(ValueError, match="shape"):
        h.off_units_backward_feats(out=outs[1:] + outs[:1])
    with pytest.raises(ValueError, match="distinct"):
        h.off_units_backward_feats(sites=[9])
    # all nine NULL: OFFK_OK, nothing enqueued
    assert lib.offk_off_units_backward_feats(h._h, stream, ws, (ctypes.c_void_p * 9)(), _lib.FEAT_NCHW, 0) == 0
    assert h.off_units_backward_feats(sites=[]) == [None] * 9
    torch.cuda.synchronize()
    assert all(torch.equal(arena_mod.bits(t), k) for t, k in zip(outs, keep))


# ---- 7. the module ----

def make_units(B, L, feat_grad, variant="rgb"):
    from offk_amd.off_module import OFFUnits
    wnp = synth.make_weights(spec.VARIANT_RGB if variant == "rgb" else spec.VARIANT_FLOW)
    u = OFFUnits(B, L, variant, feat_grad=feat_grad).cuda()
    u.load_state_dict({k: torch.from_numpy(a) for k, a in wnp.items() if k in u.state_dict()}, strict=True)
    u.train()
    return u, wnp


def module_cots(P, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).cuda() for s in ((P, 320, 28, 28), (P, 800, 14, 14), (P, 320, 7, 7))]


def test_module_feat_grad_matches_the_oracle(rt):
    B, L = 2, 3
    P = B * (L - 1)
    u, wnp = make_units(B, L, True)
    w = orc.to_torch_weights(wnp)
    feats_np = synth.make_features(B, L, 2)
    feats = [dev(f).requires_grad_(True) for f in feats_np]
    cots = module_cots(P)
    torch.autograd.backward(u(feats, drop_seed=7), cots)
    torch.cuda.synchronize()
    tf = [torch.from_numpy(f) for f in feats_np]
    masks = device_relu_masks(u._rt, tf, w, B, L)
    drops = unit_drop(7, P)
    dms = [cots[0][:, :160], cots[0][:, 160:]] + [cots[1][:, 160 * k:160 * k + 160] for k in range(5)] + [cots[2][:, :160], cots[2][:, 160:]]
    for si, ((site, _c, _h), x) in enumerate(zip(spec.SITES, tf)):
        x = x.clone().requires_grad_(True)
        orc.off_unit(x, w, site, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, drops[si], masks[si]).backward(dms[si].cpu())
        assert feats[si].grad is not None and feats[si].grad.shape == x.grad.shape
        assert rel_err(feats[si].grad, x.grad) < RTOL, site


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
    N, P = B * L, B * (L - 1)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, training=True)
    wnp = synth.make_weights(spec.VARIANT_RGB)
    assert h.load_state_dict(wnp) == []
    feats = [dev(f) for f in synth.make_features(B, L, 2)]
    h.off_units_train(feats, 21, DROP_P)
    bufs, views = random_views(P)
    h.off_units_backward(feats, views, 21, DROP_P)
    dx = h.off_units_backward_feats(layout="cl")
    gen = torch.Generator(device="cuda").manual_seed(9)
    rows = down_rows(B, L, spec.SLICE_FLAT)
    for si, (site, C, H) in enumerate(spec.SITES):
        HW = H * H
        idx = torch.randint(0, N * HW, (4096,), device="cuda", generator=gen)
        idx[:2] = torch.tensor([0, N * HW - 1], device="cuda")
        f, px = idx // HW, idx % HW
        r = torch.tensor(rows, device="cuda")[f]
        a = torch.zeros(4096, 160, dtype=torch.float64, device="cuda")
        a[:, :128] = h.region("dG_" + site, 128)[idx].double()
        ins = r >= 0
        a[ins, 128:] = h.region("dD_" + site, 32)[(r * HW + px)[ins]].double()
        wcat = torch.cat((dev(wnp["motion_conv_gen_%s.weight" % site]).reshape(128, C), dev(wnp["motion_spatial_down_%s.weight" % site]).reshape(32, C))).double()
        ref = torch.matmul(a, wcat)
        bound = 160 * U * torch.matmul(a.abs(), wcat.abs())
        got = dx[si].permute(0, 2, 3, 1).reshape(N * HW, C)[idx].double()
        assert bool(((got - ref).abs() <= bound).all()), site
        assert float(ref.abs().max()) > 0
    d1 = [t.clone() for t in dx]
    h.off_units_backward(feats, [(2.0 * t, c) for t, c in views], 21, DROP_P)
    d2 = h.off_units_backward_feats(layout="cl")
    for a, b in zip(d1, d2):
        assert float((b - 2.0 * a).abs().max()) <= 1e-6 * float((2.0 * a).abs().max())
    h.off_units_backward(feats, [(torch.zeros_like(t), c) for t, c in views], 21, DROP_P)
    d0 = h.off_units_backward_feats(layout="cl")
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in d0)
