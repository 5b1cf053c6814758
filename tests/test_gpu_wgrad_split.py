"""The units' backward with the weight-gradient GEMM in split-fp32 arithmetic on the bf16 matrix pipe (offk_off_units_backward_split,
csrc/units_wgrad_split.hip; OffForward.off_units_backward(arith="f32split"), OFFUnits(wgrad_arith="f32split")):

    dW[m][c] = sum over (frame f, pixel q) a[(f, q)][m] X[f][c][q],   a = [dGpre (128) | dD at row r(f) (32), zeros outside the slice]

 1. exact integer inputs (tests/exact.py): the whole flat gradient buffer equals the fp64 reference value for value, in all six map
    forms (NCHW / channels-last x fp32 / bf16 / fp16), accumulate twice = 2 x -- what catches a skipped K-tile or a wrong chunk edge;
 2. worst-case mantissas (synth.make_adversarial) in the maps and in dG_<site> / dD_<site>: the entry runs K2b itself, so the
    cotangents are made such that K2b LEAVES the patterns (identity depthwise taps, p = 0: dD = dS; G > 0 and one temporal pair per
    clip, or a masked middle frame: dGpre = -+ dT) and the test reads them back.  Per element of both weight gradients, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|a x| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation error on the same operands in the kernel's chunked form (tests/wgrad_split.py) -- never the
    kernel's output.  tests/test_wgrad_split_abi.py shows on the CPU that losing any one issued product breaks it;
 3. the same inequality on a real backward of random cotangents, the default entry's error printed beside (not asserted);
 4. equal bits: NCHW == channels-last per dtype, 16-bit maps == x.float() (sign of zero excepted), run to run, graph replay, every bias /
    depthwise gradient and dG_ / dD_ == the default backward's, off_units_backward_feats in both ariths behind either backward;
 5. guard bands round grads, the workspace and inside the slabs; refusals leave the buffers untouched;  6. the module.

Shapes (B, L): (1, 2) flat -- N = 2, the 7x7 sites are one chunk, the 28x28 sites end in a short chunk; (2, 3) flat -- quirk Q1, chunk
boundaries inside frames (25 and 7 K-tiles per frame against 4 per block); (3, 4) per-clip; (2, 3) flat, Flow; (8, 7) per-clip -- 13 K-tiles
per block, chunks that span several frames.  All nine sites always: C % 128 = 64 (320) and 96 (608), 49-pixel rows, 1024 channels."""
import ctypes

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth
from oracle import off_oracle as orc

from . import arena as arena_mod
from . import exact
from . import featmaps as fm
from . import exact_units as gx
from . import units_grad as ug
from .units_grad import DTS, FORMS, IDS, RTOL, SHAPES, as_form, exact_case, rt  # noqa: F401
from .wgrad_split import KPB, check_inequality, dw_t, site_operands

pytestmark = pytest.mark.gpu


def split_bwd(h, feats, views, seed, p, **kw):
    return h.off_units_backward(feats, views, seed, p, arith="f32split", **kw)


def is_matrix(key):
    return key.endswith(".weight") and (key.startswith("motion_conv_gen_") or key.startswith("motion_spatial_down_"))


# ---- 1. exact integers ----

@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_exact_integers(rt, B, L, variant, slice_mode):
    c = exact_case(B, L, variant, slice_mode)
    assert c.worst < 1.0                                  # largest sum of |terms| over its limit: measured on this data
    h = c.handle(rt)
    assert gx.k1b_plan(h)[1] == KPB[SHAPES.index((B, L, variant, slice_mode))]
    views = c.views()
    h.off_units_train(c.feats, gx.DROP_SEED, exact.DROP_P)
    nkeys = 54 if variant == spec.VARIANT_RGB else 36
    for layout, dt in FORMS:
        maps = as_form(c.feats, layout, dt)
        assert all(torch.equal(m.float(), x) for m, x in zip(maps, c.feats))         # small integers: exact in both 16-bit types
        what = "split backward (%s, %s)" % (layout, dt)
        gx.poison(h, [("dG_" + s.name, 128) for s in c.sites] + [("dD_" + s.name, 32) for s in c.sites])
        flat = torch.full_like(h.new_unit_grads(), gx.NAN)
        flat, got = split_bwd(h, maps, views, gx.DROP_SEED, exact.DROP_P, grads=flat)
        assert gx.check_backward(h, c.sites, c.ref, got, what) == nkeys
        _flat, got2 = split_bwd(h, maps, views, gx.DROP_SEED, exact.DROP_P, grads=flat, accumulate=True)
        gx.check_backward(h, c.sites, c.ref, got2, what + ", accumulated", twice=True)


# ---- 2. worst-case mantissas ----

ADV = [(p, s) for p in (0x00FFFF, 0x7FFFFF, 0x7F7F7F) for s in ("same", "alternating")]
WORST = [(1, 2) + ps for ps in ADV] + [(2, 3, 0x00FFFF, "same"), (2, 3, 0x7F7F7F, "alternating")]


def frame_signs(L):
    """What K2b leaves in frame t of a clip, as a sign: L = 2: dGpre = (-dT0, +dT0); L = 3 with the middle frame's G = 0: (-dT0, 0, +dT1)."""
    return {2: (-1.0, 1.0), 3: (-1.0, 0.0, 1.0)}[L]


@pytest.mark.parametrize("B,L,pattern,signs", WORST, ids=["b%dl%d_0x%06X_%s" % w for w in WORST])
def test_worst_case_mantissas(rt, B, L, pattern, signs):
    """Emulated c_acc, A and the measured GPU accumulation constant (maximum over the nine sites), first MI355X run (also DESIGN.md 8; at
    2 x 3 the emulation runs on a sample of 128 channel columns per site, the GPU figure is over all of them):

        shape  pattern   signs        dT relu   c_acc (emulation)   A        gpu accumulation max
        1 x 2  0x00FFFF  same         no        4.086               8.172    4.086
        1 x 2  0x00FFFF  alternating  yes       1.290               2.581    1.290
        1 x 2  0x7FFFFF  same         no        5.100               10.199   5.533
        1 x 2  0x7FFFFF  alternating  yes       3.678               7.355    3.678
        1 x 2  0x7F7F7F  same         no        4.870               9.741    4.870
        1 x 2  0x7F7F7F  alternating  yes       3.860               7.720    3.860
        2 x 3  0x00FFFF  same         no        5.618               11.236   5.618
        2 x 3  0x7F7F7F  alternating  yes       1.812               3.624    2.275
    """
    slice_mode = spec.SLICE_FLAT
    N, P, T = B * L, B * (L - 1), L - 1
    idx = WORST.index((B, L, pattern, signs))
    relu = idx % 2 == 1                                   # post-ReLU-like cotangents for half the cases
    w = synth.make_weights(spec.VARIANT_RGB)
    for name, _C, _H in spec.SITES:                       # identity depthwise taps: K2b's dD is dS itself
        k = np.zeros((32, 1, 3, 3), dtype=np.float32)
        k[:, 0, 1, 1] = 1.0
        w["motion_spatial_grad_%s.weight" % name] = k
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(w) == []
    fs = frame_signs(L)
    maps = []
    for si, (name, C, H) in enumerate(spec.SITES):
        # contraction index = (frame, pixel): the signs alternate along the pixels; "same": the map's frame sign follows a's, so that no
        # element's products cancel
        x = synth.make_adversarial((N, C, H * H), pattern, signs, seed=600 + si, k_axis=2, relu=(pattern == 0x7FFFFF))
        for n in range(N):
            if fs[n % L] < 0:
                x[n] = -x[n]
        maps.append(ug.dev(x.reshape(N, C, H, H)))
    h.off_units(maps)
    # G decides K2b's ReLU mask only: all on, the middle frame of a three-frame clip off
    for name, _C, H in spec.SITES:
        G = h.region("G_" + name, 128).view(B, L, H * H, 128)
        G.fill_(1.0)
        if L == 3:
            G[:, 1].zero_()
    # cotangents: dS = pattern, dT[b, t] = pattern (one pair per clip at L = 2; at L = 3 dT0 and dT1 reach frames 0 and 2 alone)
    bufs, views = {}, []
    for si, ((name, _C, H), (reg, cs, coff)) in enumerate(zip(spec.SITES, gx.UNIT_SLOTS)):
        if reg not in bufs:
            bufs[reg] = torch.full((P, H, H, cs), 7.0, device="cuda")
        dS = synth.make_adversarial((P, H, H, 32), pattern, "same", seed=500 + si)
        dT = synth.make_adversarial((P, H, H, 128), pattern, "same", seed=400 + si, relu=relu)
        bufs[reg][..., coff:coff + 32] = ug.dev(dS)
        bufs[reg][..., coff + 32:coff + 160] = ug.dev(dT)
        views.append((bufs[reg], coff))
    kpb = gx.k1b_plan(h)[1]
    assert kpb == 4
    _flat, got = split_bwd(h, maps, views, 0, 0.0)
    _flat, got_cl = split_bwd(h, as_form(maps, "cl", "f32"), views, 0, 0.0)
    torch.cuda.synchronize()
    worst = [0.0, 0.0]
    for si, (name, C, H) in enumerate(spec.SITES):
        # K2b left the patterns: every non-zero element of dG_ / dD_ carries the mantissa
        for reg, ch in (("dG_" + name, 128), ("dD_" + name, 32)):
            v = h.region(reg, ch)
            bits = v.view(torch.int32)
            assert bool(((bits & 0x7FFFFF) == pattern)[v != 0].all()) and int((v != 0).sum()) > v.numel() // 4, reg
        a, x = site_operands(h, B, L, slice_mode, si, maps[si])
        assert arena_mod.same_bits(dw_t(got, si), dw_t(got_cl, si))
        ce, cg = check_inequality("worst case b%dl%d 0x%06X %-11s relu %d site %s" % (B, L, pattern, signs, relu, name), dw_t(got, si), a, x, kpb,
                                  max_cols=None if N == 2 else 128)
        worst = [max(worst[0], ce), max(worst[1], cg)]
    print("worst case b%dl%d 0x%06X %-11s relu %d: emulated c_acc %.3f, A %.3f, gpu accumulation max %.3f" % (
        B, L, pattern, signs, relu, worst[0], max(1.0, 2 * worst[0]), worst[1]))


# ---- 3. random inputs from a real backward ----

@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES[:4], ids=IDS[:4])
def test_random_backward_within_the_bound(rt, B, L, variant, slice_mode):
    c = ug.case(rt, B, L, variant, slice_mode, 7)
    c.forward()
    _flat, got32 = c.backward()
    got32 = dict((k, v.clone()) for k, v in got32.items())
    _flat, got = split_bwd(c.h, c.feats, c.views, c.drop[0], c.drop[1])
    torch.cuda.synchronize()
    kpb = gx.k1b_plan(c.h)[1]
    for si, (name, _C, _H) in enumerate(spec.SITES):
        a, x = site_operands(c.h, B, L, slice_mode, si, c.feats[si])
        check_inequality("random %s site %s" % (IDS[SHAPES.index((B, L, variant, slice_mode))], name), dw_t(got, si), a, x, kpb, dw_t(got32, si),
                         max_cols=None if B * L == 2 else 96)
        assert float(dw_t(got, si).abs().max()) > 0
    # everything but the two weight matrices is the default backward's, bit for bit
    assert got.keys() == got32.keys()
    assert all(arena_mod.same_bits(got[k], got32[k]) for k in got if not is_matrix(k))


# ---- 4. equal bits ----

def test_equal_bits_properties(rt):
    B, L = 2, 3
    P = B * (L - 1)
    h = fm.make_train_handle(rt, B, L)
    _bufs, views = ug.random_views(P)
    x32 = fm.relu_maps(B, L, torch.float32, 11)
    x32 = [x - 0.25 * (x > 1.0) for x in x32]                       # some negative values too
    regions = [("dG_" + n, 128) for n, _c, _h in spec.SITES] + [("dD_" + n, 32) for n, _c, _h in spec.SITES]
    base = None
    for dt in DTS:
        xd = as_form(x32, "nchw", dt)
        wide = [x.float() for x in xd]
        h.off_units_train(xd, fm.DROP_SEED, fm.DROP_P)
        flat_d, got_d = h.off_units_backward(xd, views, fm.DROP_SEED, fm.DROP_P)          # the default backward
        left_d = [h.region(*r).clone() for r in regions]
        dx_d = [h.off_units_backward_feats(layout="nchw", arith=ar) for ar in rt.FEAT_GRAD_ARITHS]
        gx.poison(h, regions)
        flat, got = split_bwd(h, xd, views, fm.DROP_SEED, fm.DROP_P)
        left = [h.region(*r).clone() for r in regions]
        dx = [h.off_units_backward_feats(layout="nchw", arith=ar) for ar in rt.FEAT_GRAD_ARITHS]
        flat_cl, _g = split_bwd(h, as_form(x32, "cl", dt), views, fm.DROP_SEED, fm.DROP_P)
        flat_again, _g = split_bwd(h, xd, views, fm.DROP_SEED, fm.DROP_P)
        flat_wide, _g = split_bwd(h, wide, views, fm.DROP_SEED, fm.DROP_P)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(flat).all()) and float(flat.abs().max()) > 0
        assert arena_mod.same_bits(flat, flat_cl), dt                                   # NCHW == channels-last
        assert arena_mod.same_bits(flat, flat_again), dt                                # run to run
        assert torch.equal(flat, flat_wide), dt                                         # 16-bit maps == x.float(): equal values (a zero's sign aside)
        assert int((arena_mod.bits(flat) != arena_mod.bits(flat_wide)).sum()) == int(((flat == 0) & (arena_mod.bits(flat) != arena_mod.bits(flat_wide))).sum())
        # bias and depthwise gradients, dG_ / dD_: the default backward's bits; the two matrices: its own
        assert all(arena_mod.same_bits(got[k], got_d[k]) for k in got if not is_matrix(k)), dt
        assert any(not arena_mod.same_bits(got[k], got_d[k]) for k in got if is_matrix(k)), dt
        assert all(arena_mod.same_bits(a, b) for a, b in zip(left, left_d)), dt
        # off_units_backward_feats in both ariths behind the split backward == behind the default one
        for per_arith, per_arith_d in zip(dx, dx_d):
            assert all(arena_mod.same_bits(a, b) for a, b in zip(per_arith, per_arith_d)), dt
        if dt == "f32":
            base = (xd, flat)

    # capture and replay
    xd, first = base
    h.off_units_train(xd, fm.DROP_SEED, fm.DROP_P)
    grads = h.new_unit_grads()

    def launch():
        split_bwd(h, xd, views, fm.DROP_SEED, fm.DROP_P, grads=grads)

    g = ug.captured(launch)
    for _ in range(2):
        grads.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert arena_mod.same_bits(grads, first)


def test_any_handle(rt):
    """A split-fp32 handle and bound weights: the same bits as the fp32 handle with set weights; the default backward of the split-fp32
    handle stays the fp32 kernel (the entry is opt-in)."""
    B, L = 1, 2
    _bufs, views = ug.random_views(B * (L - 1))
    x = fm.relu_maps(B, L, torch.float32, 12)
    res = []
    for prec, bind in (("fp32", False), ("f32split", True)):
        h = rt.OffForward(B, L, spec.VARIANT_RGB, precision=prec, training=True)
        wnp = synth.make_weights(spec.VARIANT_RGB)
        assert h.load_state_dict(wnp) == []
        keep = []
        if bind:
            for k, v in wnp.items():
                if k.startswith(spec.UNIT_PARAM_PREFIXES):
                    keep.append(ug.dev(v))
                    h.bind_weight(k, keep[-1])
        h.off_units_train(x, 5, fm.DROP_P)
        d = h.off_units_backward(x, views, 5, fm.DROP_P)[0].clone()
        s = split_bwd(h, x, views, 5, fm.DROP_P)[0].clone()
        torch.cuda.synchronize()
        res.append((d, s))
    assert arena_mod.same_bits(res[0][0], res[1][0]) and arena_mod.same_bits(res[0][1], res[1][1])
    assert not arena_mod.same_bits(res[0][0], res[0][1])


# ---- 5. memory discipline and refusals ----

@pytest.mark.parametrize("layout,dt", [("nchw", "f32"), ("nchw", "bf16"), ("cl", "f32"), ("cl", "f16")])
@pytest.mark.parametrize("B,L,slice_mode", [(1, 2, spec.SLICE_FLAT), (3, 4, spec.SLICE_PER_CLIP)])
def test_memory_discipline(rt, B, L, slice_mode, layout, dt):
    """Workspace, gradient buffer, maps and cotangents are carves of one sentinel-filled arena: nothing outside a carve changes, the
    gradient buffer (exactly offk_unit_grad_floats, left full of NaN sentinels) is written in full and equals the run in ordinary
    allocations, and inside the workspace every slab holds finite values in its C columns and the sentinel in its pad columns."""
    P = B * (L - 1)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    maps = as_form(fm.relu_maps(B, L, torch.float32, 13), layout, dt)
    bufs, views = ug.random_views(P)
    h.off_units_train(maps, 3, fm.DROP_P)
    want = split_bwd(h, maps, views, 3, fm.DROP_P)[0].clone()
    torch.cuda.synchronize()
    n = want.numel()
    ar, _ws = ug.workspace_arena(h, maps, [4 * n] + [4 * b.numel() for b in bufs])
    grads = ar.empty("unit_grads", (n,))
    gm = ug.guarded_maps(ar, maps, layout)
    gb = [ar.put("dm_%d" % i, b) for i, b in enumerate(bufs)]
    gviews = [(gb[[id(b) for b in bufs].index(id(t))], coff) for t, coff in views]
    h.off_units_train(gm, 3, fm.DROP_P)
    flat, _got = split_bwd(h, gm, gviews, 3, fm.DROP_P, grads=grads)
    torch.cuda.synchronize()
    ar.check()
    assert flat.data_ptr() == grads.data_ptr() and bool(torch.isfinite(grads).all()) and arena_mod.same_bits(grads, want)
    counts, _kpb = gx.k1b_plan(h)
    for (name, C, _H), nchunks in zip(spec.SITES, counts):
        cpad = (C + 127) // 128 * 128
        slab = h.region("wgs_" + name, cpad)
        assert slab.shape[0] == nchunks * 160
        assert bool(torch.isfinite(slab[:, :C]).all()), name
        if cpad > C:
            assert ar.untouched(slab[:, C:]), "%s: pad columns of the slabs were written" % name
        assert bool(torch.isfinite(h.region("wgb_" + name, 160)).all()), name


def test_refusals_leave_the_buffers_untouched(rt):
    B, L = 1, 2
    P = B * (L - 1)
    lib = _lib.load()
    h = fm.make_train_handle(rt, B, L)
    x = fm.relu_maps(B, L, torch.float32, 14)
    x16 = [t.bfloat16() for t in x]
    _bufs, views = ug.random_views(P)
    h.off_units_train(x, 3, fm.DROP_P)
    h.workspace.fill_(0x5a)
    grads = torch.full((h.new_unit_grads().numel(),), 3.25, device="cuda")
    torch.cuda.synchronize()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_p = ctypes.c_void_p(h.workspace.data_ptr())
    gp = ctypes.cast(grads.data_ptr(), ctypes.POINTER(ctypes.c_float))

    def arr_of(ts):
        return (ctypes.c_void_p * 9)(*[t.data_ptr() for t in ts])

    def gv_of(vs):
        gv = (_lib.OffkGradView * 9)()
        for i, (t, coff) in enumerate(vs):
            gv[i].data, gv[i].cstride, gv[i].coff = t.data_ptr(), t.shape[-1], coff
        return gv

    def refused(needle, hh=h, fdt=_lib.FEAT_F32, layout=_lib.FEAT_NCHW, arr=None, gv=None, ws=ws_p, p=fm.DROP_P, g=gp):
        handle = hh._h if hh is not None else None
        rc = lib.offk_off_units_backward_split(handle, stream, fdt, layout, arr_of(x) if arr is None else arr, gv_of(views) if gv is None else gv,
                                               ws, ctypes.c_uint64(3), p, g, 0)
        msg = lib.offk_last_error(handle)
        assert rc == -1 and needle in msg, msg

    refused(b"offk_off_units_backward_split: null argument", hh=None)
    refused(b"offk_off_units_backward_split: null argument", ws=None)
    refused(b"offk_off_units_backward_split: null argument", g=None)
    refused(b"layout must be", layout=2)
    refused(b"layout must be", layout=-1)
    refused(b"unknown feat_dtype", fdt=3)
    refused(b"unknown feat_dtype", fdt=-1, layout=_lib.FEAT_NHWC)
    refused(b"NCHW", hh=fm.make_train_handle(rt, B, L, feat_layout=1), ws=ctypes.c_void_p(h.workspace.data_ptr()))     # an NHWC handle, NCHW maps
    refused(b"NCHW", hh=fm.make_train_handle(rt, B, L, feat_layout=1), fdt=_lib.FEAT_BF16, arr=arr_of(x16))
    null = arr_of(x)
    null[8] = None
    refused(b"null feature map", arr=null)
    refused(b"null feature map", arr=null, layout=_lib.FEAT_NHWC)
    mis = arr_of(x16)
    mis[4] = x16[4].data_ptr() + 2
    refused(b"8-byte aligned", fdt=_lib.FEAT_BF16, arr=mis)
    mis[4] = x16[4].data_ptr() + 8
    refused(b"16-byte aligned", fdt=_lib.FEAT_BF16, layout=_lib.FEAT_NHWC, arr=mis)
    mis = arr_of(x)
    mis[0] = x[0].data_ptr() + 4
    refused(b"16-byte aligned", layout=_lib.FEAT_NHWC, arr=mis)
    refused(b"dropout probability", p=1.0)
    refused(b"dropout probability", p=-0.1)
    gv = gv_of(views)
    gv[3].coff = 2
    refused(b"gradient view", gv=gv)
    gv = gv_of(views)
    gv[7].cstride = gv[7].coff + 156
    refused(b"gradient view", gv=gv, layout=_lib.FEAT_NHWC)
    gv = gv_of(views)
    gv[1].data = None
    refused(b"null feature map or gradient", gv=gv)
    with pytest.raises(ValueError, match="arith must be one of"):
        h.off_units_backward(x, views, 3, fm.DROP_P, grads=grads, arith="bf16")
    with pytest.raises(_lib.OffkError, match="training=True"):
        split_bwd(rt.OffForward(B, L, spec.VARIANT_RGB), x, views, 3, fm.DROP_P, grads=grads)
    torch.cuda.synchronize()
    assert bool((h.workspace == 0x5a).all()) and bool((grads == 3.25).all())      # nothing was enqueued
    # and none of this disturbed the handle: the next call runs
    h.off_units_train(x, 3, fm.DROP_P)
    flat, _g = split_bwd(h, x, views, 3, fm.DROP_P, grads=grads)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat).all())


# ---- 6. the module ----

@pytest.mark.parametrize("backbone", ["fp32", "autocast_bf16", "channels_last"])
def test_module_split_wgrad(rt, backbone, monkeypatch):
    """OFFUnits(wgrad_arith="f32split") behind an fp32, an autocast-bf16 and a channels_last backbone, with an eval forward between the
    forward and its backward: every parameter .grad against the oracle's autograd (the device's ReLU decisions on both sides) within the
    default path's RTOL."""
    from offk_amd.off_module import OFFUnits
    B, L = 2, 3
    P = B * (L - 1)
    lib = _lib.load()
    calls = []
    for name in ("offk_off_units_backward", "offk_off_units_backward_typed", "offk_off_units_backward_cl", "offk_off_units_backward_split"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append(name), real(*a))[1])(real, name))
    wnp = synth.make_weights(spec.VARIANT_RGB)
    u = OFFUnits(B, L, "rgb", wgrad_arith="f32split").cuda()
    u.load_state_dict({k: torch.from_numpy(a) for k, a in wnp.items() if k in u.state_dict()}, strict=True)
    u.train()
    w = orc.to_torch_weights(wnp)
    feats = [ug.dev(f) for f in synth.make_features(B, L, 2)]
    if backbone == "autocast_bf16":
        feats = [f.bfloat16() for f in feats]
    elif backbone == "channels_last":
        feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    fmt = torch.channels_last if backbone == "channels_last" else torch.contiguous_format
    other = [(0.5 * f.float().flip(0)).to(f.dtype).contiguous(memory_format=fmt) for f in feats]      # a second set of maps for the interleaved forward
    outs = u(feats, drop_seed=fm.DROP_SEED)
    node = fm._units_node(outs[0])
    assert [f.dtype for f in node.feats] == [f.dtype for f in feats]
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(node.feats, feats))          # kept as they came: no cast, no copy
    tf = [f.float().cpu().contiguous() for f in feats]
    masks = fm.device_relu_masks(u._rt, tf, w, B, L)
    ref, dm = orc.unit_backward(tf, w, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, fm.cotangents(P), fm.unit_drop(fm.DROP_SEED, P), masks)
    cots = [torch.cat([dm[i] for i in grp], dim=1).cuda() for grp in ((0, 1), (2, 3, 4, 5, 6), (7, 8))]
    u.eval()                                             # the interleaved forward: the backward finds a foreign generation and recomputes
    with torch.no_grad():
        u(other)
    u.train()
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    assert calls == ["offk_off_units_backward_split"]
    got = {k: p.grad for k, p in u.named_parameters() if p.grad is not None}
    assert set(got) == set(ref) and len(got) == 54
    errs = dict((k, fm.rel_err(got[k], ref[k])) for k in ref)
    bad = dict((k, "%.2e" % e) for k, e in errs.items() if not e < RTOL or got[k].shape != ref[k].shape)
    print("module (%s): largest error against the oracle %.2e of the tensor's max (limit %.0e)" % (backbone, max(errs.values()), RTOL))
    assert not bad, bad
    # the default module makes the default call
    del calls[:]
    u0 = OFFUnits(B, L, "rgb").cuda()
    u0.load_state_dict({k: torch.from_numpy(a) for k, a in wnp.items() if k in u0.state_dict()}, strict=True)
    u0.train()
    torch.autograd.backward(u0(feats, drop_seed=fm.DROP_SEED), cots)
    want = {"fp32": "offk_off_units_backward", "autocast_bf16": "offk_off_units_backward_typed", "channels_last": "offk_off_units_backward_cl"}[backbone]
    assert calls == [want]
    g0 = {k: p.grad for k, p in u0.named_parameters() if p.grad is not None}
    assert all(torch.equal(g0[k], got[k]) for k in got if not is_matrix(k))
