"""The units' train forward with the stacked 1x1 reduces K1 in split-fp32 arithmetic on the bf16 matrix pipe (offk_off_units_train_split,
csrc/units_fwd_split.hip; OffForward.off_units / off_units_train(arith="f32split"), OFFUnits(fwd_arith="f32split")):

    G[N HW][128] = relu(Wg X + bg) on all frames,   D[P HW][32] = Wd X + bd on the frames of the spatial slice

 1. exact integer inputs (tests/exact.py): G_, D_ and the unit channels of fusion_28 / 14 / 7 equal the fp64 reference value for value in
    all six map forms (NCHW / channels-last x fp32 / bf16 / fp16), at p = 0 and at the exact-case dropout p = 0.5, the regions poisoned
    with NaN first -- what catches a skipped k step or a wrong tile edge;
 2. equal bits with the fused split kernel: D_<site> and the temporal channels of every unit, on a split-fp32 handle with set weights;
 3. worst-case mantissas (synth.make_adversarial) in maps and weights, zero biases: per element of G (against max(ref64, 0)) and D
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|w x| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation error on the same operands (tests/units_fwd_split.py) -- never the kernel's output.
    tests/test_units_fwd_split_abi.py shows on the CPU that losing any one issued product breaks it;
 4. the same inequality on synthetic maps with real biases (magnitude sum|w x| + |b|), the default entry's error printed beside;
 5. equal bits: NCHW == channels-last per dtype, 16-bit maps == x.float(), run to run, graph replay, bound == set weights, an in-place
    weight update is picked up;  6. the backward entries behind it consume the workspace and nothing else;
 7. guard bands round the workspace, the maps and behind the G_ / D_ regions; refusals leave workspace and trace untouched;  8. the module.

Shapes (B, L): those of tests/test_gpu_wgrad_split.py -- (1, 2) flat: the 7x7 sites are one partial 98-row tile; (2, 3) flat: quirk Q1, 784- and
196-row frames straddle the 128-row tiles; (3, 4) per-clip; (2, 3) flat, Flow; (8, 7) per-clip.  All nine sites always: C = 320 and 608 give 10
and 19 k steps, 49-pixel rows, 1024 channels."""
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
from .units_fwd_split import DOWN_B, DOWN_W, GEN_B, GEN_W, check_site
from .units_grad import DTS, FORMS, IDS, RTOL, SHAPES, as_form, exact_case, rt  # noqa: F401

pytestmark = pytest.mark.gpu
SPLIT = {"arith": "f32split"}


# ---- 1. exact integers ----

@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_exact_integers(rt, B, L, variant, slice_mode):
    c = exact_case(B, L, variant, slice_mode)
    assert c.worst < 1.0
    h = c.handle(rt)
    for layout, dt in FORMS:
        maps = as_form(c.feats, layout, dt)
        assert all(torch.equal(m.float(), x) for m, x in zip(maps, c.feats))         # small integers: exact in both 16-bit types
        gx.poison(h, gx.all_regions(c))
        h.off_units(maps, **SPLIT)
        gx.check_forward(h, c, "split off_units (%s, %s)" % (layout, dt))
        gx.poison(h, gx.all_regions(c))
        h.off_units_train(maps, gx.DROP_SEED, exact.DROP_P, **SPLIT)
        gx.check_forward(h, c, "split off_units_train (%s, %s)" % (layout, dt), key="M_train")


# ---- 2. equal bits with the fused split kernel ----

def some_negative(B, L, seed, dtype=torch.float32):
    return [(x - 0.25 * (x > 1.0)).to(dtype) for x in fm.relu_maps(B, L, torch.float32, seed)]


@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_equal_bits_with_the_fused_split_kernel(rt, B, L, variant, slice_mode):
    h = fm.make_train_handle(rt, B, L, variant, slice_mode, precision="f32split")
    x = some_negative(B, L, 11)
    h.workspace.fill_(0xff)
    h.off_units(x, **SPLIT)
    mine = fm.unit_regions(h)
    h.workspace.fill_(0xff)
    h.off_units_fused(x)
    fused = fm.unit_regions(h)
    torch.cuda.synchronize()
    for i in range(0, len(mine), 2):
        assert bool(torch.isfinite(mine[i]).all()) and float(mine[i][..., 32:].abs().max()) > 0
        assert torch.equal(mine[i][..., 32:], fused[i][..., 32:]), "temporal channels of unit %d" % (i // 2)
        assert torch.equal(mine[i + 1], fused[i + 1]), "D of unit %d" % (i // 2)


# ---- 3. / 4. the inequality ----

ADV = [(p, s) for p in (0x00FFFF, 0x7FFFFF, 0x7F7F7F) for s in ("same", "alternating")]
WORST = [(1, 2) + ps for ps in ADV] + [(2, 3, 0x00FFFF, "same"), (2, 3, 0x7F7F7F, "alternating")]


@pytest.mark.parametrize("B,L,pattern,signs", WORST, ids=["b%dl%d_0x%06X_%s" % w for w in WORST])
def test_worst_case_mantissas(rt, B, L, pattern, signs):
    """Emulated c_acc, A and the measured GPU accumulation constant (maximum over the nine sites), first MI355X run (also DESIGN.md 8; at
    2 x 3 the emulation runs on a sample of 128 rows per site, the GPU figure is over all of them):

        shape  pattern   signs        c_acc (emulation)   A        gpu accumulation max
        1 x 2  0x00FFFF  same         1.265               2.530    1.265
        1 x 2  0x00FFFF  alternating  0.467               1.000    0.430
        1 x 2  0x7FFFFF  same         13.867              27.733   13.867
        1 x 2  0x7FFFFF  alternating  3.300               6.601    3.206
        1 x 2  0x7F7F7F  same         13.241              26.483   13.241
        1 x 2  0x7F7F7F  alternating  2.331               4.661    2.669
        2 x 3  0x00FFFF  same         1.316               2.631    1.265
        2 x 3  0x7F7F7F  alternating  2.090               4.180    2.688
    """
    slice_mode = spec.SLICE_FLAT
    N = B * L
    w = synth.make_weights(spec.VARIANT_RGB)
    w160 = []
    for si, (name, C, _H) in enumerate(spec.SITES):
        wa = synth.make_adversarial((160, C), pattern, "same", seed=700 + si)
        w[GEN_W % name] = wa[:128].reshape(128, C, 1, 1).copy()
        w[DOWN_W % name] = wa[128:].reshape(32, C, 1, 1).copy()
        w[GEN_B % name] = np.zeros(128, dtype=np.float32)
        w[DOWN_B % name] = np.zeros(32, dtype=np.float32)
        w160.append(wa)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(w) == []
    maps = [ug.dev(synth.make_adversarial((N, C, H, H), pattern, signs, seed=600 + si, k_axis=1, relu=(pattern == 0x7FFFFF)))
            for si, (_n, C, H) in enumerate(spec.SITES)]
    h.workspace.fill_(0xff)
    h.off_units(maps, **SPLIT)
    torch.cuda.synchronize()
    worst = [0.0, 0.0]
    for si, (name, _C, _H) in enumerate(spec.SITES):
        ce, cg = check_site("worst case b%dl%d 0x%06X %-11s site %s" % (B, L, pattern, signs, name), h, B, L, slice_mode, si, maps[si], w160[si], None,
                            max_rows=None if N == 2 else 128)
        worst = [max(worst[0], ce), max(worst[1], cg)]
    print("worst case b%dl%d 0x%06X %-11s: emulated c_acc %.3f, A %.3f, gpu accumulation max %.3f" % (
        B, L, pattern, signs, worst[0], max(1.0, 2 * worst[0]), worst[1]))


@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES[:4], ids=IDS[:4])
def test_random_inputs_within_the_bound(rt, B, L, variant, slice_mode):
    wnp = synth.make_weights(variant)
    h = rt.OffForward(B, L, variant, slice_mode, training=True)
    assert h.load_state_dict(wnp) == []
    maps = [ug.dev(f) for f in synth.make_features(B, L, 2 if B == 2 else 3)]
    h.off_units(maps)
    default = [(h.region("G_" + n, 128).cpu().numpy().astype(np.float64), h.region("D_" + n, 32).cpu().numpy().astype(np.float64)) for n, _c, _h in spec.SITES]
    h.workspace.fill_(0xff)
    h.off_units(maps, **SPLIT)
    torch.cuda.synchronize()
    for si, (name, C, _H) in enumerate(spec.SITES):
        w160 = np.concatenate((wnp[GEN_W % name].reshape(128, C), wnp[DOWN_W % name].reshape(32, C)))
        bias = np.concatenate((wnp[GEN_B % name], wnp[DOWN_B % name]))
        assert float(np.abs(bias).max()) > 0
        check_site("random %s site %s" % (IDS[SHAPES.index((B, L, variant, slice_mode))], name), h, B, L, slice_mode, si, maps[si], w160, bias,
                   max_rows=None if B * L == 2 else 96, default=default[si])


# ---- 5. equal bits ----

def run_split(h, x, train=True):
    h.workspace.fill_(0xff)                            # (NaN in every float: what the units leave unwritten shows)
    if train:
        h.off_units_train(x, fm.DROP_SEED, fm.DROP_P, **SPLIT)
    else:
        h.off_units(x, **SPLIT)
    return fm.written(h)


def assert_same(a, b, what, values_only=False):
    for (na, ta), (_nb, tb) in zip(a, b):
        if values_only:                                # a zero's sign aside
            assert torch.equal(ta, tb), "%s: %s" % (what, na)
        else:
            assert arena_mod.same_bits(ta, tb), "%s: %s" % (what, na)


def test_equal_bits_properties(rt):
    B, L = 2, 3
    h = fm.make_train_handle(rt, B, L)
    x32 = some_negative(B, L, 11)
    base = None
    for dt in DTS:
        xd = as_form(x32, "nchw", dt)
        first = run_split(h, xd)
        assert all(bool(torch.isfinite(t).all()) for _n, t in first) and all(float(t.abs().max()) > 0 for _n, t in first)
        assert_same(first, run_split(h, as_form(x32, "cl", dt)), "NCHW == channels-last (%s)" % dt)
        assert_same(first, run_split(h, xd), "run to run (%s)" % dt)
        assert_same(first, run_split(h, [x.float() for x in xd]), "16-bit maps == x.float() (%s)" % dt, values_only=True)
        default = fm.run_units(h, xd, True)
        assert any(not arena_mod.same_bits(a[1], b[1]) for a, b in zip(first, default)), dt        # bits of its own
        if dt == "f32":
            base = (xd, first)

    # capture and replay of the three launches
    xd, first = base

    def launch():
        h.off_units_train(xd, fm.DROP_SEED, fm.DROP_P, **SPLIT)

    g = ug.captured(launch)
    for _ in range(2):
        h.workspace.fill_(0xff)
        g.replay()
        torch.cuda.synchronize()
        assert_same(first, fm.written(h), "graph replay")


def test_bound_weights_and_in_place_updates(rt):
    """Bound == set weights on either precision; an in-place update of a bound weight between two calls is picked up with no library call."""
    B, L = 1, 2
    x = some_negative(B, L, 12)
    res, bound = [], None
    for prec, bind in (("fp32", False), ("f32split", True)):
        h = rt.OffForward(B, L, spec.VARIANT_RGB, precision=prec, training=True)
        wnp = synth.make_weights(spec.VARIANT_RGB)
        assert h.load_state_dict(wnp) == []
        keep = {}
        if bind:
            for k, v in wnp.items():
                if k.startswith(spec.UNIT_PARAM_PREFIXES):
                    keep[k] = ug.dev(v)
                    h.bind_weight(k, keep[k])
            bound = (h, keep, wnp)
        res.append(run_split(h, x))
    assert_same(res[0], res[1], "bound == set weights")
    h, keep, wnp = bound
    for name, _C, _H in spec.SITES:
        keep[GEN_W % name].mul_(0.5)                      # exact: every gen pre-activation's products halve
        keep[GEN_B % name].mul_(0.5)
    got = dict(run_split(h, x))
    for name, t in res[1]:
        if name.startswith("G_"):
            assert torch.equal(got[name], 0.5 * t), name
        elif name.startswith("D_"):
            assert arena_mod.same_bits(got[name], t), name


# ---- 6. the backward behind it ----

def test_the_backward_consumes_the_workspace_alone(rt):
    B, L = 2, 3
    P = B * (L - 1)
    h = fm.make_train_handle(rt, B, L)
    x = some_negative(B, L, 13)
    _bufs, views = ug.random_views(P)
    regions = [("G_" + n, 128) for n, _c, _h in spec.SITES] + [("D_" + n, 32) for n, _c, _h in spec.SITES]

    def backwards():
        out = []
        for ar in rt.WGRAD_ARITHS:
            out.append(h.off_units_backward(x, views, fm.DROP_SEED, fm.DROP_P, arith=ar)[0].clone())
            for fa in rt.FEAT_GRAD_ARITHS:
                out += [t.clone() for t in h.off_units_backward_feats(layout="nchw", arith=fa)]
        return out

    h.off_units_train(x, fm.DROP_SEED, fm.DROP_P, **SPLIT)
    saved = [h.region(*r).clone() for r in regions]
    behind_split = backwards()
    h.off_units_train(x, fm.DROP_SEED, fm.DROP_P)                      # the default route ...
    assert any(not arena_mod.same_bits(h.region(*r), s) for r, s in zip(regions, saved))
    for r, s in zip(regions, saved):
        h.region(*r).copy_(s)                                          # ... with the split forward's G_ / D_ written over its own
    behind_default = backwards()
    torch.cuda.synchronize()
    assert len(behind_split) == len(behind_default) == 2 * (1 + 2 * 9)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in behind_split)
    assert all(arena_mod.same_bits(a, b) for a, b in zip(behind_split, behind_default))


# ---- 7. memory discipline and refusals ----

@pytest.mark.parametrize("layout,dt", [("nchw", "f32"), ("nchw", "bf16"), ("cl", "f32"), ("cl", "f16")])
@pytest.mark.parametrize("B,L,slice_mode", [(1, 2, spec.SLICE_FLAT), (3, 4, spec.SLICE_PER_CLIP)])
def test_memory_discipline(rt, B, L, slice_mode, layout, dt):
    """Workspace and maps are carves of one sentinel-filled arena: nothing outside a carve changes, the regions K1 and K2 write equal the
    run in ordinary allocations, and inside the workspace every byte outside the G_ / D_ / fusion regions -- the bytes behind the last
    row of each G_ / D_ region among them -- still holds the sentinel."""
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    maps = as_form(some_negative(B, L, 14), layout, dt)
    want = run_split(h, maps)
    torch.cuda.synchronize()
    ar, ws = ug.workspace_arena(h, maps)
    gm = ug.guarded_maps(ar, maps, layout)
    h.off_units_train(gm, fm.DROP_SEED, fm.DROP_P, **SPLIT)
    torch.cuda.synchronize()
    ar.check()
    assert_same(want, fm.written(h), "arena run")
    names = ["G_" + n for n, _c, _h in spec.SITES] + ["D_" + n for n, _c, _h in spec.SITES] + ["fusion_28", "fusion_14", "fusion_7"]
    spans = sorted(ug.region_span(h, n) for n in names)
    for (off, nb), (site, _c, H) in zip([ug.region_span(h, "G_" + n) for n, _c, _h in spec.SITES], spec.SITES):
        assert nb == B * L * H * H * 128 * 4, site                     # a region ends with its last row
    cursor = 0
    for off, nb in spans + [(h.workspace_bytes, 0)]:
        if off > cursor:
            lo, hi = (cursor + 3) // 4 * 4, off // 4 * 4
            assert ar.untouched(ws[lo:hi]), "workspace bytes %d .. %d (between two written regions) were written" % (lo, hi)
        cursor = max(cursor, off + nb)


def test_refusals_leave_workspace_and_trace_untouched(rt):
    B, L = 1, 2
    lib = _lib.load()
    h = fm.make_train_handle(rt, B, L)
    x = some_negative(B, L, 15)
    x16 = [t.bfloat16() for t in x]
    h.set_profiling(2)
    h.off_units_train(x, 3, fm.DROP_P, **SPLIT)
    names = list(h.launch_times().keys())
    assert names == ["units:pw_reduce weight cut (K1, split)", "units:pw_reduce (K1, NCHW, split)", "units:sobel_tdiff (K2)"]
    h.off_units_train(as_form(x, "cl", "bf16"), 3, fm.DROP_P, **SPLIT)
    assert list(h.launch_times().keys())[1] == "units:pw_reduce (K1, NHWC, split, bf16)"
    h.off_units(as_form(x, "nchw", "f16"), **SPLIT)
    assert list(h.launch_times().keys())[1] == "units:pw_reduce (K1, NCHW, split, fp16)"
    h.workspace.fill_(0x5a)
    torch.cuda.synchronize()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws_p = ctypes.c_void_p(h.workspace.data_ptr())

    def arr_of(ts):
        return (ctypes.c_void_p * 9)(*[t.data_ptr() for t in ts])

    def refused(needle, hh=h, fdt=_lib.FEAT_F32, layout=_lib.FEAT_NCHW, arr=None, ws=ws_p, p=fm.DROP_P):
        handle = hh._h if hh is not None else None
        rc = lib.offk_off_units_train_split(handle, stream, fdt, layout, arr_of(x) if arr is None else arr, ws, ctypes.c_uint64(3), p)
        msg = lib.offk_last_error(handle)
        assert rc == -1 and needle in msg, msg

    refused(b"offk_off_units_train_split: null argument", hh=None)
    refused(b"offk_off_units_train_split: null argument", ws=None)
    refused(b"layout must be", layout=2)
    refused(b"layout must be", layout=-1)
    refused(b"unknown feat_dtype", fdt=3)
    refused(b"unknown feat_dtype", fdt=-1, layout=_lib.FEAT_NHWC)
    nhwc = fm.make_train_handle(rt, B, L, feat_layout=1)
    refused(b"NCHW", hh=nhwc, ws=ctypes.c_void_p(h.workspace.data_ptr()))                     # an NHWC handle, NCHW maps
    refused(b"NCHW", hh=nhwc, fdt=_lib.FEAT_BF16, arr=arr_of(x16))
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
    with pytest.raises(ValueError, match="arith must be one of"):
        h.off_units_train(x, 3, fm.DROP_P, arith="bf16")
    torch.cuda.synchronize()
    assert bool((h.workspace == 0x5a).all())           # nothing was enqueued
    assert list(h.launch_times().keys()) == []         # and nothing was marked
    # and none of this disturbed the handle: the next call runs
    got = run_split(h, x)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for _n, t in got)


# ---- 8. the module ----

@pytest.mark.parametrize("switches", ["fwd", "all"])
@pytest.mark.parametrize("backbone", ["fp32", "autocast_bf16", "channels_last"])
def test_module_split_forward(rt, backbone, switches, monkeypatch):
    """OFFUnits(fwd_arith="f32split"), alone and with the other two switches, behind an fp32, an autocast-bf16 and a channels_last backbone,
    with an eval forward between the forward and its backward: the three outputs and every parameter .grad against the oracle (the
    device's ReLU decisions on both sides) within the default path's RTOL; fwd_arith="fp32" makes the parent's calls and gives its bits."""
    from offk_amd.off_module import OFFUnits
    B, L = 2, 3
    P = B * (L - 1)
    lib = _lib.load()
    calls = []
    for name in ("offk_off_units_train", "offk_off_units_train_typed", "offk_off_units_train_cl", "offk_off_units", "offk_off_units_typed", "offk_off_units_cl",
                 "offk_off_units_train_split"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append(name), real(*a))[1])(real, name))
    wnp = synth.make_weights(spec.VARIANT_RGB)
    kw = {"fwd_arith": "f32split"} if switches == "fwd" else {"fwd_arith": "f32split", "wgrad_arith": "f32split", "feat_grad_arith": "f32split", "feat_grad": True}
    u = OFFUnits(B, L, "rgb", **kw).cuda()
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
    assert calls == ["offk_off_units_train_split"]
    tf = [f.float().cpu().contiguous() for f in feats]
    masks = fm.device_relu_masks(u._rt, tf, w, B, L)
    drops = fm.unit_drop(fm.DROP_SEED, P)
    # the outputs against the oracle's units (the same dropout mask)
    with torch.no_grad():
        ms = [orc.off_unit(tf[si], w, site, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, drop=drops[si]) for si, (site, _c, _h) in enumerate(spec.SITES)]
    want = [torch.cat([ms[i] for i in grp], dim=1) for grp in ((0, 1), (2, 3, 4, 5, 6), (7, 8))]
    for o, r in zip(outs, want):
        assert o.shape == r.shape and fm.rel_err(o, r) < RTOL
    ref, dm = orc.unit_backward(tf, w, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, fm.cotangents(P), drops, masks)
    cots = [torch.cat([dm[i] for i in grp], dim=1).cuda() for grp in ((0, 1), (2, 3, 4, 5, 6), (7, 8))]
    u.eval()                                             # the interleaved forward: the backward finds a foreign generation and recomputes
    with torch.no_grad():
        u(other)
    u.train()
    del calls[:]
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    assert calls == ["offk_off_units_train_split"]       # the recompute of the stale generation: the same arithmetic
    got = {k: p.grad for k, p in u.named_parameters() if p.grad is not None}
    assert set(got) == set(ref) and len(got) == 54
    errs = dict((k, fm.rel_err(got[k], ref[k])) for k in ref)
    bad = dict((k, "%.2e" % e) for k, e in errs.items() if not e < RTOL or got[k].shape != ref[k].shape)
    print("module (%s, %s): largest error against the oracle %.2e of the tensor's max (limit %.0e)" % (backbone, switches, max(errs.values()), RTOL))
    assert not bad, bad
    # the default module makes the default calls and gets the default entries' bits
    del calls[:]
    u0 = OFFUnits(B, L, "rgb").cuda()
    u0.load_state_dict({k: torch.from_numpy(a) for k, a in wnp.items() if k in u0.state_dict()}, strict=True)
    u0.train()
    outs0 = u0(feats, drop_seed=fm.DROP_SEED)
    entry = {"fp32": "offk_off_units_train", "autocast_bf16": "offk_off_units_train_typed", "channels_last": "offk_off_units_train_cl"}[backbone]
    assert calls == [entry]
    u0._rt.off_units_train(list(fm._units_node(outs0[0]).feats), fm.DROP_SEED, u0.drop_p)
    for o, (name, H, C, width) in zip(outs0, (("fusion_28", 28, 320, 320), ("fusion_14", 14, 1056, 800), ("fusion_7", 7, 832, 320))):
        again = u0._rt.region(name, C).view(P, H, H, C)[..., :width].permute(0, 3, 1, 2)
        assert torch.equal(o, again), name
