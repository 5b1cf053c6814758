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
import ctypes
import functools

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth
from oracle import off_oracle as orc

from . import arena as arena_mod
from . import exact
from . import test_gpu_exact as gx
from . import test_gpu_feat_grad as fg

pytestmark = pytest.mark.gpu
EPS = synth.SPLIT_EPS
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP),
          (2, 3, spec.VARIANT_FLOW, spec.SLICE_FLAT)]
IDS = ["b1l2_flat", "b2l3_flat", "b3l4_clip", "b2l3_flat_flow"]
DTYPES = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def split(h, **kw):
    return h.off_units_backward_feats(arith="f32split", **kw)


def rows_of(t):
    """[N, C, H, H] result of either layout -> [N*HW, C] (a view where the layout allows, values unchanged)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def bits16(t):
    return t.contiguous().view(torch.int16)


def same_bits_any(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return arena_mod.same_bits(a, b) if a.dtype == torch.float32 else torch.equal(bits16(a), bits16(b))


def operands(h, B, L, slice_mode, si, wg, wd, rows=None):
    """The kernel's own operands of site si on the host: a [M, 160] (the dD part at row r(n), zeros outside the slice) and w [C, 160],
    fp32 numpy; rows: an index tensor of rows of a to take (full-size case)."""
    site, C, H = spec.SITES[si]
    HW, N = H * H, B * L
    r_of = torch.tensor(fg.down_rows(B, L, slice_mode), device="cuda")
    idx = torch.arange(N * HW, device="cuda") if rows is None else rows
    f, px = idx // HW, idx % HW
    r = r_of[f]
    a = torch.zeros(idx.numel(), 160, device="cuda")
    a[:, :128] = h.region("dG_" + site, 128)[idx]
    ins = r >= 0
    a[ins, 128:] = h.region("dD_" + site, 32)[(r * HW + px)[ins]]
    w = torch.cat((torch.as_tensor(wg).reshape(128, C), torch.as_tensor(wd).reshape(32, C))).t().contiguous()
    return a.cpu().numpy(), w.cpu().numpy()


def check_inequality(tag, got, a, w, got32=None):
    """Asserts test 6's inequality for got [M, C] (fp32 tensor or array) on the operands (a, w); prints the emulated and the measured
    accumulation constants and the errors against fp64 (beside them the fp32 entry's, when given).  Returns (c_acc emulated, gpu)."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    ref, dropped, mag = synth.split_terms(w, a)
    assert got.shape == ref.shape
    c_emu = float(synth.split_c_acc(synth.emulate_split_dot(w, a, form="units"), ref, dropped, mag).max())
    A = max(1.0, 2.0 * c_emu)
    unit = np.maximum(EPS * mag, 1e-300)
    err = np.abs(got - ref)
    c_gpu = float((np.abs(got - (ref - dropped)) / unit).max())
    line = "%s: c_acc emulated %.3f -> A %.3f | gpu accumulation %.3f | dropped (exact) max %.3f | err max %.3e rms %.3e" % (
        tag, c_emu, A, c_gpu, float((np.abs(dropped) / unit).max()), float(err.max()), float(np.sqrt((err ** 2).mean())))
    if got32 is not None:
        e32 = np.abs(np.asarray(got32.detach().cpu(), dtype=np.float64) - ref)
        line += " | fp32 entry: err max %.3e rms %.3e" % (float(e32.max()), float(np.sqrt((e32 ** 2).mean())))
    print(line)
    zero = mag == 0
    assert not got[zero].any(), "%s: %d elements with sum|a w| = 0 are not exactly 0" % (tag, int((got[zero] != 0).sum()))
    over = err - (np.abs(dropped) + A * EPS * mag + EPS * np.abs(ref))
    assert float(over.max()) <= 0.0, "%s: element %d misses the limit by %.3e (err %.3e)" % (tag, int(over.argmax()), float(over.max()),
                                                                                            float(err.reshape(-1)[over.argmax()]))
    return c_emu, c_gpu


# ---- 5. exact integers ----

@functools.lru_cache(maxsize=None)
def exact_case(B, L, variant, slice_mode):
    return gx.Case(B, L, variant, slice_mode)           # (its constructor asserts exact.check_caps on every output, dX among them)


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
    feats = [fg.dev(f) for f in synth.make_features(B, L, 2)]
    h.off_units(feats)
    h.off_units_backward(feats, fg.random_views(P)[1])                # sets the backward-has-run flag; its dG / dD are replaced below
    for si, (name, _C, H) in enumerate(spec.SITES):
        h.region("dG_" + name, 128).copy_(fg.dev(synth.make_adversarial((N * H * H, 128), pattern, "same", seed=400 + si, relu=relu)))
        h.region("dD_" + name, 32).copy_(fg.dev(synth.make_adversarial((P * H * H, 32), pattern, "same", seed=500 + si)))
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
    c = fg.case(rt, B, L, variant, slice_mode, 7)
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
    B, L = 2, 3
    c = fg.case(rt, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    c.run()
    first = split(c.h, layout="nchw")
    cl = split(c.h, layout="cl")
    again = split(c.h, layout="nchw")
    some = split(c.h, sites=[1, 5, 7], layout="nchw")
    fp32 = c.h.off_units_backward_feats(layout="nchw")
    torch.cuda.synchronize()
    for i, (a, b, d) in enumerate(zip(first, cl, again)):
        assert float(a.abs().max()) > 0 and bool(torch.isfinite(a).all())
        assert not b.is_contiguous() and arena_mod.same_bits(a, b.contiguous()) and arena_mod.same_bits(a, d)
        assert (some[i] is not None) == (i in (1, 5, 7)) and (some[i] is None or arena_mod.same_bits(a, some[i]))
    assert any(not arena_mod.same_bits(a, b) for a, b in zip(first, fp32))          # its own bits, not the fp32 entry's
    gen = torch.Generator(device="cuda").manual_seed(17)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        for layout in ("nchw", "cl"):
            fmt = torch.contiguous_format if layout == "nchw" else torch.channels_last
            res = split(c.h, layout=layout, dtype=dt)
            old = [torch.randn(t.shape, device="cuda", generator=gen).to(dt).contiguous(memory_format=fmt) for t in first]
            acc = [t.clone(memory_format=torch.preserve_format) for t in old]
            split(c.h, layout=layout, dtype=dt, out=acc, accumulate=True)
            torch.cuda.synchronize()
            for a, r, o, e in zip(first, res, old, acc):
                want, want_acc = a.to(dt), (o.float() + a).to(dt)
                # every element takes part: nothing non-finite on either side (the sign of a zero is compared as it is)
                assert bool(torch.isfinite(want.float()).all()) and bool(torch.isfinite(want_acc.float()).all())
                assert r.dtype == dt and same_bits_any(r.contiguous(), want), (dt, layout)
                assert same_bits_any(e.contiguous(), want_acc.contiguous()), (dt, layout, "accumulate")

    # backward + the split call in one graph, one replay
    grads = c.h.new_unit_grads()
    outs = [torch.empty_like(t) for t in first]

    def launch():
        c.backward(grads=grads)
        split(c.h, layout="nchw", out=outs)

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
    B, L = 2, 3
    c = fg.Case(rt, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    dt = {"typed_bf16": torch.bfloat16, "cl_f32": torch.float32, "cl_f16": torch.float16}[kind]
    x = [f.to(dt) for f in c.feats]
    plain = [t.float() for t in x]
    other = [t.contiguous(memory_format=torch.channels_last) for t in x] if kind.startswith("cl") else x
    res = []
    for feats in (plain, other):
        c.forward(feats)
        c.backward(feats)
        res.append(split(c.h, layout="nchw"))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert float(a.abs().max()) > 0 and arena_mod.same_bits(a, b)


def test_bound_weights_are_read_at_launch_time(rt):
    """The pre-pass cuts the weights as they are when the call is enqueued: after an in-place update the result follows the new ones."""
    B, L = 1, 2
    c = fg.Case(rt, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
    bound = {}
    for k, v in c.wnp.items():
        if k.startswith(spec.UNIT_PARAM_PREFIXES):
            bound[k] = fg.dev(v)
            c.h.bind_weight(k, bound[k])
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
    c = fg.case(rt, B, L, spec.VARIANT_RGB, slice_mode, 7)
    c.run()
    shapes = spec.feature_shapes(B, L)
    esize = 4 if dt == torch.float32 else 2
    ar = arena_mod.Arena.for_sizes([esize * int(np.prod(s)) for s in shapes])
    skipped = (1, 6)

    def carve(i):
        n, ch, hh, _ = shapes[i]
        t = ar.empty("dx_%d" % i, (n, ch, hh, hh) if layout == "nchw" else (n, hh, hh, ch), dtype=dt)
        return t if layout == "nchw" else t.permute(0, 3, 1, 2)

    bufs = [carve(i) for i in range(9)]           # full of the sentinel
    want = split(c.h, layout=layout, dtype=dt)
    got = split(c.h, sites=[i for i in range(9) if i not in skipped], layout=layout, dtype=dt,
                out=[None if i in skipped else b for i, b in enumerate(bufs)])
    torch.cuda.synchronize()
    ar.check()
    for i in range(9):
        if i in skipped:
            assert got[i] is None and ar.untouched(bufs[i] if layout == "nchw" else bufs[i].permute(0, 2, 3, 1))
        else:
            assert bool(torch.isfinite(got[i].float()).all()) and same_bits_any(got[i].contiguous(), want[i].contiguous())


def test_refusals_leave_the_outputs_untouched(rt):
    B, L = 1, 2
    shapes = spec.feature_shapes(B, L)
    outs = [torch.full(tuple(s), float("nan"), device="cuda") for s in shapes]
    keep = [arena_mod.bits(t).clone() for t in outs]
    arr = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    F32 = DTYPES[torch.float32]

    def refused(h, ws, dtype, a, layout, needle):
        hh = h._h if h is not None else None
        rc = lib.offk_off_units_backward_feats_split(hh, stream, ws, dtype, a, layout, 0)
        assert rc == -1 and needle in lib.offk_last_error(hh), lib.offk_last_error(hh)
        assert b"offk_off_units_backward_feats_split" in lib.offk_last_error(hh)

    plain = rt.OffForward(B, L, spec.VARIANT_RGB)
    with pytest.raises(_lib.OffkError, match="create the handle with training=True for the units' backward"):
        split(plain, out=outs)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    ws = ctypes.c_void_p(h.workspace.data_ptr())
    refused(h, ws, F32, arr, _lib.FEAT_NCHW, b"no offk_off_units_backward has run")
    feats = [fg.dev(f) for f in synth.make_features(B, L, 3)]
    h.off_units(feats)
    h.off_units_backward(feats, fg.random_views(B * (L - 1))[1])
    refused(None, ws, F32, arr, _lib.FEAT_NCHW, b"null argument")
    refused(h, None, F32, arr, _lib.FEAT_NCHW, b"null argument")
    refused(h, ws, F32, None, _lib.FEAT_NCHW, b"null argument")
    refused(h, ws, F32, arr, 2, b"layout must be")
    refused(h, ws, F32, arr, -1, b"layout must be")
    refused(h, ws, 3, arr, _lib.FEAT_NCHW, b"grad_dtype must be")
    refused(h, ws, -1, arr, _lib.FEAT_NHWC, b"grad_dtype must be")
    mis = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    mis[4] = outs[4].data_ptr() + 4
    refused(h, ws, F32, mis, _lib.FEAT_NHWC, b"16-byte aligned")
    mis[4] = outs[4].data_ptr() + 8
    refused(h, ws, DTYPES[torch.bfloat16], mis, _lib.FEAT_NHWC, b"16-byte aligned")
    over = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    over[8] = h.workspace.data_ptr() + 256
    refused(h, ws, F32, over, _lib.FEAT_NCHW, b"overlaps the workspace")
    # a 16-bit buffer that ends exactly where the workspace begins is half as long as an fp32 one: real element sizes
    n8 = int(np.prod(shapes[8]))
    over[8] = h.workspace.data_ptr() - 2 * n8
    if over[8] % 16 == 0:
        refused(h, ws, F32, over, _lib.FEAT_NCHW, b"overlaps the workspace")
    with pytest.raises(ValueError, match="arith"):
        h.off_units_backward_feats(out=outs, arith="bf16")
    with pytest.raises(ValueError, match="layout"):
        split(h, layout="nhwc", out=outs)
    # all nine NULL: OFFK_OK, nothing enqueued
    assert lib.offk_off_units_backward_feats_split(h._h, stream, ws, F32, (ctypes.c_void_p * 9)(), _lib.FEAT_NCHW, 0) == 0
    assert split(h, sites=[]) == [None] * 9
    torch.cuda.synchronize()
    assert all(torch.equal(arena_mod.bits(t), k) for t, k in zip(outs, keep))


def test_trace_names(rt):
    c = fg.case(rt, 1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT, 7)
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

def make_units(B, L, arith=None):
    from offk_amd.off_module import OFFUnits
    wnp = synth.make_weights(spec.VARIANT_RGB)
    u = (OFFUnits(B, L, "rgb", feat_grad=True) if arith is None else OFFUnits(B, L, "rgb", feat_grad=True, feat_grad_arith=arith)).cuda()
    u.load_state_dict({k: torch.from_numpy(a) for k, a in wnp.items() if k in u.state_dict()}, strict=True)
    u.train()
    return u, wnp


def test_module_split_feat_grad(rt, monkeypatch):
    B, L = 2, 3
    P = B * (L - 1)
    lib = _lib.load()
    calls = []
    for name in ("offk_off_units_backward_feats", "offk_off_units_backward_feats_typed", "offk_off_units_backward_feats_split"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append(name), real(*a))[1])(real, name))
    u, wnp = make_units(B, L, "f32split")
    w = orc.to_torch_weights(wnp)
    feats_np = synth.make_features(B, L, 2)
    feats = [fg.dev(f).requires_grad_(True) for f in feats_np]
    cots = fg.module_cots(P)
    torch.autograd.backward(u(feats, drop_seed=7), cots)
    torch.cuda.synchronize()
    assert calls == ["offk_off_units_backward_feats_split"]
    tf = [torch.from_numpy(f) for f in feats_np]
    masks = fg.device_relu_masks(u._rt, tf, w, B, L)
    drops = fg.unit_drop(7, P)
    dms = [cots[0][:, :160], cots[0][:, 160:]] + [cots[1][:, 160 * k:160 * k + 160] for k in range(5)] + [cots[2][:, :160], cots[2][:, 160:]]
    for si, ((site, _c, _h), x) in enumerate(zip(spec.SITES, tf)):
        x = x.clone().requires_grad_(True)
        orc.off_unit(x, w, site, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, drops[si], masks[si]).backward(dms[si].cpu())
        assert feats[si].grad is not None and feats[si].grad.shape == x.grad.shape
        assert fg.rel_err(feats[si].grad, x.grad) < fg.RTOL, site
    pgrads = {k: p.grad.clone() for k, p in u.named_parameters() if p.grad is not None}
    split32 = [f.grad.clone() for f in feats]

    # the default module: the fp32 entry as before, the same parameter gradients bit for bit
    del calls[:]
    u0, _w = make_units(B, L)
    assert u0.feat_grad_arith == "fp32"
    f0 = [fg.dev(f).requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u0(f0, drop_seed=7), cots)
    assert calls == ["offk_off_units_backward_feats"]
    p0 = {k: p.grad for k, p in u0.named_parameters() if p.grad is not None}
    assert p0.keys() == pgrads.keys() and len(p0) == 54 and all(torch.equal(p0[k], pgrads[k]) for k in p0)
    assert all(fg.rel_err(a, b.grad) < fg.RTOL for a, b in zip(split32, f0))

    # bf16 maps: bf16 gradients, the split fp32 result of the same (bf16-valued) maps rounded once
    del calls[:]
    fb = [fg.dev(f).bfloat16().requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u(fb, drop_seed=7), cots)
    ff = [f.detach().float().requires_grad_(True) for f in fb]
    torch.autograd.backward(u(ff, drop_seed=7), cots)
    assert calls == ["offk_off_units_backward_feats_split"] * 2
    for a, b in zip(fb, ff):
        assert a.grad.dtype == torch.bfloat16 and torch.equal(a.grad, b.grad.bfloat16())
    # channels_last maps: channels_last gradients, the same bits
    fc = [fg.dev(f).contiguous(memory_format=torch.channels_last).requires_grad_(True) for f in feats_np]
    torch.autograd.backward(u(fc, drop_seed=7), cots)
    for f, want in zip(fc, split32):
        assert f.grad.is_contiguous(memory_format=torch.channels_last) and not f.grad.is_contiguous()
        assert torch.equal(f.grad, want)


# ---- 11. full size ----

def test_full_size(rt):
    """B = 64, L = 7: 4096 sampled rows per site (the first and the last among them) under test 6's inequality, both the fp32 NHWC
    and the bf16 NCHW form of the launch (9262 blocks); zero dM gives exactly zero."""
    B, L = 64, 7
    N, P = B * L, B * (L - 1)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, training=True)
    wnp = synth.make_weights(spec.VARIANT_RGB)
    assert h.load_state_dict(wnp) == []
    feats = [fg.dev(f) for f in synth.make_features(B, L, 2)]
    h.off_units_train(feats, 21, fg.DROP_P)
    _bufs, views = fg.random_views(P)
    h.off_units_backward(feats, views, 21, fg.DROP_P)
    dx = split(h, layout="cl")
    dxb = split(h, layout="nchw", dtype=torch.bfloat16)
    gen = torch.Generator(device="cuda").manual_seed(9)
    for si, (site, C, H) in enumerate(spec.SITES):
        HW = H * H
        idx = torch.randint(0, N * HW, (4096,), device="cuda", generator=gen)
        idx[:2] = torch.tensor([0, N * HW - 1], device="cuda")
        a, wk = operands(h, B, L, spec.SLICE_FLAT, si, wnp["motion_conv_gen_%s.weight" % site], wnp["motion_spatial_down_%s.weight" % site], rows=idx)
        got = rows_of(dx[si])[idx]
        check_inequality("full size site %s" % site, got, a, wk)
        assert float(got.abs().max()) > 0
        assert torch.equal(rows_of(dxb[si])[idx], got.bfloat16())
    h.off_units_backward(feats, [(torch.zeros_like(t), c) for t, c in views], 21, fg.DROP_P)
    d0 = split(h, layout="cl")
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in d0)
