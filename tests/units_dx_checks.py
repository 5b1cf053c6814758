"""The GPU test bodies the three dX entries share, written once against a row of tests/units_grad.py's DX_FORMS (fp32 | typed | split) and
the runtime module.  The entries share one host body (offk_api.hip's off_units_backward_feats: dtype and `split` are its only arguments), so
tests/test_gpu_feat_grad.py, tests/test_gpu_feat_grad16.py and tests/test_gpu_feat_grad_split.py keep their test functions, parametrize lists
and what one entry alone has, and each shared test there binds its form and calls in here.  Where the three copies once differed in a check
the body makes it for every form; what cannot be stated for a form is a field of its row (DxForm.takes_dtype).  No tests of its own."""
import ctypes

import numpy as np
import pytest
import torch

from offk_amd import _lib, spec, synth

from . import arena as arena_mod
from . import units_grad as ug

LAYOUTS = ("nchw", "cl")
SOME = (1, 5, 7)                # a subset of sites
SKIPPED = (1, 6)                # the sites the arena test leaves out


def fmt_of(layout):
    return torch.contiguous_format if layout == "nchw" else torch.channels_last


def old_values(like, seed, scale):
    """Random tensors of the shapes, dtypes and layouts of `like`, `scale` times their magnitudes: what accumulate=True adds to."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [(scale * float(t.float().abs().max()) * torch.randn(t.shape, device="cuda", generator=gen)).to(t.dtype).contiguous(
        memory_format=torch.channels_last if not t.is_contiguous() else torch.contiguous_format) for t in like]


def accumulated(old, wide, dtype):
    """what accumulate=True leaves: (old.float() + dx32).to(dtype), dx32 the form's fp32 result (fp32: one IEEE add, old + dx32)"""
    return (old.float() + wide).to(dtype)


def equal_bits(form, c, dtypes=None):
    """On the case's handle, for each result dtype: NHWC == NCHW (values and bits), run to run, a subset of sites == all nine, the result ==
    the form's fp32 result .to(dtype), accumulate onto the result itself (fp32: == 2 * first) and onto random values, in both layouts; then
    backward + the dX call of the first dtype in both layouts captured in one graph and replayed once onto NaN-filled outputs."""
    dtypes = form.dtypes if dtypes is None else dtypes
    c.run()
    wide = form.call(c.h, layout="nchw")
    firsts = {}
    for dt in dtypes:
        first = form.call(c.h, layout="nchw", dtype=dt)
        cl = form.call(c.h, layout="cl", dtype=dt)
        again = form.call(c.h, layout="nchw", dtype=dt)
        some = form.call(c.h, sites=list(SOME), layout="nchw", dtype=dt)
        torch.cuda.synchronize()
        for i, (a, b, d, f) in enumerate(zip(first, cl, again, wide)):
            assert a.dtype == dt and float(a.float().abs().max()) > 0 and bool(torch.isfinite(a.float()).all())
            assert a.is_contiguous() and b.is_contiguous(memory_format=torch.channels_last) and not b.is_contiguous()
            assert torch.equal(a, b) and form.same(a, b.contiguous()), (dt, "NHWC == NCHW")
            assert form.same(a, d), (dt, "run to run")
            assert (some[i] is not None) == (i in SOME) and (some[i] is None or form.same(a, some[i])), (dt, "a subset of sites")
            assert ug.same_bits_any(a, f.to(dt)), (dt, "== the fp32 result .to(dtype)")
        for layout, res in (("nchw", first), ("cl", cl)):
            for onto, old in (("itself", res), ("random values", old_values(res, 17, 1.0))):
                acc = [t.clone(memory_format=torch.preserve_format) for t in old]
                back = form.call(c.h, layout=layout, dtype=dt, out=acc, accumulate=True)
                torch.cuda.synchronize()
                for a, o, e, f in zip(back, old, acc, wide):
                    want = accumulated(o.contiguous(), f, dt)
                    # every element takes part: nothing non-finite on either side (the sign of a zero is compared as it is)
                    assert a is e and bool(torch.isfinite(want.float()).all())
                    assert ug.same_bits_any(e.contiguous(), want), (dt, layout, "accumulate onto " + onto)
                    if dt == torch.float32 and onto == "itself":
                        assert arena_mod.same_bits(e.contiguous(), 2 * f), (layout, "accumulate == 2 * first")
        firsts[dt] = first

    dt = dtypes[0]
    first = firsts[dt]
    grads = c.h.new_unit_grads()
    outs = {layout: [torch.empty_like(t, memory_format=fmt_of(layout)) for t in first] for layout in LAYOUTS}

    def launch():
        c.backward(grads=grads)
        for layout in LAYOUTS:
            form.call(c.h, layout=layout, out=outs[layout], dtype=dt)

    g = ug.captured(launch)
    for layout in LAYOUTS:
        for t in outs[layout]:
            t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for layout in LAYOUTS:
        assert all(form.same(a, b.contiguous()) for a, b in zip(first, outs[layout])), ("graph replay", layout)
    return wide, firsts


def same_bits_after_the_other_backwards(form, c, kind, dtype):
    """offk_off_units_backward, _typed and _cl on the same logical maps leave the same dG / dD, so this entry's dX is the same bits behind each,
    in both layouts.  c: a Case of its own (its handle's workspace is overwritten); kind: typed_bf16 | cl_f32 | cl_f16, the maps' form."""
    dt = {"typed_bf16": torch.bfloat16, "cl_f32": torch.float32, "cl_f16": torch.float16}[kind]
    x = [f.to(dt) for f in c.feats]
    plain = [t.float() for t in x]
    other = ug.to_cl(x) if kind.startswith("cl") else x
    res = []
    for feats in (plain, other):
        c.forward(feats)
        c.backward(feats)
        res.append([form.call(c.h, layout=layout, dtype=dtype) for layout in LAYOUTS])
    torch.cuda.synchronize()
    for lay in range(2):
        for a, b in zip(res[0][lay], res[1][lay]):
            assert float(a.float().abs().max()) > 0 and form.same(a.contiguous(), b.contiguous())


def memory_discipline(form, c, layout, dtype, accumulate):
    """Every output is a carve of exactly its elements (the form's real element size) inside one arena of sentinel (a NaN as fp32, and each
    16-bit half of the word a NaN of both 16-bit types): the bands on both sides of all nine and the carves of the skipped sites keep every
    word; the written sites hold what the call gives in ordinary allocations, or (accumulate) the old values plus the form's fp32 result."""
    c.run()
    shapes = spec.feature_shapes(c.B, c.L)
    esize = torch.empty((), dtype=dtype).element_size()
    ar = arena_mod.Arena.for_sizes([esize * int(np.prod(s)) for s in shapes])
    want = form.call(c.h, layout=layout, dtype=dtype)
    wide = form.call(c.h, layout=layout)
    old = old_values(want, 5, 1.0)

    def carve(i):
        n, ch, hh, _ = shapes[i]
        if accumulate and i not in SKIPPED:
            t = ar.put("dx_%d" % i, old[i] if layout == "nchw" else old[i].permute(0, 2, 3, 1))
        else:
            t = ar.empty("dx_%d" % i, (n, ch, hh, hh) if layout == "nchw" else (n, hh, hh, ch), dtype=dtype)
        assert t.data_ptr() % 16 == 0 and t.element_size() == esize
        return t if layout == "nchw" else t.permute(0, 3, 1, 2)

    bufs = [carve(i) for i in range(9)]           # full of the sentinel, or of the old values
    got = form.call(c.h, sites=[i for i in range(9) if i not in SKIPPED], layout=layout, dtype=dtype, accumulate=accumulate,
                    out=[None if i in SKIPPED else b for i, b in enumerate(bufs)])
    torch.cuda.synchronize()
    ar.check()
    for i in range(9):
        if i in SKIPPED:
            assert got[i] is None and ar.untouched(bufs[i] if layout == "nchw" else bufs[i].permute(0, 2, 3, 1))
        else:
            expect = accumulated(old[i], wide[i], dtype) if accumulate else want[i]
            assert bool(torch.isfinite(got[i].float()).all())
            assert torch.equal(got[i], expect) and form.same(got[i].contiguous(), expect.contiguous()), spec.SITES[i][0]


def refusals(rt, form, dtype):
    """Everything the entry refuses, on a (1, 2) handle, with the outputs (full of NaN) left as they were: every C refusal carries the needle
    and begins with the name of the entry that answers.  Returns (handle, lib, stream, workspace pointer) for what a file adds."""
    B, L = 1, 2
    shapes = spec.feature_shapes(B, L)
    outs = [torch.full(tuple(s), float("nan"), device="cuda", dtype=dtype) for s in shapes]
    esize = outs[0].element_size()
    keep = [t.contiguous().view(torch.uint8).clone() for t in outs]
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = ug.FEAT[dtype]

    def ptrs():
        return (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])

    def refused(h, ws, a, layout, needle, code=code):
        hh = h._h if h is not None else None
        rc = form.raw(lib, hh, stream, ws, code, a, layout)
        msg = lib.offk_last_error(hh)
        named = form.named_in(code) if code in ug.FEAT.values() else form.entry
        assert rc == -1 and needle in msg and named.encode() + b": " in msg, msg

    arr = ptrs()
    # a handle without the training workspace: the wrapper's refusal, in the words off_units_backward uses
    plain = rt.OffForward(B, L, spec.VARIANT_RGB)
    with pytest.raises(_lib.OffkError, match="create the handle with training=True for the units' backward"):
        form.call(plain, out=outs, dtype=dtype)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    ws = ctypes.c_void_p(h.workspace.data_ptr())
    # a fresh handle: no backward has run on it
    refused(h, ws, arr, _lib.FEAT_NCHW, b"no offk_off_units_backward has run")
    feats = [ug.dev(f) for f in synth.make_features(B, L, 3)]
    h.off_units(feats)
    h.off_units_backward(feats, ug.random_views(B * (L - 1))[1])
    refused(None, ws, arr, _lib.FEAT_NCHW, b"null argument")
    refused(h, None, arr, _lib.FEAT_NCHW, b"null argument")
    refused(h, ws, None, _lib.FEAT_NCHW, b"null argument")
    refused(h, ws, arr, 2, b"layout must be")
    refused(h, ws, arr, -1, b"layout must be")
    if form.takes_dtype:            # (the fp32 entry has no grad_dtype argument to get wrong)
        for bad, layout in ((3, _lib.FEAT_NCHW), (-1, _lib.FEAT_NHWC), (4, _lib.FEAT_NCHW)):
            refused(h, ws, arr, layout, b"grad_dtype must be", code=bad)
    codes = sorted(set(ug.FEAT[dt] for dt in form.dtypes) | {code})
    mis = ptrs()
    mis[4] = outs[4].data_ptr() + esize                  # aligned for its element, not to 16 bytes
    refused(h, ws, mis, _lib.FEAT_NHWC, b"16-byte aligned")
    mis[4] = outs[4].data_ptr() + 8
    for cd in codes if form.takes_dtype else [code]:
        refused(h, ws, mis, _lib.FEAT_NHWC, b"16-byte aligned", code=cd)
    over = ptrs()
    over[8] = h.workspace.data_ptr() + 256
    refused(h, ws, over, _lib.FEAT_NCHW, b"overlaps the workspace")
    # ... one that begins in front of the workspace and ends 16 bytes inside it (its size counted in the form's real elements)
    n8 = int(np.prod(shapes[8]))
    over[8] = h.workspace.data_ptr() - esize * n8 + 16
    assert over[8] % 16 == 0
    refused(h, ws, over, _lib.FEAT_NCHW, b"overlaps the workspace")
    # ... and one that would end exactly where the workspace begins were its elements 2 bytes, handed over as fp32: twice as long
    over[8] = h.workspace.data_ptr() - 2 * n8
    if over[8] % 16 == 0:
        refused(h, ws, over, _lib.FEAT_NCHW, b"overlaps the workspace", code=_lib.FEAT_F32)
    # the wrapper's own checks
    with pytest.raises(ValueError, match="arith"):
        h.off_units_backward_feats(out=outs, dtype=dtype, arith="bf16")
    with pytest.raises(ValueError, match="layout"):
        form.call(h, layout="nhwc", out=outs, dtype=dtype)
    with pytest.raises(ValueError, match="channels_last"):
        form.call(h, layout="cl", out=outs, dtype=dtype)
    with pytest.raises(ValueError, match="shape"):
        form.call(h, out=outs[1:] + outs[:1], dtype=dtype)
    with pytest.raises(ValueError, match="distinct"):
        form.call(h, sites=[9], dtype=dtype)
    # out= of another dtype than the one asked for
    other = torch.float16 if dtype == torch.float32 else torch.float32
    with pytest.raises(ValueError, match={torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]):
        form.call(h, out=[t.to(other) for t in outs], dtype=dtype)
    with pytest.raises(ValueError, match="fp32" if other == torch.float32 else "fp16"):
        form.call(h, out=outs, dtype=other)
    with pytest.raises(ValueError, match="dtype must be"):
        form.call(h, dtype=torch.float64)
    # all nine NULL: OFFK_OK, nothing enqueued
    assert form.raw(lib, h._h, stream, ws, code, (ctypes.c_void_p * 9)(), _lib.FEAT_NCHW) == 0
    assert form.call(h, sites=[], dtype=dtype) == [None] * 9
    torch.cuda.synchronize()
    assert all(torch.equal(t.contiguous().view(torch.uint8), k) for t, k in zip(outs, keep))
    return h, lib, stream, ws


def full_size(rt, form, check_rows):
    """B = 64, L = 7 (thousands of blocks in the grouped launch): 4096 sampled rows per site, the first and the last among them, of the
    channels-last fp32 result handed to the form's own check `check_rows(si, h, wnp, idx, got)`; doubling dM doubles dX to 1e-6; zero dM
    gives exactly zero."""
    B, L = 64, 7
    N, P = B * L, B * (L - 1)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, training=True)
    wnp = synth.make_weights(spec.VARIANT_RGB)
    assert h.load_state_dict(wnp) == []
    feats = [ug.dev(f) for f in synth.make_features(B, L, 2)]
    h.off_units_train(feats, 21, ug.DROP_P)
    _bufs, views = ug.random_views(P)
    h.off_units_backward(feats, views, 21, ug.DROP_P)
    dx = form.call(h, layout="cl")
    gen = torch.Generator(device="cuda").manual_seed(9)
    for si, (site, C, H) in enumerate(spec.SITES):
        HW = H * H
        idx = torch.randint(0, N * HW, (4096,), device="cuda", generator=gen)
        idx[:2] = torch.tensor([0, N * HW - 1], device="cuda")
        got = ug.rows_of(dx[si])[idx]
        assert float(got.abs().max()) > 0
        check_rows(si, h, wnp, idx, got)
    d1 = [t.clone() for t in dx]
    h.off_units_backward(feats, [(2.0 * t, c) for t, c in views], 21, ug.DROP_P)
    d2 = form.call(h, layout="cl")
    for a, b in zip(d1, d2):
        assert float((b - 2.0 * a).abs().max()) <= 1e-6 * float((2.0 * a).abs().max())
    h.off_units_backward(feats, [(torch.zeros_like(t), c) for t, c in views], 21, ug.DROP_P)
    d0 = form.call(h, layout="cl")
    torch.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in d0)
