"""dX in the maps' own 16-bit dtype (offk_off_units_backward_feats_typed, csrc/units_dx_f16.hip; OFFUnits(feat_grad=True) on bf16 /
fp16 maps).  The fp32 entry is checked against fp64, the oracle and exact integers in tests/test_gpu_feat_grad.py and
tests/test_gpu_exact.py; here the contract of the 16-bit forms is checked:

1. the rounding, pinned without the fp32 kernel: chosen fp32 bit patterns pass through the kernel untouched (a 0 / 1 gen weight)
   and must come out as torch's CPU `.to(dtype)` of them, bit for bit;
2. the contract: dx16 == dx32.to(dtype) and, accumulated, (old.float() + dx32).to(dtype), on random and on exact integer inputs;
   NCHW and NHWC hold the same bits; two runs and a graph replay are equal; equal after the plain, _typed and _cl backward;
3. memory discipline in a guarded arena (the sentinel's 16-bit halves are NaNs of both 16-bit types);
4. refusals leave the outputs untouched;
5. the module: 16-bit gradients straight from the kernel, no fp32 dX tensor.

Shapes: those of tests/test_gpu_feat_grad.py that stress the kernel's edges -- (1, 2): 98 rows at the 7x7 sites, less than one
128-row tile, a partial last tile at 28x28; (2, 3) flat: frames outside the slice; (3, 4) per-clip; (5, 9) per-clip, Flow.  All
nine sites always: 320 and 608 channels end in half a 64-channel tile."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from . import arena as arena_mod
from . import exact
from .test_gpu_feat_grad import Case, case, dev, make_units, module_cots, random_views

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]
LAYOUTS = ["nchw", "cl"]
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP),
          (5, 9, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP)]
IDS = ["b1l2", "b2l3_flat", "b3l4_clip", "b5l9_clip_flow"]
FEAT = {torch.bfloat16: _lib.FEAT_BF16, torch.float16: _lib.FEAT_F16}


@pytest.fixture(scope="module")
def rt():
    from offk_amd import runtime
    return runtime


def bits16(t):
    return t.contiguous().view(torch.int16)


def same_bits16(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits16(a), bits16(b))


def rows16(t, layout):
    """[N, C, H, H] 16-bit result of either layout -> [N * HW, C], on the device."""
    assert t.dim() == 4 and (t.permute(0, 2, 3, 1).is_contiguous() if layout == "cl" else t.is_contiguous())
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ---- 1. the rounding, pinned independently of the fp32 kernel ----

def rounding_patterns(dtype):
    """fp32 bit patterns (uint32, an odd number of them) around every rounding decision of `dtype`.  Left out on purpose: fp32
    subnormals (the matrix pipe's treatment of them is not this test's subject), non-finite values and -0.0 / zeros (a NaN and the
    sign of a zero sum are outside the contract)."""
    bf = dtype == torch.bfloat16
    drop, mant = (16, 7) if bf else (13, 10)
    half = 1 << (drop - 1)
    # exponent fields of fp32: bf16 shares fp32's range; fp16's normal range is 2^-14 .. 2^15 (fields 113 .. 142)
    exps = [1, 2, 60, 126, 127, 128, 200, 253, 254] if bf else [113, 114, 120, 126, 127, 128, 135, 141, 142]
    rng = np.random.RandomState(16)
    out = []
    for e in exps:
        kept = [0, 1, 2, (1 << mant) - 1, (1 << mant) - 2] + [int(k) for k in rng.randint(0, 1 << mant, 12)]
        for k in kept:
            base = (e << 23) | (k << drop)
            low = int(rng.randint(1, half - 1))
            out += [base, base | half, (base | half) + 1, (base | half) - 1, base | low, base | half | low]
    if bf:
        out += [0x7F7FFFFF, 0x7F7FFFFE, 0x7F7F8000, 0x7F7F8001, 0x7F7F7FFF, 0x7F7F0000]      # just under FLT_MAX: -> Inf from 0x7F7F8000 on
    else:
        past = np.array([65504.0, 65519.0, 65519.996, 65520.0, 65520.004, 65536.0, 7.0e4, 1.0e5, 3.0e38], dtype=np.float32)
        out += [int(b) for b in past.view(np.uint32)]
        # results in fp16's subnormal range, 2^-24 .. 2^-14: ties (j + 1/2) 2^-24, one fp32 ulp either side, exact values, random ones
        for j in [1, 2, 3, 4, 5, 510, 511, 512, 1021, 1022, 1023] + [int(k) for k in rng.randint(1, 1023, 12)]:
            tie = int(np.array([(j + 0.5) * 2.0 ** -24], dtype=np.float32).view(np.uint32)[0])
            out += [tie, tie + 1, tie - 1, int(np.array([j * 2.0 ** -24], dtype=np.float32).view(np.uint32)[0])]
        for e in range(103, 113):
            out += [(e << 23) | int(m) for m in rng.randint(0, 1 << 23, 6)]
    u = np.array(out, dtype=np.uint32)
    u = np.concatenate([u, u | np.uint32(0x80000000)])          # both signs
    if len(u) % 2 == 0:
        u = np.concatenate([u, np.array([0x3F800000], dtype=np.uint32)])       # odd length: the tiling below walks over all 128 columns
    return u


def check_patterns(u, dtype):
    """The data does hold what the test claims to exercise (asserted on the host, before it is used)."""
    bf = dtype == torch.bfloat16
    drop, mant = (16, 7) if bf else (13, 10)
    half = 1 << (drop - 1)
    u = u.astype(np.int64)
    e = (u >> 23) & 0xFF
    assert ((e >= 1) & (e <= 254)).all()                                     # normal, finite, nonzero fp32 only
    normal = np.ones_like(e, dtype=bool) if bf else (e >= 113) & (e <= 142)  # where exactly `drop` bits go
    rem, lsb, kept = u & (2 * half - 1), (u >> drop) & 1, (u >> drop) & ((1 << mant) - 1)
    tie = normal & (rem == half)
    assert (tie & (lsb == 0)).sum() > 0 and (tie & (lsb == 1)).sum() > 0                       # exact ties, even and odd kept mantissa
    assert (normal & (rem == half + 1)).sum() > 0 and (normal & (rem == half - 1)).sum() > 0   # one ulp either side of a tie
    carry = tie & (kept == (1 << mant) - 1)
    assert carry.sum() > 0                                                                    # a round-up that carries into the exponent
    x = torch.from_numpy(u.astype(np.uint32).view(np.float32).copy())
    y = x.to(dtype)
    yc = y[torch.from_numpy(carry)].double().abs()                                            # ... lands on the next power of two (or Inf)
    assert bool(((yc == torch.from_numpy(2.0 ** (e[carry].astype(np.float64) - 126))) | torch.isinf(yc)).all())
    assert bool(torch.isfinite(x).all()) and int(torch.isinf(y).sum()) >= 4                    # finite sums past the largest finite value
    if not bf:
        a = x.double().abs()
        assert int(((a > 65504) & torch.isinf(y)).sum()) > 0
        sub = (y.float().abs() > 0) & (y.float().abs() < 2.0 ** -14)
        assert int(sub.sum()) > 20                                                            # results in the subnormal range
        t = a * 2.0 ** 24
        assert int(((a < 2.0 ** -14) & (t - t.floor() == 0.5)).sum()) > 10                      # ties among them
    return y


@functools.lru_cache(maxsize=None)
def passthrough_handle(rt):
    """A (1, 2) handle whose gen weights are Wg[o, c] = 1 if o == c % 128 else 0 and whose down weights are zero, after one real
    backward (which sets the handle's flag): every dX sum is then exactly dG[row, c % 128] -- every other product is a zero."""
    B, L = 1, 2
    w = synth.make_weights(spec.VARIANT_RGB)
    for site, C, _H in spec.SITES:
        wg = np.zeros((128, C, 1, 1), dtype=np.float32)
        wg[np.arange(C) % 128, np.arange(C), 0, 0] = 1.0
        w["motion_conv_gen_%s.weight" % site] = wg
        w["motion_spatial_down_%s.weight" % site] = np.zeros((32, C, 1, 1), dtype=np.float32)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, training=True)
    assert h.load_state_dict(w) == []
    feats = [dev(f) for f in synth.make_features(B, L, 3)]
    h.off_units(feats)
    h.off_units_backward(feats, random_views(B * (L - 1))[1])
    return h


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_rounding_is_nearest_even(rt, dtype, layout):
    """All nine sites at (1, 2): both 28x28 sites, 3c (576 channels), 4c / 4d (608: half a tile), the 7x7 sites (98 rows)."""
    h = passthrough_handle(rt)
    u = rounding_patterns(dtype)
    y = check_patterns(u, dtype)
    want = {}
    for si, (site, C, H) in enumerate(spec.SITES):
        dG, dD = h.region("dG_" + site, 128), h.region("dD_" + site, 32)
        idx = (np.arange(dG.numel(), dtype=np.int64) + 977 * si) % len(u)
        dG.copy_(torch.from_numpy(u[idx].view(np.float32).copy()).view_as(dG))
        dD.zero_()
        # what torch's own conversion makes of the very same numbers, on the CPU
        want[si] = y[torch.from_numpy(idx)].view(dG.shape[0], 128)[:, torch.arange(C) % 128]
    got = h.off_units_backward_feats(layout=layout, dtype=dtype)
    torch.cuda.synchronize()
    for si, (site, C, H) in enumerate(spec.SITES):
        g = rows16(got[si], layout).cpu()
        assert g.dtype == dtype and tuple(g.shape) == (2 * H * H, C)
        ne = bits16(g) != bits16(want[si])
        assert not bool(ne.any()), (site, int(ne.sum()), ne.nonzero()[:4].tolist())


# ---- 2. the contract ----

def old_values(like, seed, scale):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return [(scale * float(t.float().abs().max()) * torch.randn(t.shape, device="cuda", generator=gen)).to(t.dtype).contiguous(
        memory_format=torch.channels_last if not t.is_contiguous() else torch.contiguous_format) for t in like]


def check_contract(h, dtype, what):
    """dx16 == dx32.to(dtype); accumulate: (old.float() + dx32).to(dtype); both layouts the same bits."""
    dx32 = h.off_units_backward_feats(layout="nchw")
    res = {}
    for layout in LAYOUTS:
        dx16 = h.off_units_backward_feats(layout=layout, dtype=dtype)
        old = old_values(dx16, 31, 1.0)
        acc = [t.clone(memory_format=torch.preserve_format) for t in old]
        back = h.off_units_backward_feats(layout=layout, out=acc, accumulate=True, dtype=dtype)
        torch.cuda.synchronize()
        for si, (a, b, o, f) in enumerate(zip(dx16, acc, old, dx32)):
            site = spec.SITES[si][0]
            assert back[si] is b and a.dtype == dtype and float(f.abs().max()) > 0
            assert a.is_contiguous() if layout == "nchw" else (a.is_contiguous(memory_format=torch.channels_last) and not a.is_contiguous())
            assert not bool(torch.isnan(a.float()).any()) and not bool(torch.isnan(b.float()).any())
            assert torch.equal(a, f.to(dtype)), (what, layout, site)
            assert torch.equal(b, (o.float() + f).to(dtype)), (what, layout, site, "accumulate")
        res[layout] = dx16
    for a, b in zip(res["nchw"], res["cl"]):
        assert same_bits16(a, b.contiguous())
    return res["nchw"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,L,variant,slice_mode", SHAPES, ids=IDS)
def test_contract_on_random_inputs(rt, B, L, variant, slice_mode, dtype):
    c = case(rt, B, L, variant, slice_mode, 7)
    c.run()
    check_contract(c.h, dtype, "random")


@functools.lru_cache(maxsize=None)
def exact_handle(rt):
    """(2, 3) flat, RGB on tests/exact.py's integer inputs, after the training forward and one backward: every dX sum is an integer."""
    B, L, variant = 2, 3, spec.VARIANT_RGB
    sites = [exact.SiteInputs(si, B, L, variant, drop_seed=21) for si in range(spec.NUM_SITES)]
    h = rt.OffForward(B, L, variant, spec.SLICE_FLAT, training=True)
    assert h.load_state_dict(exact.weights(variant, sites)) == []
    feats = [s.x.cuda() for s in sites]
    P = B * (L - 1)
    bufs = [torch.full((P, H, H, C), 7.0, device="cuda") for H, C in ((28, 320), (14, 1056), (7, 832))]
    views = [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]
    for s, (buf, coff) in zip(sites, views):
        buf[..., coff:coff + 160] = s.dm.cuda().permute(0, 2, 3, 1)
    h.off_units_train(feats, 21, exact.DROP_P)
    h.off_units_backward(feats, views, 21, exact.DROP_P)
    return h


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_contract_on_exact_integer_inputs(rt, dtype):
    h = exact_handle(rt)
    dx32 = h.off_units_backward_feats(layout="nchw")
    assert all(bool((t == t.round()).all()) and float(t.abs().max()) > 0 for t in dx32)         # integers, every sum exact in fp32
    check_contract(h, dtype, "integers")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_two_runs_and_a_graph_replay_are_equal(rt, dtype):
    c = case(rt, 3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, 7)
    c.run()
    first = c.h.off_units_backward_feats(layout="nchw", dtype=dtype)
    again = c.h.off_units_backward_feats(layout="nchw", dtype=dtype)
    torch.cuda.synchronize()
    assert all(float(a.float().abs().max()) > 0 and same_bits16(a, b) for a, b in zip(first, again))
    # backward + the 16-bit dX call in one graph, one replay, for either layout
    grads = c.h.new_unit_grads()
    outs = {"nchw": [torch.empty_like(t) for t in first], "cl": [torch.empty_like(t, memory_format=torch.channels_last) for t in first]}

    def launch():
        c.backward(grads=grads)
        for layout in LAYOUTS:
            c.h.off_units_backward_feats(layout=layout, out=outs[layout], dtype=dtype)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for layout in LAYOUTS:
        for t in outs[layout]:
            t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for layout in LAYOUTS:
        assert all(same_bits16(a, b.contiguous()) for a, b in zip(first, outs[layout])), layout


@pytest.mark.parametrize("kind,dtype", [("typed_bf16", torch.bfloat16), ("cl_f32", torch.float16), ("cl_f16", torch.float16)],
                         ids=["typed_bf16", "cl_f32", "cl_f16"])
def test_same_bits_after_the_plain_typed_and_cl_backward(rt, kind, dtype):
    """The three backward forms leave the same dG / dD on the same logical maps, so the 16-bit dX is the same too."""
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
        res.append([c.h.off_units_backward_feats(layout=layout, dtype=dtype) for layout in LAYOUTS])
    torch.cuda.synchronize()
    for lay in range(2):
        for a, b in zip(res[0][lay], res[1][lay]):
            assert float(a.float().abs().max()) > 0 and same_bits16(a.contiguous(), b.contiguous())


# ---- 3. memory discipline ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,L,slice_mode", [(1, 2, spec.SLICE_FLAT), (3, 4, spec.SLICE_PER_CLIP)], ids=["b1l2", "b3l4_clip"])
def test_memory_discipline(rt, B, L, slice_mode, dtype, layout, accumulate):
    """Every output is a carve of exactly its 2-byte elements inside one arena of sentinel (each 16-bit half of the sentinel word is
    a NaN of both types): the bands on both sides of all nine and the carves of the skipped sites keep every half-word."""
    c = case(rt, B, L, spec.VARIANT_RGB, slice_mode, 7)
    c.run()
    shapes = spec.feature_shapes(B, L)
    ar = arena_mod.Arena.for_sizes([2 * int(np.prod(s)) for s in shapes])
    skipped = (1, 6)
    want = c.h.off_units_backward_feats(layout=layout, dtype=dtype)
    dx32 = c.h.off_units_backward_feats(layout=layout)
    old = old_values(want, 5, 1.0)

    def carve(i):
        n, ch, hh, _ = shapes[i]
        shape = (n, ch, hh, hh) if layout == "nchw" else (n, hh, hh, ch)
        if accumulate and i not in skipped:
            t = ar.put("dx_%d" % i, old[i] if layout == "nchw" else old[i].permute(0, 2, 3, 1))
        else:
            t = ar.empty("dx_%d" % i, shape, dtype=dtype)
        assert t.data_ptr() % 16 == 0 and t.element_size() == 2
        return t if layout == "nchw" else t.permute(0, 3, 1, 2)

    bufs = [carve(i) for i in range(9)]
    got = c.h.off_units_backward_feats(sites=[i for i in range(9) if i not in skipped], layout=layout,
                                       out=[None if i in skipped else b for i, b in enumerate(bufs)], accumulate=accumulate, dtype=dtype)
    torch.cuda.synchronize()
    ar.check()
    for i in range(9):
        if i in skipped:
            assert got[i] is None and ar.untouched(bufs[i] if layout == "nchw" else bufs[i].permute(0, 2, 3, 1))
        else:
            assert not bool(torch.isnan(got[i].float()).any())
            assert torch.equal(got[i], (old[i].float() + dx32[i]).to(dtype) if accumulate else want[i]), spec.SITES[i][0]


# ---- 4. refusals ----

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_refusals_leave_the_outputs_untouched(rt, dtype):
    B, L = 1, 2
    shapes = spec.feature_shapes(B, L)
    outs = [torch.full(tuple(s), float("nan"), device="cuda", dtype=dtype) for s in shapes]
    keep = [bits16(t).clone() for t in outs]
    arr = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    lib = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fd = FEAT[dtype]

    def refused(h, ws, a, gd, layout, needle):
        rc = lib.offk_off_units_backward_feats_typed(h._h, stream, ws, gd, a, layout, 0)
        assert rc == -1 and needle in lib.offk_last_error(h._h), lib.offk_last_error(h._h)

    h = rt.OffForward(B, L, spec.VARIANT_RGB, training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    ws = ctypes.c_void_p(h.workspace.data_ptr())
    # a fresh handle: no backward has run on it
    refused(h, ws, arr, fd, _lib.FEAT_NCHW, b"no offk_off_units_backward has run")
    feats = [dev(f) for f in synth.make_features(B, L, 3)]
    h.off_units(feats)
    h.off_units_backward(feats, random_views(B * (L - 1))[1])
    for bad in (3, -1, 4):
        refused(h, ws, arr, bad, _lib.FEAT_NCHW, b"grad_dtype must be")
    refused(h, ws, arr, fd, 2, b"layout must be")
    mis = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    mis[4] = outs[4].data_ptr() + 2                      # aligned for its element, not to 16 bytes
    refused(h, ws, mis, fd, _lib.FEAT_NHWC, b"16-byte aligned")
    over = (ctypes.c_void_p * 9)(*[t.data_ptr() for t in outs])
    over[8] = h.workspace.data_ptr() + 256
    refused(h, ws, over, fd, _lib.FEAT_NCHW, b"overlaps the workspace")
    # ... and one that begins in front of the workspace and ends 16 bytes inside it (its size counted in 2-byte elements)
    n8 = 2 * int(np.prod(shapes[8]))
    over[8] = h.workspace.data_ptr() - n8 + 16
    refused(h, ws, over, fd, _lib.FEAT_NCHW, b"overlaps the workspace")
    # the wrapper: out= of another dtype than the one asked for
    with pytest.raises(ValueError, match="bf16" if dtype == torch.bfloat16 else "fp16"):
        h.off_units_backward_feats(out=[t.float() for t in outs], dtype=dtype)
    with pytest.raises(ValueError, match="fp32"):
        h.off_units_backward_feats(out=outs)
    with pytest.raises(ValueError, match="dtype must be"):
        h.off_units_backward_feats(dtype=torch.float64)
    # all nine NULL: OFFK_OK, nothing enqueued
    assert lib.offk_off_units_backward_feats_typed(h._h, stream, ws, fd, (ctypes.c_void_p * 9)(), _lib.FEAT_NCHW, 0) == 0
    assert h.off_units_backward_feats(sites=[], dtype=dtype) == [None] * 9
    torch.cuda.synchronize()
    assert all(torch.equal(bits16(t), k) for t, k in zip(outs, keep))
    # OFFK_FEAT_F32 through the typed entry is the fp32 entry: same bits
    a = h.off_units_backward_feats(layout="nchw")
    b = [torch.empty_like(t) for t in a]
    assert lib.offk_off_units_backward_feats_typed(h._h, stream, ws, _lib.FEAT_F32, (ctypes.c_void_p * 9)(*[t.data_ptr() for t in b]),
                                                   _lib.FEAT_NCHW, 0) == 0
    torch.cuda.synchronize()
    assert all(arena_mod.same_bits(x, y) for x, y in zip(a, b))


# ---- 5. the module ----

@pytest.mark.parametrize("dtype,cl", [(torch.bfloat16, False), (torch.float16, True)], ids=["bf16_contiguous", "fp16_channels_last"])
def test_module_hands_out_16bit_gradients_from_the_kernel(rt, monkeypatch, dtype, cl):
    B, L = 2, 3
    P = B * (L - 1)
    u, _w = make_units(B, L, True)
    cots = module_cots(P)
    fmt = torch.channels_last if cl else torch.contiguous_format
    x16 = [dev(f).to(dtype).contiguous(memory_format=fmt).requires_grad_(True) for f in synth.make_features(B, L, 2)]
    x32 = [f.detach().float().requires_grad_(True) for f in x16]          # the same values (and the same layout) as fp32 maps
    seen = []
    real = rt.OffForward.off_units_backward_feats

    def spy(self, sites=None, layout="nchw", out=None, accumulate=False, dtype=torch.float32):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = real(self, sites, layout, out, accumulate, dtype=dtype)
        torch.cuda.synchronize()
        seen.append((dtype, layout, torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before, res))
        return res

    monkeypatch.setattr(rt.OffForward, "off_units_backward_feats", spy)
    torch.autograd.backward(u(x16, drop_seed=7), cots)
    torch.cuda.synchronize()
    p16 = {k: p.grad.clone() for k, p in u.named_parameters() if p.grad is not None}
    for p in u.parameters():
        p.grad = None
    torch.autograd.backward(u(x32, drop_seed=7), cots)
    torch.cuda.synchronize()
    p32 = {k: p.grad for k, p in u.named_parameters() if p.grad is not None}
    assert [(s[0], s[1]) for s in seen] == [(dtype, "cl" if cl else "nchw"), (torch.float32, "cl" if cl else "nchw")]
    # what the wrapper allocated for the 16-bit call: the nine 16-bit tensors, at no moment more.  torch's caching allocator hands out
    # a cached block whole when what would be left of it is under 1 MiB (its large pool; small requests are rounded up to 512
    # bytes), so each tensor may count for up to 1 MiB more than its bytes; an fp32 dX would count for bytes16 more, which is more
    # than that slack at this shape
    bytes16 = sum(2 * f.numel() for f in x16)
    slack = 9 << 20
    assert bytes16 > slack
    _dt, _lay, grown, peak, res = seen[0]
    assert all(t.dtype == dtype for t in res)
    assert bytes16 <= grown <= bytes16 + slack and peak <= bytes16 + slack, (bytes16, grown, peak)
    assert seen[1][2] >= 2 * bytes16
    for a, b in zip(x16, x32):
        assert a.grad.dtype == dtype and b.grad.dtype == torch.float32 and float(b.grad.abs().max()) > 0
        assert a.grad.is_contiguous(memory_format=fmt) and (not cl or not a.grad.is_contiguous())
        assert torch.equal(a.grad, b.grad.to(dtype))
    assert p16.keys() == p32.keys() and len(p16) == 54 and all(arena_mod.same_bits(p16[k], p32[k]) for k in p16)
