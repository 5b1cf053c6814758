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
from . import units_dx_checks as checks
from .units_dx_checks import LAYOUTS, old_values
from .units_grad import DX_TYPED as FORM
from .units_grad import Case, bits16, case, dev, make_units, module_cots, random_views, rows16, rt, same_bits16  # noqa: F401

pytestmark = pytest.mark.gpu
DTYPES = list(FORM.dtypes)
DT_IDS = ["bf16", "fp16"]
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP),
          (5, 9, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP)]
IDS = ["b1l2", "b2l3_flat", "b3l4_clip", "b5l9_clip_flow"]


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
    checks.equal_bits(FORM, case(rt, 3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, 7), (dtype,))


# (the id names the maps' form, the dtype beside it is the gradient's: fp32 channels_last maps hand out an fp16 gradient here)
@pytest.mark.parametrize("kind,dtype", [("typed_bf16", torch.bfloat16), ("cl_f32", torch.float16), ("cl_f16", torch.float16)],
                         ids=["typed_bf16", "cl_f32", "cl_f16"])
def test_same_bits_after_the_plain_typed_and_cl_backward(rt, kind, dtype):
    """The three backward forms leave the same dG / dD on the same logical maps, so the 16-bit dX is the same too."""
    checks.same_bits_after_the_other_backwards(FORM, Case(rt, 2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT, 7), kind, dtype)


# ---- 3. memory discipline ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("B,L,slice_mode", [(1, 2, spec.SLICE_FLAT), (3, 4, spec.SLICE_PER_CLIP)], ids=["b1l2", "b3l4_clip"])
def test_memory_discipline(rt, B, L, slice_mode, dtype, layout, accumulate):
    checks.memory_discipline(FORM, case(rt, B, L, spec.VARIANT_RGB, slice_mode, 7), layout, dtype, accumulate)


# ---- 4. refusals ----

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_refusals_leave_the_outputs_untouched(rt, dtype):
    h, lib, stream, ws = checks.refusals(rt, FORM, dtype)
    # OFFK_FEAT_F32 through the typed entry is the fp32 entry: same bits
    a = h.off_units_backward_feats(layout="nchw")
    b = [torch.empty_like(t) for t in a]
    assert FORM.raw(lib, h._h, stream, ws, _lib.FEAT_F32, (ctypes.c_void_p * 9)(*[t.data_ptr() for t in b]), _lib.FEAT_NCHW) == 0
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
