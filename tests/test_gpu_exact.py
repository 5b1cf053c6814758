"""Exact integer-input tests of the OFF units (forward and backward), the direct convs and the batched GEMM.

Every other value check in the suite is a tolerance against a float reference or a bit-comparison of two runs of the same kernels.
The first is blind to one lost 32-pixel K-tile in a weight gradient summed over 3.5e5 rows (1e-5 of its magnitude, inside
RTOL = 2e-4), the second to whatever both sides share.  Here the inputs are small integers (tests/exact.py; the condition that makes
every fp32 partial sum exact is asserted on the CPU by tests/test_exact_inputs.py and again, from the reference's own absolute-term
sums, wherever this file draws other inputs) and every result must equal an fp64 reference value for value: exact.assert_exact, no
tolerance anywhere in this file.

Shapes (exact.SHAPES): the smallest that reach each temporal-step count -- K2's ST_TGROUP = 6 and the fused kernel's overlapping
groups take a third from L = 14, K2b's UB_TGROUP = 7 from L = 15 (one frame long there), L = 13 fills two groups exactly -- both slice
modes and both variants; their K1b plans (wg_kpb = max(4, ceil(332 N / 1536))) cover four chunk lengths, asserted below.  All nine
sites always.  One full-size case, B = 64, L = 7: the check the K1b plan at the benchmark shape (97 K-tiles per block, chunk
boundaries inside frames, more than a hundred slabs per site) never had.

Winograd, the chains that contain it and the average pools divide: not covered here.
"""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec

from . import exact
from .exact_units import (DROP_SEED, NAN, UNIT_SLOTS, Case, all_regions, check_forward, conv_inputs, conv_ref, gemm_ref, k1b_plan, poison,
                          units_backward_exact, units_forward_exact)
from .featmaps import rt  # noqa: F401
from .forward import CONV_CASES, PATCH_CASES, nhwc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=exact.SHAPES, ids=exact.IDS)
def case(request):
    """(module scope and parametrised: pytest runs the tests of one shape together, so each reference is computed once)"""
    c = Case(*request.param)
    print("B = %d, L = %d: largest sum of |terms| is %.4f of its limit" % (c.B, c.L, c.worst))
    return c


# ---- forward ----

@pytest.mark.parametrize("prec", ["fp32", "f32split"])
def test_units_forward_exact(rt, case, prec):
    """G_<site>, D_<site> and the unit channels of fusion_28/14/7 after the default units call (K1 + K2), the three temporal-difference
    algorithms of K2 over the same G / D, the fused entry (the handle's arithmetic: the 16-pixel fp32 kernel or the split-fp32 plane
    kernel; it leaves G unwritten), a handle created with OFFK_FUSED_UNITS=0, and the training forward at p = 0.5."""
    units_forward_exact(rt, case, prec)


def test_units_forward_exact_16bit_channels_last(rt):
    """bf16 and fp16 channels-last maps (small integers are exact in both 16-bit types): the fused split-fp32 kernel and the training
    side of the same handle, at the shape whose fused kernel runs three temporal groups."""
    c = Case(2, 14, spec.VARIANT_FLOW, spec.SLICE_FLAT)
    h = c.handle(rt, "f32split")
    for dtype in (torch.bfloat16, torch.float16):
        maps = [x.to(dtype).contiguous(memory_format=torch.channels_last) for x in c.feats]
        assert all(torch.equal(m.float(), x) and not m.is_contiguous() for m, x in zip(maps, c.feats))
        poison(h, all_regions(c, G=False))
        h.off_units_fused(maps)
        check_forward(h, c, "off_units_fused (channels-last %s)" % dtype, G=False)
        poison(h, all_regions(c))
        h.off_units(maps)
        check_forward(h, c, "off_units (channels-last %s)" % dtype)
        poison(h, all_regions(c))
        h.off_units_train(maps, DROP_SEED, exact.DROP_P)
        check_forward(h, c, "off_units_train (channels-last %s)" % dtype, key="M_train")


# ---- backward ----

def test_k1b_chunk_lengths_covered(rt):
    lengths = []
    for (B, L, variant, slice_mode), name in zip(exact.SHAPES, exact.IDS):
        h = rt.OffForward(B, L, variant, slice_mode, training=True)
        counts, k = k1b_plan(h)
        print("%s: K1b chunks per site %s, %d K-tiles per block" % (name, counts, k))
        lengths.append(k)
    assert len(set(lengths)) >= 3, lengths
    hf = rt.OffForward(*exact.FULL_SIZE, training=True)
    counts, k = k1b_plan(hf)
    print("full size: K1b chunks per site %s, %d K-tiles per block" % (counts, k))
    assert k > max(lengths) and min(counts) > 1


def test_units_backward_exact(rt, case):
    """After offk_off_units_train + offk_off_units_backward: dG_<site>, dD_<site>, all 54 (RGB) / 36 (Flow) parameter gradients; a
    second call with accumulate=1 gives exactly twice the reference; offk_off_units_backward_feats in both layouts."""
    units_backward_exact(rt, case)


def test_units_full_size_exact(rt):
    """B = 64, L = 7, RGB, flat, p = 0.5.  Inputs drawn on the device from the same integer recipe, the reference per site on the
    device in fp64, the exactness condition asserted from the reference's own absolute-term sums before anything is compared.
    Checked: G, D, the unit channels, dGpre, dD, every parameter gradient in full (once and accumulated), dX on 4096 sampled rows per
    site, the first and the last row among them."""
    B, L, variant, slice_mode = exact.FULL_SIZE
    N = B * L
    c = Case.__new__(Case)
    c.B, c.L, c.variant, c.slice_mode, c.N, c.P = B, L, variant, slice_mode, N, B * (L - 1)
    c.sites = [exact.SiteInputs(si, B, L, variant, drop_seed=DROP_SEED, device="cuda") for si in range(spec.NUM_SITES)]
    c.weights = exact.weights(variant, c.sites)
    c.feats = [s.x for s in c.sites]
    h = c.handle(rt)
    _counts, kpb = k1b_plan(h)
    assert kpb == 97
    views = c.views()
    h.off_units_train(c.feats, DROP_SEED, exact.DROP_P)
    flat = torch.full_like(h.new_unit_grads(), NAN)
    flat, got = h.off_units_backward(c.feats, views, DROP_SEED, exact.DROP_P, grads=flat)
    dx = h.off_units_backward_feats(layout="cl")
    once = flat.clone()
    _flat, got2 = h.off_units_backward(c.feats, views, DROP_SEED, exact.DROP_P, grads=flat, accumulate=True)
    got1 = dict((k, once[v.storage_offset():v.storage_offset() + v.numel()].view(v.shape)) for k, v in got.items())
    torch.cuda.synchronize()
    gen = torch.Generator(device="cuda").manual_seed(9)
    worst, mm = {}, exact.Mismatches()
    for s, (reg, cs, coff), t in zip(c.sites, UNIT_SLOTS, dx):
        rows = N * s.H * s.H
        idx = torch.randint(0, rows, (4096,), device="cuda", generator=gen)
        idx[:2] = torch.tensor([0, rows - 1], device="cuda")
        ref, cap = exact.unit_reference(s, B, L, variant, slice_mode, dx_rows=idx)
        share = exact.check_caps(cap, s.name)
        big = max(cap, key=lambda k: cap[k] / (exact.LIMIT_ACC if k in exact.PARAM_OUTPUTS else exact.LIMIT))
        print("full size, site %s: largest sum of |terms| %.0f (%s), %.3f of its limit" % (s.name, cap[big], big, share))
        worst[s.name] = share
        what = "full size: "
        mm.check(h.region("G_" + s.name, 128), ref["G"], what + "G_" + s.name)
        mm.check(h.region("D_" + s.name, 32), ref["D"], what + "D_" + s.name)
        mm.check(h.region(reg, cs)[:, coff:coff + 160], ref["M_train"], what + "unit " + s.name)
        mm.check(h.region("dG_" + s.name, 128), ref["dG"], what + "dG_" + s.name)
        mm.check(h.region("dD_" + s.name, 32), ref["dD"], what + "dD_" + s.name)
        for short, key in exact.PARAM_KEYS.items():
            mm.check(got1[key % s.name], ref[short], what + key % s.name)
            mm.check(got2[key % s.name], 2.0 * ref[short], what + "accumulated " + key % s.name)
        mm.check(t.permute(0, 2, 3, 1).reshape(rows, s.C)[idx], ref["dX"], what + "dX " + s.name)
        del ref
    mm.raise_if_any()
    assert max(worst.values()) < 1.0


# ---- offk_conv2d_ex ----

@pytest.mark.parametrize("Ci,Co,k,stride,pad,H,n", CONV_CASES)
def test_conv2d_exact(rt, Ci, Co, k, stride, pad, H, n):
    Ho = (H + 2 * pad - k) // stride + 1
    x, w, b, _res = conv_inputs(Ci + Co + k, n, Ci, Co, k, H, Ho)
    y = rt.conv2d_nhwc(nhwc(x), w.cuda(), b.cuda(), stride, pad)
    exact.assert_exact(y.cpu(), conv_ref(x, w, b, stride, pad), "conv2d")


@pytest.mark.parametrize("cfg,splitk", [(0, 1), (1, 3), (2, 2), (3, 4), (4, 1), (5, 2), (-1, 0)])   # (tests/test_gpu_parity.py's seven pairs)
def test_conv2d_tile_plans_and_splitk_exact(rt, cfg, splitk):
    n, H, Ci, Co = 5, 7, 128, 256
    x, w, b, res = conv_inputs(77, n, Ci, Co, 3, H, H)
    flags = _lib.CONV_RELU_PRE | _lib.CONV_RELU_POST
    y = rt.conv2d_nhwc(nhwc(x), w.cuda(), b.cuda(), 1, 1, res=nhwc(res), flags=flags, tile_cfg=cfg, splitk=splitk)
    exact.assert_exact(y.cpu(), conv_ref(x, w, b, 1, 1, res, flags), "conv2d plan %d, split-K %d" % (cfg, splitk))
    y = rt.conv2d_nhwc(nhwc(x), w.cuda(), b.cuda(), 1, 1, tile_cfg=cfg, splitk=splitk)
    exact.assert_exact(y.cpu(), conv_ref(x, w, b, 1, 1), "conv2d plan %d, split-K %d, plain" % (cfg, splitk))


@pytest.mark.parametrize("k,stride,H,Ci,Co,n,cfg,splitk", PATCH_CASES)
def test_conv2d_patch_kernel_exact(rt, k, stride, H, Ci, Co, n, cfg, splitk):
    pad = k // 2
    Ho = (H + 2 * pad - k) // stride + 1
    xs, w, b, res = conv_inputs(k * 1000 + Ci + Co + n, n, Ci, Co, k, H, Ho, x_extra=32)     # the conv reads channels 32.. of a wider buffer
    x = xs[:, 32:]
    flags = _lib.CONV_RELU_IN | _lib.CONV_RELU_PRE | _lib.CONV_RELU_POST
    ybuf = torch.full((n, Ho, Ho, Co + 64), 7.0, device="cuda")
    rt.conv2d_nhwc(nhwc(xs), w.cuda(), b.cuda(), stride, pad, res=nhwc(res), flags=flags, x_coff=32, ci=Ci, y=ybuf, y_coff=32,
                   tile_cfg=cfg, splitk=splitk)
    exact.assert_exact(ybuf[..., 32:32 + Co].cpu(), conv_ref(x, w, b, stride, pad, res, flags), "patch conv")
    assert torch.all(ybuf[..., :32] == 7.0) and torch.all(ybuf[..., 32 + Co:] == 7.0)
    y = rt.conv2d_nhwc(nhwc(x), w.cuda(), b.cuda(), stride, pad, tile_cfg=cfg, splitk=1)
    exact.assert_exact(y.cpu(), conv_ref(x, w, b, stride, pad), "patch conv, plain")


def test_conv2d_epilogues_and_slices_exact(rt):
    n, H, Ci, Co = 3, 7, 64, 128
    xs, w, b, res = conv_inputs(5, n, Ci, Co, 3, H, H, x_extra=32)          # the conv reads channels 32..95 of a 96-channel buffer
    x = xs[:, 32:]
    for flags in (0, _lib.CONV_RELU_IN | _lib.CONV_RELU_PRE, _lib.CONV_RELU_POST, _lib.CONV_RELU_PRE | _lib.CONV_RELU_POST):
        r = res if flags & _lib.CONV_RELU_POST else None
        ybuf = torch.full((n, H, H, Co + 64), 7.0, device="cuda")           # write channels 32..159 of a wider buffer
        rt.conv2d_nhwc(nhwc(xs), w.cuda(), b.cuda(), 1, 1, res=nhwc(r) if r is not None else None, flags=flags, x_coff=32, y=ybuf, y_coff=32)
        exact.assert_exact(ybuf[..., 32:32 + Co].cpu(), conv_ref(x, w, b, 1, 1, r, flags), "conv2d flags %d" % flags)
        assert torch.all(ybuf[..., :32] == 7.0) and torch.all(ybuf[..., 32 + Co:] == 7.0)
    y = rt.conv2d_nhwc(nhwc(x), w.cuda(), b.cuda(), 1, 1, res=nhwc(res), flags=0)       # residual add without any ReLU
    exact.assert_exact(y.cpu(), conv_ref(x, w, b, 1, 1, res, 0), "conv2d + residual")


# ---- offk_batched_gemm_nt ----

GEMM_SHAPES = [(5, 384, 832, 256), (121, 384, 256, 256), (3, 100, 128, 128), (7, 64, 64, 512), (2, 777, 1056, 128), (9, 200, 320, 64),
               (3, 130, 1280, 192), (70, 3456, 64, 64)]                    # (test_batched_gemm_split_shapes' list, tests/test_gpu_split.py)


@pytest.mark.parametrize("batch,M,K,Co", GEMM_SHAPES)
def test_batched_gemm_exact(rt, batch, M, K, Co):
    """8-bit integers on both sides (the top bf16 plane alone) in both precisions; 12-bit x against w in {-1, 0, 1} in split precision
    (top and middle planes; every kept product and sum is still exact)."""
    seed = batch + M + K + Co
    x = exact.ints(exact.stream(seed, 12), (batch, M, K), -127, 127, "cuda")
    w = exact.ints(exact.stream(seed, 13), (batch, Co, K), -127, 127, "cuda")
    ref = gemm_ref(x, w)
    for prec in ("fp32", "f32split"):
        exact.assert_exact(rt.batched_gemm_nt(x, w, prec), ref, "batched GEMM %s, 8-bit" % prec)
    x = exact.ints(exact.stream(seed, 14), (batch, M, K), -4095, 4095, "cuda")
    w = exact.ints(exact.stream(seed, 15), (batch, Co, K), -1, 1, "cuda")
    assert float(x.abs().max()) > 2048
    exact.assert_exact(rt.batched_gemm_nt(x, w, "f32split"), gemm_ref(x, w), "batched GEMM f32split, 12-bit")
