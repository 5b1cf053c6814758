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
import ctypes

import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import _lib, spec

from . import exact
from .test_gpu_parity import CONV_CASES, PATCH_CASES

pytestmark = pytest.mark.gpu
DROP_SEED = 21
# (workspace region, its channels per pixel, first channel) of every site's unit [S 32 | T 128]
UNIT_SLOTS = [("fusion_28", 320, 0), ("fusion_28", 320, 160)] + [("fusion_14", 1056, 160 * k) for k in range(5)] + [("fusion_7", 832, 0), ("fusion_7", 832, 160)]
NAN = float("nan")


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


class Case:
    """Inputs and fp64 references of one shape, the references on the device."""

    def __init__(self, B, L, variant, slice_mode):
        self.B, self.L, self.variant, self.slice_mode = B, L, variant, slice_mode
        self.N, self.P = B * L, B * (L - 1)
        self.sites = [exact.SiteInputs(si, B, L, variant, drop_seed=DROP_SEED) for si in range(spec.NUM_SITES)]
        self.worst = 0.0
        self.ref = []
        for s in self.sites:
            out, cap = exact.unit_reference(s, B, L, variant, slice_mode)
            self.worst = max(self.worst, exact.check_caps(cap, s.name))
            self.ref.append(dict((k, v.cuda()) for k, v in out.items()))
        self.weights = exact.weights(variant, self.sites)
        self.feats = [s.x.cuda() for s in self.sites]

    def handle(self, rt, precision="fp32", training=True):
        h = rt.OffForward(self.B, self.L, self.variant, self.slice_mode, precision=precision, training=training)
        assert h.load_state_dict(self.weights) == []
        return h

    def views(self):
        """The gradients w.r.t. the three fusion buffers (channels-last; the carried-over channels hold a value nothing may read
        into a unit's gradient) and the nine (tensor, coff) views of the units in them."""
        bufs = {}
        out = []
        for s, (reg, cs, coff) in zip(self.sites, UNIT_SLOTS):
            if reg not in bufs:
                bufs[reg] = torch.full((self.P, s.H, s.H, cs), 7.0, device="cuda")
            bufs[reg][..., coff:coff + 160] = s.dm.cuda().permute(0, 2, 3, 1)
            out.append((bufs[reg], coff))
        return out


@pytest.fixture(scope="module", params=exact.SHAPES, ids=exact.IDS)
def case(request):
    """(module scope and parametrised: pytest runs the tests of one shape together, so each reference is computed once)"""
    c = Case(*request.param)
    print("B = %d, L = %d: largest sum of |terms| is %.4f of its limit" % (c.B, c.L, c.worst))
    return c


def poison(h, regions):
    for name, ch in regions:
        h.region(name, ch).fill_(NAN)


def check_forward(h, c, what, key="M", G=True, D=True):
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    for s, ref, (reg, cs, coff) in zip(c.sites, c.ref, UNIT_SLOTS):
        if G:
            mm.check(h.region("G_" + s.name, 128), ref["G"], "%s: G_%s" % (what, s.name))
        if D:
            mm.check(h.region("D_" + s.name, 32), ref["D"], "%s: D_%s" % (what, s.name))
        mm.check(h.region(reg, cs)[:, coff:coff + 160], ref[key], "%s: unit %s in %s" % (what, s.name, reg))
    mm.raise_if_any()


def all_regions(c, G=True):
    r = [("fusion_28", 320), ("fusion_14", 1056), ("fusion_7", 832)] + [("D_" + s.name, 32) for s in c.sites]
    return r + ([("G_" + s.name, 128) for s in c.sites] if G else [])


# ---- forward ----

@pytest.mark.parametrize("prec", ["fp32", "f32split"])
def test_units_forward_exact(rt, case, prec, monkeypatch):
    """G_<site>, D_<site> and the unit channels of fusion_28/14/7 after the default units call (K1 + K2), the three temporal-difference
    algorithms of K2 over the same G / D, the fused entry (the handle's arithmetic: the 16-pixel fp32 kernel or the split-fp32 plane
    kernel; it leaves G unwritten), a handle created with OFFK_FUSED_UNITS=0, and the training forward at p = 0.5."""
    c = case
    h = c.handle(rt, prec)
    poison(h, all_regions(c))
    h.off_units(c.feats)
    check_forward(h, c, "off_units")
    for algo in (0, 1, 4):
        poison(h, all_regions(c)[:3])
        h.sobel_tdiff_all(algo)
        check_forward(h, c, "sobel_tdiff_all(algo %d)" % algo, G=False, D=False)
    poison(h, all_regions(c, G=False))
    h.off_units_fused(c.feats)
    check_forward(h, c, "off_units_fused", G=False)
    poison(h, all_regions(c))
    h.off_units_train(c.feats, DROP_SEED, exact.DROP_P)
    check_forward(h, c, "off_units_train", key="M_train")
    monkeypatch.setenv("OFFK_FUSED_UNITS", "0")               # (read once, at offk_create)
    h0 = c.handle(rt, prec, training=False)
    monkeypatch.delenv("OFFK_FUSED_UNITS")
    poison(h0, all_regions(c))
    h0.off_units_fused(c.feats)
    check_forward(h0, c, "off_units_fused, OFFK_FUSED_UNITS=0")


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

def k1b_plan(h):
    """(chunk count of every site, the chunk length they imply): nchunks from the size of wgb_<site> ([nchunks][160] floats), the
    length as the one k with ceil(N ceil(HW / 32) / k) == nchunks at all nine sites."""
    counts = []
    for name, _C, _H in spec.SITES:
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(h.lib.offk_workspace_region(h._h, ("wgb_" + name).encode(), ctypes.byref(off), ctypes.byref(nb)), h._h)
        assert nb.value % (4 * spec.UNIT_CH) == 0
        counts.append(nb.value // (4 * spec.UNIT_CH))
    kts = [h.N * ((H * H + 31) // 32) for _n, _C, H in spec.SITES]
    fits = [k for k in range(1, max(kts) + 1) if all((kt + k - 1) // k == n for kt, n in zip(kts, counts))]
    assert len(fits) == 1, (counts, fits)
    return counts, fits[0]


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


def check_backward(h, c_sites, refs, got, what, twice=False):
    """dG_<site>, dD_<site> and every parameter gradient (twice: only the gradients, against twice the reference)"""
    torch.cuda.synchronize()
    n, mm = 0, exact.Mismatches()
    for s, ref in zip(c_sites, refs):
        if not twice:
            mm.check(h.region("dG_" + s.name, 128), ref["dG"], "%s: dG_%s" % (what, s.name))
            mm.check(h.region("dD_" + s.name, 32), ref["dD"], "%s: dD_%s" % (what, s.name))
        for short, key in exact.PARAM_KEYS.items():
            if short in ref:
                mm.check(got[key % s.name], 2.0 * ref[short] if twice else ref[short], "%s: %s" % (what, key % s.name))
                n += 1
    mm.raise_if_any()
    assert n == len(got)
    return n


def test_units_backward_exact(rt, case):
    """After offk_off_units_train + offk_off_units_backward: dG_<site>, dD_<site>, all 54 (RGB) / 36 (Flow) parameter gradients; a
    second call with accumulate=1 gives exactly twice the reference; offk_off_units_backward_feats in both layouts."""
    c = case
    h = c.handle(rt)
    views = c.views()
    h.off_units_train(c.feats, DROP_SEED, exact.DROP_P)
    poison(h, [("dG_" + s.name, 128) for s in c.sites] + [("dD_" + s.name, 32) for s in c.sites])
    flat = torch.full_like(h.new_unit_grads(), NAN)
    flat, got = h.off_units_backward(c.feats, views, DROP_SEED, exact.DROP_P, grads=flat)
    n = check_backward(h, c.sites, c.ref, got, "off_units_backward")
    assert n == (54 if c.variant == spec.VARIANT_RGB else 36)
    _flat, got2 = h.off_units_backward(c.feats, views, DROP_SEED, exact.DROP_P, grads=flat, accumulate=True)
    check_backward(h, c.sites, c.ref, got2, "off_units_backward(accumulate)", twice=True)
    for layout in ("nchw", "cl"):
        dx = h.off_units_backward_feats(layout=layout)
        torch.cuda.synchronize()
        mm = exact.Mismatches()
        for s, ref, t in zip(c.sites, c.ref, dx):
            assert t.is_contiguous() if layout == "nchw" else t.permute(0, 2, 3, 1).is_contiguous()
            mm.check(t.permute(0, 2, 3, 1).reshape(-1, s.C), ref["dX"], "off_units_backward_feats(%s): dX %s" % (layout, s.name))
        mm.raise_if_any()


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

def conv_inputs(seed, n, Ci, Co, k, H, Ho, x_extra=0):
    x = exact.ints(exact.stream(seed, 8), (n, Ci + x_extra, H, H), -2, 2)
    w = exact.ints(exact.stream(seed, 9), (Co, Ci, k, k), -1, 1)
    b = exact.ints(exact.stream(seed, 10), (Co,), -3, 3)
    res = exact.ints(exact.stream(seed, 11), (n, Co, Ho, Ho), -3, 3)
    return x, w, b, res


def conv_ref(x, w, b, stride, pad, res=None, flags=0):
    """fp64 conv2d with the library's epilogue y = post(pre(conv(in(x)) + bias) + res), after the exactness condition on the data"""
    x, w, b = x.double(), w.double(), b.double()
    if flags & _lib.CONV_RELU_IN:
        x = torch.relu(x)
    cap = F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=pad)
    y = F.conv2d(x, w, b, stride=stride, padding=pad)
    if flags & _lib.CONV_RELU_PRE:
        y = torch.relu(y)
    if res is not None:
        cap, y = cap + res.double().abs(), y + res.double()
    if flags & _lib.CONV_RELU_POST:
        y = torch.relu(y)
    assert float(cap.max()) < exact.LIMIT
    return y.permute(0, 2, 3, 1).contiguous()          # channels-last, as the library writes it


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


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


def gemm_ref(x, w):
    """fp64 product on the device, after the exactness condition on the data"""
    ref = torch.matmul(x.double(), w.double().transpose(1, 2))
    cap = torch.matmul(x.double().abs(), w.double().abs().transpose(1, 2))
    assert float(cap.max()) < exact.LIMIT, float(cap.max())
    return ref


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
