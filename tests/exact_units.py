"""What the exact integer-input GPU tests of the OFF units, the direct convs and the batched GEMM share (tests/test_gpu_exact.py,
test_gpu_sobel_taps.py, test_gpu_units_fwd_split.py, test_gpu_wgrad_split.py, test_gpu_feat_grad_split.py, test_gpu_big_slabs.py and
tests/units_grad.py): the Case of one shape (inputs of tests/exact.py, fp64 references on the device), poisoning and the value-for-value
checks of the units' forward and backward, the bodies of the units' exact forward / backward tests as functions of (runtime, case), the
K1b plan read back from the workspace layout, and the integer inputs and fp64 references of the conv and GEMM tests.  A helper module: no
tests of its own."""
import ctypes

import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import _lib, spec

from . import exact
from .forward import make_handle

DROP_SEED = 21
# (workspace region, its channels per pixel, first channel) of every site's unit [S 32 | T 128]
UNIT_SLOTS = [("fusion_28", 320, 0), ("fusion_28", 320, 160)] + [("fusion_14", 1056, 160 * k) for k in range(5)] + [("fusion_7", 832, 0), ("fusion_7", 832, 160)]
NAN = float("nan")


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

    def handle(self, rt, precision="fp32", training=True, env=None):
        return make_handle(rt, self.B, self.L, self.variant, self.slice_mode, weights=self.weights, precision=precision, env=env,
                           training=training)[0]

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


# ---- the units' forward and backward, value for value ----

def units_forward_exact(rt, c, prec):
    """G_<site>, D_<site> and the unit channels of fusion_28/14/7 after the default units call (K1 + K2), the three temporal-difference
    algorithms of K2 over the same G / D, the fused entry (the handle's arithmetic: the 16-pixel fp32 kernel or the split-fp32 plane
    kernel; it leaves G unwritten), a handle created with OFFK_FUSED_UNITS=0, and the training forward at p = 0.5."""
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
    h0 = c.handle(rt, prec, training=False, env={"OFFK_FUSED_UNITS": "0"})
    poison(h0, all_regions(c))
    h0.off_units_fused(c.feats)
    check_forward(h0, c, "off_units_fused, OFFK_FUSED_UNITS=0")


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


def units_backward_exact(rt, c):
    """After offk_off_units_train + offk_off_units_backward: dG_<site>, dD_<site>, all 54 (RGB) / 36 (Flow) parameter gradients; a
    second call with accumulate=1 gives exactly twice the reference; offk_off_units_backward_feats in both layouts."""
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


# ---- offk_conv2d_ex, offk_batched_gemm_nt ----

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


def gemm_ref(x, w):
    """fp64 product on the device, after the exactness condition on the data"""
    ref = torch.matmul(x.double(), w.double().transpose(1, 2))
    cap = torch.matmul(x.double().abs(), w.double().abs().transpose(1, 2))
    assert float(cap.max()) < exact.LIMIT, float(cap.max())
    return ref
