"""The range contract of the training kernels on a device (include/offk.h states it per entry; tests/ranges.py has the draw and the reach):

 1. the wide draw (16 octaves, three in ten zeros, g at 2^-24: gradient-like magnitudes) against fp64: each of the five split training
    entries within the inequality of its own test file, A from that file's emulation on the same operands; the fp32 conv and head entries
    within their derived gamma bounds (tests/test_gpu_conv_bwd.py, tests/test_gpu_head_bwd.py).  No new constant;
 2. tiny operands: split entries with one operand at 2^-100 (its planes reach down to bf16's subnormals) and the other at 2^20, the same
    inequality; fp32 entries with one operand entirely in fp32's subnormal range (exponent field 0) and the other at 2^24, within the
    same gamma bound -- a kernel that flushed subnormals would return zeros;
 3. non-finite values: one +Inf, -Inf or NaN planted at one index of one operand per run (offk_conv2d and the six conv gradients,
    offk_relu_backward, the heads' training forward and backward, the units' training forward, parameter backward and map gradient
    in both arithmetics).
    (i)   nothing is swallowed: every output element the planted element reaches (ranges.reach) is non-finite, NaN on the split entries;
          the documented exceptions are asserted as documented (relu_in / offk_relu_backward / the max-pool count a NaN, and -Inf, as
          not there);
    (ii)  every output of another image (dX), another input channel (dW under an x plant) or another output channel (a g plant) is
          finite and bit-equal to the clean run;
    (iii) the device's non-finite set lies inside the set include/offk.h states for the entry (STATED below): the kernels that remove
          a term by zeroing one operand turn 0 * Inf into NaN in outputs the planted element does not belong to."""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import arena
from . import conv_grad_checks as chk
from .conv_bwd import S1 as cb
from .conv_bwd import S2 as cs2
from . import featmaps as fx
from . import head_bwd as hb
from . import ranges as rg
from . import units_fwd_split as tuf
from . import units_grad as ug
from . import wgrad_split as twg
from .featmaps import rt  # noqa: F401

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
G_SCALE = -24                                  # gradients behind a mean-reduced loss

S1 = [cb.Case(3, 2, 7, 7, 64, 128), cb.Case(1, 3, 7, 7, 128, 64), cb.Case(3, 2, 3, 9, 64, 64)]
S2 = [cb.Case(7, 2, 6, 10, 64, 64), cb.Case(5, 2, 6, 4, 96, 64)]       # (the second: a last ci tile of 32)
# every test prints its measured / bound figures ("RATIO ...", "... / gamma bound", "SET ..."): DESIGN.md 8.6 holds the table of a run


def cuda(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda().contiguous()


def conv_draw(stride, c, seed, x_kw=None, g_kw=None, w_kw=None):
    """x (post-ReLU), g, w from the wide draw; *_kw: another exponent window for that operand"""
    oh, ow = c.H // stride, c.W // stride
    return {"x": rg.wide_t((c.n, c.H, c.W, c.ci), seed, relu=True, **(x_kw or {})), "g": rg.wide_t((c.n, oh, ow, c.co), seed + 1, **(g_kw or {})),
            "w": rg.wide_t((c.co, c.ci, c.k, c.k), seed + 2, **(w_kw or {}))}


def subnormals(shape, seed):
    """fp32 bit patterns with exponent field 0 (tests/test_split_contract.py::_subnormals): 23 random mantissa bits, either sign, 3 in 10 zeros"""
    n = int(np.prod(shape))
    bits = synth.raw_u64(0x5B + 31 * seed, 0, n)
    v = (((bits >> np.uint64(41)).astype(np.uint32)) | (((bits >> np.uint64(3)) & np.uint64(1)).astype(np.uint32) << np.uint32(31))).view(np.float32).copy()
    v[((bits >> np.uint64(8)) % np.uint64(10)) < np.uint64(3)] = 0.0
    assert bool((np.abs(v[v != 0]) < 2.0 ** -126).all()) and (v != 0).mean() > 0.5
    return torch.from_numpy(v.reshape(shape))


def fp32_conv_ratios(rt, what, stride, c, inp):
    """dX, dW, db of the fp32 entries against the fp64 reference (torch, tests/conv_bwd.py) in units of the derived gamma bound"""
    pad = (c.k - 1) // 2
    mod = cb if stride == 1 else cs2
    ref = mod.reference(c, inp, False)
    g, w, x = cuda(inp["g"]), cuda(inp["w"]), cuda(inp["x"])
    if stride == 1:
        dx = rt.conv2d_backward_data(g, w, pad)
        dw, db = rt.conv2d_backward_weight(x, g, c.k, pad)
        terms = {"dX": c.co * c.k * c.k, "dW": c.n * c.H * c.W, "db": c.n * c.H * c.W}
    else:
        dx = rt.conv2d_s2_backward_data(g, w, pad)
        dw, db = rt.conv2d_s2_backward_weight(x, g, c.k, pad)
        px = c.n * (c.H // 2) * (c.W // 2)
        terms = {"dX": cs2.dx_terms(c), "dW": px, "db": px}
    torch.cuda.synchronize()
    out = {}
    for name, t in (("dX", dx), ("dW", dw), ("db", db)):
        assert bool(torch.isfinite(t).all()), name
        err = (t.cpu().double() - ref[name]).abs()
        bound = cb.gamma(terms[name] + 1) * ref[name + "_abs"]
        assert bool((err[bound == 0] == 0).all()), "%s %s: an element without terms is not 0" % (what, name)
        assert bool((ref[name] != 0).any())
        out[name] = float((err / bound.clamp_min(1e-300)).max())
        print("%s %s: largest error / gamma bound %.3f" % (what, name, out[name]))
    return out, (dx, dw, db)


# ---- 1. the wide draw against fp64 ----

@pytest.mark.parametrize("c", S1, ids=cb.case_id)
def test_wide_draw_conv_weight_gradient_split(rt, c):
    inp = conv_draw(1, c, 300 + c.k)
    g = rg.scale(inp["g"], G_SCALE)
    dw, _db = rt.conv2d_backward_weight(cuda(inp["x"]), cuda(g), c.k, (c.k - 1) // 2, arith="f32split")
    torch.cuda.synchronize()
    ce, cg, cf = chk.wgrad_inequality(rt, cb, "wide draw %s" % cb.case_id(c), c, g.numpy(), inp["x"].numpy(), dw)
    print("RATIO conv2d_backward_weight_split %s: gpu accumulation / A = %.3f" % (cb.case_id(c), cg / max(1.0, 2 * ce)))


@pytest.mark.parametrize("c", S2, ids=cs2.case_id)
def test_wide_draw_s2_data_gradient_split(rt, c):
    inp = conv_draw(2, c, 310 + c.k)
    g = rg.scale(inp["g"], G_SCALE)
    dx = rt.conv2d_s2_backward_data(cuda(g), cuda(inp["w"]), (c.k - 1) // 2, arith="f32split")
    torch.cuda.synchronize()
    ce, cg, cf = chk.dgrad_inequality(rt, cs2, "wide draw %s" % cs2.case_id(c), c.k, g.numpy(), inp["w"].numpy(), dx)
    print("RATIO conv2d_s2_backward_data_split %s: gpu accumulation / A = %.3f" % (cs2.case_id(c), cg / max(1.0, 2 * ce)))


@pytest.mark.parametrize("stride,c", [(1, c) for c in S1] + [(2, c) for c in S2], ids=lambda v: cb.case_id(v) if isinstance(v, tuple) else "s%d" % v)
def test_wide_draw_conv_fp32_entries(rt, stride, c):
    inp = conv_draw(stride, c, 320 + c.k)
    inp["g"] = rg.scale(inp["g"], G_SCALE)
    ratios, _ = fp32_conv_ratios(rt, "wide draw s%d %s" % (stride, cb.case_id(c)), stride, c, inp)
    for name, r in ratios.items():
        assert r <= 1.0, "%s: error is %.3f of the derived bound" % (name, r)


def unit_weights(seed, w_kw=None, b_kw=None):
    """synth's weights with the units' two 1x1 matrices and their biases from the wide draw; returns (state dict, [w160], [bias160])"""
    w = synth.make_weights(spec.VARIANT_RGB)
    w160, b160 = [], []
    for si, (name, C, _H) in enumerate(spec.SITES):
        wa = rg.wide((160, C), seed + si, **(w_kw or {}))
        ba = rg.wide((160,), seed + 20 + si, **(b_kw or {}))
        w[tuf.GEN_W % name], w[tuf.DOWN_W % name] = wa[:128].reshape(128, C, 1, 1).copy(), wa[128:].reshape(32, C, 1, 1).copy()
        w[tuf.GEN_B % name], w[tuf.DOWN_B % name] = ba[:128].copy(), ba[128:].copy()
        w160.append(wa)
        b160.append(ba)
    return w, w160, b160


def units_case(rt, tag, map_kw, w_kw, b_kw, g_scale, g_kw=None):
    """B = 1, L = 2: the split training forward, the split weight gradient and the split map gradient on wide operands, each held to the
    inequality of its own test file at all nine sites"""
    B, L, slice_mode = 1, 2, spec.SLICE_FLAT
    P = B * (L - 1)
    w, w160, b160 = unit_weights(400, w_kw, b_kw)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(w) == []
    maps = [cuda(rg.wide((B * L, C, H, H), 440 + si, relu=True, **(map_kw or {}))) for si, (_n, C, H) in enumerate(spec.SITES)]
    h.workspace.fill_(0xff)
    h.off_units_train(maps, fx.DROP_SEED, fx.DROP_P, arith="f32split")
    torch.cuda.synchronize()
    for si, (name, _C, _H) in enumerate(spec.SITES):
        tuf.check_site("%s forward site %s" % (tag, name), h, B, L, slice_mode, si, maps[si], w160[si], b160[si])
    bufs = [cuda(rg.scale(rg.wide_t((P, H, H, C), 460 + i, **(g_kw or {})), g_scale)) for i, (H, C) in enumerate(((28, 320), (14, 1056), (7, 832)))]
    views = [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]
    _, got = h.off_units_backward(maps, views, fx.DROP_SEED, fx.DROP_P, arith="f32split")
    dx = h.off_units_backward_feats(layout="nchw", arith="f32split")
    torch.cuda.synchronize()
    for si, (name, _C, _H) in enumerate(spec.SITES):
        a, x = twg.site_operands(h, B, L, slice_mode, si, maps[si])
        assert float(np.abs(a).max()) > 0
        twg.check_inequality("%s weight gradient site %s" % (tag, name), twg.dw_t(got, si), a, x, twg.KPB[0], max_cols=128)
        a2, wk = ug.dx_operands(h, B, L, slice_mode, si, w160[si][:128], w160[si][128:])
        ug.dx_check_inequality("%s map gradient site %s" % (tag, name), ug.rows_of(dx[si]), a2, wk)


def test_wide_draw_units_split_entries(rt):
    units_case(rt, "wide draw", None, None, None, G_SCALE)


@pytest.mark.parametrize("c", [hb.EXACT_CASES[0], hb.EXACT_CASES[5]], ids=hb.case_id)
def test_wide_draw_heads(rt, c):
    c = c._replace(p=0.8)
    x, w = rg.wide_t((c.n, c.H, c.W, c.C), 500, relu=True), rg.wide_t((c.cls, c.C), 501)
    b, g = rg.wide_t((c.cls,), 502), rg.scale(rg.wide_t((c.n, c.cls), 503), G_SCALE)
    ref = hb.reference(c, x, w, b, g)
    drop = (c.seed, c.p)
    xd, wd = cuda(x), cuda(w)
    out, z = rt.head_train(xd, wd, cuda(b), c.maxpool, c.head, drop)
    dx, dw, db = rt.head_backward(cuda(g), xd, wd, z, c.maxpool, c.head, drop)
    torch.cuda.synchronize()
    nw = hb.nwin(c)
    zd, gd = z.cpu().double(), g.double()
    for name, got, want, mag, k in (("out", out, ref["out"], ref["mag_out"], nw + c.C + 4), ("z", z, ref["z"], ref["z"].abs(), nw + 2),
                                    ("dW", dw, gd.t() @ zd, gd.abs().t() @ zd.abs(), c.n + 1), ("db", db, gd.sum(0), gd.abs().sum(0), c.n + 1),
                                    ("dX", dx, ref["dX"], ref["mag_dX"], c.cls + 5)):
        err = (got.cpu().double() - want).abs()
        bound = hb.gamma(k) * mag
        r = float((err / bound.clamp_min(1e-300)).max())
        print("RATIO head %s %s: largest error / gamma_%d bound %.3f" % (hb.case_id(c), name, k, r))
        assert bool((err <= bound).all()), "%s: %.3f of the derived bound" % (name, r)


# ---- 2. tiny operands ----

TINY = dict(lo=-3, hi=1)                        # times 2^-100: [2^-103, 2^-99), planes down to 2^-126: bf16 subnormals, all above 2^-133
BIG = dict(lo=18, hi=22)


@pytest.mark.parametrize("side", ["g", "x"])
@pytest.mark.parametrize("c", S1, ids=cb.case_id)
def test_tiny_conv_weight_gradient_split(rt, c, side):
    other = "x" if side == "g" else "g"
    inp = conv_draw(1, c, 600 + c.k, **{side + "_kw": TINY, other + "_kw": BIG})
    inp[side] = rg.scale(inp[side], -100)
    assert float(inp[side][inp[side] != 0].abs().min()) >= synth.SPLIT_EXACT_MIN
    dw, _db = rt.conv2d_backward_weight(cuda(inp["x"]), cuda(inp["g"]), c.k, (c.k - 1) // 2, arith="f32split")
    torch.cuda.synchronize()
    assert bool((dw != 0).any())
    chk.wgrad_inequality(rt, cb, "tiny %s %s" % (side, cb.case_id(c)), c, inp["g"].numpy(), inp["x"].numpy(), dw)


@pytest.mark.parametrize("side", ["g", "w"])
@pytest.mark.parametrize("c", S2, ids=cs2.case_id)
def test_tiny_s2_data_gradient_split(rt, c, side):
    other = "w" if side == "g" else "g"
    inp = conv_draw(2, c, 610 + c.k, **{side + "_kw": TINY, other + "_kw": BIG})
    inp[side] = rg.scale(inp[side], -100)
    dx = rt.conv2d_s2_backward_data(cuda(inp["g"]), cuda(inp["w"]), (c.k - 1) // 2, arith="f32split")
    torch.cuda.synchronize()
    assert bool((dx != 0).any())
    chk.dgrad_inequality(rt, cs2, "tiny %s %s" % (side, cs2.case_id(c)), c.k, inp["g"].numpy(), inp["w"].numpy(), dx)


@pytest.mark.parametrize("tiny", ["maps", "gradient"])
def test_tiny_units_split_entries(rt, tiny):
    """tiny maps (and biases) under weights at 2^20: the forward's x planes in bf16's subnormals; a tiny gradient under maps and weights at
    2^20: the a planes of both backward GEMMs"""
    if tiny == "maps":          # (the gradient at 2^20 as well: a 2^-24 gradient on 2^-100 maps would put dW itself under fp32's normal range)
        units_case(rt, "tiny maps", dict(lo=-103, hi=-99), BIG, dict(lo=-83, hi=-79), 0, BIG)
    else:
        units_case(rt, "tiny gradient", BIG, BIG, BIG, -100, TINY)


@pytest.mark.parametrize("side", ["g", "other"])
@pytest.mark.parametrize("stride,c", [(1, S1[0]), (1, S1[1]), (2, S2[0]), (2, S2[1])], ids=lambda v: cb.case_id(v) if isinstance(v, tuple) else "s%d" % v)
def test_subnormal_operands_fp32_conv_entries(rt, stride, c, side):
    """one operand entirely subnormal, the others in [2^24, 2^28): every product is a multiple of 2^-149 * 2^24 and at least 2^-125, so
    the fp64 sums are representable and the gamma bound applies unchanged; a flushing kernel would return zeros"""
    big = dict(lo=24, hi=28)
    inp = conv_draw(stride, c, 620 + c.k, x_kw=big, g_kw=big, w_kw=big)
    names = ("g",) if side == "g" else ("x", "w")
    for i, n in enumerate(names):
        inp[n] = subnormals(tuple(inp[n].shape), 630 + i)
    ratios, outs = fp32_conv_ratios(rt, "subnormal %s s%d %s" % (side, stride, cb.case_id(c)), stride, c, inp)
    for t in outs:
        assert bool((t != 0).any()), "a result of subnormal operands is all zero: flushed"
    for name, r in ratios.items():
        assert r <= 1.0, "%s: error is %.3f of the derived bound" % (name, r)


@pytest.mark.parametrize("side", ["x", "w", "g"])
@pytest.mark.parametrize("c", [hb.EXACT_CASES[0], hb.EXACT_CASES[5]], ids=hb.case_id)
def test_subnormal_operands_heads(rt, c, side):
    c = c._replace(p=0.8)
    big = dict(lo=24, hi=28)
    t = {"x": rg.wide_t((c.n, c.H, c.W, c.C), 640, relu=True, **big), "w": rg.wide_t((c.cls, c.C), 641, **big),
         "b": rg.wide_t((c.cls,), 642, **big), "g": rg.wide_t((c.n, c.cls), 643, **big)}
    t[side] = subnormals(tuple(t[side].shape), 650).abs() if side == "x" else subnormals(tuple(t[side].shape), 650)
    ref = hb.reference(c, t["x"], t["w"], t["b"], t["g"])
    drop = (c.seed, c.p)
    xd, wd = cuda(t["x"]), cuda(t["w"])
    out, z = rt.head_train(xd, wd, cuda(t["b"]), c.maxpool, c.head, drop)
    dx, dw, db = rt.head_backward(cuda(t["g"]), xd, wd, z, c.maxpool, c.head, drop)
    torch.cuda.synchronize()
    nw = hb.nwin(c)
    zd, gd = z.cpu().double(), t["g"].double()
    # where a result itself is subnormal, fp32 keeps it to within half of 2^-149: an absolute term beside the relative bound (a
    # property of the format, not of the kernel; every rounded operation of the chain may add it)
    tiny = 2.0 ** -150
    for name, got, want, mag, k in (("out", out, ref["out"], ref["mag_out"], nw + c.C + 4), ("z", z, ref["z"], ref["z"].abs(), nw + 2),
                                    ("dW", dw, gd.t() @ zd, gd.abs().t() @ zd.abs(), c.n + 1), ("db", db, gd.sum(0), gd.abs().sum(0), c.n + 1),
                                    ("dX", dx, ref["dX"], ref["mag_dX"], c.cls + 5)):
        err = (got.cpu().double() - want).abs()
        bound = hb.gamma(k) * mag + k * tiny
        assert bool(torch.isfinite(got).all()) and bool((err <= bound).all()), "%s: %.3f of the bound" % (name, float((err / bound).max()))
        if bool((want != 0).any()):
            assert bool((got != 0).any()), "%s of a subnormal %s is all zero: flushed" % (name, side)


# ---- 3. non-finite values ----

VALUES = {"+inf": INF, "-inf": -INF, "nan": NAN}


def nonfinite(t):
    return ~torch.isfinite(t.detach().cpu())


def check_plant(what, split, got, clean, need, allowed, isolated):
    """got / clean: dict output -> device tensor of the planted / the clean run; need, allowed, isolated: dict output -> bool mask (CPU):
    need must be non-finite (NaN on a split entry), nothing outside allowed may be, and isolated must be finite and bit-equal to clean"""
    for name, t in got.items():
        bad = nonfinite(t)
        print("SET %s %s: reach %d <= non-finite on the device %d <= stated %d" % (what, name, int(need[name].sum()), int(bad.sum()), int(allowed[name].sum())))
        assert bool(bad[need[name]].all()), "%s %s: %d of the %d elements the plant reaches are finite: swallowed" % (
            what, name, int((~bad[need[name]]).sum()), int(need[name].sum()))
        if split and name != "db":               # (db is an fp32 sum of g itself on the split entry too: +-Inf stays +-Inf)
            assert bool(torch.isnan(t.cpu())[need[name]].all()), "%s %s: a split entry gives NaN, not Inf" % (what, name)
        assert not bool(bad[~allowed[name]].any()), "%s %s: %d non-finite elements outside the set include/offk.h states" % (
            what, name, int(bad[~allowed[name]].sum()))
        assert bool((need[name] <= allowed[name]).all()), "%s %s: the stated set does not hold the reach" % (what, name)
        iso = isolated[name]
        assert not bool((iso & allowed[name]).any())
        assert torch.equal(t.cpu().view(torch.int32)[iso], clean[name].cpu().view(torch.int32)[iso]), "%s %s: an isolated element changed" % (what, name)
        # an element the value does not enter either took a stray NaN (inside the stated set) or is what the clean run gave
        same = ~bad & ~need[name]
        assert torch.equal(t.cpu().view(torch.int32)[same], clean[name].cpu().view(torch.int32)[same]), "%s %s: a finite element outside the reach changed" % (what, name)


def full(shape, value=False):
    return torch.full(tuple(shape), value, dtype=torch.bool)


def s2_rows(c, R, pad):
    """kernel rows kh of a stride-2 conv that read input row R: R = 2 oh + kh - pad with 0 <= oh < H / 2"""
    return [kh for kh in range(c.k) if (R + pad - kh) % 2 == 0 and 0 <= (R + pad - kh) // 2 < c.H // 2]


def stated(entry, c, operand, index):
    """The set include/offk.h states for the entry: dict output -> mask of the elements that MAY be non-finite for a non-finite value at
    `index` of `operand` (the reach is inside it; ranges.reach is the lower side)."""
    k, pad = c.k, (c.k - 1) // 2
    if entry in ("conv2d_backward_weight", "conv2d_s2_backward_weight"):
        dW, db = full((c.co, c.ci, k, k)), full((c.co,))
        if operand == "g" and entry == "conv2d_s2_backward_weight":
            # every kernel row (a row outside the map is a row of zeros times it), but only the column taps whose x column lies inside
            # the map: the wrapped ones are removed by a select on g and stay clean.  Column of tap kw: 2 (ow + fw) + sph, d = kw - pad
            ow, OW = index[2], c.W // 2
            for kw in range(k):
                d = kw - pad
                fw = (d - (d & 1)) // 2
                if 0 <= ow + fw < OW:
                    dW[index[3], :, :, kw] = True
            db[index[3]] = True
        elif operand == "g":                     # every tap of the plant's output channel (0 * Inf on the zero ring), db[co]
            dW[index[3]] = True
            db[index[3]] = True
        elif entry == "conv2d_backward_weight":  # every tap of the plant's input channel: g is zero on the ring around the pixel
            dW[:, index[3]] = True
        else:                                    # stride 2: the kernel rows that read the pixel's row, and in them every kw of the pixel's column parity
            _n, R, C, ci = index
            for kh in s2_rows(c, R, pad):
                for kw in range(k):
                    if (C + pad - kw) % 2 == 0:
                        dW[:, ci, kh, kw] = True
        return {"dW": dW, "db": db}
    dX = full((c.n, c.H, c.W, c.ci))
    if operand == "g":
        return None                              # the footprint itself: the reach
    _co, ci, kh, kw = index
    if entry == "conv2d_backward_data":          # every pixel of the plant's input channel: out-of-map taps multiply it by 0
        dX[..., ci] = True
    else:                                        # stride 2: every pixel of the tap's phase
        dX[:, (kh + pad) % 2::2, (kw + pad) % 2::2, ci] = True
    return {"dX": dX}


def isolation(entry, c, operand, index):
    """(ii): what must stay finite and bit-equal whatever the kernel does inside a tile"""
    if entry in ("conv2d_backward_weight", "conv2d_s2_backward_weight"):
        dW, db = full((c.co, c.ci, c.k, c.k), True), full((c.co,), True)
        if operand == "g":
            dW[index[3]] = False
            db[index[3]] = False
        else:
            dW[:, index[3]] = False
        return {"dW": dW, "db": db}
    dX = full((c.n, c.H, c.W, c.ci), True)
    if operand == "g":
        dX[index[0]] = False
    else:
        dX[..., index[1]] = False
    return {"dX": dX}


def run_conv_entry(rt, entry, arith, c, inp, relu_in=False):
    pad = (c.k - 1) // 2
    x, g, w = cuda(inp["x"]), cuda(inp["g"]), cuda(inp["w"])
    if entry == "conv2d_backward_data":
        out = {"dX": rt.conv2d_backward_data(g, w, pad)}
    elif entry == "conv2d_s2_backward_data":
        out = {"dX": rt.conv2d_s2_backward_data(g, w, pad, arith=arith)}
    elif entry == "conv2d_backward_weight":
        out = dict(zip(("dW", "db"), rt.conv2d_backward_weight(x, g, c.k, pad, relu_in=relu_in, arith=arith)))
    else:
        out = dict(zip(("dW", "db"), rt.conv2d_s2_backward_weight(x, g, c.k, pad, relu_in=relu_in)))
    torch.cuda.synchronize()
    return out


def plant_sites(entry, c, stride):
    """(operand, index): one interior and one border element per operand"""
    oh, ow = c.H // stride, c.W // stride
    sites = [("g", (c.n - 1, oh // 2, ow // 2, 5)), ("g", (0, 0, ow - 1, c.co - 1))]
    if "weight" in entry:
        sites += [("x", (c.n - 1, c.H // 2, c.W // 2, 7)), ("x", (0, c.H - 1, 0, c.ci - 1))]
    else:
        sites += [("w", (5, 7, c.k // 2, c.k // 2)), ("w", (c.co - 1, c.ci - 1, 0, c.k - 1))]
    return sites


CONV_PLANTS = ([("conv2d_backward_data", "fp32", 1, c) for c in S1] + [("conv2d_backward_weight", a, 1, c) for a in ("fp32", "f32split") for c in S1]
               + [("conv2d_s2_backward_data", a, 2, c) for a in ("fp32", "f32split") for c in S2] + [("conv2d_s2_backward_weight", "fp32", 2, c) for c in S2])


@pytest.mark.parametrize("entry,arith,stride,c", CONV_PLANTS, ids=["%s_%s_%s" % (e, a, cb.case_id(c)) for e, a, _s, c in CONV_PLANTS])
def test_nonfinite_conv_entries(rt, entry, arith, stride, c):
    inp = conv_draw(stride, c, 700 + c.k)
    inp["x"] = rg.wide_t(tuple(inp["x"].shape), 705)                   # signed: the relu_in runs below see negatives
    inp["g"] = rg.scale(inp["g"], G_SCALE)
    split = arith == "f32split"
    clean = run_conv_entry(rt, entry, arith, c, inp)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    ref_inp = dict(inp, b=torch.zeros(c.co), stride=stride, pad=(c.k - 1) // 2)
    for operand, index in plant_sites(entry, c, stride):
        need = rg.reach(entry, rg.Plant(ref_inp, operand, index, INF))
        allowed = stated(entry, c, operand, index) or need
        iso = isolation(entry, c, operand, index)
        assert all(bool(need[o].any()) or o == "db" for o in need)
        for vname, value in VALUES.items():
            got = run_conv_entry(rt, entry, arith, c, rg.planted(rg.Plant(inp, operand, index, value)))
            check_plant("%s %s %s, %s at %s%s" % (entry, arith, cb.case_id(c), vname, operand, index), split, got, clean, need, allowed, iso)
    if "weight" in entry:
        # relu_in: the ReLU is max(x, 0) in hardware -- a NaN in x counts as 0 (torch's relu would keep it), and so does -Inf, by definition
        index = (c.n - 1, c.H // 2, c.W // 2, 7)
        zero = run_conv_entry(rt, entry, arith, c, rg.planted(rg.Plant(inp, "x", index, 0.0)), relu_in=True)
        for value in (NAN, -INF):
            got = run_conv_entry(rt, entry, arith, c, rg.planted(rg.Plant(inp, "x", index, value)), relu_in=True)
            for name in got:
                assert arena.same_bits(got[name], zero[name]), "%s %s relu_in: x = %r does not count as 0 in %s" % (entry, arith, value, name)
        got = run_conv_entry(rt, entry, arith, c, rg.planted(rg.Plant(inp, "x", index, INF)), relu_in=True)
        need = rg.reach(entry, rg.Plant(ref_inp, "x", index, INF))
        check_plant("%s %s %s relu_in, +inf at x%s" % (entry, arith, cb.case_id(c), index), split, got, zero, need,
                    stated(entry, c, "x", index), isolation(entry, c, "x", index))


def test_nonfinite_relu_backward(rt):
    """offk_relu_backward selects: dy reaches its own element where y > 0 and nothing else; y = NaN, -Inf give exactly 0, y = +Inf passes dy"""
    dy, y = rg.wide_t((2, 3, 9, 64), 710), rg.wide_t((2, 3, 9, 64), 711)
    clean = rt.relu_backward(cuda(dy), cuda(y)).cpu()
    pos = tuple(int(v) for v in (y > 0).nonzero()[17])
    neg = tuple(int(v) for v in (y <= 0).nonzero()[17])
    for value in VALUES.values():
        for idx in (pos, neg):
            got = rt.relu_backward(cuda(rg.planted(rg.Plant({"g": dy}, "g", idx, value))["g"]), cuda(y)).cpu()
            want = clean.clone()
            want[idx] = value if idx == pos else 0.0
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (value, idx)
        got = rt.relu_backward(cuda(dy), cuda(rg.planted(rg.Plant({"x": y}, "x", neg, value))["x"])).cpu()
        want = clean.clone()
        want[neg] = dy[neg] if value == INF else 0.0
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), ("y", value)


@pytest.mark.parametrize("arith", ["fp32", "f32split"])
def test_nonfinite_units_map_gradient(rt, arith):
    """offk_off_units_backward_feats(_split): dX[n, q, c] = sum_o dGpre[n, q, o] Wg[o, c] + sum_j dD[r(n), q, j] Wd[j, c] on operands written
    straight into the dG_ / dD_ regions (as tests/test_gpu_feat_grad_split.py does).  A value in dGpre or dD reaches all channels of its own
    pixel (dD: of the frame whose row it is) and nothing else; a value in Wg[o, c] channel c of every pixel of every frame; a value in
    Wd[j, c] channel c of the frames inside the slice -- and at most of every frame (a frame outside the slice is a row of zeros times it).
    (2, 3) flat: frames 4 and 5 lie outside the slice; site 3b ends in half a 64-channel tile, site 5a has 49 pixels per frame."""
    B, L, slice_mode = 2, 3, spec.SLICE_FLAT
    N, P = B * L, B * (L - 1)
    w, _w160, _b160 = unit_weights(800)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(w) == []
    maps = [cuda(rg.wide((N, C, H, H), 840 + si, relu=True)) for si, (_n, C, H) in enumerate(spec.SITES)]
    h.off_units(maps)
    h.off_units_backward(maps, ug.random_views(P)[1])             # sets the backward-has-run flag; its dG / dD are replaced below
    fills = [(cuda(rg.scale(rg.wide_t((N * H * H, 128), 860 + si), G_SCALE)), cuda(rg.scale(rg.wide_t((P * H * H, 32), 880 + si), G_SCALE)))
             for si, (_n, _C, H) in enumerate(spec.SITES)]

    def fill():
        for (name, _C, _H), (dg, dd) in zip(spec.SITES, fills):
            h.region("dG_" + name, 128).copy_(dg)
            h.region("dD_" + name, 32).copy_(dd)

    def run():
        dx = h.off_units_backward_feats(layout="nchw", arith=arith)
        torch.cuda.synchronize()
        return [t.cpu() for t in dx]

    fill()
    clean = run()
    assert all(bool(torch.isfinite(t).all()) and bool((t != 0).any()) for t in clean)
    r_of = ug.down_rows(B, L, slice_mode)
    inside = torch.tensor([r >= 0 for r in r_of])
    assert not bool(inside.all())

    def check(what, si, got, need, allowed):
        for sj, (t, c0) in enumerate(zip(got, clean)):
            bad = ~torch.isfinite(t)
            nd = need if sj == si else torch.zeros_like(bad)
            al = allowed if sj == si else torch.zeros_like(bad)
            if sj == si:
                print("SET units map gradient %s %s: reach %d <= non-finite on the device %d <= stated %d" % (arith, what, int(nd.sum()), int(bad.sum()), int(al.sum())))
            assert bool(bad[nd].all()), "%s: swallowed at %d elements" % (what, int((~bad[nd]).sum()))
            if arith == "f32split":
                assert bool(torch.isnan(t)[nd].all()), "%s: a split entry gives NaN" % what
            assert not bool(bad[~al].any()), "%s, site %d: %d non-finite elements outside the stated set" % (what, sj, int(bad[~al].sum()))
            assert torch.equal(t.view(torch.int32)[~al], c0.view(torch.int32)[~al]), "%s, site %d: an element outside the stated set changed" % (what, sj)

    for si in (1, 7):
        name, C, H = spec.SITES[si]
        HW = H * H
        shape = (N, C, H, H)
        for vname, value in VALUES.items():
            n, q, o = 3, HW // 2 + 1, 77
            h.region("dG_" + name, 128)[n * HW + q, o] = value
            need = full(shape)
            need[n, :, q // H, q % H] = True
            check("%s in dGpre[%d, %d, %d] of %s" % (vname, n, q, o, name), si, run(), need, need)
            fill()
            r, j = 2, 5
            h.region("dD_" + name, 32)[r * HW + q, j] = value
            need = full(shape)
            need[r_of.index(r), :, q // H, q % H] = True
            check("%s in dD[%d, %d, %d] of %s" % (vname, r, q, j, name), si, run(), need, need)
            fill()
            for key, row, inner in ((tuf.GEN_W % name, 77, False), (tuf.DOWN_W % name, 5, True)):
                c = C - 3
                w2 = dict(w)
                w2[key] = w[key].copy()
                w2[key][row, c, 0, 0] = value
                assert h.load_state_dict(w2) == []
                need, allowed = full(shape), full(shape)
                need[inside if inner else slice(None), c] = True
                allowed[:, c] = True
                check("%s in %s[%d, %d]" % (vname, key, row, c), si, run(), need, allowed)
                assert h.load_state_dict(w) == []


@pytest.mark.parametrize("stride,c", [(1, S1[0]), (1, S1[1]), (1, S1[2]), (2, S2[0]), (2, S2[1])], ids=lambda v: cb.case_id(v) if isinstance(v, tuple) else "s%d" % v)
def test_nonfinite_conv_forward(rt, stride, c):
    """offk_conv2d, the fusion convs' training forward: y = conv(x, w) + b.  A value in x reaches its footprint in its own image, all output
    channels; a value in w[co, ci, kh, kw] at most every pixel of y[.., co] (the taps that leave the map are zeros times it), a value in
    b[co] every pixel of y[.., co]; other images / other output channels are bit-equal."""
    pad = (c.k - 1) // 2
    oh, ow = c.H // stride, c.W // stride
    inp = conv_draw(stride, c, 730 + c.k)
    inp["x"] = rg.wide_t(tuple(inp["x"].shape), 735)
    inp["b"] = rg.wide_t((c.co,), 736)
    ref_inp = dict(inp, stride=stride, pad=pad)

    def run(v):
        y = rt.conv2d_nhwc(cuda(v["x"]), cuda(v["w"]), cuda(v["b"]), stride, pad)
        torch.cuda.synchronize()
        return {"y": y}

    clean = run(inp)
    assert bool(torch.isfinite(clean["y"]).all())
    sites = [("x", (c.n - 1, c.H // 2, c.W // 2, 7)), ("x", (0, c.H - 1, 0, c.ci - 1)), ("w", (5, 7, c.k // 2, c.k // 2)), ("w", (c.co - 1, c.ci - 1, 0, c.k - 1)),
             ("b", (5,))]
    for operand, index in sites:
        need = rg.reach("conv2d_nhwc", rg.Plant(ref_inp, operand, index, INF))
        allowed, iso = full((c.n, oh, ow, c.co)), full((c.n, oh, ow, c.co), True)
        if operand == "x":
            allowed = need["y"].clone()
            iso[index[0]] = False
        else:
            allowed[..., index[0]] = True
            iso[..., index[0]] = False
        assert bool(need["y"].any())
        for vname, value in VALUES.items():
            got = run(rg.planted(rg.Plant(inp, operand, index, value)))
            check_plant("conv2d_nhwc %s, %s at %s%s" % (cb.case_id(c), vname, operand, index), False, got, clean, need, {"y": allowed}, {"y": iso})


UNIT_PLANT_SITES = (1, 7)       # 3b: 320 channels end in half a 64-channel tile, 28 x 28; 5a: 1024 channels, 49 pixels per frame


def units_plant_setup(rt, seed):
    B, L, slice_mode = 2, 3, spec.SLICE_FLAT
    N = B * L
    w, _w160, _b160 = unit_weights(seed)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, slice_mode, training=True)
    assert h.load_state_dict(w) == []
    maps = [rg.wide_t((N, C, H, H), seed + 40 + si, relu=True) for si, (_n, C, H) in enumerate(spec.SITES)]
    return B, L, slice_mode, w, h, maps


def same_bits_cpu(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("arith", ["fp32", "f32split"])
def test_nonfinite_units_training_forward(rt, arith):
    """offk_off_units_train / offk_off_units_train_split: v = W x + b per pixel, G = max(v, 0) in hardware (128 gen outputs, every frame),
    D = v (32 down outputs, the frames of the slice), then K2 (the depthwise 3x3 on D times the dropout, the temporal difference of G).
      a value in x[n, c, y, x]: D of that pixel non-finite in all 32 channels (NaN in split arithmetic); G of that pixel is +Inf or exactly 0
        in each of its 128 channels -- the hardware max takes a NaN and -Inf as not there; K2 carries the D part into the 3 x 3 neighbourhood
        of the pixel, all 32 spatial channels, of the pair the frame is the spatial row of (non-finite, kept or dropped), and the G part at
        most into the 128 temporal channels of that pixel in the one or two pairs of the clip that hold the frame;
      a value in Wg[o, c] or bg[o]: column o of G is +Inf or 0 (bg[o] = +Inf: +Inf everywhere), at most channel 32 + o of the unit output;
      a value in Wd[j, c] or bd[j]: column j of D non-finite everywhere, at most channel j of the unit output.
    Everything else -- other pixels, other columns, the other eight sites -- is bit-equal to the clean run."""
    B, L, slice_mode, w, h, maps = units_plant_setup(rt, 900)
    N, P = B * L, B * (L - 1)
    split = arith == "f32split"
    r_of = ug.down_rows(B, L, slice_mode)

    def run(weights, feats):
        if weights is not None:
            assert h.load_state_dict(weights) == []
        h.workspace.fill_(0xff)
        h.off_units_train([cuda(f) for f in feats], fx.DROP_SEED, fx.DROP_P, arith=arith)
        torch.cuda.synchronize()
        return dict((k, v.cpu()) for k, v in fx.written(h))

    clean = run(None, maps)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())

    def check(what, si, got, Gal, Dal, Ual, g_inf=False, d_nan=False):
        own = spec.SITES[si][0]
        for name, t in got.items():
            kind, site = name.split("_", 1)
            c0 = clean[name]
            if site != own:
                assert same_bits_cpu(t, c0), "%s: %s of another site changed" % (what, name)
                continue
            bad = ~torch.isfinite(t)
            if kind == "G":
                al = Gal.reshape(t.shape)
                v = t[al]
                assert bool(((v == 0) | (v == INF)).all()), "%s: G holds something other than +Inf or 0 where the value enters" % what
                assert not g_inf or bool((v == INF).all()), "%s: a +Inf bias is swallowed" % what
            elif kind == "D":
                al = Dal.reshape(t.shape)
                assert bool(bad[al].all()), "%s: %d of %d elements of D the value enters are finite" % (what, int((~bad[al]).sum()), int(al.sum()))
                assert not d_nan or bool(torch.isnan(t)[al].all()), "%s: split arithmetic gives NaN in D" % what
            else:
                al = Ual.reshape(t.shape)
                print("SET units forward %s %s: non-finite in the unit output %d <= stated %d" % (arith, what, int(bad.sum()), int(al.sum())))
            assert not bool(bad[~al].any()), "%s: %s non-finite outside the stated set" % (what, name)
            assert torch.equal(t.view(torch.int32)[~al], c0.view(torch.int32)[~al]), "%s: %s changed outside the stated set" % (what, name)

    for si in UNIT_PLANT_SITES:
        name, C, H = spec.SITES[si]
        HW = H * H
        n, c, y, x = 1, C - 3, H // 2, H // 2 + 1
        q = y * H + x
        gen_w, gen_b, down_w, down_b = tuf.GEN_W % name, tuf.GEN_B % name, tuf.DOWN_W % name, tuf.DOWN_B % name
        for vname, value in VALUES.items():
            feats = list(maps)
            feats[si] = maps[si].clone()
            feats[si][n, c, y, x] = value
            Gal, Dal, Ual = full((N, HW, 128)), full((P, HW, 32)), full((P, H, H, 160))
            Gal[n, q] = True
            Dal[r_of[n], q] = True
            Ual[r_of[n], y - 1:y + 2, x - 1:x + 2, :32] = True                  # the depthwise 3 x 3 on D, in the pair the frame is the row of
            Uneed = Ual.clone()                                                 # (0 * NaN under the dropout is NaN: all 288 of them)
            t_in = n % L                                                        # the temporal difference of G: the pairs (t - 1, t) of the clip, that pixel
            Ual[[(n // L) * (L - 1) + t for t in (t_in - 1, t_in) if 0 <= t < L - 1], y, x, 32:] = True
            got = run(None, feats)
            check("%s in x[%d, %d, %d, %d] of %s" % (vname, n, c, y, x, name), si, got, Gal, Dal, Ual, d_nan=split)
            assert bool((~torch.isfinite(got["unit_" + name]))[Uneed].all()), "%s in x: the spatial gradient swallowed it" % vname
            for key, idx, is_gen in ((gen_w, (77, c, 0, 0), True), (gen_b, (77,), True), (down_w, (5, c, 0, 0), False), (down_b, (5,), False)):
                w2 = dict(w)
                w2[key] = w[key].copy()
                w2[key][idx] = value
                Gal, Dal, Ual = full((N, HW, 128)), full((P, HW, 32)), full((P, H, H, 160))
                if is_gen:
                    Gal[..., 77] = True
                    Ual[..., 32 + 77] = True
                else:
                    Dal[..., 5] = True
                    Ual[..., 5] = True
                bias = key.endswith(".bias")
                check("%s in %s%s" % (vname, key, list(idx)), si, run(w2, maps), Gal, Dal, Ual, g_inf=(is_gen and bias and value == INF),
                      d_nan=(split and not bias))
            run(w, maps)


@pytest.mark.parametrize("arith", ["fp32", "f32split"])
def test_nonfinite_units_parameter_backward(rt, arith):
    """offk_off_units_backward / offk_off_units_backward_split (drop_p = 0) behind its own forward.  The parameter gradients read the maps, the
    incoming gradient and the forward's G (as a mask); they do not read Wg, Wd or the biases.
      a value in g, spatial channel j of a site: down.weight[j, :], down.bias[j] and the depthwise conv's weight[j] and bias[j] of that site
        are non-finite (the weight row NaN in split arithmetic), everything else is bit-equal;
      a value in g, temporal channel 32 + o where the forward's G is positive in one of the pair's two frames: gen.weight[o, :] and gen.bias[o];
      a value in x[n, c, y, x] (forward and backward see the same map): gen.weight[:, c], down.weight[:, c] (a frame of the slice) and the
        depthwise weight (D of that pixel is NaN) are non-finite; the rest of the site stays finite -- its values move, the ReLU mask of that
        pixel changed -- and the other eight sites are bit-equal."""
    B, L, slice_mode, w, h, maps = units_plant_setup(rt, 950)
    P = B * (L - 1)
    split = arith == "f32split"
    bufs = [rg.scale(rg.wide_t((P, H, H, C), 990 + i), G_SCALE) for i, (H, C) in enumerate(((28, 320), (14, 1056), (7, 832)))]
    where = {1: (0, 160), 7: (2, 0)}                # site -> (gradient buffer, first channel)

    def run(feats, gb):
        dev = [cuda(f) for f in feats]
        b = [cuda(t) for t in gb]
        views = [(b[0], 0), (b[0], 160)] + [(b[1], 160 * k) for k in range(5)] + [(b[2], 0), (b[2], 160)]
        h.off_units(dev)
        _, gv = h.off_units_backward(dev, views, 0, 0.0, arith=arith)
        torch.cuda.synchronize()
        return dict((k, v.cpu().clone()) for k, v in gv.items())

    clean = run(maps, bufs)
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())

    def check(what, site, got, need, finite_only=()):
        """need: dict key -> mask of the elements that must be non-finite (nothing else may be); finite_only: keys of the site whose other
        elements need only stay finite; every other element of every key is bit-equal to the clean run"""
        for key, t in got.items():
            bad = ~torch.isfinite(t)
            nd = need.get(key, torch.zeros_like(bad))
            assert torch.equal(bad, nd), "%s: %s is non-finite at %d elements, stated %d" % (what, key, int(bad.sum()), int(nd.sum()))
            if split and key.endswith(".weight") and key.startswith(("motion_conv_gen_", "motion_spatial_down_")):
                assert bool(torch.isnan(t)[nd].all()), "%s: split arithmetic gives NaN in %s" % (what, key)
            if key in finite_only:
                continue
            assert torch.equal(t.view(torch.int32)[~nd], clean[key].view(torch.int32)[~nd]), "%s: %s changed outside the stated set" % (what, key)
        print("SET units backward %s %s: %s" % (arith, what, ", ".join("%s %d" % (k, int(m.sum())) for k, m in need.items())))

    for si in UNIT_PLANT_SITES:
        name, C, H = spec.SITES[si]
        HW = H * H
        gen_w, gen_b, down_w, down_b = tuf.GEN_W % name, tuf.GEN_B % name, tuf.DOWN_W % name, tuf.DOWN_B % name
        sg_w, sg_b = "motion_spatial_grad_%s.weight" % name, "motion_spatial_grad_%s.bias" % name
        p, y, x = 1, H // 2, H // 2 + 1
        q = y * H + x
        bi, coff = where[si]
        Gc = h.region("G_" + name, 128).cpu().view(B * L, HW, 128)          # the clean forward's G (the last run above)
        o = int(((Gc[1, q] > 0) | (Gc[2, q] > 0)).nonzero()[0])             # pair 1 = frames 1 and 2 of clip 0
        like = lambda key: torch.zeros_like(clean[key], dtype=torch.bool)   # noqa: E731
        for vname, value in VALUES.items():
            gb = list(bufs)
            gb[bi] = bufs[bi].clone()
            gb[bi][p, y, x, coff + 5] = value
            need = {down_w: like(down_w), down_b: like(down_b), sg_w: like(sg_w), sg_b: like(sg_b)}
            for key in need:
                need[key][5] = True
            check("%s in g[%d, %d, %d, spatial 5] of %s" % (vname, p, y, x, name), name, run(maps, gb), need)
            gb[bi] = bufs[bi].clone()
            gb[bi][p, y, x, coff + 32 + o] = value
            need = {gen_w: like(gen_w), gen_b: like(gen_b)}
            for key in need:
                need[key][o] = True
            check("%s in g[%d, %d, %d, temporal %d] of %s" % (vname, p, y, x, o, name), name, run(maps, gb), need)
            n, c = 1, C - 3
            feats = list(maps)
            feats[si] = maps[si].clone()
            feats[si][n, c, y, x] = value
            need = {gen_w: like(gen_w), down_w: like(down_w), sg_w: like(sg_w)}
            need[gen_w][:, c] = True
            need[down_w][:, c] = True
            need[sg_w][:] = True
            check("%s in x[%d, %d, %d, %d] of %s" % (vname, n, c, y, x, name), name, run(feats, bufs), need,
                  finite_only=(gen_w, gen_b, down_w, down_b, sg_w, sg_b))
        run(maps, bufs)


@pytest.mark.parametrize("c", [hb.EXACT_CASES[0], hb.EXACT_CASES[5]], ids=hb.case_id)
def test_nonfinite_heads(rt, c):
    """The heads have no tiles that zero an operand: the device's non-finite set IS the reach (the fp64 reference of tests/head_bwd.py
    on the planted inputs, Inf and NaN spreading by IEEE rules).  Under the max-pool a NaN or a -Inf in x is not there (fmaxf drops
    the NaN, -Inf is never a maximum of a window with a finite value): asserted finite."""
    c = c._replace(p=0.8)
    t = {"x": rg.wide_t((c.n, c.H, c.W, c.C), 720, relu=True), "w": rg.wide_t((c.cls, c.C), 721), "b": rg.wide_t((c.cls,), 722),
         "g": rg.scale(rg.wide_t((c.n, c.cls), 723), G_SCALE)}
    drop = (c.seed, c.p)

    def run(v):
        xd, wd = cuda(v["x"]), cuda(v["w"])
        out, z = rt.head_train(xd, wd, cuda(v["b"]), c.maxpool, c.head, drop)
        dx, dw, db = rt.head_backward(cuda(v["g"]), xd, wd, z, c.maxpool, c.head, drop)
        torch.cuda.synchronize()
        return {"out": out.cpu(), "z": z.cpu(), "dX": dx.cpu(), "dW": dw.cpu(), "db": db.cpu()}

    def ref(v):
        r = hb.reference(c, v["x"], v["w"], v["b"], v["g"])
        return dict((k, r[k]) for k in ("out", "z", "dX", "dW", "db"))

    clean, clean_ref = run(t), ref(t)
    assert all(bool(torch.isfinite(v).all()) for v in clean.values())
    n = c.n - 1
    sites = [("g", (n, 3)), ("w", (3, 9)), ("b", (3,)), ("x", (n, c.H // 2, c.W // 2, 9)), ("x", (0, c.H - 1, 0, c.C - 1))]
    for operand, index in sites:
        for vname, value in VALUES.items():
            v = rg.planted(rg.Plant(t, operand, index, value))
            got = run(v)
            if operand == "x" and c.maxpool and vname != "+inf":
                # not there: bit-equal to the run with the most negative finite value in that cell (x >= 0 elsewhere: it is never a
                # maximum either).  dX under a NaN only finite: a NaN in a window's FIRST tap keeps the route (no tap compares greater)
                assert all(bool(torch.isfinite(o).all()) for o in got.values()), "max-pool, %s in x" % vname
                low = run(rg.planted(rg.Plant(t, operand, index, -3.4028234663852886e38)))
                for name in got:
                    if name != "dX" or vname == "-inf":
                        assert torch.equal(got[name].view(torch.int32), low[name].view(torch.int32)), "max-pool, %s in x: %s" % (vname, name)
                continue
            want = ref(v)
            for name in got:
                reach = ~torch.isfinite(want[name])
                bad = ~torch.isfinite(got[name])
                if operand == "x" and c.maxpool and name == "dX":
                    # x = +Inf becomes the first maximum of its windows: the ROUTE changes (finite values move), nothing non-finite by it
                    assert not bool(bad.any())
                    continue
                assert torch.equal(bad, reach), "head %s, %s at %s%s: %s is non-finite at %d elements, the reach has %d" % (
                    hb.case_id(c), vname, operand, index, name, int(bad.sum()), int(reach.sum()))
                same = ~reach & (want[name] == clean_ref[name])
                assert torch.equal(got[name].view(torch.int32)[same], clean[name].view(torch.int32)[same]), (name, operand, vname)
            assert bool((~torch.isfinite(want["out"])).any()) or operand == "g"
