"""The range tests' own foundations, on the CPU (tests/ranges.py; the GPU files are tests/test_gpu_scale_equivariance.py and
tests/test_gpu_train_ranges.py):

 1. the wide draw is what it says (16 octaves, 23 mantissa bits, three in ten zeros, seeded) and synth.cut3 is exact on it at 2^+-24;
 2. the CPU model of the split arithmetic -- synth.emulate_split_dot in both forms and the four kernel emulations built on it -- is
    scale-equivariant BIT FOR BIT in either operand at a = -24, +1, +24;
 3. mutants of the model that the GPU equivariance test is there to catch break that equality on more than half of the outputs at
    a = -24 or +24: a plane through fp16, planes below 2^-30 flushed, a constant 2^-20 added once per output.  The fp16 mutant shows
    nothing at a = +1 -- which is why the sweep is +-24.  A fourth candidate, "the last plane rounded to nearest where the code
    truncates", is NOT a mutant: the remainder behind two 8-bit cuts of a 24-bit significand has at most 8 significant bits, so it is a
    bf16 value already and every rounding mode returns it unchanged (asserted);
 4. the project's inequality |out - ref64| <= |dropped| + A 2^-24 sum|.| + 2^-24 |ref64|, A = max(1, 2 c_acc) of the intact emulation,
    holds on the wide draw, and losing any one of the six kept products violates it on more than half of the outputs;
 5. the table of degrees agrees with the fp64 references: an operand class times 2^3 multiplies the output by exactly 2^(3 degree)."""
import contextlib

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

from . import conv_s2_dgrad_split as ds
from . import conv_wgrad_split as cw
from . import head_bwd as hb
from . import ranges as rg
from . import units_fwd_split as uf
from . import wgrad_split as wg

EPS = synth.SPLIT_EPS
SCALES = (-24, 1, 24)


# ---- 1. the draw ----

def test_wide_draw():
    v = rg.wide((64, 1024), 5)
    assert v.dtype == np.float32 and v.shape == (64, 1024)
    assert np.array_equal(v, rg.wide((64, 1024), 5)) and not np.array_equal(v, rg.wide((64, 1024), 6))
    nz = v != 0
    assert 0.28 < 1.0 - nz.mean() < 0.32, "three in ten are exact zeros"
    a = np.abs(v[nz])
    assert a.min() >= 2.0 ** -12 and a.max() < 2.0 ** 4
    octave = np.frexp(a)[1]
    counts = np.bincount(octave - octave.min())
    assert len(counts) == 16 and counts.min() > 0.8 * nz.sum() / 16 and counts.max() < 1.2 * nz.sum() / 16, "uniform over 16 octaves"
    assert 0.48 < (v[nz] < 0).mean() < 0.52
    mant = v[nz].view(np.uint32) & np.uint32(0x7FFFFF)
    for bit in range(23):
        assert 0.47 < ((mant >> np.uint32(bit)) & 1).mean() < 0.53, "mantissa bit %d is not random" % bit
    r = rg.wide((64, 1024), 5, relu=True)
    assert (r >= 0).all() and np.array_equal(r[v > 0], v[v > 0]) and not r[v <= 0].any()
    s = rg.wide((4096,), 9, lo=-3, hi=3)
    assert np.abs(s[s != 0]).min() >= 0.125 and np.abs(s).max() < 8.0


def test_scale_is_exact_and_says_when_it_is_not():
    v = rg.wide((4096,), 1)
    for a in SCALES:
        s = rg.scale(v, a)
        assert np.array_equal(s.astype(np.float64), v.astype(np.float64) * 2.0 ** a)
        t = rg.scale(torch.from_numpy(v), a)
        assert np.array_equal(t.numpy(), s)
    with pytest.raises(AssertionError):
        rg.scale(v, -130)                       # into the subnormals: bits are lost
    with pytest.raises(AssertionError):
        rg.scale(torch.from_numpy(v).half(), 24)


def test_cut_is_exact_on_the_scaled_draw():
    v = rg.wide((1 << 16,), 2)
    h0, m0, l0 = synth.cut3(v)
    assert (l0 != 0).mean() > 0.5
    for a in SCALES:
        s = rg.scale(v, a)
        h, m, l = synth.cut3(s)
        assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), s.astype(np.float64))
        for p, p0 in ((h, h0), (m, m0), (l, l0)):
            assert np.array_equal(p, rg.scale(p0, a)), "the cut commutes with 2^%d" % a


# ---- 2. the emulations are equivariant ----

def operands(N=40, M=48, K=96, seed=11):
    return rg.wide((N, K), seed), rg.wide((M, K), seed + 1, relu=True)


def emu_dot(form):
    return lambda w, x: synth.emulate_split_dot(w, x, form)


def emu_conv_wgrad(k):
    n, H, W, ci, co = 2, 3, 9, 8, 8

    def run(gflat, xflat):
        g, x = gflat.reshape(n, H, W, co), xflat.reshape(n, H, W, ci)
        G, taps = cw.operands(g, x, k)
        return cw.emulate_chunked(G, taps, cw.chunk_bounds(n, H, W, k, 2), k)
    return run, (n * H * W * co,), (n * H * W * ci,)


def emu_s2_dgrad(k):
    n, OH, OW, ci, co = 1, 3, 2, 8, 64

    def run(wflat, gflat):
        return ds.emulate(gflat.reshape(n, OH, OW, co), wflat.reshape(co, ci, k, k))
    return run, (co * ci * k * k,), (n * OH * OW * co,)


def emu_units_wgrad():
    def run(a, x):
        return wg.emulate_chunked(wg.pad_ktiles(a.reshape(2, 49, 160)), wg.pad_ktiles(x.reshape(2, 49, 24)), 2)
    return run, (2 * 49 * 160,), (2 * 49 * 24,)


def emu_units_fwd():
    bias = rg.wide((160,), 77)

    def run(w, x, a_bias=0):
        return uf.emulate(w.reshape(160, 64), x.reshape(40, 64), bias=rg.scale(bias, a_bias))
    return run, (160 * 64,), (40 * 64,)


EMULATIONS = {
    "dot_units": lambda: (emu_dot("units"), (40, 96), (48, 96)),
    "dot_gemm": lambda: (emu_dot("gemm"), (40, 96), (48, 96)),
    "conv_wgrad_k3": lambda: emu_conv_wgrad(3),
    "conv_wgrad_k1": lambda: emu_conv_wgrad(1),
    "conv_s2_dgrad_k5": lambda: emu_s2_dgrad(5),
    "conv_s2_dgrad_k7": lambda: emu_s2_dgrad(7),
    "units_wgrad": emu_units_wgrad,
    "units_fwd": emu_units_fwd,
}


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b)) and bool(np.isfinite(np.asarray(a)).all())


@pytest.mark.parametrize("name", list(EMULATIONS))
def test_emulations_are_bit_equivariant(name):
    run, s0, s1 = EMULATIONS[name]()
    p, q = rg.wide(s0, 21), rg.wide(s1, 22, relu=True)
    base = run(p, q)
    assert (base != 0).mean() > 0.5 and rg.base_in_range(base)
    for a in SCALES:
        if name == "units_fwd":                       # affine: the bias goes with whichever operand is scaled
            assert same(run(rg.scale(p, a), q, a), rg.scale(base, a)) and same(run(p, rg.scale(q, a), a), rg.scale(base, a)), a
        else:
            assert same(run(rg.scale(p, a), q), rg.scale(base, a)), "first operand, a = %d" % a
            assert same(run(p, rg.scale(q, a)), rg.scale(base, a)), "second operand, a = %d" % a


# ---- 3. the mutants ----

def rne_bf16(v):
    """fp32 -> the nearest bf16 value (ties to even), as fp32"""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32)


def cut_fp16(x):
    h, m, l = CUT3(x)
    with np.errstate(over="ignore"):
        return h.astype(np.float16).astype(np.float32), m, l


def cut_flush(x):
    return tuple(np.where(np.abs(p) < np.float32(2.0 ** -30), np.float32(0), p) for p in CUT3(x))


def cut_rne_last(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    h, m, _l = CUT3(x)
    return h, m, rne_bf16((x - h) - m)


CUT3 = synth.cut3


@contextlib.contextmanager
def mutant_cut(cut):
    synth.cut3 = cut
    try:
        yield
    finally:
        synth.cut3 = CUT3


def mutant_run(kind, form):
    if kind == "plus_2^-20":
        return lambda w, x: synth.emulate_split_dot(w, x, form) + np.float32(2.0 ** -20)

    def run(w, x):
        with mutant_cut({"fp16_plane": cut_fp16, "flush_2^-30": cut_flush, "rne_last_plane": cut_rne_last}[kind]):
            return synth.emulate_split_dot(w, x, form)
    return run


def broken_fraction(run, w, x, a, side):
    """the fraction of outputs at which run(scaled) differs from run(base) * 2^a (a non-finite value differs)"""
    base = run(w, x)
    with np.errstate(over="ignore", invalid="ignore"):
        got = run(rg.scale(w, a), x) if side == "w" else run(w, rg.scale(x, a))
        want = base * np.float32(2.0 ** a)
    return float(((got != want) | ~np.isfinite(got)).mean())


@pytest.mark.parametrize("form", ["units", "gemm"])
@pytest.mark.parametrize("kind", ["fp16_plane", "flush_2^-30", "plus_2^-20"])
def test_mutants_break_the_equality_at_24(kind, form):
    w, x = operands()
    run = mutant_run(kind, form)
    for side in ("w", "x"):
        frac = dict((a, broken_fraction(run, w, x, a, side)) for a in SCALES)
        print("%s %s, %s scaled: broken outputs at a = -24 / +1 / +24: %.3f / %.3f / %.3f" % (kind, form, side, frac[-24], frac[1], frac[24]))
        assert max(frac[-24], frac[24]) > 0.5, (kind, form, side, frac)
        if kind == "fp16_plane":
            assert frac[1] == 0.0, "a plane of 8 significant bits in [2^-12, 2^5) is an fp16 value: a = +1 cannot see this mutant"
    assert broken_fraction(emu_dot(form), w, x, 24, "w") == 0.0, "the intact emulation under the same measure"


def test_flush_mutant_is_almost_invisible_at_plus_1():
    """Planes below 2^-30 flushed: at a = +1 only the planes within one octave of the threshold change, each by less than 2^-29 under outputs of
    order 1 and more -- a handful of outputs move.  At +-24 every last plane crosses the threshold (or none does where some did)."""
    w, x = operands()
    for form in ("units", "gemm"):
        run = mutant_run("flush_2^-30", form)
        lo = max(broken_fraction(run, w, x, 1, s) for s in ("w", "x"))
        hi = min(max(broken_fraction(run, w, x, a, s) for a in (-24, 24)) for s in ("w", "x"))
        print("flush mutant, %s: broken at a = +1 %.4f, at +-24 %.3f" % (form, lo, hi))
        assert lo < 0.05 and hi > 0.5


def test_rounding_the_last_plane_is_no_mutant():
    v = np.concatenate([rg.scale(rg.wide((1 << 16,), 3), a) for a in (0,) + SCALES])
    for got, want in zip(cut_rne_last(v), synth.cut3(v)):
        assert np.array_equal(got, want), "the remainder behind two cuts is a bf16 value: rounding it changes nothing"
    x = np.ascontiguousarray(v)
    h, m, _ = synth.cut3(x)
    assert not np.any(((x - h) - m).view(np.uint32) & np.uint32(0xFFFF))
    # rounding the MIDDLE plane instead does change the cut, and commutes with 2^a like the truncation does: not a range fault either
    assert not np.array_equal(rne_bf16(x - h), m)


# ---- 4. the inequality on the wide draw ----

@pytest.mark.parametrize("form", ["units", "gemm"])
@pytest.mark.parametrize("a", (0,) + SCALES)
def test_inequality_holds_on_the_wide_draw_and_sees_a_lost_product(form, a):
    w, x = operands(K=256, seed=31)
    w = rg.scale(w, a)
    ref, dropped, mag = synth.split_terms(w, x)
    good = synth.emulate_split_dot(w, x, form)
    c = float(synth.split_c_acc(good, ref, dropped, mag).max())
    A = max(1.0, 2.0 * c)
    limit = np.abs(dropped) + A * EPS * mag + EPS * np.abs(ref)
    print("wide draw, %s, a = %d: c_acc %.3f, A %.3f, dropped / (2^-24 mag) max %.3f" % (form, a, c, A, float((np.abs(dropped) / (EPS * mag)).max())))
    assert c < 8.0 and np.all(np.abs(dropped) <= synth.SPLIT_DROP_BOUND * EPS * mag)
    assert np.all(np.abs(good.astype(np.float64) - ref) <= limit)
    for skip in range(6):
        bad = synth.emulate_split_dot(w, x, form, skip=skip)
        viol = np.abs(bad.astype(np.float64) - ref) > limit
        assert viol.mean() > 0.5, (form, skip, synth.SPLIT_PRODUCTS[skip], float(viol.mean()))


# ---- 5. the degrees ----

A3 = 3


def conv_inputs(stride, k, relu_in, seed):
    n, H, W, ci, co = 2, 4, 6, 8, 8
    pad = (k - 1) // 2
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return {"x": rg.wide_t((n, H, W, ci), seed), "w": rg.wide_t((co, ci, k, k), seed + 1), "b": rg.wide_t((co,), seed + 2),
            "g": rg.wide_t((n, OH, OW, co), seed + 3), "stride": stride, "pad": pad, "relu_in": relu_in}


def conv_out(inp):
    return rg.conv_ref64(inp["x"], inp["w"], inp["b"], inp["g"], inp["stride"], inp["pad"], relu_in=inp["relu_in"], relu=True)


@pytest.mark.parametrize("entry,stride,k", [("conv2d_backward_data", 1, 3), ("conv2d_backward_weight", 1, 3), ("conv2d_backward_weight", 1, 1),
                                            ("conv2d_s2_backward_data", 2, 5), ("conv2d_s2_backward_weight", 2, 7)])
@pytest.mark.parametrize("relu_in", [False, True])
def test_degrees_of_the_conv_gradients(entry, stride, k, relu_in):
    inp = conv_inputs(stride, k, relu_in, 40 + k)
    base = conv_out(inp)
    for out, table in rg.degrees[entry].items():
        for cls in ("x", "w", "g"):
            scaled = conv_out(dict(inp, **{cls: rg.scale(inp[cls], A3)}))
            assert bool((base[out] != 0).any())
            assert torch.equal(scaled[out], base[out] * 2.0 ** (A3 * table[cls])), (entry, out, cls)


def test_degrees_of_the_conv_forward_and_relu_backward():
    inp = conv_inputs(1, 3, True, 50)
    res = rg.wide_t(tuple(inp["g"].shape), 54)
    y = lambda i, r: rg.conv_ref64(i["x"], i["w"], i["b"], i["g"], 1, 1, relu_in=True, relu=True, res=r)["y"]      # noqa: E731
    base = y(inp, res)
    assert bool((base > 0).any()) and bool((base == 0).any())
    d = rg.degrees["conv2d_nhwc"]["y"]
    assert torch.equal(y(dict(inp, x=rg.scale(inp["x"], A3), b=rg.scale(inp["b"], A3)), rg.scale(res, A3)), base * 2.0 ** (A3 * d["x+b"]))
    assert torch.equal(y(dict(inp, w=rg.scale(inp["w"], A3), b=rg.scale(inp["b"], A3)), rg.scale(res, A3)), base * 2.0 ** (A3 * d["w+b"]))
    assert not torch.equal(y(dict(inp, x=rg.scale(inp["x"], A3)), res), base * 2.0 ** A3), "x alone: the bias does not follow"
    rb = lambda g, yy: rg._entry_ref("relu_backward", {"g": g, "x": yy})["out"]                                      # noqa: E731
    g, yy = rg.wide_t((2, 3, 4, 8), 55), rg.wide_t((2, 3, 4, 8), 56)
    d = rg.degrees["relu_backward"]["out"]
    assert torch.equal(rb(rg.scale(g, A3), yy), rb(g, yy) * 2.0 ** (A3 * d["g"])) and torch.equal(rb(g, rg.scale(yy, A3)), rb(g, yy) * 2.0 ** (A3 * d["x"]))


def test_reach_is_the_definition_not_the_padding():
    """ranges.reach on a 7x7 / 2 / 3 conv: an x pixel reaches the taps that read it, all output channels, its own input channel; a g
    element reaches its own output channel.  The IEEE form (the planted Inf itself) agrees for x -- and says every tap for g, 0 * Inf on
    the zero padding torch materialises: more than the operation's definition, which is why the GPU test asks the default form."""
    inp = conv_inputs(2, 7, False, 90)
    n, H, W, ci = inp["x"].shape
    co, OH, OW = inp["w"].shape[0], H // 2, W // 2
    for R, C in ((0, 0), (1, 2), (H - 1, W - 1)):
        r = rg.reach("conv2d_s2_backward_weight", rg.Plant(inp, "x", (1, R, C, 3), float("inf")))
        want = torch.zeros(co, ci, 7, 7, dtype=torch.bool)
        for kh in range(7):
            for kw in range(7):
                oh, ow = R + 3 - kh, C + 3 - kw
                if oh % 2 == 0 and ow % 2 == 0 and 0 <= oh // 2 < OH and 0 <= ow // 2 < OW:
                    want[:, 3, kh, kw] = True
        assert torch.equal(r["dW"], want) and not bool(r["db"].any())
        ieee = rg.reach("conv2d_s2_backward_weight", rg.Plant(inp, "x", (1, R, C, 3), float("inf")), ieee=True)
        assert torch.equal(ieee["dW"], want)
    g = rg.reach("conv2d_s2_backward_weight", rg.Plant(inp, "g", (0, 0, OW - 1, 5), float("nan")))
    assert bool(g["dW"][5].any()) and not bool(g["dW"][5].all()) and not bool(g["dW"][:5].any()) and g["db"].tolist() == [i == 5 for i in range(co)]
    gi = rg.reach("conv2d_s2_backward_weight", rg.Plant(inp, "g", (0, 0, OW - 1, 5), float("nan")), ieee=True)
    assert bool(gi["dW"][5].all()) and bool((g["dW"] <= gi["dW"]).all())
    d = rg.reach("conv2d_s2_backward_data", rg.Plant(inp, "g", (1, 1, 1, 2), float("inf")))
    assert bool(d["dX"][1].all()) and not bool(d["dX"][0].any()), "a 7x7 footprint covers the whole 4x6 map of its own image"
    d5 = rg.reach("conv2d_s2_backward_data", rg.Plant(conv_inputs(2, 5, False, 93), "w", (2, 3, 0, 4), float("inf")))
    assert bool(d5["dX"][..., 3].any()) and not bool(d5["dX"][..., 3].all()) and not bool(d5["dX"][..., :3].any())
    rb = rg.reach("relu_backward", rg.Plant({"g": rg.wide_t((2, 8), 91), "x": rg.wide_t((2, 8), 92)}, "g", (1, 3), 1.0))
    assert int(rb["out"].sum()) == 1 and bool(rb["out"][1, 3])


@pytest.mark.parametrize("c", hb.EXACT_CASES[:1] + hb.EXACT_CASES[5:6], ids=hb.case_id)
def test_degrees_of_the_heads(c):
    c = c._replace(p=0.8)
    x, w = rg.wide_t((c.n, c.H, c.W, c.C), 60, relu=True), rg.wide_t((c.cls, c.C), 61)
    b, g = rg.wide_t((c.cls,), 62), rg.wide_t((c.n, c.cls), 63)
    base = hb.reference(c, x, w, b, g)
    s = 2.0 ** A3
    runs = {"x+b": hb.reference(c, rg.scale(x, A3), w, rg.scale(b, A3), g), "w+b": hb.reference(c, x, rg.scale(w, A3), rg.scale(b, A3), g),
            "g": hb.reference(c, x, w, b, rg.scale(g, A3))}
    fwd, bwd = rg.degrees["head_train"], rg.degrees["head_backward"]
    for cls in ("x+b", "w+b"):
        assert torch.equal(runs[cls]["out"], base["out"] * s ** fwd["out"][cls]) and torch.equal(runs[cls]["z"], base["z"] * s ** fwd["z"][cls])
    for out in ("dX", "dW", "db"):
        assert bool((base[out] != 0).any())
        assert torch.equal(runs["g"][out], base[out] * s ** bwd[out]["g"]), out
        assert torch.equal(runs["x+b"][out], base[out] * s ** bwd[out]["x"]), out
        assert torch.equal(runs["w+b"][out], base[out] * s ** bwd[out]["w"]), out
    assert torch.equal(runs["x+b"]["dX"] != 0, base["dX"] != 0), "the max-pool selects the same cells"


def test_degrees_of_the_units_and_the_forward():
    B, L, variant = 1, 2, spec.VARIANT_RGB
    w = dict((k, v.double()) for k, v in orc.to_torch_weights(synth.make_weights(variant)).items())
    feats = [torch.from_numpy(f * rg.wide(f.shape, 70 + i, lo=-4, hi=4)).double() for i, f in enumerate(synth.make_features(B, L, 9))]
    s = 2.0 ** A3
    wb = dict((k, v * s if k.endswith(".bias") else v) for k, v in w.items())
    first = ("motion_conv_gen_", "motion_spatial_down_")
    w1b = dict((k, v * s if k.endswith(".bias") or (k.endswith(".weight") and k.startswith(first)) else v) for k, v in w.items())
    with torch.no_grad():
        base = orc.off_forward(feats, w, B, L, variant)
        xb = orc.off_forward([f * s for f in feats], wb, B, L, variant)
        w1 = orc.off_forward(feats, w1b, B, L, variant)
    d = rg.degrees["forward"]["logits"]
    for o, a, b in zip(base, xb, w1):
        assert bool((o != 0).any())
        assert torch.equal(a, o * s ** d["x+b"]) and torch.equal(b, o * s ** d["w1+b"])
    # the units' gradients: dM scaled -> every parameter gradient scaled; maps and biases scaled -> dW scaled, db unchanged
    P = B * (L - 1)
    dm = [torch.from_numpy(rg.wide((P, 160, H, H), 80 + i)).double() for i, (_n, _c, H) in enumerate(spec.SITES)]
    g0 = orc.unit_param_grads_from_dm(feats, w, B, L, variant, spec.SLICE_FLAT, dm)
    gg = orc.unit_param_grads_from_dm(feats, w, B, L, variant, spec.SLICE_FLAT, [t * s for t in dm])
    gx = orc.unit_param_grads_from_dm([f * s for f in feats], wb, B, L, variant, spec.SLICE_FLAT, dm)
    t = rg.degrees["off_units_backward"]
    for key in g0:
        kind = "db" if key.endswith(".bias") else "dW"
        assert bool((g0[key] != 0).any()), key
        assert torch.equal(gg[key], g0[key] * s ** t[kind]["g"]) and torch.equal(gx[key], g0[key] * s ** t[kind]["x+b"]), key
