"""Scale equivariance, bit for bit, of the inference forward and of every training entry (tests/ranges.py has the argument and the table of
degrees; tests/test_range_cases.py shows on the CPU what the check can see).

Every case runs twice: on the base operands and with one operand class multiplied by 2^a, a = -24 and +24 (and a = +1 on one case per
entry as a cheap sanity check).  Every output must be EQUAL IN VALUE, with no non-finite value, to the base output times
2^(a degree).  No tolerance, no reference, no composed bound.  Before comparing, the base run's non-zero |outputs| are asserted to lie in
[2^-90, 2^90] -- a condition on the inputs (it leaves 12 octaves to 2^+-126 after scaling), not a tolerance.

Operands come from ranges.wide: 16 octaves, 23 random mantissa bits, three in ten exact zeros.  What an exact check of this kind sees
that an inequality against fp64 lets through: an fp16 or rounded-bf16 intermediate, a flushed plane, a stale or uninitialised value
added into a sum, an absolute threshold, a derived weight that is not re-derived."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from .conv_bwd import S1 as cb
from . import featmaps as fx
from . import head_bwd as hb
from . import ranges as rg
from .featmaps import rt  # noqa: F401
from .forward import HEAD_PATHS as PATHS

pytestmark = pytest.mark.gpu
SWEEP = rg.SWEEP


def sweep(sanity):
    return SWEEP + ((rg.SANITY,) if sanity else ())


def cuda(t):
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t).cuda().contiguous()


def check_outputs(what, base, got, factors):
    """base, got: dict name -> tensor; factors: dict name -> the exponent a * degree"""
    bad = []
    for name, b in base.items():
        if b is None:
            continue
        g = got[name]
        if not rg.same_values(g.float() if g.dtype != torch.float32 else g, b.float() if b.dtype != torch.float32 else b, factors[name]):
            gf, want = g.detach().float().cpu(), rg.scale(b.detach().float().cpu(), factors[name])
            diff = gf != want
            bad.append("%s: %d of %d elements differ from base * 2^%d (%d non-finite); first at %d: got %r, want %r" % (
                name, int(diff.sum()), diff.numel(), factors[name], int((~torch.isfinite(gf)).sum()), int(diff.flatten().nonzero()[0]),
                float(gf.flatten()[diff.flatten()][0]), float(want.flatten()[diff.flatten()][0])))
    assert not bad, "%s: %s" % (what, "; ".join(bad))


def check_base(what, base, some_zero_ok=()):
    for name, b in base.items():
        if b is None:
            continue
        assert rg.base_in_range(b.float()), "%s %s: the base run leaves [2^-90, 2^90]" % (what, name)
        assert name in some_zero_ok or bool((b != 0).any()), "%s %s: all zero" % (what, name)


def run_entry(what, run, ops, classes, degs, olds=None, sanity=False):
    """run(ops, olds) -> dict of outputs.  ops: dict name -> CPU tensor; classes: dict class -> the operand names scaled together;
    degs: dict output -> dict class -> degree; olds: dict output -> CPU tensor an accumulating call adds to (scaled by the output's factor)"""
    olds = olds or {}
    base = run(ops, olds)
    torch.cuda.synchronize()
    check_base(what, base)
    for cls, names in classes.items():
        for a in sweep(sanity):
            sc = dict(ops, **dict((n, rg.scale(ops[n], a)) for n in names))
            so = dict((o, rg.scale(t, a * degs[o][cls])) for o, t in olds.items())
            got = run(sc, so)
            torch.cuda.synchronize()
            check_outputs("%s, %s * 2^%d" % (what, cls, a), base, got, dict((o, a * degs[o][cls]) for o in base))


# ---- fusion convs ----

S1 = [cb.Case(3, 2, 7, 7, 64, 128), cb.Case(1, 3, 7, 7, 128, 64), cb.Case(3, 2, 3, 9, 64, 64)]       # the last: three rows of W = 9 straddle the pitch of 16
S2 = [cb.Case(7, 2, 6, 10, 64, 64), cb.Case(5, 2, 6, 4, 96, 64)]
CONVS = [(1, c) for c in S1] + [(2, c) for c in S2]
CONV_IDS = ["s%d_%s" % (s, cb.case_id(c)) for s, c in CONVS]


def conv_ops(stride, c, signed_x, seed):
    oh, ow = c.H // stride, c.W // stride
    return {"x": rg.wide_t((c.n, c.H, c.W, c.ci), seed, relu=not signed_x), "w": rg.wide_t((c.co, c.ci, c.k, c.k), seed + 1),
            "b": rg.wide_t((c.co,), seed + 2), "g": rg.wide_t((c.n, oh, ow, c.co), seed + 3), "res": rg.wide_t((c.n, oh, ow, c.co), seed + 4)}


@pytest.mark.parametrize("mode", ["plain", "res_relu", "relu_in"])
@pytest.mark.parametrize("stride,c", CONVS, ids=CONV_IDS)
def test_conv_forward(rt, stride, c, mode):
    pad = (c.k - 1) // 2
    ops = conv_ops(stride, c, mode == "relu_in", 100 + c.k)
    flags = {"plain": 0, "res_relu": _lib.CONV_RELU_POST, "relu_in": _lib.CONV_RELU_IN | _lib.CONV_RELU_POST}[mode]

    def run(o, _olds):
        res = cuda(o["res"]) if mode == "res_relu" else None
        return {"y": rt.conv2d_nhwc(cuda(o["x"]), cuda(o["w"]), cuda(o["b"]), stride, pad, res=res, flags=flags)}

    run_entry("conv2d_nhwc %s %s" % (cb.case_id(c), mode), run, ops, {"x+b": ("x", "b", "res"), "w+b": ("w", "b", "res")},
              rg.degrees["conv2d_nhwc"], sanity=(c is S1[0] or c is S2[0]))


def test_relu_backward(rt):
    ops = {"g": rg.wide_t((2, 3, 9, 64), 110), "x": rg.wide_t((2, 3, 9, 64), 111)}
    old = {"out": rg.wide_t((2, 3, 9, 64), 112)}
    for accumulate in (False, True):
        def run(o, olds):
            out = cuda(olds["out"]) if accumulate else None
            return {"out": rt.relu_backward(cuda(o["g"]), cuda(o["x"]), out=out, accumulate=accumulate)}
        run_entry("relu_backward", run, ops, {"g": ("g",), "x": ("x",)}, rg.degrees["relu_backward"], old if accumulate else None, sanity=True)


DGRADS = [(s, c, "fp32") for s, c in CONVS] + [(2, c, "f32split") for c in S2]           # the stride-1 data gradient has no split form
WGRADS = [(s, c, "fp32") for s, c in CONVS] + [(1, c, "f32split") for c in S1]           # the stride-2 weight gradient has none


def arith_ids(cases):
    return ["s%d_%s_%s" % (s, cb.case_id(c), a) for s, c, a in cases]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("stride,c,arith", DGRADS, ids=arith_ids(DGRADS))
def test_conv_backward_data(rt, stride, c, arith, accumulate):
    pad = (c.k - 1) // 2
    entry = "conv2d_backward_data" if stride == 1 else "conv2d_s2_backward_data"
    ops = conv_ops(stride, c, False, 120 + c.k)
    old = {"dX": rg.wide_t((c.n, c.H, c.W, c.ci), 125)}

    def run(o, olds):
        dx = cuda(olds["dX"]) if accumulate else None
        if stride == 1:
            return {"dX": rt.conv2d_backward_data(cuda(o["g"]), cuda(o["w"]), pad, dx=dx, accumulate=accumulate)}
        return {"dX": rt.conv2d_s2_backward_data(cuda(o["g"]), cuda(o["w"]), pad, dx=dx, accumulate=accumulate, arith=arith)}

    run_entry("%s %s %s" % (entry, arith, cb.case_id(c)), run, ops, {"g": ("g",), "w": ("w",)}, rg.degrees[entry], old if accumulate else None,
              sanity=(c is S1[0] or c is S2[0]))


@pytest.mark.parametrize("form", ["write_db", "accumulate_db", "write_nodb", "relu_in_db"])
@pytest.mark.parametrize("stride,c,arith", WGRADS, ids=arith_ids(WGRADS))
def test_conv_backward_weight(rt, stride, c, arith, form):
    pad = (c.k - 1) // 2
    entry = "conv2d_backward_weight" if stride == 1 else "conv2d_s2_backward_weight"
    relu_in, accumulate, want_db = form == "relu_in_db", form == "accumulate_db", form != "write_nodb"
    ops = conv_ops(stride, c, relu_in, 130 + c.k)
    old = {"dW": rg.wide_t((c.co, c.ci, c.k, c.k), 135), "db": rg.wide_t((c.co,), 136)}

    def run(o, olds):
        kw = dict(relu_in=relu_in, accumulate=accumulate, want_db=want_db)
        if accumulate:
            kw.update(dw=cuda(olds["dW"]), db=cuda(olds["db"]))
        if stride == 1:
            dw, db = rt.conv2d_backward_weight(cuda(o["x"]), cuda(o["g"]), c.k, pad, arith=arith, **kw)
        else:
            dw, db = rt.conv2d_s2_backward_weight(cuda(o["x"]), cuda(o["g"]), c.k, pad, **kw)
        assert (db is None) == (not want_db)
        return {"dW": dw, "db": db}

    run_entry("%s %s %s %s" % (entry, arith, cb.case_id(c), form), run, ops, {"x": ("x",), "g": ("g",)}, rg.degrees[entry],
              old if accumulate else None, sanity=(c is S1[0] or c is S2[0]))


# ---- heads ----

HEADS = [hb.EXACT_CASES[0], hb.EXACT_CASES[5]]           # 2x2 mean, 64 -> 7, n = 1; 5x5 max-pool, 64 -> 101, n = 3: the two smallest


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("p", [0.8, 0.0])
@pytest.mark.parametrize("c", HEADS, ids=hb.case_id)
def test_heads(rt, c, p, accumulate):
    c = c._replace(p=p)
    drop = (c.seed, c.p)
    ops = {"x": rg.wide_t((c.n, c.H, c.W, c.C), 140, relu=True), "w": rg.wide_t((c.cls, c.C), 141), "b": rg.wide_t((c.cls,), 142),
           "g": rg.wide_t((c.n, c.cls), 143)}
    old = {"dX": rg.wide_t((c.n, c.H, c.W, c.C), 144), "dW": rg.wide_t((c.cls, c.C), 145), "db": rg.wide_t((c.cls,), 146)}
    fwd, bwd = rg.degrees["head_train"], rg.degrees["head_backward"]
    degs = {"out": fwd["out"], "z": fwd["z"]}
    for o in ("dX", "dW", "db"):
        degs[o] = {"x+b": bwd[o]["x"], "w+b": bwd[o]["w"], "g": bwd[o]["g"]}
    degs["out"] = dict(degs["out"], g=0)
    degs["z"] = dict(degs["z"], g=0)
    patterns = []

    def run(o, olds):
        x, w = cuda(o["x"]), cuda(o["w"])
        out, z = rt.head_train(x, w, cuda(o["b"]), c.maxpool, c.head, drop)
        kw = dict(dx=cuda(olds["dX"]), dw=cuda(olds["dW"]), db=cuda(olds["db"]), accumulate_dx=True, accumulate_w=True) if accumulate else {}
        dx, dw, db = rt.head_backward(cuda(o["g"]), x, w, z, c.maxpool, c.head, drop, **kw)
        if not accumulate:
            patterns.append((dx != 0).cpu())
        return {"out": out, "z": z, "dX": dx, "dW": dw, "db": db}

    run_entry("head %s" % hb.case_id(c), run, ops, {"x+b": ("x", "b"), "w+b": ("w", "b"), "g": ("g",)}, degs, old if accumulate else None,
              sanity=True)
    if not accumulate:
        assert bool(patterns[0].any()) and not bool(patterns[0].all())
        assert all(torch.equal(patterns[0], q) for q in patterns[1:]), "the max-pool's tie rule selected other cells at another scale"


# ---- the inference forward ----

FIRST_LAYER = ("motion_conv_gen_", "motion_spatial_down_")
REGIONS = (("fusion_28", 320), ("fusion_14", 1056), ("fusion_7", 832), ("sum_7", 1024))


def wide_maps(B, L, dtype, seed, layout="nchw", lo=-12, hi=4):
    """featmaps.relu_maps times a wide factor, element by element (computed in fp32, rounded once to dtype)"""
    out = []
    for i, m in enumerate(fx.relu_maps(B, L, torch.float32, seed)):
        t = (m * cuda(rg.wide(tuple(m.shape), seed * 16 + i, lo=lo, hi=hi)).abs()).to(dtype)
        if dtype == torch.float16:
            t = torch.where(t.float().abs() < 2.0 ** -4, torch.zeros_like(t), t)         # keep 2^-8 t out of fp16's subnormals
        out.append(t.contiguous(memory_format=torch.channels_last) if layout == "cl" else t.contiguous())
    return out


def scaled_weights(w, a, first_layer=False):
    return dict((k, rg.scale(v, a) if k.endswith(".bias") or (first_layer and k.endswith(".weight") and k.startswith(FIRST_LAYER)) else v)
                for k, v in w.items())


def forward_outputs(h, maps):
    outs = h.forward(maps)
    torch.cuda.synchronize()
    d = dict(("logits%d" % i, o.clone()) for i, o in enumerate(outs))
    for name, ch in REGIONS:
        d[name] = h.region(name, ch).clone()
    return d


def forward_case(rt, monkeypatch, path, prec, variant, B, L, dtype=torch.float32, layout="nchw", sanity=False):
    for k, v in PATHS[path][0].items():
        monkeypatch.setenv(k, v)
    w = synth.make_weights(variant)
    maps = wide_maps(B, L, dtype, 7 + B, layout)

    def run(weights, feats):
        h = rt.OffForward(B, L, variant, precision=prec)
        assert h.load_state_dict(weights) == [] and h.missing_weights()[0] == 0
        h.workspace.fill_(0xff)
        return forward_outputs(h, feats)

    what = "forward %s %s variant %d (%d, %d) %s %s" % (path, prec, variant, B, L, dtype, layout)
    base = run(w, maps)
    check_base(what, base)
    for a in sweep(sanity):
        got = run(scaled_weights(w, a), [rg.scale(m, a) for m in maps])
        check_outputs("%s, maps and biases * 2^%d" % (what, a), base, got, dict((k, a) for k in base))
        got = run(scaled_weights(w, a, first_layer=True), maps)
        check_outputs("%s, first-layer weights and biases * 2^%d" % (what, a), base, got, dict((k, a) for k in base))


@pytest.mark.parametrize("B,L", [(1, 2), (2, 3)])
@pytest.mark.parametrize("variant", [spec.VARIANT_RGB, spec.VARIANT_FLOW], ids=["rgb", "flow"])
@pytest.mark.parametrize("prec", ["fp32", "f32split"])
@pytest.mark.parametrize("path", list(PATHS))
def test_inference_forward(rt, monkeypatch, path, prec, variant, B, L):
    forward_case(rt, monkeypatch, path, prec, variant, B, L, sanity=(path == "default" and B == 1 and variant == spec.VARIANT_RGB))


@pytest.mark.parametrize("dtype,layout", [(torch.bfloat16, "nchw"), (torch.float32, "cl")], ids=["typed_bf16", "channels_last"])
def test_inference_forward_split_map_kinds(rt, monkeypatch, dtype, layout):
    forward_case(rt, monkeypatch, "default", "f32split", spec.VARIANT_RGB, 2, 3, dtype, layout)


# ---- the units, training side ----

UNIT_SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP), (2, 3, spec.VARIANT_FLOW, spec.SLICE_FLAT)]
UNIT_IDS = ["b1l2_flat", "b3l4_clip", "b2l3_flat_flow"]
MAP_KINDS = {"f32": (torch.float32, "nchw", SWEEP), "typed_bf16": (torch.bfloat16, "nchw", SWEEP),
             # fp16 holds 2^-14 .. 2^15: the maps lie in [2^-4, 2^5) and move by 2^+-8, the gradients by 2^+-24 as everywhere
             "cl_f16": (torch.float16, "cl", (-8, 8))}


def wide_views(P, seed):
    """the three fusion-buffer gradients (channels-last, CPU) from the wide draw"""
    return [rg.wide_t((P, H, H, C), seed + i) for i, (H, C) in enumerate(((28, 320), (14, 1056), (7, 832)))]


def views_of(bufs):
    b = [cuda(t) for t in bufs]
    return [(b[0], 0), (b[0], 160)] + [(b[1], 160 * k) for k in range(5)] + [(b[2], 0), (b[2], 160)]


@pytest.mark.parametrize("kind", list(MAP_KINDS))
@pytest.mark.parametrize("arith", ["fp32", "f32split"])
@pytest.mark.parametrize("B,L,variant,slice_mode", UNIT_SHAPES, ids=UNIT_IDS)
def test_units_forward_and_backward(rt, B, L, variant, slice_mode, arith, kind):
    dtype, layout, map_sweep = MAP_KINDS[kind]
    P = B * (L - 1)
    w = synth.make_weights(variant)
    maps = wide_maps(B, L, dtype, 11 + B, layout, lo=-2, hi=2) if dtype == torch.float16 else wide_maps(B, L, dtype, 11 + B, layout)
    bufs = wide_views(P, 150)
    olds = None
    h = rt.OffForward(B, L, variant, slice_mode, training=True)
    deg_b, deg_f = rg.degrees["off_units_backward"], rg.degrees["off_units_backward_feats"]["dX"]

    def run(weights, feats, gbufs, a_grad=0, a_dx=0):
        """eval units, training units, the parameter backward (write, then accumulate onto scaled olds) and the map gradient in fp32
        and bf16 (write and accumulate); a_grad / a_dx: what the accumulate bases of dW / dX are scaled by (db follows g alone)"""
        assert h.load_state_dict(weights) == []
        out = {}
        h.workspace.fill_(0xff)
        h.off_units(feats, arith=arith)
        out.update(("eval " + k, v) for k, v in fx.written(h))
        h.workspace.fill_(0xff)
        h.off_units_train(feats, fx.DROP_SEED, fx.DROP_P, arith=arith)
        out.update(("train " + k, v) for k, v in fx.written(h))
        views = views_of(gbufs)
        grads, gv = h.off_units_backward(feats, views, fx.DROP_SEED, fx.DROP_P, arith=arith)
        out.update(("grad " + k, v.clone()) for k, v in gv.items())
        acc = h.new_unit_grads()
        for k, (off, shape) in h.unit_grad_slots().items():
            acc[off:off + int(np.prod(shape))].view(shape).copy_(cuda(rg.scale(olds["grad " + k], a_dx if k.endswith(".bias") else a_grad)))
        _, av = h.off_units_backward(feats, views, fx.DROP_SEED, fx.DROP_P, grads=acc, accumulate=True, arith=arith)
        out.update(("grad+ " + k, v.clone()) for k, v in av.items())
        for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            dx = h.off_units_backward_feats(layout="nchw", dtype=dt, arith=arith)
            out.update(("dX %s %d" % (tag, i), t) for i, t in enumerate(dx))
            into = [cuda(rg.scale(olds["dX %d" % i], a_dx)).to(dt) for i in range(spec.NUM_SITES)]
            h.off_units_backward_feats(layout="nchw", dtype=dt, out=into, accumulate=True, arith=arith)
            out.update(("dX+ %s %d" % (tag, i), t) for i, t in enumerate(into))
        torch.cuda.synchronize()
        return out

    olds = dict(("grad " + k, rg.wide_t(shape, 160 + i)) for i, (k, (_off, shape)) in enumerate(h.unit_grad_slots().items()))
    # accumulate bases of dX: bf16 values, so that the 16-bit form starts from the same numbers
    olds.update(("dX %d" % i, rg.wide_t((B * L, C, H, H), 180 + i).bfloat16().float()) for i, (_n, C, H) in enumerate(spec.SITES))
    what = "units %s %s %s" % (UNIT_IDS[UNIT_SHAPES.index((B, L, variant, slice_mode))], arith, kind)
    base = run(w, maps, bufs)
    check_base(what, base)

    def factor(name, a, cls):
        if name.startswith(("eval ", "train ")):
            return a if cls == "x+b" else 0
        if name.startswith("grad"):
            return a * deg_b["db" if name.endswith(".bias") else "dW"][cls]
        return a * deg_f[cls]

    for a in map_sweep + (rg.SANITY,):
        got = run(scaled_weights(w, a), [rg.scale(m, a) for m in maps], bufs, a_grad=a, a_dx=0)
        check_outputs("%s, maps and biases * 2^%d" % (what, a), base, got, dict((k, factor(k, a, "x+b")) for k in base))
    for a in SWEEP:
        got = run(w, maps, [rg.scale(t, a) for t in bufs], a_grad=a, a_dx=a)
        check_outputs("%s, g * 2^%d" % (what, a), base, got, dict((k, factor(k, a, "g")) for k in base))


# ---- modules ----

class Net(nn.Module):
    """OFFUnits -> a stride-2 FusionConv2d -> two stride-1 FusionConv2d (the second with the residual) -> MotionHead"""

    def __init__(self, mods, arith, B, L):
        super().__init__()
        self.units = mods.OFFUnits(B, L, feat_grad=False, wgrad_arith=arith, fwd_arith=arith, feat_grad_arith=arith)
        self.open = mods.FusionConv2d(320, 64, 7, stride=2, padding=3, relu=True, wgrad_arith="fp32", dgrad_arith=arith)
        self.c1 = mods.FusionConv2d(64, 64, 3, padding=1, relu=True, wgrad_arith=arith)
        self.c2 = mods.FusionConv2d(64, 64, 1, relu=True, wgrad_arith=arith)
        self.head = mods.MotionHead(64, 101, maxpool=True, head_index=0, drop_p=0.8)

    def forward(self, feats):
        u28, u14, u7 = self.units(feats, drop_seed=5)
        y = self.open(u28)
        logits = self.head(self.c2(self.c1(y), res=y), drop_seed=5)
        return logits.sum() + u14.sum() + u7.sum()


@pytest.mark.parametrize("arith", ["fp32", "f32split"])
def test_modules(rt, arith):
    from offk_amd import off_module as mods
    B, L = 1, 2
    gen = torch.Generator().manual_seed(0x5CA1)
    net = Net(mods, arith, B, L)
    sd = dict((k, v) for k, v in net.state_dict().items())
    unit_w = synth.make_weights(spec.VARIANT_RGB)
    for k in sd:
        if k.startswith("units."):
            sd[k] = torch.from_numpy(unit_w[k[6:]]).reshape(sd[k].shape)
        else:
            sd[k] = rg.wide_t(tuple(sd[k].shape), 200 + len(k), lo=-6, hi=-2) if k.endswith(".weight") else torch.randn(sd[k].shape, generator=gen) * 0.1
    maps = wide_maps(B, L, torch.float32, 13)

    def run(a):
        net.load_state_dict(dict((k, rg.scale(v, a) if k.endswith(".bias") else v) for k, v in sd.items()))
        net.cuda().train()
        for p in net.parameters():
            p.grad = None
        loss = net([rg.scale(m, a) for m in maps])
        loss.backward()
        torch.cuda.synchronize()
        out = {"loss": loss.detach().reshape(1)}
        out.update((k, p.grad.clone()) for k, p in net.named_parameters() if p.requires_grad)
        return out

    base = run(0)
    check_base("modules %s" % arith, base)
    assert len(base) > 20
    for a in SWEEP:
        got = run(a)
        check_outputs("modules %s, maps and biases * 2^%d" % (arith, a), base, got,
                      dict((k, 0 if k.endswith(".bias") else a) for k in base))
