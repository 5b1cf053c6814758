"""The fusion convs' weight / bias gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_backward_weight_split,
csrc/conv_wgrad_split.hip; runtime.conv2d_backward_weight(arith="f32split"), FusionConv2d(wgrad_arith="f32split")).

 1. exact integers: every case of tests/conv_bwd.S1.cases() (the plan-chosen n from the SPLIT plan) and 2. the maps on both sides of the pitch's
    boundaries (W = 7, 8, 15, 16) and of the staged windows' (W = 23, 24: adjacent from pitch 32 on; W = 31, 32: disjoint from pitch 40 on): dW and db EQUAL the fp64 reference, with and without accumulate, with relu_in, without db, on middle
    channel slices in a guarded arena;
 3. wide integers: one operand 17-bit odd integers whose three planes are all non-zero, on either side: equal to fp64 -- the plane indexing
    of the five products with a leading plane, exactly;
 4. worst-case mantissas on g and x: per element of dW, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|g x| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation constant on the same operands in the kernel's chunked K layout (tests/conv_wgrad_split.py) --
    never the kernel's output; tests/test_conv_wgrad_split_abi.py shows on the CPU that losing any one issued product breaks it;
 5. the same inequality on normal data at the 13 fusion shapes, db within gamma(n H W) sum|g|;
 6. discipline: equal bits from NaN- and -3-filled scratch, graph replay == eager, guard bands, a refused call writes nothing;  7. the module.

The bodies the two strides share are tests/conv_grad_checks.py's, written against tests/conv_bwd.py's forms; this file keeps the test
names, the parametrize lists and what this stride alone has."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from . import arena
from . import conv_grad_checks as chk
from . import conv_wgrad_split as cs
from .conv_bwd import S1 as cb
from .conv_grad_checks import rt  # noqa: F401

pytestmark = pytest.mark.gpu
# pitch 8 | 16 | 16 | 24 (one zero column ... eight), then 24 | 32 where the kernel rows' windows stop overlapping (pg = pitch / 8 clamps at 4, 12 k
# groups staged) and 32 | 40 where they stop touching (the rows' shifts are no longer consecutive k groups; the 120 KB launch)
EDGES = [cb.Case(3, 2, 3, W, 64, 64) for W in (7, 8, 15, 16, 23, 24, 31, 32)]
CASES = cb.cases() + EDGES
IDS = [cb.case_id(c) for c in CASES]


def split_wgrad(rt, x, g, c, **kw):
    return chk.split_wgrad(rt, cb, x, g, c, **kw)


# ---- 1. / 2. exact integers ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    chk.wgrad_dense(rt, cb, c, accumulate)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bias_gradient_is_optional(rt, c):
    chk.wgrad_bias_optional(rt, cb, c)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relu_in_and_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    chk.wgrad_relu_in_slices(rt, cb, c, accumulate)


# ---- 3. wide integers ----

@pytest.mark.parametrize("side", ["g", "x"])
@pytest.mark.parametrize("c", chk.WIDE[1, "wgrad"][1], ids=lambda c: cb.case_id(c))
def test_wide_integers_equal_fp64(rt, c, side):
    chk.wgrad_wide(rt, cb, c, side)


# ---- 4. / 5. the inequality ----

WORST_SHAPES = [cb.Case(3, 2, 5, 3, 128, 128), cb.Case(3, 2, 7, 7, 128, 128), cb.Case(3, 1, 14, 14, 64, 64), cb.Case(1, 2, 7, 7, 64, 256)]


@pytest.mark.parametrize("pattern,signs", chk.ADV, ids=chk.ADV_IDS)
@pytest.mark.parametrize("c", WORST_SHAPES, ids=lambda c: cb.case_id(c))
def test_worst_case_mantissas(rt, c, pattern, signs):
    """x alternates in sign along the pixels (the contraction index) in the "alternating" mode: sum g x << sum |g x|."""
    px = c.n * c.H * c.W
    g = synth.make_adversarial((c.n, c.H, c.W, c.co), pattern, "same", seed=21 + c.H, relu=(pattern == 0x7FFFFF))
    x = synth.make_adversarial((px, c.ci), pattern, signs, seed=22 + c.H, k_axis=0).reshape(c.n, c.H, c.W, c.ci) * np.float32(2.0 ** -4)
    chk.wgrad_worst(rt, cb, c, pattern, signs, g, x)


FUSION = [cb.Case(k, 2, H, H, ci, co) for H, ci, co, k in cb.FUSION_SHAPES]


@pytest.mark.parametrize("c", FUSION, ids=lambda c: cb.case_id(c))
def test_normal_data_within_the_bound(rt, c):
    chk.wgrad_normal(rt, cb, c)


# ---- 6. discipline ----

DISCIPLINE = [cb.Case(3, 5, 7, 7, 128, 64), cb.Case(1, 9, 7, 7, 64, 128), cb.Case(3, 3, 14, 14, 64, 64)]


@pytest.mark.parametrize("c", DISCIPLINE, ids=lambda c: cb.case_id(c))
def test_scratch_contents_never_show_and_replay_equals_eager(rt, c):
    chk.wgrad_discipline(rt, cb, c, 2)


def test_a_refused_call_writes_nothing(rt):
    c = cb.Case(3, 2, 7, 7, 64, 64)
    inp = cb.normal_inputs(c)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes = rt.conv2d_backward_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)[0]
    A = arena.Arena.for_sizes([c.co * c.ci * 9 * 4, c.co * 4, wbytes])
    dw, db, s = A.empty("dw", (c.co, c.ci, 3, 3)), A.empty("db", (c.co,)), A.carve("scratch", wbytes)
    with pytest.raises(_lib.OffkError, match="offk_conv2d_backward_weight_split: pad must be"):
        rt.conv2d_backward_weight(x, g, 3, 0, dw=dw, db=db, scratch=s, arith="f32split")
    with pytest.raises(_lib.OffkError, match="offk_conv2d_backward_weight_split: x: cstride < coff \\+ C"):
        rt.conv2d_backward_weight(x, g, 3, 1, x_coff=4, ci=64, dw=dw, db=db, scratch=s, arith="f32split")
    lib = _lib.load()
    rc = lib.offk_conv2d_backward_weight_split(None, x.data_ptr(), 64, 0, g.data_ptr(), 64, 0, c.n, 7, 7, 64, 64, 3, 3, 1, 0, dw.data_ptr(), db.data_ptr(), 0,
                                               s.data_ptr(), wbytes - 1)
    assert rc == -1 and b"offk_conv2d_backward_weight_split: scratch too small" in lib.offk_last_error(None)
    torch.cuda.synchronize()
    assert A.untouched(dw) and A.untouched(db) and A.untouched(s)
    A.check()


# ---- 7. the module ----

LAYERS = [("c1", 256, 64, 1, False), ("c2", 64, 64, 3, True), ("c3", 64, 256, 1, False)]
MOD_N, MOD_HW = 2, 14


def make_stack(arith, params, frozen=()):
    from offk_amd.off_module import FusionConv2d
    seq = nn.ModuleDict((name, FusionConv2d(ci, co, k, padding=(k - 1) // 2, relu=relu, **({} if arith is None else {"wgrad_arith": arith})))
                        for name, ci, co, k, relu in LAYERS)
    seq.load_state_dict(params)
    for name in frozen:
        for p in seq[name].parameters():
            p.requires_grad_(False)
    return seq.cuda()


def run_module_stack(seq, x):
    x = x.clone().requires_grad_(True)
    for p in seq.parameters():
        p.grad = None
    h, trace = x, {}
    for name, *_ in LAYERS:
        y = seq[name](h)
        y.retain_grad()
        trace[name] = (h, y)
        h = y
    (h * h).sum().backward()
    return x, trace


def module_params():
    gen = torch.Generator().manual_seed(0x5B17)
    out = {}
    for name, ci, co, k, _relu in LAYERS:
        out[name + ".weight"] = torch.randn(co, ci, k, k, generator=gen) / (ci * k * k) ** 0.5
        out[name + ".bias"] = torch.randn(co, generator=gen) * 0.1
    return out, torch.randn(MOD_N, 256, MOD_HW, MOD_HW, generator=gen)


def test_module_routes_only_the_weight_gradient(rt):
    from offk_amd.off_module import FusionConv2d
    params, x0 = module_params()
    xd = x0.cuda().contiguous(memory_format=torch.channels_last)
    fp32, split, plain = make_stack("fp32", params), make_stack("f32split", params), make_stack(None, params)
    assert all(m.wgrad_arith == "f32split" for m in split.values()) and all(m.wgrad_arith == "fp32" for m in plain.values())
    xf, tf = run_module_stack(fp32, xd)
    xs, ts = run_module_stack(split, xd)
    xp, _tp = run_module_stack(plain, xd)
    torch.cuda.synchronize()
    assert arena.same_bits(xf.grad, xs.grad), "the input gradient"
    for name, ci, co, k, relu in LAYERS:
        assert arena.same_bits(tf[name][1].detach(), ts[name][1].detach()), "forward of %s" % name
        assert arena.same_bits(tf[name][1].grad, ts[name][1].grad), "data gradient into %s" % name
        # operands as the fp32 stack saw them: the layer's input rows and the gradient behind its ReLU mask
        h, y = tf[name]
        g = y.grad * (y.detach() > 0) if relu else y.grad
        gr, hr = g.permute(0, 2, 3, 1).contiguous(), h.detach().permute(0, 2, 3, 1).contiguous()
        c = cb.Case(k, MOD_N, MOD_HW, MOD_HW, ci, co)
        chk.wgrad_inequality(rt, cb, "module %s" % name, c, gr.cpu().numpy(), hr.cpu().numpy(), split[name].weight.grad)
        # the fp64 nn.Conv2d layer on the same operands gives the reference the inequality was asserted against
        conv = nn.Conv2d(ci, co, k, padding=(k - 1) // 2).double()
        conv(h.detach().cpu().double()).backward(g.cpu().double())
        G, taps = cs.operands(gr.cpu().numpy(), hr.cpu().numpy(), k)
        ref, _d, mag = cs.terms(G, taps, k)
        assert np.allclose(conv.weight.grad.numpy(), ref, rtol=0, atol=1e-12 * float(mag.max()))
        gsum = gr.double().reshape(-1, co)
        err = (split[name].bias.grad.double() - gsum.sum(0)).abs()
        assert bool((err <= cb.gamma(MOD_N * MOD_HW * MOD_HW) * gsum.abs().sum(0)).all()), "bias gradient of %s" % name
        # the default module is the fp32 entry, bit for bit
        dw, db = rt.conv2d_backward_weight(hr, gr, k, (k - 1) // 2)
        assert arena.same_bits(plain[name].weight.grad, dw) and arena.same_bits(plain[name].bias.grad, db), "default module of %s" % name
        assert arena.same_bits(fp32[name].weight.grad, dw)
        assert not arena.same_bits(split[name].weight.grad, dw), "the switch reached the kernel of %s" % name
    assert arena.same_bits(xp.grad, xf.grad)
    # a frozen layer launches no weight gradient
    before = FusionConv2d.weight_grad_launches
    run_module_stack(split, xd)
    assert FusionConv2d.weight_grad_launches - before == 3
    frozen = make_stack("f32split", params, frozen=("c2",))
    before = FusionConv2d.weight_grad_launches
    run_module_stack(frozen, xd)
    torch.cuda.synchronize()
    assert FusionConv2d.weight_grad_launches - before == 2, "the frozen conv ran its weight gradient"
    assert frozen["c2"].weight.grad is None and arena.same_bits(frozen["c1"].weight.grad, split["c1"].weight.grad)
