"""The stride-2 fusion convs' weight / bias gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_s2_backward_weight_split,
csrc/conv_wgrad_s2_split.hip; runtime.conv2d_s2_backward_weight(arith="f32split"), FusionConv2d(s2_wgrad_arith="f32split")).

 1. exact integers: the ten cases of tests/conv_bwd.S2.cases() (the plan-chosen n from the SPLIT plan: >= 3 chunks, a shorter last one) and
    two-row output maps at the 8-position group boundaries and the real width (OW = 7, 8, 9, 14), both k: dW and db EQUAL the fp64
    reference, with and without accumulate, with relu_in, without db, on middle channel slices in a guarded arena.  With the 1x1-output,
    OW = 2, OW = 5, half-ci-tile and two-co-tile cases these are the smallest shapes at which the K tail, a step that straddles rows and
    images, the column wrap, the row leaving the map and the half tile can each go wrong;
 2. wide integers: one operand 17-bit odd integers whose three planes are all non-zero, on either side: equal to fp64;
 3. worst-case mantissas on g and x: per element of dW, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|g x| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation constant on the same operands in the kernel's chunked K layout (tests/conv_s2_wgrad_split.py) --
    never the kernel's output; tests/test_conv_s2_wgrad_split_abi.py shows on the CPU that losing any one issued product breaks it;
 4. the same inequality on normal data, db within gamma(positions) sum|g|;
 5. equal bits from NaN- and -3-filled scratch, graph replay == eager;  6. a refused call writes nothing;
 7. range: operands scaled by 2^+-20 scale dW and db bit for bit; one +-Inf in x and one in g reach exactly the set include/offk.h names;
 8. the module.

The bodies the two strides share are tests/conv_grad_checks.py's, written against tests/conv_bwd.py's forms; this file keeps the test
names, the parametrize lists and what this stride alone has."""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from . import arena
from . import conv_grad_checks as chk
from .conv_bwd import S2 as s2
from .conv_grad_checks import rt  # noqa: F401

pytestmark = pytest.mark.gpu
EDGES = [s2.Case(k, 2, 4, W, 64, 64) for k in (7, 5) for W in (14, 16, 18, 28)]
CASES = s2.cases() + EDGES
IDS = [s2.case_id(c) for c in CASES]


def split_wgrad(rt, x, g, c, **kw):
    return chk.split_wgrad(rt, s2, x, g, c, **kw)


# ---- 1. exact integers ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    chk.wgrad_dense(rt, s2, c, accumulate)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bias_gradient_is_optional(rt, c):
    chk.wgrad_bias_optional(rt, s2, c)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relu_in_and_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    chk.wgrad_relu_in_slices(rt, s2, c, accumulate)


# ---- 2. wide integers ----

@pytest.mark.parametrize("side", ["g", "x"])
@pytest.mark.parametrize("c", chk.WIDE[2, "wgrad"][1], ids=s2.case_id)
def test_wide_integers_equal_fp64(rt, c, side):
    chk.wgrad_wide(rt, s2, c, side)


# ---- 3. / 4. the inequality ----

def check_inequality(rt, what, c, g, x, dw_gpu, relu_in=False):
    return chk.wgrad_inequality(rt, s2, what, c, g, x, dw_gpu, relu_in=relu_in)


# both real channel shapes at n = 1, and two small cases (two images: a step that straddles them; a half ci tile)
WORST_SHAPES = [s2.Case(7, 1, 28, 28, 320, 64), s2.Case(5, 1, 14, 14, 1056, 128), s2.Case(7, 2, 6, 10, 64, 64), s2.Case(5, 2, 6, 4, 160, 64)]


@pytest.mark.parametrize("pattern,signs", chk.ADV, ids=chk.ADV_IDS)
@pytest.mark.parametrize("c", WORST_SHAPES, ids=s2.case_id)
def test_worst_case_mantissas(rt, c, pattern, signs):
    """x alternates in sign along the map's column pairs in the "alternating" mode, so along the positions of every tap's stride-2 sample:
    sum g x << sum |g x|."""
    OH, OW = c.H // 2, c.W // 2
    g = synth.make_adversarial((c.n * OH * OW, c.co), pattern, "same", seed=21 + c.H, relu=(pattern == 0x7FFFFF)).reshape(c.n, OH, OW, c.co)
    x = synth.make_adversarial((c.n * c.H * OW, c.ci), pattern, signs, seed=22 + c.H, k_axis=0).reshape(c.n, c.H, OW, 1, c.ci)
    x = np.ascontiguousarray(np.broadcast_to(x, (c.n, c.H, OW, 2, c.ci))).reshape(c.n, c.H, c.W, c.ci) * np.float32(2.0 ** -4)
    chk.wgrad_worst(rt, s2, c, pattern, signs, g, x)


@pytest.mark.parametrize("c", s2.cases(), ids=s2.case_id)
def test_normal_data_within_the_bound(rt, c):
    chk.wgrad_normal(rt, s2, c)


# ---- 5. scratch and replay ----

DISCIPLINE = [s2.Case(7, 37, 6, 10, 64, 64), s2.Case(5, 88, 6, 4, 32, 64)]          # three chunks each, the last one shorter


@pytest.mark.parametrize("c", DISCIPLINE, ids=s2.case_id)
def test_scratch_contents_never_show_and_replay_equals_eager(rt, c):
    chk.wgrad_discipline(rt, s2, c, 3)


# ---- 6. refusal ----

def test_a_refused_call_writes_nothing(rt):
    c = s2.Case(5, 2, 6, 4, 96, 64)
    inp = s2.normal_inputs(c)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes = rt.conv2d_s2_backward_weight_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)[0]
    A = arena.Arena.for_sizes([c.co * c.ci * 25 * 4, c.co * 4, wbytes])
    dw, db, s = A.empty("dw", (c.co, c.ci, 5, 5)), A.empty("db", (c.co,)), A.carve("scratch", wbytes)
    with pytest.raises(_lib.OffkError, match="offk_conv2d_s2_backward_weight_split: the form must be"):
        rt.conv2d_s2_backward_weight(x, g, 5, 3, dw=dw, db=db, scratch=s, arith="f32split")
    with pytest.raises(_lib.OffkError, match="offk_conv2d_s2_backward_weight_split: x: cstride < coff \\+ C"):
        rt.conv2d_s2_backward_weight(x, g, 5, 2, x_coff=4, ci=96, dw=dw, db=db, scratch=s, arith="f32split")
    lib = _lib.load()
    rc = lib.offk_conv2d_s2_backward_weight_split(None, x.data_ptr(), c.ci, 0, g.data_ptr(), c.co, 0, c.n, c.H, c.W, c.ci, c.co, 5, 5, 2, 0, dw.data_ptr(),
                                                  db.data_ptr(), 0, s.data_ptr(), wbytes - 1)
    assert rc == -1 and b"offk_conv2d_s2_backward_weight_split: scratch too small (offk_conv2d_s2_backward_weight_plan_split)" in lib.offk_last_error(None)
    torch.cuda.synchronize()
    assert A.untouched(dw) and A.untouched(db) and A.untouched(s)
    A.check()


# ---- 7. range ----

RANGE = [s2.Case(7, 3, 6, 10, 64, 64), s2.Case(5, 3, 6, 4, 96, 64)]


@pytest.mark.parametrize("a", [20, -20])
@pytest.mark.parametrize("c", RANGE, ids=s2.case_id)
def test_power_of_two_scaling_is_exact(rt, c, a):
    inp = s2.normal_inputs(c)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    dw, db = split_wgrad(rt, x, g, c)
    sc = float(2.0 ** a)
    dwx, dbx = split_wgrad(rt, x * sc, g, c)
    dwg, dbg = split_wgrad(rt, x, g * sc, c)
    torch.cuda.synchronize()
    assert arena.same_bits(dwx, dw * sc) and arena.same_bits(dbx, db), "x scaled by 2^%d" % a
    assert arena.same_bits(dwg, dw * sc) and arena.same_bits(dbg, db * sc), "g scaled by 2^%d" % a
    assert bool(torch.isfinite(dwx).all() and torch.isfinite(dwg).all() and (dwx != 0).any())


@pytest.mark.parametrize("value", [float("inf"), float("-inf")], ids=["plus_inf", "minus_inf"])
@pytest.mark.parametrize("c", RANGE, ids=s2.case_id)
def test_a_non_finite_value_reaches_exactly_the_set_the_header_names(rt, c, value):
    inp = s2.normal_inputs(c)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    pad, OH, OW = s2.FORMS[c.k], c.H // 2, c.W // 2
    dw, db = split_wgrad(rt, x, g, c)
    # x[n, R, C, ci]: exactly the taps whose sum it enters
    n0, R, C, ci0 = 1, 1, c.W - 1, 37
    xi = x.clone()
    xi[n0, R, C, ci0] = value
    dwx, dbx = split_wgrad(rt, xi, g, c)
    khs = [kh for kh in range(c.k) if (R + pad - kh) % 2 == 0 and 0 <= (R + pad - kh) // 2 < OH]
    kws = [kw for kw in range(c.k) if (C + pad - kw) % 2 == 0 and 0 <= (C + pad - kw) // 2 < OW]
    assert khs and kws and len(khs) < c.k and len(kws) < c.k
    want = torch.zeros(c.co, c.ci, c.k, c.k, dtype=torch.bool)
    for kh in khs:
        for kw in kws:
            want[:, ci0, kh, kw] = True
    # g[n, oh, ow, co]: every tap of dw[co, :] (a tap that leaves the map is a zero on the x side: NaN) and db[co]
    co0 = 5
    gi = g.clone()
    gi[n0, 0, OW - 1, co0] = value
    dwg, dbg = split_wgrad(rt, x, gi, c)
    torch.cuda.synchronize()
    bad = ~torch.isfinite(dwx).cpu()
    assert torch.equal(bad, want), "x = %s: %d non-finite elements, %d expected" % (value, int(bad.sum()), int(want.sum()))
    assert bool(dwx.cpu()[want].isnan().all()), "NaN (Inf - Inf in the cut)"
    assert arena.same_bits(dwx.cpu()[~want], dw.cpu()[~want]) and arena.same_bits(dbx, db), "every other element: the clean run's bits"
    wantg = torch.zeros(c.co, c.ci, c.k, c.k, dtype=torch.bool)
    wantg[co0] = True
    assert torch.equal(dwg.cpu().isnan(), wantg), "g = %s" % value
    assert arena.same_bits(dwg.cpu()[~wantg], dw.cpu()[~wantg])
    keep = torch.ones(c.co, dtype=torch.bool)
    keep[co0] = False
    assert not bool(torch.isfinite(dbg[co0])) and arena.same_bits(dbg.cpu()[keep], db.cpu()[keep])
    # relu_in: max(x, 0) in hardware: -Inf counts as 0, +Inf stays
    dwr, _ = split_wgrad(rt, xi, g, c, relu_in=True)
    torch.cuda.synchronize()
    if value < 0:
        x0 = x.clone()
        x0[n0, R, C, ci0] = 0.0
        assert arena.same_bits(dwr, split_wgrad(rt, x0, g, c, relu_in=True)[0])
    else:
        assert torch.equal(~torch.isfinite(dwr).cpu(), want)


# ---- 8. the module ----

OPENERS = [("open28", 64, 64, 7, dict(), 12, 20), ("open14", 96, 64, 5, dict(relu=True), 12, 8),
           ("open14_relu_in", 32, 64, 5, dict(relu=True, relu_in=True), 8, 12)]         # name, ci, co, k, flags, H, W
MOD_N = 3


def make_opener(spec, params, **arith):
    from offk_amd.off_module import FusionConv2d
    _name, ci, co, k, flags, _H, _W = spec
    m = FusionConv2d(ci, co, k, stride=2, padding=s2.FORMS[k], **flags, **arith)
    m.load_state_dict(params)
    return m.cuda()


def run_opener(m, x):
    x = x.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    y = m(x)
    y.retain_grad()
    (y * y).sum().backward()
    return x, y


def node_operands(spec, x, y):
    """the operands as the autograd node saw them: the gradient behind the ReLU mask and the input, channels-last rows"""
    g = y.grad * (y.detach() > 0) if spec[4].get("relu") else y.grad
    return g.permute(0, 2, 3, 1).contiguous(), x.detach().permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("spec", OPENERS, ids=[s[0] for s in OPENERS])
def test_module_routes_only_the_weight_gradient(rt, spec, monkeypatch):
    from offk_amd.off_module import FusionConv2d
    name, ci, co, k, flags, H, W = spec
    relu_in = bool(flags.get("relu_in"))
    gen = torch.Generator().manual_seed(0x2E7 + k)
    params = {"weight": torch.randn(co, ci, k, k, generator=gen) / (ci * k * k) ** 0.5, "bias": torch.randn(co, generator=gen) * 0.1}
    xd = torch.randn(MOD_N, ci, H, W, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    split, fp32, plain = make_opener(spec, params, s2_wgrad_arith="f32split"), make_opener(spec, params, s2_wgrad_arith="fp32"), make_opener(spec, params)
    both = make_opener(spec, params, s2_wgrad_arith="f32split", dgrad_arith="f32split")
    bwd = make_opener(spec, params, bwd_arith="f32split")
    assert split.s2_wgrad_arith == "f32split" and plain.s2_wgrad_arith == "fp32" and bwd.s2_wgrad_arith == "fp32"
    xs, ys = run_opener(split, xd)
    xf, yf = run_opener(fp32, xd)
    xp, yp = run_opener(plain, xd)
    torch.cuda.synchronize()
    assert arena.same_bits(ys.detach(), yf.detach()) and arena.same_bits(yp.detach(), yf.detach()), "the forward"
    assert arena.same_bits(xs.grad, xf.grad) and arena.same_bits(xp.grad, xf.grad), "dX"
    gr, hr = node_operands(spec, xf, yf)
    c = s2.Case(k, MOD_N, H, W, ci, co)
    dw_s, db_s = split_wgrad(rt, hr, gr, c, relu_in=relu_in)
    dw_f, db_f = rt.conv2d_s2_backward_weight(hr, gr, k, s2.FORMS[k], relu_in=relu_in)
    torch.cuda.synchronize()
    assert arena.same_bits(split.weight.grad, dw_s) and arena.same_bits(split.bias.grad, db_s), "the split module is the new entry, bit for bit"
    for m in (plain, fp32):
        assert arena.same_bits(m.weight.grad, dw_f) and arena.same_bits(m.bias.grad, db_f), "the default module is the fp32 entry, bit for bit"
    assert not arena.same_bits(split.weight.grad, fp32.weight.grad), "the switch reached the kernel"
    check_inequality(rt, "module %s" % name, c, gr.cpu().numpy(), hr.cpu().numpy(), split.weight.grad, relu_in=relu_in)
    # bwd_arith alone keeps dW / db on the fp32 entry; with dgrad_arith both split entries are taken
    calls = []
    real_w, real_d = rt.conv2d_s2_backward_weight, rt.conv2d_s2_backward_data
    monkeypatch.setattr(rt, "conv2d_s2_backward_weight", lambda *a, **kw: (calls.append(("w", kw.get("arith", "fp32"))), real_w(*a, **kw))[1])
    monkeypatch.setattr(rt, "conv2d_s2_backward_data", lambda *a, **kw: (calls.append(("d", kw.get("arith", "fp32"))), real_d(*a, **kw))[1])
    xb, _yb = run_opener(both, xd)
    xw, _yw = run_opener(bwd, xd)
    torch.cuda.synchronize()
    assert calls == [("w", "f32split"), ("d", "f32split"), ("w", "fp32"), ("d", "f32split")], calls
    assert arena.same_bits(both.weight.grad, dw_s) and arena.same_bits(both.bias.grad, db_s) and arena.same_bits(xb.grad, xw.grad)
    assert arena.same_bits(bwd.weight.grad, dw_f) and arena.same_bits(bwd.bias.grad, db_f)
    # a frozen layer launches nothing
    del calls[:]
    before = FusionConv2d.weight_grad_launches
    run_opener(split, xd)
    assert FusionConv2d.weight_grad_launches - before == 1 and calls[0] == ("w", "f32split")
    frozen = make_opener(spec, params, s2_wgrad_arith="f32split")
    for p in frozen.parameters():
        p.requires_grad_(False)
    del calls[:]
    before = FusionConv2d.weight_grad_launches
    xz, _ = run_opener(frozen, xd)
    torch.cuda.synchronize()
    assert FusionConv2d.weight_grad_launches == before and [w for w in calls if w[0] == "w"] == [], "the frozen conv ran its weight gradient"
    assert frozen.weight.grad is None and arena.same_bits(xz.grad, xf.grad)
    # optimizer.step() is seen by the next call: the parameters are read in place
    opt = torch.optim.SGD(split.parameters(), lr=0.05)
    before_dw = split.weight.grad.clone()
    opt.step()
    x2, y2 = run_opener(split, xd)
    ref_mod = make_opener(spec, {"weight": split.weight.detach().cpu(), "bias": split.bias.detach().cpu()}, s2_wgrad_arith="f32split")
    x3, y3 = run_opener(ref_mod, xd)
    torch.cuda.synchronize()
    assert not arena.same_bits(y2.detach(), ys.detach()) and not arena.same_bits(split.weight.grad, before_dw)
    g2, h2 = node_operands(spec, x2, y2)
    assert arena.same_bits(split.weight.grad, real_w(h2, g2, k, s2.FORMS[k], relu_in=relu_in, arith="f32split")[0])
    assert arena.same_bits(y2.detach(), y3.detach()) and arena.same_bits(split.weight.grad, ref_mod.weight.grad)
