"""The stride-1 fusion convs' data gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_backward_data_split,
csrc/conv_dgrad_split.hip; runtime.conv2d_backward_data(arith="f32split"), FusionConv2d(bwd_arith="f32split")).

 1. exact integers: dX EQUAL to the fp64 reference at every case of tests/conv_bwd.S1.cases(), with and without accumulate, and again on
    middle channel slices of g and dx inside a NaN-guarded arena; then the kernel's own edges at k = 3 and k = 1, in each of its three
    block forms: M exactly a pixel tile and one either side, one-column / 1x1 / 2x2 maps, a block row and a half of ci, two steps per tap,
    an image boundary inside a pixel tile;
 2. 17-bit integers: three non-zero planes in g against single-plane weights and the reverse: equal to fp64 -- the plane indexing of the
    five products with a leading plane, exactly;
 3. worst-case mantissas and normal data at the 13 fusion shapes (n = 1): per element of dX, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|g w| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation constant on the same operands in the kernel's K order (tests/conv_dgrad_split.py) -- never
    the kernel's output; tests/test_conv_dgrad_split_abi.py shows on the CPU that losing any one issued product breaks it;
 4. discipline: equal bits from NaN- and -3-filled scratch, graph replay == eager, a refused call writes nothing;  5. the module.

The bodies the two strides share are tests/conv_grad_checks.py's, written against tests/conv_bwd.py's forms; this file keeps the test
names, the parametrize lists and what this stride alone has."""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib

from . import arena
from . import conv_dgrad_split as dg
from . import conv_grad_checks as chk
from . import exact
from . import split_bound as sb
from .conv_bwd import S1 as cb
from .conv_grad_checks import rt  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = cb.cases()
IDS = [cb.case_id(c) for c in CASES]


def resolve(rt, c):
    """the plan-chosen case of tests/conv_bwd.py: n = 3 here (the data gradient has no chunks to exercise)"""
    return c._replace(n=3) if c.n is None else c


def split_dgrad(rt, g, w, k, **kw):
    return chk.split_dgrad(rt, cb, g, w, k, **kw)


# ---- 1. exact integers ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    chk.dgrad_dense(rt, cb, resolve(rt, c), accumulate)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    chk.dgrad_slices(rt, cb, resolve(rt, c), accumulate)


# The kernel's own edges (n, H, W, ci), each at k = 3 and k = 1 with Co = 64 (two 32-co steps per tap), and the block form the plan must
# choose there.  64 x 256: Ci = 64.  128 x 128: at most 128 blocks of 128 x 256.  128 x 256: more than that -- 1088 channels (eight block
# rows and a half) from 15 pixel tiles on.
EDGES = [
    ((1, 15, 17, 64), (64, 256)), ((1, 16, 16, 64), (64, 256)), ((1, 1, 257, 64), (64, 256)),            # M = 255 / 256 / 257
    ((1, 5, 1, 64), (64, 256)), ((1, 1, 1, 64), (64, 256)), ((1, 2, 2, 64), (64, 256)),                  # every kw != 1 tap leaves the row; ...
    ((2, 5, 3, 64), (64, 256)),                                                                          # the image boundary inside a tile
    ((1, 1, 127, 128), (128, 128)), ((1, 8, 16, 128), (128, 128)), ((1, 3, 43, 128), (128, 128)),        # M = 127 / 128 / 129
    ((1, 15, 17, 128), (128, 128)), ((1, 16, 16, 128), (128, 128)), ((1, 1, 257, 128), (128, 128)),
    ((1, 5, 1, 192), (128, 128)), ((1, 1, 1, 192), (128, 128)), ((1, 2, 2, 192), (128, 128)),            # Ci = 192: a block row and a half
    ((2, 9, 7, 192), (128, 128)), ((3, 16, 16, 192), (128, 128)),                                        # image boundaries inside / at a tile edge
    ((1, 11, 349, 1088), (128, 256)), ((1, 60, 64, 1088), (128, 256)), ((1, 23, 167, 1088), (128, 256)),  # M = 3839 / 3840 / 3841
    ((2, 30, 65, 1088), (128, 256)),                                                                     # M = 3900, the boundary at 1950
]
EDGE_CO = 64


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("edge,form", EDGES, ids=["%dx%dx%d_ci%d" % e for e, _f in EDGES])
def test_the_kernels_own_edges_equal_fp64(rt, edge, form, k):
    n, H, W, ci = edge
    c = cb.Case(k, n, H, W, ci, EDGE_CO)
    assert rt.conv2d_backward_data_form_split(n, H, W, ci, EDGE_CO, k) == form, "these sizes are chosen for this block form"
    inp = cb.int_inputs(c)
    g, w = inp["g"].numpy(), inp["w"].numpy()
    ref = torch.from_numpy(dg.direct(g, w))                          # (equal to torch's fp64 dX: tests/test_conv_dgrad_split_abi.py)
    cap = float(dg.direct(np.abs(g), np.abs(w)).max()) + 64.0
    assert cap < cb.LIMIT, "%s: sum of |terms| %.0f is not below 2^23" % (cb.case_id(c), cap)
    gd, wd = inp["g"].cuda(), inp["w"].cuda()
    dx = torch.full((n, H, W, ci), NAN, device="cuda")
    split_dgrad(rt, gd, wd, k, dx=dx)
    acc = inp["dx0"].cuda()
    split_dgrad(rt, gd, wd, k, dx=acc, accumulate=True)
    torch.cuda.synchronize()
    exact.assert_exact(dx.cpu(), ref, "%s dX" % cb.case_id(c))
    exact.assert_exact(acc.cpu(), ref + inp["dx0"].double(), "%s dX, accumulate" % cb.case_id(c))


# ---- 2. 17-bit integers ----

@pytest.mark.parametrize("side", ["g", "w"])
@pytest.mark.parametrize("c", chk.WIDE[1, "dgrad"][1], ids=cb.case_id)
def test_wide_integers_equal_fp64(rt, c, side):
    chk.dgrad_wide(rt, cb, c, side)


# ---- 3. the inequality ----

def check_inequality(rt, what, k, g, w, dx_gpu, base=None):
    return chk.dgrad_inequality(rt, cb, what, k, g, w, dx_gpu, base=base)


SHAPE_IDS = ["%dx%d_%dto%d_k%d" % (s[0], s[0], s[1], s[2], s[3]) for s in cb.FUSION_SHAPES]


@pytest.mark.parametrize("pattern,signs", chk.ADV, ids=chk.ADV_IDS)
@pytest.mark.parametrize("shape", cb.FUSION_SHAPES, ids=SHAPE_IDS)
def test_worst_case_mantissas(rt, shape, pattern, signs):
    H, ci, co, k = shape
    chk.dgrad_worst(rt, cb, SHAPE_IDS[cb.FUSION_SHAPES.index(shape)], (k, 1, H, H, ci, co), pattern, signs)


@pytest.mark.parametrize("shape", cb.FUSION_SHAPES, ids=SHAPE_IDS)
def test_normal_data_within_the_bound(rt, shape):
    H, ci, co, k = shape
    c = cb.Case(k, 1, H, H, ci, co)
    chk.dgrad_normal(rt, cb, cb.case_id(c), c)


# ---- 4. discipline ----

DISCIPLINE = [cb.Case(3, 3, 14, 14, 64, 128), cb.Case(1, 2, 5, 3, 192, 64), cb.Case(3, 2, 30, 65, 1088, 64)]      # one per block form


@pytest.mark.parametrize("c", DISCIPLINE, ids=cb.case_id)
def test_scratch_contents_never_show_and_replay_equals_eager(rt, c):
    chk.dgrad_discipline(rt, cb, c)


def test_a_refused_call_writes_nothing(rt):
    c = cb.Case(3, 2, 5, 3, 128, 64)
    inp = cb.normal_inputs(c)
    g, w = inp["g"].cuda(), inp["w"].cuda()
    nbytes = rt.conv2d_backward_data_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)
    A = arena.Arena.for_sizes([c.n * c.H * c.W * c.ci * 4, nbytes])
    dx, s = A.empty("dx", (c.n, c.H, c.W, c.ci)), A.carve("scratch", nbytes)
    with pytest.raises(_lib.OffkError, match="offk_conv2d_backward_data_split: pad must be"):
        rt.conv2d_backward_data(g, w, 0, dx=dx, scratch=s, arith="f32split")
    with pytest.raises(_lib.OffkError, match="offk_conv2d_backward_data_split: dx: cstride < coff \\+ C"):
        rt.conv2d_backward_data(g, w, 1, dx=dx, dx_coff=4, scratch=s, arith="f32split")
    lib = _lib.load()
    rc = lib.offk_conv2d_backward_data_split(None, g.data_ptr(), c.co, 0, c.n, c.H, c.W, c.co, w.data_ptr(), c.ci, 3, 3, 1, dx.data_ptr(), c.ci, 0, 0,
                                             s.data_ptr(), nbytes - 1)
    assert rc == -1 and b"offk_conv2d_backward_data_split: scratch too small" in lib.offk_last_error(None)
    rc = lib.offk_conv2d_backward_data_split(None, g.data_ptr(), c.co, 0, c.n, c.H, c.W, c.co, w.data_ptr(), c.ci, 3, 3, 1, dx.data_ptr(), c.ci, 0, 0,
                                             s.data_ptr() + 8, nbytes)
    assert rc == -1 and b"offk_conv2d_backward_data_split: scratch must be 16-byte aligned" in lib.offk_last_error(None)
    torch.cuda.synchronize()
    assert A.untouched(dx) and A.untouched(s)
    A.check()


# ---- 5. the module ----

MODULES = [("conv3x3", 64, 128, 3, 1, True, 9, 7), ("conv1x1", 192, 64, 1, 1, False, 9, 7), ("open28", 64, 64, 7, 2, True, 12, 20)]  # name, ci, co, k, stride, relu, H, W
MOD_N = 2


def make_module(spec, params, **kw):
    from offk_amd.off_module import FusionConv2d
    _name, ci, co, k, stride, relu, _H, _W = spec
    m = FusionConv2d(ci, co, k, stride=stride, padding=(k - 1) // 2, relu=relu, **kw)
    m.load_state_dict(params)
    return m.cuda()


def run_module(m, x, t, x_grad=True):
    x = x.clone().requires_grad_(x_grad)
    for p in m.parameters():
        p.grad = None
    y = m(x)
    y.retain_grad()
    (y * t).sum().backward()
    return x, y


@pytest.mark.parametrize("spec", MODULES, ids=[s[0] for s in MODULES])
def test_module_bwd_arith_routes_every_gradient_that_has_a_split_entry(rt, spec, monkeypatch):
    from offk_amd.off_module import FusionConv2d
    from . import conv_s2_dgrad_split as ds
    name, ci, co, k, stride, relu, H, W = spec
    gen = torch.Generator().manual_seed(0x3D5 + k)
    params = {"weight": torch.randn(co, ci, k, k, generator=gen) / (ci * k * k) ** 0.5, "bias": torch.randn(co, generator=gen) * 0.1}
    xd = torch.randn(MOD_N, ci, H, W, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    td = torch.randn(MOD_N, co, H // stride, W // stride, generator=gen).cuda().contiguous(memory_format=torch.channels_last)
    split, plain = make_module(spec, params, bwd_arith="f32split"), make_module(spec, params)
    # the module the older keywords give: the same dW / db (stride 1) or the same dX (stride 2), bit for bit
    older = make_module(spec, params, **({"wgrad_arith": "f32split"} if stride == 1 else {"dgrad_arith": "f32split"}))
    assert split.bwd_arith == "f32split" and plain.bwd_arith == "fp32"
    xs, ys = run_module(split, xd, td)
    xp, yp = run_module(plain, xd, td)
    xo, yo = run_module(older, xd, td)
    torch.cuda.synchronize()
    assert arena.same_bits(ys.detach(), yp.detach()) and arena.same_bits(yo.detach(), yp.detach()), "the forward"
    # the operands as the node saw them: the gradient behind the ReLU mask, channels-last rows
    g = yp.grad * (yp.detach() > 0) if relu else yp.grad
    gr = g.permute(0, 2, 3, 1).contiguous()
    wt = plain.weight.detach()
    pad = (k - 1) // 2
    fp32_dx = rt.conv2d_backward_data(gr, wt, pad) if stride == 1 else rt.conv2d_s2_backward_data(gr, wt, pad)
    assert arena.same_bits(xp.grad.permute(0, 2, 3, 1), fp32_dx), "the default module is the fp32 entry, bit for bit"
    xr = xd.permute(0, 2, 3, 1).contiguous()
    if stride == 1:
        dw, db = rt.conv2d_backward_weight(xr, gr, k, pad)
        assert arena.same_bits(split.weight.grad, older.weight.grad) and arena.same_bits(split.bias.grad, older.bias.grad), "dW and db: the split entry"
        assert not arena.same_bits(split.weight.grad, plain.weight.grad), "the switch reached the weight gradient"
        assert arena.same_bits(xo.grad, xp.grad), "wgrad_arith alone leaves dX on the fp32 entry"
    else:
        dw, db = rt.conv2d_s2_backward_weight(xr, gr, k, pad)
        assert arena.same_bits(split.weight.grad, dw) and arena.same_bits(split.bias.grad, db), "stride 2: dW and db stay on the fp32 entry"
        assert arena.same_bits(xs.grad, xo.grad), "stride 2: the dgrad_arith module's dX"
    assert arena.same_bits(plain.weight.grad, dw) and arena.same_bits(plain.bias.grad, db), "the default module's dW and db"
    got = xs.grad.permute(0, 2, 3, 1).contiguous()
    assert not arena.same_bits(xs.grad, xp.grad), "the switch reached the data gradient"
    if stride == 1:
        assert arena.same_bits(got, rt.conv2d_backward_data(gr, wt, pad, arith="f32split")), "the split entry, bit for bit"
        check_inequality(rt, "module %s" % name, k, gr.cpu().numpy(), wt.cpu().numpy(), got)
    else:
        ref, dropped, mag = ds.terms(gr.cpu().numpy(), wt.cpu().numpy())
        emu = ds.emulate(gr.cpu().numpy(), wt.cpu().numpy())
        A = max(1.0, 2.0 * sb.c_acc(emu, ref, dropped, mag))
        assert sb.excess(got.cpu().numpy(), ref, dropped, mag, A) <= 0.0, "the stride-2 entry's inequality"
    # a frozen layer launches no weight gradient; an input that needs no gradient no data gradient
    calls = []
    real_s1, real_s2 = rt.conv2d_backward_data, rt.conv2d_s2_backward_data
    monkeypatch.setattr(rt, "conv2d_backward_data", lambda *a, **kw: (calls.append(("s1", kw.get("arith", "fp32"))), real_s1(*a, **kw))[1])
    monkeypatch.setattr(rt, "conv2d_s2_backward_data", lambda *a, **kw: (calls.append(("s2", kw.get("arith", "fp32"))), real_s2(*a, **kw))[1])
    before = FusionConv2d.weight_grad_launches
    run_module(split, xd, td, x_grad=False)
    assert calls == [] and FusionConv2d.weight_grad_launches == before + 1
    for p in split.parameters():
        p.requires_grad_(False)
    xf, _yf = run_module(split, xd, td)
    torch.cuda.synchronize()
    assert FusionConv2d.weight_grad_launches == before + 1, "a frozen layer launches no weight gradient"
    assert split.weight.grad is None and arena.same_bits(xf.grad, xs.grad)
    run_module(plain, xd, td)
    assert calls == [("s%d" % stride, "f32split"), ("s%d" % stride, "fp32")]
