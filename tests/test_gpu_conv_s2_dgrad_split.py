"""The stride-2 fusion convs' data gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_s2_backward_data_split,
csrc/conv_dgrad_s2_split.hip; runtime.conv2d_s2_backward_data(arith="f32split"), FusionConv2d(dgrad_arith="f32split")).

 1. exact integers: dX EQUAL to the fp64 reference at all ten cases of tests/conv_bwd.S2.cases() (both real shapes at n = 1, the half ci
    tiles 96 / 160 / 1056, the non-square 6x10 and 6x4 maps, the 2x2 map with M = 1), with and without accumulate, and again on middle
    channel slices of g and dx inside a NaN-guarded arena;
 2. 17-bit integers: three non-zero planes in g against single-plane weights and the reverse: equal to fp64 -- the plane indexing of the
    five products with a leading plane, exactly;
 3. worst-case mantissas: per element of dX, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|g w| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation constant on the same operands in the kernel's K order (tests/conv_s2_dgrad_split.py) -- never
    the kernel's output; tests/test_conv_s2_dgrad_split_abi.py shows on the CPU that losing any one issued product breaks it;
 4. the same inequality on normal data at both real shapes (n = 1); emulated against measured c_acc and the fp32 entry's error are printed;
 5. discipline: equal bits from NaN- and -3-filled scratch, graph replay == eager, a refused call writes nothing;  6. the module.

The bodies the two strides share are tests/conv_grad_checks.py's, written against tests/conv_bwd.py's forms; this file keeps the test
names, the parametrize lists and what this stride alone has."""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib

from . import arena
from . import conv_grad_checks as chk
from .conv_bwd import S2 as cs
from .conv_grad_checks import rt  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = cs.cases()
IDS = [cs.case_id(c) for c in CASES]


def resolve(rt, c):
    return chk.resolve(rt, cs, c)


def split_dgrad(rt, g, w, k, **kw):
    return chk.split_dgrad(rt, cs, g, w, k, **kw)


# ---- 1. exact integers ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    chk.dgrad_dense(rt, cs, resolve(rt, c), accumulate)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    chk.dgrad_slices(rt, cs, resolve(rt, c), accumulate)


# ---- 2. 17-bit integers ----

@pytest.mark.parametrize("side", ["g", "w"])
@pytest.mark.parametrize("c", chk.WIDE[2, "dgrad"][1], ids=cs.case_id)
def test_wide_integers_equal_fp64(rt, c, side):
    chk.dgrad_wide(rt, cs, c, side)


# ---- 3. / 4. the inequality ----

@pytest.mark.parametrize("pattern,signs", chk.ADV, ids=chk.ADV_IDS)
@pytest.mark.parametrize("shape", cs.WORST, ids=["k7_2x6x10_64to64", "k5_2x6x4_96to64"])
def test_worst_case_mantissas(rt, shape, pattern, signs):
    chk.dgrad_worst(rt, cs, "k%d" % shape[0], shape, pattern, signs)


@pytest.mark.parametrize("real", cs.REAL, ids=[r[0] for r in cs.REAL])
def test_normal_data_within_the_bound(rt, real):
    key, ci, co, k, H = real
    chk.dgrad_normal(rt, cs, key, cs.Case(k, 1, H, H, ci, co))


# ---- 5. discipline ----

DISCIPLINE = [cs.Case(7, 3, 14, 14, 96, 128), cs.Case(5, 2, 6, 4, 160, 64)]


@pytest.mark.parametrize("c", DISCIPLINE, ids=cs.case_id)
def test_scratch_contents_never_show_and_replay_equals_eager(rt, c):
    chk.dgrad_discipline(rt, cs, c)


def test_a_refused_call_writes_nothing(rt):
    c = cs.Case(5, 2, 6, 4, 96, 64)
    inp = cs.normal_inputs(c)
    g, w = inp["g"].cuda(), inp["w"].cuda()
    nbytes = rt.conv2d_s2_backward_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)
    A = arena.Arena.for_sizes([c.n * c.H * c.W * c.ci * 4, nbytes])
    dx, s = A.empty("dx", (c.n, c.H, c.W, c.ci)), A.carve("scratch", nbytes)
    with pytest.raises(_lib.OffkError, match="offk_conv2d_s2_backward_data_split: the form must be"):
        rt.conv2d_s2_backward_data(g, w, 3, dx=dx, scratch=s, arith="f32split")
    with pytest.raises(_lib.OffkError, match="offk_conv2d_s2_backward_data_split: dx: cstride < coff \\+ C"):
        rt.conv2d_s2_backward_data(g, w, 2, dx=dx, dx_coff=4, scratch=s, arith="f32split")
    lib = _lib.load()
    rc = lib.offk_conv2d_s2_backward_data_split(None, g.data_ptr(), c.co, 0, c.n, c.H, c.W, c.co, w.data_ptr(), c.ci, 5, 5, 2, dx.data_ptr(), c.ci, 0, 0,
                                                s.data_ptr(), nbytes - 1)
    assert rc == -1 and b"offk_conv2d_s2_backward_data_split: scratch too small" in lib.offk_last_error(None)
    torch.cuda.synchronize()
    assert A.untouched(dx) and A.untouched(s)
    A.check()


# ---- 6. the module ----

OPENERS = [("open28", 64, 64, 7, True, 12, 20), ("open14", 96, 64, 5, False, 12, 8)]         # name, ci, co, k, relu, H, W
MOD_N = 2


def make_opener(spec, arith, params):
    from offk_amd.off_module import FusionConv2d
    _name, ci, co, k, relu, _H, _W = spec
    m = FusionConv2d(ci, co, k, stride=2, padding=cs.FORMS[k], relu=relu, **({} if arith is None else {"dgrad_arith": arith}))
    m.load_state_dict(params)
    return m.cuda()


def run_opener(m, x, t, x_grad=True):
    x = x.clone().requires_grad_(x_grad)
    for p in m.parameters():
        p.grad = None
    y = m(x)
    y.retain_grad()
    (y * t).sum().backward()
    return x, y


@pytest.mark.parametrize("spec", OPENERS, ids=[s[0] for s in OPENERS])
@pytest.mark.parametrize("kind", ["normal", "int"])
def test_module_routes_only_the_data_gradient(rt, spec, kind, monkeypatch):
    name, ci, co, k, relu, H, W = spec
    gen = torch.Generator().manual_seed(0x2D5 + k)
    if kind == "normal":
        params = {"weight": torch.randn(co, ci, k, k, generator=gen) / (ci * k * k) ** 0.5, "bias": torch.randn(co, generator=gen) * 0.1}
        x0, t0 = torch.randn(MOD_N, ci, H, W, generator=gen), torch.randn(MOD_N, co, H // 2, W // 2, generator=gen)
    else:
        params = {"weight": torch.randint(-2, 3, (co, ci, k, k), generator=gen).float(), "bias": torch.randint(-4, 5, (co,), generator=gen).float()}
        x0 = torch.randint(-2, 3, (MOD_N, ci, H, W), generator=gen).float()
        t0 = torch.randint(-4, 5, (MOD_N, co, H // 2, W // 2), generator=gen).float()
    xd = x0.cuda().contiguous(memory_format=torch.channels_last)
    td = t0.cuda().contiguous(memory_format=torch.channels_last)
    split, fp32, plain = make_opener(spec, "f32split", params), make_opener(spec, "fp32", params), make_opener(spec, None, params)
    assert split.dgrad_arith == "f32split" and plain.dgrad_arith == "fp32"
    xs, ys = run_opener(split, xd, td)
    xf, yf = run_opener(fp32, xd, td)
    xp, yp = run_opener(plain, xd, td)
    torch.cuda.synchronize()
    assert arena.same_bits(ys.detach(), yf.detach()) and arena.same_bits(yp.detach(), yf.detach()), "the forward"
    for a in (split, plain):
        assert arena.same_bits(a.weight.grad, fp32.weight.grad) and arena.same_bits(a.bias.grad, fp32.bias.grad), "dW and db"
    assert arena.same_bits(xp.grad, xf.grad)
    # the operands as the node saw them: the gradient behind the ReLU mask, channels-last rows
    g = yf.grad * (yf.detach() > 0) if relu else yf.grad
    gr = g.permute(0, 2, 3, 1).contiguous()
    direct = rt.conv2d_s2_backward_data(gr, fp32.weight.detach(), cs.FORMS[k])
    assert arena.same_bits(xp.grad.permute(0, 2, 3, 1), direct), "the default module is the fp32 entry, bit for bit"
    got = xs.grad.permute(0, 2, 3, 1).contiguous()
    if kind == "int":
        assert torch.equal(xs.grad, xf.grad), "integers are exact in both arithmetics"
        assert bool((xs.grad != 0).any())
    else:
        chk.dgrad_inequality(rt, cs, "module %s" % name, k, gr.cpu().numpy(), fp32.weight.detach().cpu().numpy(), got)
        assert not arena.same_bits(xs.grad, xf.grad), "the switch reached the kernel"
    # an input that needs no gradient: no data-gradient launch
    calls = []
    real_entry = rt.conv2d_s2_backward_data
    monkeypatch.setattr(rt, "conv2d_s2_backward_data", lambda *a, **kw: (calls.append(kw.get("arith", "fp32")), real_entry(*a, **kw))[1])
    run_opener(split, xd, td, x_grad=False)
    assert calls == []
    run_opener(split, xd, td)
    run_opener(plain, xd, td)
    torch.cuda.synchronize()
    assert calls == ["f32split", "fp32"]
    assert arena.same_bits(split.weight.grad, fp32.weight.grad)
