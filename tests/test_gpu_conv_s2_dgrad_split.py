"""The stride-2 fusion convs' data gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_s2_backward_data_split,
csrc/conv_dgrad_s2_split.hip; runtime.conv2d_s2_backward_data(arith="f32split"), FusionConv2d(dgrad_arith="f32split")).

 1. exact integers: dX EQUAL to the fp64 reference at all ten cases of tests/conv_bwd_s2.cases() (both real shapes at n = 1, the half ci
    tiles 96 / 160 / 1056, the non-square 6x10 and 6x4 maps, the 2x2 map with M = 1), with and without accumulate, and again on middle
    channel slices of g and dx inside a NaN-guarded arena;
 2. 17-bit integers: three non-zero planes in g against single-plane weights and the reverse: equal to fp64 -- the plane indexing of the
    five products with a leading plane, exactly;
 3. worst-case mantissas: per element of dX, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|g w| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation constant on the same operands in the kernel's K order (tests/conv_s2_dgrad_split.py) -- never
    the kernel's output; tests/test_conv_s2_dgrad_split_abi.py shows on the CPU that losing any one issued product breaks it;
 4. the same inequality on normal data at both real shapes (n = 1); emulated against measured c_acc and the fp32 entry's error are printed;
 5. discipline: equal bits from NaN- and -3-filled scratch, graph replay == eager, a refused call writes nothing;  6. the module."""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from . import arena
from . import conv_bwd_s2 as cs
from . import conv_s2_dgrad_split as ds
from . import exact
from .test_conv_s2_dgrad_split_abi import WORST, worst_inputs

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = cs.cases()
IDS = [cs.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def resolve(rt, c):
    return cs.resolve(rt.conv2d_s2_backward_plan, c)


def filled_bytes(n, value=NAN):
    return torch.full(((n + 3) // 4,), value, device="cuda").view(torch.uint8)[:n]


def split_dgrad(rt, g, w, k, **kw):
    return rt.conv2d_s2_backward_data(g, w, cs.FORMS[k], arith="f32split", **kw)


# ---- 1. exact integers ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    c = resolve(rt, c)
    inp, ref = cs.cached(c, "int", False)
    cs.check_caps(c, inp, ref)
    nbytes = rt.conv2d_s2_backward_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)
    dx = inp["dx0"].cuda() if accumulate else torch.full((c.n, c.H, c.W, c.ci), NAN, device="cuda")
    split_dgrad(rt, inp["g"].cuda(), inp["w"].cuda(), c.k, dx=dx, accumulate=accumulate, scratch=filled_bytes(nbytes))
    torch.cuda.synchronize()
    exact.assert_exact(dx.cpu(), ref["dX"] + (inp["dx0"].double() if accumulate else 0.0), "%s dX" % cs.case_id(c))


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    c = resolve(rt, c)
    inp, ref = cs.cached(c, "int", False)
    n, H, W, ci, co, k = c.n, c.H, c.W, c.ci, c.co, c.k
    nbytes = rt.conv2d_s2_backward_plan_split(n, H, W, ci, co, k)
    A = arena.Arena.for_sizes([n * (H // 2) * (W // 2) * 3 * co * 4, n * H * W * 3 * ci * 4, co * ci * k * k * 4, nbytes])
    gb = A.empty("g", (n, H // 2, W // 2, 3 * co))             # outer slices: the arena's NaN sentinel
    dxb = A.empty("dx", (n, H, W, 3 * ci))
    gb[..., co:2 * co] = inp["g"].cuda()
    if accumulate:
        dxb[..., ci:2 * ci] = inp["dx0"].cuda()
    w = A.put("w", inp["w"].cuda())
    s = A.carve("scratch", nbytes)
    split_dgrad(rt, gb, w, k, g_coff=co, dx=dxb, dx_coff=ci, accumulate=accumulate, scratch=s)
    torch.cuda.synchronize()
    exact.assert_exact(dxb[..., ci:2 * ci].cpu(), ref["dX"] + (inp["dx0"].double() if accumulate else 0.0), "%s dX slice" % cs.case_id(c))
    assert A.untouched(dxb[..., :ci]) and A.untouched(dxb[..., 2 * ci:]) and A.untouched(gb[..., :co]) and A.untouched(gb[..., 2 * co:])
    assert torch.equal(w.cpu(), inp["w"]), "the weight is read in place"
    A.check()


# ---- 2. 17-bit integers ----

def wide_ints(seed, shape, one_in):
    """sparse odd integers of 17 significant bits, either sign: bit 16, seven random bits, bit 8, seven random bits, bit 0 -- the leading
    plane takes bits 16 .. 9, the middle one bits 8 .. 1, the last one bit 0"""
    hi = exact.ints(exact.stream(seed, 1, 0), shape, 0, 127)
    lo = exact.ints(exact.stream(seed, 2, 0), shape, 0, 127)
    sign = exact.ints(exact.stream(seed, 3, 0), shape, 0, 1) * 2 - 1
    on = (exact.ints(exact.stream(seed, 4, 0), shape, 0, one_in - 1) == 0).float()
    return (65536 + hi * 512 + 256 + lo * 2 + 1) * sign * on


@pytest.mark.parametrize("side", ["g", "w"])
@pytest.mark.parametrize("c", [cs.Case(7, 2, 6, 10, 64, 64), cs.Case(5, 2, 6, 4, 96, 64)], ids=cs.case_id)
def test_wide_integers_equal_fp64(rt, c, side):
    inp = dict(cs.int_inputs(c))
    inp[side] = wide_ints(0x5D2 + c.k + (7 if side == "g" else 0), tuple(inp[side].shape), 64 if side == "g" else 256)
    v = inp[side].numpy()
    nz = v != 0
    h, m, l = synth.cut3(v)
    assert nz.sum() > v.size // 1024 and bool((h[nz] != 0).all() and (m[nz] != 0).all() and (l[nz] != 0).all()), "three non-zero planes"
    assert bool((np.abs(v[nz]) >= 65536).all() and (np.abs(v[nz]) < 131072).all() and (v[nz] % 2 != 0).all()), "17 significant bits, odd"
    ref = cs.reference(c, inp, False)
    cap = float(ref["dX_abs"].max())
    assert cap < cs.LIMIT, "%s: sum of |terms| %.0f is not below 2^23" % (cs.case_id(c), cap)
    assert float(ref["dX"].abs().max()) >= 65536
    dx = split_dgrad(rt, inp["g"].cuda(), inp["w"].cuda(), c.k)
    torch.cuda.synchronize()
    exact.assert_exact(dx.cpu(), ref["dX"], "%s dX, wide %s" % (cs.case_id(c), side))


# ---- 3. / 4. the inequality ----

def check_inequality(rt, what, k, g, w, dx_gpu, base=None):
    """asserts the inequality per element of dX; returns (emulated c_acc, measured accumulation constant, the fp32 entry's error in the same
    unit).  g [n, OH, OW, co], w [co, ci, k, k]: numpy"""
    ref, dropped, mag = ds.terms(g, w)
    emu = ds.emulate(g, w)
    ce = ds.c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * ce)
    got = dx_gpu.cpu().numpy()
    assert ds.excess(emu, ref, dropped, mag, A) <= 0.0, "the emulation itself"
    f32 = rt.conv2d_s2_backward_data(torch.from_numpy(g).cuda(), torch.from_numpy(w).cuda(), cs.FORMS[k]).cpu().numpy()
    cf = float((np.abs(f32.astype(np.float64) - ref) / np.maximum(ds.EPS * mag, 1e-300)).max())
    if base is None:
        cg = ds.c_acc(got, ref, dropped, mag)
        print("%s: emulated c_acc %.3f, A %.3f, gpu accumulation %.3f, dropped max %.3f; the fp32 entry's error %.3f (all x 2^-24 sum|g w|)" % (
            what, ce, A, cg, float((np.abs(dropped) / np.maximum(ds.EPS * mag, 1e-300)).max()), cf))
    else:
        cg = float("nan")
    ex = ds.excess_map(got, ref, dropped, mag, A, base=base)
    assert float(ex.max()) <= 0.0, "%s: %d of %d elements break the inequality, worst excess %.3g" % (what, int((ex > 0).sum()), ex.size, float(ex.max()))
    if base is None:
        zero = mag == 0
        assert np.array_equal(got[zero], np.zeros(int(zero.sum()), dtype=np.float32)), "an element without terms is exactly 0"
    return ce, cg, cf


ADV = [(p, s) for p in (0x00FFFF, 0x7FFFFF, 0x7F7F7F) for s in ("same", "alternating")]


@pytest.mark.parametrize("pattern,signs", ADV, ids=["0x%06X_%s" % a for a in ADV])
@pytest.mark.parametrize("shape", WORST, ids=["k7_2x6x10_64to64", "k5_2x6x4_96to64"])
def test_worst_case_mantissas(rt, shape, pattern, signs):
    """g alternates in sign along co (the contraction index) in the "alternating" mode: sum g w << sum |g w|."""
    g, w = worst_inputs(shape, pattern, signs)
    for v in (g, w):
        nz = v != 0
        assert bool(((v.view(np.uint32) & 0x7FFFFF) == pattern)[nz].all()) and nz.sum() > v.size // 4
    dx = split_dgrad(rt, torch.from_numpy(g).cuda(), torch.from_numpy(w).cuda(), shape[0])
    torch.cuda.synchronize()
    check_inequality(rt, "worst case k%d 0x%06X %-11s" % (shape[0], pattern, signs), shape[0], g, w, dx)


@pytest.mark.parametrize("real", cs.REAL, ids=[r[0] for r in cs.REAL])
def test_normal_data_within_the_bound(rt, real):
    key, ci, co, k, H = real
    c = cs.Case(k, 1, H, H, ci, co)
    inp = cs.normal_inputs(c)
    g, w = inp["g"].numpy(), inp["w"].numpy()
    dx = split_dgrad(rt, inp["g"].cuda(), inp["w"].cuda(), k)
    torch.cuda.synchronize()
    check_inequality(rt, "normal data %s" % key, k, g, w, dx)
    # accumulate: one more 2^-24 |result|
    gen = torch.Generator().manual_seed(7)
    base = torch.randn(1, H, H, ci, generator=gen)
    dxa = base.cuda()
    split_dgrad(rt, inp["g"].cuda(), inp["w"].cuda(), k, dx=dxa, accumulate=True)
    torch.cuda.synchronize()
    check_inequality(rt, "normal data %s, accumulate" % key, k, g, w, dxa, base=base.numpy())


# ---- 5. discipline ----

DISCIPLINE = [cs.Case(7, 3, 14, 14, 96, 128), cs.Case(5, 2, 6, 4, 160, 64)]


@pytest.mark.parametrize("c", DISCIPLINE, ids=cs.case_id)
def test_scratch_contents_never_show_and_replay_equals_eager(rt, c):
    inp = cs.normal_inputs(c)
    g, w = inp["g"].cuda(), inp["w"].cuda()
    nbytes = rt.conv2d_s2_backward_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)
    A = arena.Arena.for_sizes([c.n * c.H * c.W * c.ci * 4, nbytes] * 3)

    def buffers(tag, fill):
        b = {"dx": A.empty("dx" + tag, (c.n, c.H, c.W, c.ci)), "s": A.carve("scratch" + tag, nbytes)}
        if fill is not None:
            b["s"].view(torch.float32).fill_(fill)
        return b

    def run(b):
        split_dgrad(rt, g, w, c.k, dx=b["dx"], scratch=b["s"])

    first, second, cap = buffers("1", None), buffers("2", -3.0), buffers("3", None)        # NaN sentinel | -3 | NaN sentinel
    run(first)
    run(second)
    torch.cuda.synchronize()
    assert arena.same_bits(first["dx"], second["dx"]), "dx depends on what the scratch held"
    assert not bool(first["dx"].isnan().any())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: the three launches of the entry in order
        run(cap)
    for _ in range(2):
        cap["dx"].fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert arena.same_bits(cap["dx"], first["dx"]), "replay differs from the eager run"
    A.check()


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
        check_inequality(rt, "module %s" % name, k, gr.cpu().numpy(), fp32.weight.detach().cpu().numpy(), got)
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
