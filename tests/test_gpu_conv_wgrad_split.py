"""The fusion convs' weight / bias gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_backward_weight_split,
csrc/conv_wgrad_split.hip; runtime.conv2d_backward_weight(arith="f32split"), FusionConv2d(wgrad_arith="f32split")).

 1. exact integers: every case of tests/conv_bwd.cases() (the plan-chosen n from the SPLIT plan) and 2. the maps on both sides of the pitch's
    boundaries (W = 7, 8, 15, 16) and of the staged windows' (W = 23, 24: adjacent from pitch 32 on; W = 31, 32: disjoint from pitch 40 on): dW and db EQUAL the fp64 reference, with and without accumulate, with relu_in, without db, on middle
    channel slices in a guarded arena;
 3. wide integers: one operand 17-bit odd integers whose three planes are all non-zero, on either side: equal to fp64 -- the plane indexing
    of the five products with a leading plane, exactly;
 4. worst-case mantissas on g and x: per element of dW, none excluded,
        |gpu - ref64| <= |dropped64| + A 2^-24 sum|g x| + 2^-24 |ref64|,   A = max(1, 2 c_acc),
    c_acc the CPU EMULATION's accumulation constant on the same operands in the kernel's chunked K layout (tests/conv_wgrad_split.py) --
    never the kernel's output; tests/test_conv_wgrad_split_abi.py shows on the CPU that losing any one issued product breaks it;
 5. the same inequality on normal data at the 13 fusion shapes, db within gamma(n H W) sum|g|;
 6. discipline: equal bits from NaN- and -3-filled scratch, graph replay == eager, guard bands, a refused call writes nothing;  7. the module."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from . import arena
from . import conv_bwd as cb
from . import conv_wgrad_split as cs
from . import exact

pytestmark = pytest.mark.gpu
NAN = float("nan")
# pitch 8 | 16 | 16 | 24 (one zero column ... eight), then 24 | 32 where the kernel rows' windows stop overlapping (pg = pitch / 8 clamps at 4, 12 k
# groups staged) and 32 | 40 where they stop touching (the rows' shifts are no longer consecutive k groups; the 120 KB launch)
EDGES = [cb.Case(3, 2, 3, W, 64, 64) for W in (7, 8, 15, 16, 23, 24, 31, 32)]
CASES = cb.cases() + EDGES
IDS = [cb.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def split_plan3(rt):
    """the split plan in the shape tests/conv_bwd.chunked_n reads ((data bytes, weight bytes, chunks))"""
    return lambda *a: (0,) + rt.conv2d_backward_plan_split(*a)


def resolve(rt, c):
    """the plan-chosen case: n such that the SPLIT weight gradient runs in >= 3 chunks with a shorter last one (asserted here)"""
    if c.n is not None:
        return c
    n = cb.chunked_n(split_plan3(rt), c)
    chunks = rt.conv2d_backward_plan_split(n, c.H, c.W, c.ci, c.co, c.k)[1]
    ipc = -(-n // chunks)
    assert chunks >= 3 and 0 < n - (chunks - 1) * ipc < ipc, (n, chunks, ipc)
    return c._replace(n=n)


def filled_bytes(n, value=NAN):
    return torch.full(((n + 3) // 4,), value, device="cuda").view(torch.uint8)[:n]


def split_wgrad(rt, x, g, c, **kw):
    return rt.conv2d_backward_weight(x, g, c.k, (c.k - 1) // 2, arith="f32split", **kw)


# ---- 1. / 2. exact integers ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    c = resolve(rt, c)
    inp, ref = cb.cached(c, "int", False)
    cb.check_caps(c, inp, ref)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes = rt.conv2d_backward_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)[0]
    if accumulate:
        dw, db = inp["dw0"].cuda(), inp["db0"].cuda()
    else:
        dw, db = torch.full((c.co, c.ci, c.k, c.k), NAN, device="cuda"), torch.full((c.co,), NAN, device="cuda")
    split_wgrad(rt, x, g, c, dw=dw, db=db, accumulate=accumulate, scratch=filled_bytes(wbytes))
    torch.cuda.synchronize()
    base = {"dW": inp["dw0"].double(), "db": inp["db0"].double()} if accumulate else {}
    mm = exact.Mismatches()
    for name, got in (("dW", dw), ("db", db)):
        mm.check(got.cpu(), ref[name] + base.get(name, 0.0), "%s %s" % (cb.case_id(c), name))
    mm.raise_if_any()
    if c.k == 3 and c.H == 1 and c.W == 1 and not accumulate:
        taps = dw.cpu().reshape(c.co, c.ci, 9)
        assert torch.equal(taps[:, :, [0, 1, 2, 3, 5, 6, 7, 8]], torch.zeros(c.co, c.ci, 8)), "a 1x1 map feeds the centre tap only"
        assert bool((taps[:, :, 4] != 0).any())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bias_gradient_is_optional(rt, c):
    c = resolve(rt, c)
    inp, ref = cb.cached(c, "int", False)
    A = arena.Arena.for_sizes([c.co * c.ci * c.k * c.k * 4])
    dw = A.empty("dw", (c.co, c.ci, c.k, c.k))
    got, db = split_wgrad(rt, inp["x"].cuda(), inp["g"].cuda(), c, dw=dw, want_db=False)
    torch.cuda.synchronize()
    assert db is None
    exact.assert_exact(got.cpu(), ref["dW"], "dW without db")
    A.check()


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relu_in_and_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    c = resolve(rt, c)
    inp, ref = cb.cached(c, "int", True)
    cb.check_caps(c, inp, ref)
    n, H, W, ci, co, k = c.n, c.H, c.W, c.ci, c.co, c.k
    wbytes = rt.conv2d_backward_plan_split(n, H, W, ci, co, k)[0]
    px = n * H * W
    A = arena.Arena.for_sizes([px * 3 * ci * 4, px * 3 * co * 4, co * ci * k * k * 4, co * 4, wbytes])
    xb = A.empty("x", (n, H, W, 3 * ci))               # outer slices: the arena's NaN sentinel
    gb = A.empty("g", (n, H, W, 3 * co))
    xb[..., ci:2 * ci] = inp["x"].cuda()
    gb[..., co:2 * co] = inp["g"].cuda()
    if accumulate:
        dw, db = A.put("dw", inp["dw0"].cuda()), A.put("db", inp["db0"].cuda())
    else:
        dw, db = A.empty("dw", (co, ci, k, k)), A.empty("db", (co,))
    sw = A.carve("weight_scratch", wbytes)
    split_wgrad(rt, xb, gb, c, relu_in=True, x_coff=ci, ci=ci, g_coff=co, co=co, dw=dw, db=db, accumulate=accumulate, scratch=sw)
    torch.cuda.synchronize()
    b = (lambda name: inp[name].double()) if accumulate else (lambda name: 0.0)
    mm = exact.Mismatches()
    mm.check(dw.cpu(), ref["dW"] + b("dw0"), "%s dW, relu_in" % cb.case_id(c))
    mm.check(db.cpu(), ref["db"] + b("db0"), "%s db" % cb.case_id(c))
    mm.raise_if_any()
    assert A.untouched(xb[..., :ci]) and A.untouched(xb[..., 2 * ci:]) and A.untouched(gb[..., :co]) and A.untouched(gb[..., 2 * co:])
    assert not bool(sw.view(torch.float32).isnan().any()), "every slab element is written (by exactly one thread)"
    A.check()


# ---- 3. wide integers ----

def wide_ints(seed, shape):
    """sparse (one in thirty-two: about five wide terms per output, sum of |terms| near 2^22) odd integers of 17 significant bits, either sign: bit 16, seven random bits, bit 8, seven random bits, bit 0 --
    the leading plane takes bits 16 .. 9, the middle one bits 8 .. 1, the last one bit 0"""
    hi = exact.ints(exact.stream(seed, 1, 0), shape, 0, 127)
    lo = exact.ints(exact.stream(seed, 2, 0), shape, 0, 127)
    sign = exact.ints(exact.stream(seed, 3, 0), shape, 0, 1) * 2 - 1
    on = (exact.ints(exact.stream(seed, 4, 0), shape, 0, 31) == 0).float()
    return (65536 + hi * 512 + 256 + lo * 2 + 1) * sign * on


@pytest.mark.parametrize("side", ["g", "x"])
@pytest.mark.parametrize("c", [cb.Case(3, 2, 7, 7, 64, 128), cb.Case(1, 3, 7, 7, 128, 64)], ids=lambda c: cb.case_id(c))
def test_wide_integers_equal_fp64(rt, c, side):
    inp = dict(cb.int_inputs(c))
    inp[side] = wide_ints(0x71D + c.k + (7 if side == "g" else 0), tuple(inp[side].shape))
    v = inp[side].numpy()
    nz = v != 0
    h, m, l = synth.cut3(v)
    assert nz.sum() > v.size // 64 and bool((h[nz] != 0).all() and (m[nz] != 0).all() and (l[nz] != 0).all()), "three non-zero planes"
    assert bool((np.abs(v[nz]) >= 65536).all() and (np.abs(v[nz]) < 131072).all() and (v[nz] % 2 != 0).all()), "17 significant bits, odd"
    ref = cb.reference(c, inp, False)
    for name in ("dW", "db"):
        cap = float(ref[name + "_abs"].max())
        assert cap < cb.LIMIT, "%s %s: sum of |terms| %.0f is not below 2^23" % (cb.case_id(c), name, cap)
    dw, db = split_wgrad(rt, inp["x"].cuda(), inp["g"].cuda(), c)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    mm.check(dw.cpu(), ref["dW"], "%s dW, wide %s" % (cb.case_id(c), side))
    mm.check(db.cpu(), ref["db"], "%s db, wide %s" % (cb.case_id(c), side))
    mm.raise_if_any()


# ---- 4. / 5. the inequality ----

def check_inequality(rt, what, c, g, x, dw_gpu, relu_in=False):
    """asserts the inequality per element of dW; returns (emulated c_acc, measured accumulation constant, the fp32 entry's error in the same
    unit).  g, x: numpy, channels-last"""
    chunks = rt.conv2d_backward_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)[1]
    G, taps = cs.operands(g, x, c.k, relu_in=relu_in)
    ref, dropped, mag = cs.terms(G, taps, c.k)
    emu = cs.emulate_chunked(G, taps, cs.chunk_bounds(c.n, c.H, c.W, c.k, chunks), c.k)
    ce = cs.c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * ce)
    got = dw_gpu.cpu().numpy()
    assert cs.excess(emu, ref, dropped, mag, A) <= 0.0, "the emulation itself"
    cg = cs.c_acc(got, ref, dropped, mag)
    f32 = rt.conv2d_backward_weight(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), c.k, (c.k - 1) // 2, relu_in=relu_in)[0].cpu().numpy()
    cf = float((np.abs(f32.astype(np.float64) - ref) / np.maximum(cs.EPS * mag, 1e-300)).max())
    print("%s: emulated c_acc %.3f, A %.3f, gpu accumulation %.3f, dropped max %.3f; the fp32 entry's error %.3f (all x 2^-24 sum|g x|)" % (
        what, ce, A, cg, float((np.abs(dropped) / np.maximum(cs.EPS * mag, 1e-300)).max()), cf))
    ex = cs.excess_map(got, ref, dropped, mag, A)
    assert float(ex.max()) <= 0.0, "%s: %d of %d elements break the inequality, worst excess %.3g" % (what, int((ex > 0).sum()), ex.size, float(ex.max()))
    zero = mag == 0
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()), dtype=np.float32)), "an element without terms is exactly 0"
    return ce, cg, cf


ADV = [(p, s) for p in (0x00FFFF, 0x7FFFFF, 0x7F7F7F) for s in ("same", "alternating")]
WORST_SHAPES = [cb.Case(3, 2, 5, 3, 128, 128), cb.Case(3, 2, 7, 7, 128, 128), cb.Case(3, 1, 14, 14, 64, 64), cb.Case(1, 2, 7, 7, 64, 256)]


@pytest.mark.parametrize("pattern,signs", ADV, ids=["0x%06X_%s" % a for a in ADV])
@pytest.mark.parametrize("c", WORST_SHAPES, ids=lambda c: cb.case_id(c))
def test_worst_case_mantissas(rt, c, pattern, signs):
    """x alternates in sign along the pixels (the contraction index) in the "alternating" mode: sum g x << sum |g x|."""
    px = c.n * c.H * c.W
    g = synth.make_adversarial((c.n, c.H, c.W, c.co), pattern, "same", seed=21 + c.H, relu=(pattern == 0x7FFFFF))
    x = synth.make_adversarial((px, c.ci), pattern, signs, seed=22 + c.H, k_axis=0).reshape(c.n, c.H, c.W, c.ci) * np.float32(2.0 ** -4)
    for v in (g, x):
        nz = v != 0
        assert bool(((v.view(np.uint32) & 0x7FFFFF) == pattern)[nz].all()) and nz.sum() > v.size // 4
    dw, _db = split_wgrad(rt, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), c)
    torch.cuda.synchronize()
    check_inequality(rt, "worst case %s 0x%06X %-11s" % (cb.case_id(c), pattern, signs), c, g, x, dw)


FUSION = [cb.Case(k, 2, H, H, ci, co) for H, ci, co, k in cb.FUSION_SHAPES]


@pytest.mark.parametrize("c", FUSION, ids=lambda c: cb.case_id(c))
def test_normal_data_within_the_bound(rt, c):
    inp = cb.normal_inputs(c)
    x, g = inp["x"].numpy(), inp["g"].numpy()
    dw, db = split_wgrad(rt, inp["x"].cuda(), inp["g"].cuda(), c)
    torch.cuda.synchronize()
    check_inequality(rt, "normal data %s" % cb.case_id(c), c, g, x, dw)
    g64 = g.astype(np.float64).reshape(-1, c.co)
    err = np.abs(db.cpu().numpy().astype(np.float64) - g64.sum(0))
    bound = cb.gamma(c.n * c.H * c.W) * np.abs(g64).sum(0)
    assert bool((err <= bound).all()), "db: worst error / bound %.3f" % float((err / bound).max())


# ---- 6. discipline ----

DISCIPLINE = [cb.Case(3, 5, 7, 7, 128, 64), cb.Case(1, 9, 7, 7, 64, 128), cb.Case(3, 3, 14, 14, 64, 64)]


@pytest.mark.parametrize("c", DISCIPLINE, ids=lambda c: cb.case_id(c))
def test_scratch_contents_never_show_and_replay_equals_eager(rt, c):
    inp = cb.normal_inputs(c)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes, chunks = rt.conv2d_backward_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)
    assert chunks >= 2
    A = arena.Arena.for_sizes([c.co * c.ci * c.k * c.k * 4, c.co * 4, wbytes] * 3)

    def buffers(tag, fill):
        b = {"dw": A.empty("dw" + tag, (c.co, c.ci, c.k, c.k)), "db": A.empty("db" + tag, (c.co,)), "s": A.carve("scratch" + tag, wbytes)}
        if fill is not None:
            b["s"].view(torch.float32).fill_(fill)
        return b

    def run(b):
        split_wgrad(rt, x, g, c, dw=b["dw"], db=b["db"], scratch=b["s"])

    first, second, cap = buffers("1", None), buffers("2", -3.0), buffers("3", None)        # NaN sentinel | -3 | NaN sentinel
    run(first)
    run(second)
    torch.cuda.synchronize()
    for k in ("dw", "db"):
        assert arena.same_bits(first[k], second[k]), "%s depends on what the scratch held" % k
        assert not bool(first[k].isnan().any())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(cap)
    for _ in range(2):
        for k in ("dw", "db"):
            cap[k].fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for k in ("dw", "db"):
            assert arena.same_bits(cap[k], first[k]), "replay differs from the eager run in %s" % k
    A.check()


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
        check_inequality(rt, "module %s" % name, c, gr.cpu().numpy(), hr.cpu().numpy(), split[name].weight.grad)
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
