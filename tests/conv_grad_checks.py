"""The GPU test bodies of the fusion convs' backward that are the same for both strides, written once against a form of
tests/conv_bwd.py (S1 | S2) and the runtime module.  tests/test_gpu_conv_bwd*.py (the fp32 entries: exact integers, the derived bound),
tests/test_gpu_conv*_dgrad_split.py and tests/test_gpu_conv*_wgrad_split.py (the split-fp32 entries) keep their test functions, their
parametrize lists and what only one stride has (the stride-1 kernel's own edges, the stride-2 range tests, the refusal texts, the module
tests); each shared test there is a call into this module.  Where the two strides' copies once differed in an assertion the body here
asserts both.  `filled_bytes` and the one-layer bound of the module tests (`one_layer`, `within`) live here once; the `rt` fixture is tests/featmaps.py's,
re-exported here for the conv files.  No tests of its own."""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

from offk_amd import synth

from . import arena
from . import conv_bwd
from . import conv_dgrad_split, conv_s2_dgrad_split, conv_s2_wgrad_split, conv_wgrad_split
from . import exact
from . import split_bound as sb
from .featmaps import rt  # noqa: F401

NAN = float("nan")
ADV = [(p, s) for p in (0x00FFFF, 0x7FFFFF, 0x7F7F7F) for s in ("same", "alternating")]
ADV_IDS = ["0x%06X_%s" % a for a in ADV]
# per stride: the helper module with the kernel's operands and CPU emulation (and, for the weight gradient, its chunk bounds of a case)
DGRAD = {1: conv_dgrad_split, 2: conv_s2_dgrad_split}
WGRAD = {1: (conv_wgrad_split, lambda c, chunks: conv_wgrad_split.chunk_bounds(c.n, c.H, c.W, c.k, chunks)),
         2: (conv_s2_wgrad_split, lambda c, chunks: conv_s2_wgrad_split.chunk_bounds(c.n, c.H, c.W, chunks))}
# the wide-integer tests, per (stride, gradient): (seed base, cases)
WIDE = {(1, "dgrad"): (0x6D1, [conv_bwd.Case(3, 2, 6, 10, 128, 64), conv_bwd.Case(1, 2, 7, 7, 64, 128)]),
        (1, "wgrad"): (0x71D, [conv_bwd.Case(3, 2, 7, 7, 64, 128), conv_bwd.Case(1, 3, 7, 7, 128, 64)]),
        (2, "dgrad"): (0x5D2, [conv_bwd.Case(7, 2, 6, 10, 64, 64), conv_bwd.Case(5, 2, 6, 4, 96, 64)]),
        (2, "wgrad"): (0x72D, [conv_bwd.Case(7, 2, 12, 12, 64, 64), conv_bwd.Case(5, 3, 8, 8, 96, 64)])}


def filled_bytes(n, value=NAN):
    return torch.full(((n + 3) // 4,), value, device="cuda").view(torch.uint8)[:n]


def dims(c):
    return c.n, c.H, c.W, c.ci, c.co, c.k


def plan(rt, form, c):
    """(data scratch bytes, weight scratch bytes, chunks) of the fp32 entries"""
    return getattr(rt, form.plan)(*dims(c))


def resolve(rt, form, c):
    """the plan-chosen case against the fp32 plan: >= 3 chunks with a shorter last one (asserted in Form.resolve)"""
    return form.resolve(getattr(rt, form.plan), c)


def data(rt, form, g, w, k, **kw):
    return getattr(rt, form.data)(g, w, form.FORMS[k], **kw)


def weight(rt, form, x, g, k, **kw):
    return getattr(rt, form.weight)(x, g, k, form.FORMS[k], **kw)


def assert_lone_taps(form, c, dw):
    inner = form.lone_taps(c)
    if inner is not None:
        taps = dw.cpu()
        assert torch.equal(taps[:, :, ~inner], torch.zeros(c.co, c.ci, int((~inner).sum()))), "the smallest map feeds its %d taps only" % int(inner.sum())
        assert bool((taps[:, :, inner] != 0).any())


def wide_inputs(form, c, side, split="dgrad"):
    """the integer inputs of `c` with one operand replaced by 17-bit odd integers of three non-zero planes (tests/conv_bwd.wide_ints):
    g one in 64 and w one in 256 for the data gradient, one in 32 on either side for the weight gradient"""
    inp = dict(form.int_inputs(c))
    seed = WIDE[form.stride, split][0] + c.k + (7 if side == "g" else 0)
    one_in = 32 if split == "wgrad" else 64 if side == "g" else 256
    inp[side] = conv_bwd.wide_ints(seed, tuple(inp[side].shape), one_in)
    return inp


def assert_wide(v, least):
    """v holds more than v.size / `least` non-zeros, each an odd integer of 17 significant bits with three non-zero planes"""
    nz = v != 0
    h, m, l = synth.cut3(v)
    assert nz.sum() > v.size // least and bool((h[nz] != 0).all() and (m[nz] != 0).all() and (l[nz] != 0).all()), "three non-zero planes"
    assert bool((np.abs(v[nz]) >= 65536).all() and (np.abs(v[nz]) < 131072).all() and (v[nz] % 2 != 0).all()), "17 significant bits, odd"


def assert_pattern(pattern, *operands):
    for v in operands:
        nz = v != 0
        assert bool(((v.view(np.uint32) & 0x7FFFFF) == pattern)[nz].all()) and nz.sum() > v.size // 4


# ---- the fp32 entries: exact integers (tests/test_gpu_conv_bwd_exact.py, tests/test_gpu_conv_bwd_s2_exact.py) ----

def exact_dense(rt, form, c, accumulate):
    c = resolve(rt, form, c)
    inp, ref = form.cached(c, "int", False)
    form.check_caps(c, inp, ref)
    x, g, w = inp["x"].cuda(), inp["g"].cuda(), inp["w"].cuda()
    dbytes, wbytes, _ = plan(rt, form, c)
    if accumulate:
        dx, dw, db = inp["dx0"].cuda(), inp["dw0"].cuda(), inp["db0"].cuda()
    else:
        dx, dw, db = (torch.full(s, NAN, device="cuda") for s in ((c.n, c.H, c.W, c.ci), (c.co, c.ci, c.k, c.k), (c.co,)))
    data(rt, form, g, w, c.k, dx=dx, accumulate=accumulate, scratch=filled_bytes(dbytes))
    weight(rt, form, x, g, c.k, dw=dw, db=db, accumulate=accumulate, scratch=filled_bytes(wbytes))
    torch.cuda.synchronize()
    base = {"dX": inp["dx0"].double(), "dW": inp["dw0"].double(), "db": inp["db0"].double()} if accumulate else {}
    mm = exact.Mismatches()
    for name, got in (("dX", dx), ("dW", dw), ("db", db)):
        mm.check(got.cpu(), ref[name] + base.get(name, 0.0), "%s %s" % (form.case_id(c), name))
    mm.raise_if_any()
    if not accumulate:
        assert_lone_taps(form, c, dw)


def exact_bias_optional(rt, form, c):
    inp, ref = form.cached(c, "int", False)
    dw, db = weight(rt, form, inp["x"].cuda(), inp["g"].cuda(), c.k, want_db=False)
    assert db is None
    exact.assert_exact(dw.cpu(), ref["dW"], "dW without db")


def exact_relu_in_slices(rt, form, c, accumulate):
    c = resolve(rt, form, c)
    inp, ref = form.cached(c, "int", True)
    _, plain = form.cached(c, "int", False)
    form.check_caps(c, inp, ref)
    form.check_caps(c, inp, plain)
    n, H, W, ci, co, k = dims(c)
    OH, OW = form.out_hw(c)
    dbytes, wbytes, _ = plan(rt, form, c)
    px, gpx = n * H * W, n * OH * OW
    A = arena.Arena.for_sizes([px * 3 * ci * 4, gpx * 3 * co * 4, px * 3 * ci * 4, co * ci * k * k * 4, co * 4, co * ci * k * k * 4, dbytes, wbytes])
    xb = A.empty("x", (n, H, W, 3 * ci))               # outer slices: the arena's NaN sentinel
    gb = A.empty("g", (n, OH, OW, 3 * co))
    dxb = A.empty("dx", (n, H, W, 3 * ci))
    xb[..., ci:2 * ci] = inp["x"].cuda()
    gb[..., co:2 * co] = inp["g"].cuda()
    w = A.put("w", inp["w"].cuda())
    if accumulate:
        dxb[..., ci:2 * ci] = inp["dx0"].cuda()
        dw, db = A.put("dw", inp["dw0"].cuda()), A.put("db", inp["db0"].cuda())
    else:
        dw, db = A.empty("dw", (co, ci, k, k)), A.empty("db", (co,))
    sd, sw = A.carve("data_scratch", dbytes), A.carve("weight_scratch", wbytes)
    data(rt, form, gb, w, k, dx=dxb, dx_coff=ci, accumulate=accumulate, scratch=sd, g_coff=co)
    weight(rt, form, xb, gb, k, relu_in=True, x_coff=ci, ci=ci, g_coff=co, co=co, dw=dw, db=db, accumulate=accumulate, scratch=sw)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    dx_mid = dxb[..., ci:2 * ci].cpu()
    b = (lambda name: inp[name].double()) if accumulate else (lambda name: 0.0)
    mm.check(dx_mid, plain["dX"] + b("dx0"), "%s dX (before the mask)" % form.case_id(c))
    mm.check(dw.cpu(), ref["dW"] + b("dw0"), "%s dW, relu_in" % form.case_id(c))
    mm.check(db.cpu(), ref["db"] + b("db0"), "%s db" % form.case_id(c))
    # OFFK_CONV_RELU_IN's mask on the conv's dX: in place, mask = the conv's input
    rt.relu_backward(dxb, xb, out=dxb, dy_coff=ci, y_coff=ci, out_coff=ci, c=ci)
    torch.cuda.synchronize()
    want = (plain["dX"] + b("dx0")) * (inp["x"] > 0).double()
    got = dxb[..., ci:2 * ci].cpu().double()
    assert torch.equal(got, want), "%s: masked dX differs at %d elements" % (form.case_id(c), int((got != want).sum()))
    if not accumulate:
        assert torch.equal(got, ref["dX"]), "the masked dX is autograd's dX of conv(relu(x))"
    mm.raise_if_any()
    assert A.untouched(dxb[..., :ci]) and A.untouched(dxb[..., 2 * ci:]), "dx's neighbour slices were written"
    assert A.untouched(xb[..., :ci]) and A.untouched(gb[..., 2 * co:])
    A.check()


# ---- the fp32 entries: the derived bound on normal data (tests/test_gpu_conv_bwd.py, tests/test_gpu_conv_bwd_s2.py) ----

def run_fp32(rt, form, c, x, g, w, relu_in, fill):
    """dX (masked by x where relu_in), dW, db from scratch buffers pre-filled with `fill`"""
    dbytes, wbytes, _ = plan(rt, form, c)
    dx = data(rt, form, g, w, c.k, scratch=filled_bytes(dbytes, fill))
    if relu_in:
        rt.relu_backward(dx, x, out=dx)
    dw, db = weight(rt, form, x, g, c.k, relu_in=relu_in, scratch=filled_bytes(wbytes, fill))
    torch.cuda.synchronize()
    return dx, dw, db


def within_the_derived_bound_and_reproducible(rt, form, c, relu_in):
    c = resolve(rt, form, c)
    inp, ref = form.cached(c, "normal", relu_in)
    x, g, w = inp["x"].cuda(), inp["g"].cuda(), inp["w"].cuda()
    got = run_fp32(rt, form, c, x, g, w, relu_in, NAN)
    OH, OW = form.out_hw(c)
    terms = {"dX": form.dx_terms(c), "dW": c.n * OH * OW, "db": c.n * OH * OW}
    worst = {}
    for name, t in zip(("dX", "dW", "db"), got):
        err = (t.cpu().double() - ref[name]).abs()
        bound = form.gamma(terms[name] + 1) * ref[name + "_abs"]
        assert bool(torch.isfinite(t).all()), name
        assert bool((err[bound == 0] == 0).all()), "%s %s: an element without terms is not 0" % (form.case_id(c), name)
        worst[name] = float((err / bound.clamp_min(1e-300)).max())
        print("%s %s: largest error %.3e, largest error / bound %.3f" % (form.case_id(c), name, float(err.max()), worst[name]))
    for name in worst:
        assert worst[name] <= 1.0, "%s %s: error is %.3f of the derived bound" % (form.case_id(c), name, worst[name])
    again = run_fp32(rt, form, c, x, g, w, relu_in, -3.0)
    for name, a, b in zip(("dX", "dW", "db"), got, again):
        assert torch.equal(a, b), "%s %s: two runs from differently pre-filled scratch differ" % (form.case_id(c), name)


def capture_and_replay(rt, form, c):
    """relu_backward -> data -> weight on one stream, captured once, replayed twice: equal to the eager results bit for bit"""
    inp, _ = form.cached(c, "normal", False)
    x, gy, w = inp["x"].cuda(), inp["g"].cuda(), inp["w"].cuda()
    y = torch.randn(gy.shape, generator=torch.Generator().manual_seed(7)).cuda()       # the stored output whose ReLU is undone
    dbytes, wbytes, _ = plan(rt, form, c)

    def buffers():
        return dict(g=torch.full_like(gy, NAN), dx=torch.full_like(x, NAN), dw=torch.full_like(w, NAN),
                    db=torch.full((c.co,), NAN, device="cuda"), sd=filled_bytes(dbytes), sw=filled_bytes(wbytes))

    def chain(b):
        rt.relu_backward(gy, y, out=b["g"])
        data(rt, form, b["g"], w, c.k, dx=b["dx"], scratch=b["sd"])
        weight(rt, form, x, b["g"], c.k, dw=b["dw"], db=b["db"], scratch=b["sw"])

    eager = buffers()
    chain(eager)
    torch.cuda.synchronize()
    cap = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(cap)
    for _ in range(2):
        for k in ("g", "dx", "dw", "db"):
            cap[k].fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for k in ("g", "dx", "dw", "db"):
            assert torch.equal(cap[k], eager[k]), "replay differs from the eager run in %s" % k
    assert bool(torch.isfinite(eager["dw"]).all()) and bool((eager["g"] == 0).any())


def scratch_never_shows_and_replay_equals_eager(outs, nbytes, run):
    """`run(buffers)` writes the outputs named in `outs` ({name: shape}) using buffers["s"], `nbytes` of scratch: equal bits from the
    arena's NaN sentinel and from -3 in the scratch, and a captured run replayed twice equals the eager one"""
    A = arena.Arena.for_sizes([4 * int(np.prod(s)) for s in outs.values()] * 3 + [nbytes] * 3)

    def buffers(tag, fill):
        b = dict((k, A.empty(k + tag, s)) for k, s in outs.items())
        b["s"] = A.carve("scratch" + tag, nbytes)
        if fill is not None:
            b["s"].view(torch.float32).fill_(fill)
        return b

    first, second, cap = buffers("1", None), buffers("2", -3.0), buffers("3", None)        # NaN sentinel | -3 | NaN sentinel
    run(first)
    run(second)
    torch.cuda.synchronize()
    for k in outs:
        assert arena.same_bits(first[k], second[k]), "%s depends on what the scratch held" % k
        assert not bool(first[k].isnan().any())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: the launches of the entry in order
        run(cap)
    for _ in range(2):
        for k in outs:
            cap[k].fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert arena.same_bits(cap[k], first[k]), "replay differs from the eager run in %s" % k
    A.check()


# ---- the split-fp32 data gradient (tests/test_gpu_conv_dgrad_split.py, tests/test_gpu_conv_s2_dgrad_split.py) ----

def split_dgrad(rt, form, g, w, k, **kw):
    return data(rt, form, g, w, k, arith="f32split", **kw)


def dgrad_plan(rt, form, c):
    """the split data gradient's scratch bytes"""
    return getattr(rt, form.data_plan_split)(*dims(c))


def dgrad_dense(rt, form, c, accumulate):
    inp, ref = form.cached(c, "int", False)
    form.check_caps(c, inp, ref)
    nbytes = dgrad_plan(rt, form, c)
    dx = inp["dx0"].cuda() if accumulate else torch.full((c.n, c.H, c.W, c.ci), NAN, device="cuda")
    split_dgrad(rt, form, inp["g"].cuda(), inp["w"].cuda(), c.k, dx=dx, accumulate=accumulate, scratch=filled_bytes(nbytes))
    torch.cuda.synchronize()
    exact.assert_exact(dx.cpu(), ref["dX"] + (inp["dx0"].double() if accumulate else 0.0), "%s dX" % form.case_id(c))


def dgrad_slices(rt, form, c, accumulate):
    inp, ref = form.cached(c, "int", False)
    form.check_caps(c, inp, ref)
    n, H, W, ci, co, k = dims(c)
    OH, OW = form.out_hw(c)
    nbytes = dgrad_plan(rt, form, c)
    A = arena.Arena.for_sizes([n * OH * OW * 3 * co * 4, n * H * W * 3 * ci * 4, co * ci * k * k * 4, nbytes])
    gb = A.empty("g", (n, OH, OW, 3 * co))             # outer slices: the arena's NaN sentinel
    dxb = A.empty("dx", (n, H, W, 3 * ci))
    gb[..., co:2 * co] = inp["g"].cuda()
    if accumulate:
        dxb[..., ci:2 * ci] = inp["dx0"].cuda()
    w = A.put("w", inp["w"].cuda())
    s = A.carve("scratch", nbytes)
    split_dgrad(rt, form, gb, w, k, g_coff=co, dx=dxb, dx_coff=ci, accumulate=accumulate, scratch=s)
    torch.cuda.synchronize()
    exact.assert_exact(dxb[..., ci:2 * ci].cpu(), ref["dX"] + (inp["dx0"].double() if accumulate else 0.0), "%s dX slice" % form.case_id(c))
    assert A.untouched(dxb[..., :ci]) and A.untouched(dxb[..., 2 * ci:]) and A.untouched(gb[..., :co]) and A.untouched(gb[..., 2 * co:])
    assert torch.equal(w.cpu(), inp["w"]), "the weight is read in place"
    A.check()


def dgrad_wide(rt, form, c, side):
    inp = wide_inputs(form, c, side)
    assert_wide(inp[side].numpy(), 1024)
    ref = form.reference(c, inp, False)
    cap = float(ref["dX_abs"].max())
    assert cap < form.LIMIT, "%s: sum of |terms| %.0f is not below 2^23" % (form.case_id(c), cap)
    assert float(ref["dX"].abs().max()) >= 65536
    dx = split_dgrad(rt, form, inp["g"].cuda(), inp["w"].cuda(), c.k)
    torch.cuda.synchronize()
    exact.assert_exact(dx.cpu(), ref["dX"], "%s dX, wide %s" % (form.case_id(c), side))


def dgrad_inequality(rt, form, what, k, g, w, dx_gpu, base=None):
    """asserts the inequality per element of dX; returns (emulated c_acc, measured accumulation constant, the fp32 entry's error in the same
    unit).  g [n, OH, OW, co], w [co, ci, k, k]: numpy"""
    helper = DGRAD[form.stride]
    ref, dropped, mag = helper.terms(g, w)
    emu = helper.emulate(g, w)
    ce = sb.c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * ce)
    got = dx_gpu.cpu().numpy()
    assert sb.excess(emu, ref, dropped, mag, A) <= 0.0, "the emulation itself"
    f32 = data(rt, form, torch.from_numpy(g).cuda(), torch.from_numpy(w).cuda(), k).cpu().numpy()
    cf = float((np.abs(f32.astype(np.float64) - ref) / np.maximum(sb.EPS * mag, 1e-300)).max())
    if base is None:
        cg = sb.c_acc(got, ref, dropped, mag)
        print("%s: emulated c_acc %.3f, A %.3f, gpu accumulation %.3f, dropped max %.3f; the fp32 entry's error %.3f (all x 2^-24 sum|g w|)" % (
            what, ce, A, cg, float((np.abs(dropped) / np.maximum(sb.EPS * mag, 1e-300)).max()), cf))
    else:
        cg = float("nan")
    ex = sb.excess_map(got, ref, dropped, mag, A, base=base)
    assert float(ex.max()) <= 0.0, "%s: %d of %d elements break the inequality, worst excess %.3g" % (what, int((ex > 0).sum()), ex.size, float(ex.max()))
    if base is None:
        zero = mag == 0
        assert np.array_equal(got[zero], np.zeros(int(zero.sum()), dtype=np.float32)), "an element without terms is exactly 0"
    return ce, cg, cf


def dgrad_worst(rt, form, what, shape, pattern, signs):
    """g alternates in sign along co (the contraction index) in the "alternating" mode: sum g w << sum |g w|.  shape: (k, n, H, W, ci, co)"""
    g, w = form.worst_inputs(shape, pattern, signs)
    assert_pattern(pattern, g, w)
    dx = split_dgrad(rt, form, torch.from_numpy(g).cuda(), torch.from_numpy(w).cuda(), shape[0])
    torch.cuda.synchronize()
    dgrad_inequality(rt, form, "worst case %s 0x%06X %-11s" % (what, pattern, signs), shape[0], g, w, dx)


def dgrad_normal(rt, form, what, c):
    inp = form.normal_inputs(c)
    g, w = inp["g"].numpy(), inp["w"].numpy()
    dx = split_dgrad(rt, form, inp["g"].cuda(), inp["w"].cuda(), c.k)
    torch.cuda.synchronize()
    dgrad_inequality(rt, form, "normal data %s" % what, c.k, g, w, dx)
    # accumulate: one more 2^-24 |result|
    gen = torch.Generator().manual_seed(7)
    base = torch.randn(c.n, c.H, c.W, c.ci, generator=gen)
    dxa = base.cuda()
    split_dgrad(rt, form, inp["g"].cuda(), inp["w"].cuda(), c.k, dx=dxa, accumulate=True)
    torch.cuda.synchronize()
    dgrad_inequality(rt, form, "normal data %s, accumulate" % what, c.k, g, w, dxa, base=base.numpy())


def dgrad_discipline(rt, form, c):
    inp = form.normal_inputs(c)
    g, w = inp["g"].cuda(), inp["w"].cuda()
    scratch_never_shows_and_replay_equals_eager({"dx": (c.n, c.H, c.W, c.ci)}, dgrad_plan(rt, form, c),
                                                lambda b: split_dgrad(rt, form, g, w, c.k, dx=b["dx"], scratch=b["s"]))


# ---- the split-fp32 weight gradient (tests/test_gpu_conv_wgrad_split.py, tests/test_gpu_conv_s2_wgrad_split.py) ----

def split_wgrad(rt, form, x, g, c, **kw):
    return weight(rt, form, x, g, c.k, arith="f32split", **kw)


def wgrad_plan(rt, form, c):
    """(scratch bytes, chunks) of the split weight gradient"""
    return getattr(rt, form.weight_plan_split)(*dims(c))


def wgrad_resolve(rt, form, c):
    """the plan-chosen case against the SPLIT plan, taken in the shape Form.chunked_n reads ((data bytes, weight bytes, chunks)): >= 3
    chunks with a shorter last one (asserted in Form.resolve)"""
    return form.resolve(lambda *a: (0,) + getattr(rt, form.weight_plan_split)(*a), c)


def wgrad_dense(rt, form, c, accumulate):
    c = wgrad_resolve(rt, form, c)
    inp, ref = form.cached(c, "int", False)
    form.check_caps(c, inp, ref)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes = wgrad_plan(rt, form, c)[0]
    if accumulate:
        dw, db = inp["dw0"].cuda(), inp["db0"].cuda()
    else:
        dw, db = torch.full((c.co, c.ci, c.k, c.k), NAN, device="cuda"), torch.full((c.co,), NAN, device="cuda")
    split_wgrad(rt, form, x, g, c, dw=dw, db=db, accumulate=accumulate, scratch=filled_bytes(wbytes))
    torch.cuda.synchronize()
    base = {"dW": inp["dw0"].double(), "db": inp["db0"].double()} if accumulate else {}
    mm = exact.Mismatches()
    for name, got in (("dW", dw), ("db", db)):
        mm.check(got.cpu(), ref[name] + base.get(name, 0.0), "%s %s" % (form.case_id(c), name))
    mm.raise_if_any()
    assert bool((dw != 0).any())
    if not accumulate:
        assert_lone_taps(form, c, dw)


def wgrad_bias_optional(rt, form, c):
    c = wgrad_resolve(rt, form, c)
    inp, ref = form.cached(c, "int", False)
    A = arena.Arena.for_sizes([c.co * c.ci * c.k * c.k * 4])
    dw = A.empty("dw", (c.co, c.ci, c.k, c.k))
    got, db = split_wgrad(rt, form, inp["x"].cuda(), inp["g"].cuda(), c, dw=dw, want_db=False)
    torch.cuda.synchronize()
    assert db is None
    exact.assert_exact(got.cpu(), ref["dW"], "dW without db")
    A.check()


def wgrad_relu_in_slices(rt, form, c, accumulate):
    c = wgrad_resolve(rt, form, c)
    inp, ref = form.cached(c, "int", True)
    form.check_caps(c, inp, ref)
    n, H, W, ci, co, k = dims(c)
    OH, OW = form.out_hw(c)
    wbytes = wgrad_plan(rt, form, c)[0]
    px, opx = n * H * W, n * OH * OW
    A = arena.Arena.for_sizes([px * 3 * ci * 4, opx * 3 * co * 4, co * ci * k * k * 4, co * 4, wbytes])
    xb = A.empty("x", (n, H, W, 3 * ci))               # outer slices: the arena's NaN sentinel
    gb = A.empty("g", (n, OH, OW, 3 * co))
    xb[..., ci:2 * ci] = inp["x"].cuda()
    gb[..., co:2 * co] = inp["g"].cuda()
    if accumulate:
        dw, db = A.put("dw", inp["dw0"].cuda()), A.put("db", inp["db0"].cuda())
    else:
        dw, db = A.empty("dw", (co, ci, k, k)), A.empty("db", (co,))
    sw = A.carve("weight_scratch", wbytes)
    split_wgrad(rt, form, xb, gb, c, relu_in=True, x_coff=ci, ci=ci, g_coff=co, co=co, dw=dw, db=db, accumulate=accumulate, scratch=sw)
    torch.cuda.synchronize()
    b = (lambda name: inp[name].double()) if accumulate else (lambda name: 0.0)
    mm = exact.Mismatches()
    mm.check(dw.cpu(), ref["dW"] + b("dw0"), "%s dW, relu_in" % form.case_id(c))
    mm.check(db.cpu(), ref["db"] + b("db0"), "%s db" % form.case_id(c))
    mm.raise_if_any()
    assert A.untouched(xb[..., :ci]) and A.untouched(xb[..., 2 * ci:]) and A.untouched(gb[..., :co]) and A.untouched(gb[..., 2 * co:])
    assert not bool(sw.view(torch.float32).isnan().any()), "every slab element is written (by exactly one thread)"
    A.check()


def wgrad_wide(rt, form, c, side):
    inp = wide_inputs(form, c, side, "wgrad")
    assert_wide(inp[side].numpy(), 64)
    ref = form.reference(c, inp, False)
    for name in ("dW", "db"):
        cap = float(ref[name + "_abs"].max())
        assert cap < form.LIMIT, "%s %s: sum of |terms| %.0f is not below 2^23" % (form.case_id(c), name, cap)
    dw, db = split_wgrad(rt, form, inp["x"].cuda(), inp["g"].cuda(), c)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    mm.check(dw.cpu(), ref["dW"], "%s dW, wide %s" % (form.case_id(c), side))
    mm.check(db.cpu(), ref["db"], "%s db, wide %s" % (form.case_id(c), side))
    mm.raise_if_any()


def wgrad_inequality(rt, form, what, c, g, x, dw_gpu, relu_in=False):
    """asserts the inequality per element of dW; returns (emulated c_acc, measured accumulation constant, the fp32 entry's error in the same
    unit).  g, x: numpy, channels-last"""
    helper, chunk_bounds = WGRAD[form.stride]
    chunks = wgrad_plan(rt, form, c)[1]
    G, taps = helper.operands(g, x, c.k, relu_in=relu_in)
    ref, dropped, mag = helper.terms(G, taps, c.k)
    emu = helper.emulate_chunked(G, taps, chunk_bounds(c, chunks), c.k)
    ce = sb.c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * ce)
    got = dw_gpu.cpu().numpy()
    assert sb.excess(emu, ref, dropped, mag, A) <= 0.0, "the emulation itself"
    cg = sb.c_acc(got, ref, dropped, mag)
    f32 = weight(rt, form, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), c.k, relu_in=relu_in)[0].cpu().numpy()
    cf = float((np.abs(f32.astype(np.float64) - ref) / np.maximum(sb.EPS * mag, 1e-300)).max())
    print("%s: emulated c_acc %.3f, A %.3f, gpu accumulation %.3f, dropped max %.3f; the fp32 entry's error %.3f (all x 2^-24 sum|g x|)" % (
        what, ce, A, cg, float((np.abs(dropped) / np.maximum(sb.EPS * mag, 1e-300)).max()), cf))
    ex = sb.excess_map(got, ref, dropped, mag, A)
    assert float(ex.max()) <= 0.0, "%s: %d of %d elements break the inequality, worst excess %.3g" % (what, int((ex > 0).sum()), ex.size, float(ex.max()))
    zero = mag == 0
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()), dtype=np.float32)), "an element without terms is exactly 0"
    return ce, cg, cf


def wgrad_worst(rt, form, c, pattern, signs, g, x):
    """g, x: the file's own worst-case operands on `pattern` (x alternates in sign along the contraction index in the "alternating" mode)"""
    assert_pattern(pattern, g, x)
    dw, _db = split_wgrad(rt, form, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), c)
    torch.cuda.synchronize()
    wgrad_inequality(rt, form, "worst case %s 0x%06X %-11s" % (form.case_id(c), pattern, signs), c, g, x, dw)


def wgrad_normal(rt, form, c):
    c = wgrad_resolve(rt, form, c)
    inp = form.normal_inputs(c)
    x, g = inp["x"].numpy(), inp["g"].numpy()
    dw, db = split_wgrad(rt, form, inp["x"].cuda(), inp["g"].cuda(), c)
    torch.cuda.synchronize()
    wgrad_inequality(rt, form, "normal data %s" % form.case_id(c), c, g, x, dw)
    g64 = g.astype(np.float64).reshape(-1, c.co)
    err = np.abs(db.cpu().numpy().astype(np.float64) - g64.sum(0))
    bound = form.gamma(g64.shape[0]) * np.abs(g64).sum(0)
    assert bool((err <= bound).all()), "db: worst error / bound %.3f" % float((err / bound).max())


def wgrad_discipline(rt, form, c, least_chunks):
    inp = form.normal_inputs(c)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes, chunks = wgrad_plan(rt, form, c)
    assert chunks >= least_chunks
    scratch_never_shows_and_replay_equals_eager({"dw": (c.co, c.ci, c.k, c.k), "db": (c.co,)}, wbytes,
                                                lambda b: split_wgrad(rt, form, x, g, c, dw=b["dw"], db=b["db"], scratch=b["s"]))


# ---- the one-layer bound of the module tests ----
def one_layer(m, fl, x, gy):
    """(tests/test_gpu_fusion_conv_s2_module.py, tests/test_gpu_motion_head_module.py)  fp64 values, elementwise error bounds and caps (largest sum of |terms|) of one layer from exact inputs x and gy.
    m: the fp64 nn.Conv2d.  -> {"y" | "dx" | "weight" | "bias": (value, bound)}, caps, (undecided masks, masks)"""
    W, b, s, pad = m.weight.detach(), m.bias.detach(), m.stride[0], m.padding[0]
    co, ci, k, _ = W.shape
    a = torch.relu(x) if fl.get("relu_in") else x
    z = F.conv2d(a, W, b, stride=s, padding=pad)
    S = F.conv2d(a.abs(), W.abs(), b.abs(), stride=s, padding=pad)
    Ez = conv_bwd.gamma(ci * k * k + 2) * S
    relu = bool(fl.get("relu"))
    unstable = (z.abs() <= Ez) & (Ez > 0) if relu else torch.zeros_like(z, dtype=torch.bool)
    gz = gy * (z > 0).double() if relu else gy
    Egz = torch.where(unstable, gy.abs(), torch.zeros_like(gy))
    P = gz.shape[0] * gz.shape[2] * gz.shape[3]
    op = x.shape[-1] - ((gz.shape[-1] - 1) * s - 2 * pad + k)

    def cw(g, v):
        return conv2d_weight(v, W.shape, g, stride=s, padding=pad)

    def ct(g, w):
        return F.conv_transpose2d(g, w, stride=s, padding=pad, output_padding=op)

    Sw, Sb, Sx = cw(gz.abs() + Egz, a.abs()), (gz.abs() + Egz).sum((0, 2, 3)), ct(gz.abs() + Egz, W.abs())
    mx = co * (-(-k // s)) ** 2
    dx, Edx = ct(gz, W), ct(Egz, W.abs()) + conv_bwd.gamma(mx + 1) * Sx
    if fl.get("relu_in"):
        dx, Edx = dx * (x > 0).double(), Edx * (x > 0).double()
    out = {"y": (torch.relu(z) if relu else z, Ez), "dx": (dx, Edx),
           "weight": (cw(gz, a), cw(Egz, a.abs()) + conv_bwd.gamma(P + 1) * Sw), "bias": (gz.sum((0, 2, 3)), Egz.sum((0, 2, 3)) + conv_bwd.gamma(P + 1) * Sb)}
    caps = {"z": float(S.max()), "dW": float(Sw.max()), "db": float(Sb.max()), "dx": float(Sx.max())}
    return out, caps, (int(unstable.sum()), z.numel() if relu else 0)


def within(got, val, bound, what):
    err = (got.detach().cpu().double() - val).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0
    print("%s: largest error %.3e, largest error / bound %.3f" % (what, float(err.max()), ratio))
    assert bool((err <= bound).all()), "%s: error is %.3f of the derived bound" % (what, ratio)
