"""The stride-2 fusion convs' weight / bias gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_s2_backward_weight_split,
csrc/conv_wgrad_s2_split.hip; runtime.conv2d_s2_backward_weight(arith="f32split"), FusionConv2d(s2_wgrad_arith="f32split")).

 1. exact integers: the ten cases of tests/conv_bwd_s2.cases() (the plan-chosen n from the SPLIT plan: >= 3 chunks, a shorter last one) and
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
 8. the module."""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from . import arena
from . import conv_bwd_s2 as s2
from . import conv_s2_wgrad_split as ws
from . import exact

pytestmark = pytest.mark.gpu
NAN = float("nan")
EDGES = [s2.Case(k, 2, 4, W, 64, 64) for k in (7, 5) for W in (14, 16, 18, 28)]
CASES = s2.cases() + EDGES
IDS = [s2.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def split_plan3(rt):
    """the split plan in the shape tests/conv_bwd_s2.chunked_n reads ((data bytes, weight bytes, chunks))"""
    return lambda *a: (0,) + rt.conv2d_s2_backward_weight_plan_split(*a)


def resolve(rt, c):
    """the plan-chosen case against the NEW plan: >= 3 chunks with a shorter last one (asserted in tests/conv_bwd_s2.resolve)"""
    return s2.resolve(split_plan3(rt), c)


def filled_bytes(n, value=NAN):
    return torch.full(((n + 3) // 4,), value, device="cuda").view(torch.uint8)[:n]


def split_wgrad(rt, x, g, c, **kw):
    return rt.conv2d_s2_backward_weight(x, g, c.k, s2.FORMS[c.k], arith="f32split", **kw)


# ---- 1. exact integers ----

@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    c = resolve(rt, c)
    inp, ref = s2.cached(c, "int", False)
    s2.check_caps(c, inp, ref)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes = rt.conv2d_s2_backward_weight_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)[0]
    if accumulate:
        dw, db = inp["dw0"].cuda(), inp["db0"].cuda()
    else:
        dw, db = torch.full((c.co, c.ci, c.k, c.k), NAN, device="cuda"), torch.full((c.co,), NAN, device="cuda")
    split_wgrad(rt, x, g, c, dw=dw, db=db, accumulate=accumulate, scratch=filled_bytes(wbytes))
    torch.cuda.synchronize()
    base = {"dW": inp["dw0"].double(), "db": inp["db0"].double()} if accumulate else {}
    mm = exact.Mismatches()
    for name, got in (("dW", dw), ("db", db)):
        mm.check(got.cpu(), ref[name] + base.get(name, 0.0), "%s %s" % (s2.case_id(c), name))
    mm.raise_if_any()
    assert bool((dw != 0).any())


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_bias_gradient_is_optional(rt, c):
    c = resolve(rt, c)
    inp, ref = s2.cached(c, "int", False)
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
    inp, ref = s2.cached(c, "int", True)
    s2.check_caps(c, inp, ref)
    n, H, W, ci, co, k = c.n, c.H, c.W, c.ci, c.co, c.k
    wbytes = rt.conv2d_s2_backward_weight_plan_split(n, H, W, ci, co, k)[0]
    px, opx = n * H * W, n * (H // 2) * (W // 2)
    A = arena.Arena.for_sizes([px * 3 * ci * 4, opx * 3 * co * 4, co * ci * k * k * 4, co * 4, wbytes])
    xb = A.empty("x", (n, H, W, 3 * ci))               # outer slices: the arena's NaN sentinel
    gb = A.empty("g", (n, H // 2, W // 2, 3 * co))
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
    mm.check(dw.cpu(), ref["dW"] + b("dw0"), "%s dW, relu_in" % s2.case_id(c))
    mm.check(db.cpu(), ref["db"] + b("db0"), "%s db" % s2.case_id(c))
    mm.raise_if_any()
    assert A.untouched(xb[..., :ci]) and A.untouched(xb[..., 2 * ci:]) and A.untouched(gb[..., :co]) and A.untouched(gb[..., 2 * co:])
    assert not bool(sw.view(torch.float32).isnan().any()), "every slab element is written (by exactly one thread)"
    A.check()


# ---- 2. wide integers ----

def wide_ints(seed, shape):
    """sparse (one in thirty-two) odd integers of 17 significant bits, either sign: bit 16, seven random bits, bit 8, seven random bits,
    bit 0 -- the leading plane takes bits 16 .. 9, the middle one bits 8 .. 1, the last one bit 0 (tests/test_gpu_conv_wgrad_split.py's)"""
    hi = exact.ints(exact.stream(seed, 1, 0), shape, 0, 127)
    lo = exact.ints(exact.stream(seed, 2, 0), shape, 0, 127)
    sign = exact.ints(exact.stream(seed, 3, 0), shape, 0, 1) * 2 - 1
    on = (exact.ints(exact.stream(seed, 4, 0), shape, 0, 31) == 0).float()
    return (65536 + hi * 512 + 256 + lo * 2 + 1) * sign * on


WIDE = [s2.Case(7, 2, 12, 12, 64, 64), s2.Case(5, 3, 8, 8, 96, 64)]


def wide_inputs(c, side):
    inp = dict(s2.int_inputs(c))
    inp[side] = wide_ints(0x72D + c.k + (7 if side == "g" else 0), tuple(inp[side].shape))
    return inp


@pytest.mark.parametrize("side", ["g", "x"])
@pytest.mark.parametrize("c", WIDE, ids=s2.case_id)
def test_wide_integers_equal_fp64(rt, c, side):
    inp = wide_inputs(c, side)
    v = inp[side].numpy()
    nz = v != 0
    h, m, l = synth.cut3(v)
    assert nz.sum() > v.size // 64 and bool((h[nz] != 0).all() and (m[nz] != 0).all() and (l[nz] != 0).all()), "three non-zero planes"
    assert bool((np.abs(v[nz]) >= 65536).all() and (np.abs(v[nz]) < 131072).all() and (v[nz] % 2 != 0).all()), "17 significant bits, odd"
    ref = s2.reference(c, inp, False)
    for name in ("dW", "db"):
        cap = float(ref[name + "_abs"].max())
        assert cap < s2.LIMIT, "%s %s: sum of |terms| %.0f is not below 2^23" % (s2.case_id(c), name, cap)
    dw, db = split_wgrad(rt, inp["x"].cuda(), inp["g"].cuda(), c)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    mm.check(dw.cpu(), ref["dW"], "%s dW, wide %s" % (s2.case_id(c), side))
    mm.check(db.cpu(), ref["db"], "%s db, wide %s" % (s2.case_id(c), side))
    mm.raise_if_any()


# ---- 3. / 4. the inequality ----

def check_inequality(rt, what, c, g, x, dw_gpu, relu_in=False, fp32_entry=True):
    """asserts the inequality per element of dW; returns (emulated c_acc, measured accumulation constant, the fp32 entry's error in the same
    unit).  g, x: numpy, channels-last"""
    chunks = rt.conv2d_s2_backward_weight_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)[1]
    G, taps = ws.operands(g, x, c.k, relu_in=relu_in)
    ref, dropped, mag = ws.terms(G, taps, c.k)
    emu = ws.emulate_chunked(G, taps, ws.chunk_bounds(c.n, c.H, c.W, chunks), c.k)
    ce = ws.c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * ce)
    got = dw_gpu.cpu().numpy()
    assert ws.excess(emu, ref, dropped, mag, A) <= 0.0, "the emulation itself"
    cg = ws.c_acc(got, ref, dropped, mag)
    cf = float("nan")
    if fp32_entry:
        f32 = rt.conv2d_s2_backward_weight(torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), c.k, s2.FORMS[c.k], relu_in=relu_in)[0].cpu().numpy()
        cf = float((np.abs(f32.astype(np.float64) - ref) / np.maximum(ws.EPS * mag, 1e-300)).max())
    print("%s: emulated c_acc %.3f, A %.3f, gpu accumulation %.3f, dropped max %.3f; the fp32 entry's error %.3f (all x 2^-24 sum|g x|)" % (
        what, ce, A, cg, float((np.abs(dropped) / np.maximum(ws.EPS * mag, 1e-300)).max()), cf))
    ex = ws.excess_map(got, ref, dropped, mag, A)
    assert float(ex.max()) <= 0.0, "%s: %d of %d elements break the inequality, worst excess %.3g" % (what, int((ex > 0).sum()), ex.size, float(ex.max()))
    zero = mag == 0
    assert np.array_equal(got[zero], np.zeros(int(zero.sum()), dtype=np.float32)), "an element without terms is exactly 0"
    return ce, cg, cf


ADV = [(p, s) for p in (0x00FFFF, 0x7FFFFF, 0x7F7F7F) for s in ("same", "alternating")]
# both real channel shapes at n = 1, and two small cases (two images: a step that straddles them; a half ci tile)
WORST_SHAPES = [s2.Case(7, 1, 28, 28, 320, 64), s2.Case(5, 1, 14, 14, 1056, 128), s2.Case(7, 2, 6, 10, 64, 64), s2.Case(5, 2, 6, 4, 160, 64)]


@pytest.mark.parametrize("pattern,signs", ADV, ids=["0x%06X_%s" % a for a in ADV])
@pytest.mark.parametrize("c", WORST_SHAPES, ids=s2.case_id)
def test_worst_case_mantissas(rt, c, pattern, signs):
    """x alternates in sign along the map's column pairs in the "alternating" mode, so along the positions of every tap's stride-2 sample:
    sum g x << sum |g x|."""
    OH, OW = c.H // 2, c.W // 2
    g = synth.make_adversarial((c.n * OH * OW, c.co), pattern, "same", seed=21 + c.H, relu=(pattern == 0x7FFFFF)).reshape(c.n, OH, OW, c.co)
    x = synth.make_adversarial((c.n * c.H * OW, c.ci), pattern, signs, seed=22 + c.H, k_axis=0).reshape(c.n, c.H, OW, 1, c.ci)
    x = np.ascontiguousarray(np.broadcast_to(x, (c.n, c.H, OW, 2, c.ci))).reshape(c.n, c.H, c.W, c.ci) * np.float32(2.0 ** -4)
    for v in (g, x):
        nz = v != 0
        assert bool(((v.view(np.uint32) & 0x7FFFFF) == pattern)[nz].all()) and nz.sum() > v.size // 4
    dw, _db = split_wgrad(rt, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), c)
    torch.cuda.synchronize()
    check_inequality(rt, "worst case %s 0x%06X %-11s" % (s2.case_id(c), pattern, signs), c, g, x, dw)


@pytest.mark.parametrize("c", s2.cases(), ids=s2.case_id)
def test_normal_data_within_the_bound(rt, c):
    c = resolve(rt, c)
    inp = s2.normal_inputs(c)
    x, g = inp["x"].numpy(), inp["g"].numpy()
    dw, db = split_wgrad(rt, inp["x"].cuda(), inp["g"].cuda(), c)
    torch.cuda.synchronize()
    check_inequality(rt, "normal data %s" % s2.case_id(c), c, g, x, dw)
    g64 = g.astype(np.float64).reshape(-1, c.co)
    err = np.abs(db.cpu().numpy().astype(np.float64) - g64.sum(0))
    bound = s2.gamma(g64.shape[0]) * np.abs(g64).sum(0)
    assert bool((err <= bound).all()), "db: worst error / bound %.3f" % float((err / bound).max())


# ---- 5. scratch and replay ----

DISCIPLINE = [s2.Case(7, 37, 6, 10, 64, 64), s2.Case(5, 88, 6, 4, 32, 64)]          # three chunks each, the last one shorter


@pytest.mark.parametrize("c", DISCIPLINE, ids=s2.case_id)
def test_scratch_contents_never_show_and_replay_equals_eager(rt, c):
    inp = s2.normal_inputs(c)
    x, g = inp["x"].cuda(), inp["g"].cuda()
    wbytes, chunks = rt.conv2d_s2_backward_weight_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)
    assert chunks >= 3
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
