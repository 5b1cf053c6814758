"""Exact integer-input tests of the fusion convs' backward (offk_relu_backward, offk_conv2d_backward_data, offk_conv2d_backward_weight).

Inputs are small integers from the project's generator (tests/conv_bwd.py: g, x in [-8, 8] with a quarter exact zeros, w in [-4, 4],
accumulate bases in [-64, 64]).  The test first checks the reference's own condition on the data -- every output's sum of |terms| is
below 2^23 -- under which every partial sum in any order is an integer fp32 holds exactly; dX, dW and db must then EQUAL the fp64
reference (torch's conv2d + autograd on the CPU), with and without accumulate.  No tolerance anywhere in this file: one lost term, one
tap read a row off, one K-tile that straddles an image boundary wrongly is a failure.

The same cases run once more with relu_in = 1 and with x, g and dx as the middle slices of three-times-wider buffers, every buffer
carved from a guarded arena (tests/arena.py) whose sentinels must be intact afterwards; the outer slices hold NaN (x, g) or must keep
their sentinel (dx).
"""
import pytest
import torch

import offk_amd  # noqa: F401

from . import arena
from . import conv_bwd as cb
from . import exact

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = cb.cases()
IDS = [cb.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def resolve(rt, c):
    """the plan-chosen case: n such that the weight gradient runs in >= 3 chunks with a shorter last one (asserted here)"""
    if c.n is not None:
        return c
    n = cb.chunked_n(rt.conv2d_backward_plan, c)
    chunks = rt.conv2d_backward_plan(n, c.H, c.W, c.ci, c.co, c.k)[2]
    ipc = -(-n // chunks)
    assert chunks >= 3, (n, chunks)
    assert 0 < n - (chunks - 1) * ipc < ipc, (n, chunks, ipc)
    return c._replace(n=n)


def nan_bytes(n):
    return torch.full(((n + 3) // 4,), NAN, device="cuda").view(torch.uint8)[:n]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    c = resolve(rt, c)
    inp, ref = cb.cached(c, "int", False)
    cb.check_caps(c, inp, ref)
    pad = (c.k - 1) // 2
    x, g, w = inp["x"].cuda(), inp["g"].cuda(), inp["w"].cuda()
    dbytes, wbytes, _ = rt.conv2d_backward_plan(c.n, c.H, c.W, c.ci, c.co, c.k)
    if accumulate:
        dx, dw, db = inp["dx0"].cuda(), inp["dw0"].cuda(), inp["db0"].cuda()
    else:
        dx, dw, db = (torch.full(s, NAN, device="cuda") for s in ((c.n, c.H, c.W, c.ci), (c.co, c.ci, c.k, c.k), (c.co,)))
    rt.conv2d_backward_data(g, w, pad, dx=dx, accumulate=accumulate, scratch=nan_bytes(dbytes))
    rt.conv2d_backward_weight(x, g, c.k, pad, dw=dw, db=db, accumulate=accumulate, scratch=nan_bytes(wbytes))
    torch.cuda.synchronize()
    base = {"dX": inp["dx0"].double(), "dW": inp["dw0"].double(), "db": inp["db0"].double()} if accumulate else {}
    mm = exact.Mismatches()
    for name, got in (("dX", dx), ("dW", dw), ("db", db)):
        mm.check(got.cpu(), ref[name] + base.get(name, 0.0), "%s %s" % (cb.case_id(c), name))
    mm.raise_if_any()
    if c.k == 3 and c.H == 1 and c.W == 1 and not accumulate:
        taps = dw.cpu().reshape(c.co, c.ci, 9)
        assert torch.equal(taps[:, :, [0, 1, 2, 3, 5, 6, 7, 8]], torch.zeros(c.co, c.ci, 8)), "a 1x1 map feeds the centre tap only"
        assert bool((taps[:, :, 4] != 0).any())


def test_bias_gradient_is_optional(rt):
    c = CASES[0]
    inp, ref = cb.cached(c, "int", False)
    dw, db = rt.conv2d_backward_weight(inp["x"].cuda(), inp["g"].cuda(), c.k, 0, want_db=False)
    assert db is None
    exact.assert_exact(dw.cpu(), ref["dW"], "dW without db")


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relu_in_and_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    c = resolve(rt, c)
    inp, ref = cb.cached(c, "int", True)
    _, plain = cb.cached(c, "int", False)
    cb.check_caps(c, inp, ref)
    cb.check_caps(c, inp, plain)
    pad = (c.k - 1) // 2
    n, H, W, ci, co, k = c.n, c.H, c.W, c.ci, c.co, c.k
    dbytes, wbytes, _ = rt.conv2d_backward_plan(n, H, W, ci, co, k)
    px = n * H * W
    A = arena.Arena.for_sizes([px * 3 * ci * 4, px * 3 * co * 4, px * 3 * ci * 4, co * ci * k * k * 4, co * 4, co * ci * k * k * 4, dbytes, wbytes])
    xb = A.empty("x", (n, H, W, 3 * ci))               # outer slices: the arena's NaN sentinel
    gb = A.empty("g", (n, H, W, 3 * co))
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
    rt.conv2d_backward_data(gb, w, pad, dx=dxb, dx_coff=ci, accumulate=accumulate, scratch=sd, g_coff=co)
    rt.conv2d_backward_weight(xb, gb, k, pad, relu_in=True, x_coff=ci, ci=ci, g_coff=co, co=co, dw=dw, db=db, accumulate=accumulate, scratch=sw)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    dx_mid = dxb[..., ci:2 * ci].cpu()
    b = (lambda name: inp[name].double()) if accumulate else (lambda name: 0.0)
    mm.check(dx_mid, plain["dX"] + b("dx0"), "%s dX (before the mask)" % cb.case_id(c))
    mm.check(dw.cpu(), ref["dW"] + b("dw0"), "%s dW, relu_in" % cb.case_id(c))
    mm.check(db.cpu(), ref["db"] + b("db0"), "%s db" % cb.case_id(c))
    # OFFK_CONV_RELU_IN's mask on the conv's dX: in place, mask = the conv's input
    rt.relu_backward(dxb, xb, out=dxb, dy_coff=ci, y_coff=ci, out_coff=ci, c=ci)
    torch.cuda.synchronize()
    want = (plain["dX"] + b("dx0")) * (inp["x"] > 0).double()
    got = dxb[..., ci:2 * ci].cpu().double()
    assert torch.equal(got, want), "%s: masked dX differs at %d elements" % (cb.case_id(c), int((got != want).sum()))
    if not accumulate:
        assert torch.equal(got, ref["dX"]), "the masked dX is autograd's dX of conv(relu(x))"
    mm.raise_if_any()
    assert A.untouched(dxb[..., :ci]) and A.untouched(dxb[..., 2 * ci:]), "dx's neighbour slices were written"
    assert A.untouched(xb[..., :ci]) and A.untouched(gb[..., 2 * co:])
    A.check()


def test_relu_backward_special_values(rt):
    """the mask holds +0.0, -0.0, negatives, a positive subnormal and NaN; where it does not pass, the result is exactly 0 whatever dy is"""
    vals = torch.tensor([0.0, -0.0, -1.0, -1e-30, 1e-45, NAN, 2.0, 1e-30, float("inf"), -float("inf"), 3.0, 0.5])
    rows, C = 35, 24
    y = vals.repeat(rows * C // vals.numel()).reshape(1, 5, 7, C).contiguous()
    assert y.flatten()[4] > 0 and y.flatten()[4] < 1.2e-38, "the subnormal survived"
    dy = exact.ints(0xB0B, (1, 5, 7, C), -8, 8)
    dy.flatten()[::5] = NAN                     # NaN / inf upstream values under every kind of mask value
    dy.flatten()[3::7] = float("inf")
    base = exact.ints(0xB0C, (1, 5, 7, C), -64, 64)
    want = torch.where(y > 0, dy, torch.zeros_like(dy))
    A = arena.Arena.for_sizes([rows * C * 4] * 4)
    yd, dyd = A.put("y", y.cuda()), A.put("dy", dy.cuda())
    out = A.empty("out", (1, 5, 7, C))
    rt.relu_backward(dyd, yd, out=out)
    acc = A.put("acc", base.cuda())
    rt.relu_backward(dyd, yd, out=acc, accumulate=True)
    torch.cuda.synchronize()
    assert arena.same_bits(out.cpu(), want), "g = dy where y > 0, +0.0 elsewhere"
    masked = ~(y > 0)
    assert bool(masked.any()) and torch.equal(out.cpu()[masked], torch.zeros(int(masked.sum())))
    got, both = acc.cpu(), base + want          # (a NaN's payload after an addition is not pinned: NaN where NaN, equal elsewhere)
    assert torch.equal(got.isnan(), both.isnan()) and torch.equal(got[~both.isnan()], both[~both.isnan()])
    rt.relu_backward(dyd, yd, out=dyd)          # in place
    torch.cuda.synchronize()
    assert arena.same_bits(dyd.cpu(), want)
    assert arena.same_bits(yd.cpu(), y), "the mask is read only"
    A.check()
