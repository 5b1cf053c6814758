"""Exact integer-input tests of the stride-2 fusion convs' backward (offk_conv2d_s2_backward_data, offk_conv2d_s2_backward_weight).

Inputs are small integers with the stride-1 tests' ranges (tests/conv_bwd_s2.py: g, x in [-8, 8] with a quarter exact zeros, w in
[-4, 4], accumulate bases in [-64, 64]).  The test first checks the reference's own condition on the data -- every output's sum of
|terms|, plus the base, is below 2^23 (the worst case over the table is 65,600 for dX and 12,608 for dW) -- under which every partial
sum in any order is an integer fp32 holds exactly; dX, dW and db must then EQUAL the fp64 reference (torch's conv2d(stride=2) +
autograd on the CPU), with and without accumulate.  No tolerance anywhere in this file: one tap of one phase read a pixel off, one
K-tile that straddles a padded row wrongly, the upper half of a 32-wide ci tile stored, is a failure.

The same cases run once more with relu_in = 1 and with x, g and dx as the middle slices of three-times-wider buffers, every buffer
carved from a guarded arena (tests/arena.py) whose sentinels must be intact afterwards.
"""
import pytest
import torch

import offk_amd  # noqa: F401

from . import arena
from . import conv_bwd_s2 as cs
from . import exact

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = cs.cases()
IDS = [cs.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def nan_bytes(n):
    return torch.full(((n + 3) // 4,), NAN, device="cuda").view(torch.uint8)[:n]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    c = cs.resolve(rt.conv2d_s2_backward_plan, c)
    inp, ref = cs.cached(c, "int", False)
    cs.check_caps(c, inp, ref)
    pad = cs.FORMS[c.k]
    x, g, w = inp["x"].cuda(), inp["g"].cuda(), inp["w"].cuda()
    dbytes, wbytes, _ = rt.conv2d_s2_backward_plan(c.n, c.H, c.W, c.ci, c.co, c.k)
    if accumulate:
        dx, dw, db = inp["dx0"].cuda(), inp["dw0"].cuda(), inp["db0"].cuda()
    else:
        dx, dw, db = (torch.full(s, NAN, device="cuda") for s in ((c.n, c.H, c.W, c.ci), (c.co, c.ci, c.k, c.k), (c.co,)))
    rt.conv2d_s2_backward_data(g, w, pad, dx=dx, accumulate=accumulate, scratch=nan_bytes(dbytes))
    rt.conv2d_s2_backward_weight(x, g, c.k, pad, dw=dw, db=db, accumulate=accumulate, scratch=nan_bytes(wbytes))
    torch.cuda.synchronize()
    base = {"dX": inp["dx0"].double(), "dW": inp["dw0"].double(), "db": inp["db0"].double()} if accumulate else {}
    mm = exact.Mismatches()
    for name, got in (("dX", dx), ("dW", dw), ("db", db)):
        mm.check(got.cpu(), ref[name] + base.get(name, 0.0), "%s %s" % (cs.case_id(c), name))
    mm.raise_if_any()
    if c.H == 2 and c.W == 2 and not accumulate:
        # a 1x1 output reads the 2x2 input under taps (pad, pad) .. (pad + 1, pad + 1) only
        taps = dw.cpu()
        inner = torch.zeros(c.k, c.k, dtype=torch.bool)
        inner[pad:pad + 2, pad:pad + 2] = True
        assert torch.equal(taps[:, :, ~inner], torch.zeros(c.co, c.ci, int((~inner).sum()))), "a 2x2 map feeds four taps only"
        assert bool((taps[:, :, inner] != 0).any())


def test_bias_gradient_is_optional(rt):
    c = CASES[2]
    inp, ref = cs.cached(c, "int", False)
    dw, db = rt.conv2d_s2_backward_weight(inp["x"].cuda(), inp["g"].cuda(), c.k, cs.FORMS[c.k], want_db=False)
    assert db is None
    exact.assert_exact(dw.cpu(), ref["dW"], "dW without db")


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relu_in_and_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    c = cs.resolve(rt.conv2d_s2_backward_plan, c)
    inp, ref = cs.cached(c, "int", True)
    _, plain = cs.cached(c, "int", False)
    cs.check_caps(c, inp, ref)
    cs.check_caps(c, inp, plain)
    pad = cs.FORMS[c.k]
    n, H, W, ci, co, k = c.n, c.H, c.W, c.ci, c.co, c.k
    OH, OW = H // 2, W // 2
    dbytes, wbytes, _ = rt.conv2d_s2_backward_plan(n, H, W, ci, co, k)
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
    rt.conv2d_s2_backward_data(gb, w, pad, dx=dxb, dx_coff=ci, accumulate=accumulate, scratch=sd, g_coff=co)
    rt.conv2d_s2_backward_weight(xb, gb, k, pad, relu_in=True, x_coff=ci, ci=ci, g_coff=co, co=co, dw=dw, db=db, accumulate=accumulate, scratch=sw)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    dx_mid = dxb[..., ci:2 * ci].cpu()
    b = (lambda name: inp[name].double()) if accumulate else (lambda name: 0.0)
    mm.check(dx_mid, plain["dX"] + b("dx0"), "%s dX (before the mask)" % cs.case_id(c))
    mm.check(dw.cpu(), ref["dW"] + b("dw0"), "%s dW, relu_in" % cs.case_id(c))
    mm.check(db.cpu(), ref["db"] + b("db0"), "%s db" % cs.case_id(c))
    # OFFK_CONV_RELU_IN's mask on the conv's dX: in place, mask = the conv's input
    rt.relu_backward(dxb, xb, out=dxb, dy_coff=ci, y_coff=ci, out_coff=ci, c=ci)
    torch.cuda.synchronize()
    want = (plain["dX"] + b("dx0")) * (inp["x"] > 0).double()
    got = dxb[..., ci:2 * ci].cpu().double()
    assert torch.equal(got, want), "%s: masked dX differs at %d elements" % (cs.case_id(c), int((got != want).sum()))
    if not accumulate:
        assert torch.equal(got, ref["dX"]), "the masked dX is autograd's dX of conv(relu(x))"
    mm.raise_if_any()
    assert A.untouched(dxb[..., :ci]) and A.untouched(dxb[..., 2 * ci:]), "dx's neighbour slices were written"
    assert A.untouched(xb[..., :ci]) and A.untouched(gb[..., 2 * co:])
    A.check()
