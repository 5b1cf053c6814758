"""Exact integer-input tests of the heads' training entries (offk_head_train, offk_head_backward).

Inputs are small integers (tests/head_bwd.py: x in 0 .. 4, w in -2 .. 2, b in -3 .. 3, g in -4 .. 4, accumulate bases in -64 .. 64), the
maps have power-of-two window counts (mean over 2x2, 4x4, 2x8; MaxPool(3, 2, ceil) on 5x5, 9x9, 5x9: 4, 16, 8 windows, the border ones
clipped) and drop_p is 0, 0.5 or 0.75 (scales 1, 2, 4), so 1 / nwin and every product are exact.  The test first checks the reference's
own condition on the data (head_bwd.check_exactness_condition); out, z, dX, dW and db must then EQUAL the fp64 reference -- torch ops and
autograd on the CPU with the numpy mask --, with and without both accumulate flags.  No tolerance anywhere in this file: a window read
one pixel off, a tie sent to the last maximum instead of the first, a mask drawn for the wrong quad, a chunk's slab left out of the
sum is a failure.
"""
import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401

from . import arena
from . import exact
from . import head_bwd as hb
from .featmaps import rt  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = hb.EXACT_CASES
IDS = [hb.case_id(c) for c in CASES]


def nan_bytes(n):
    return torch.full(((n + 3) // 4,), NAN, device="cuda").view(torch.uint8)[:n]


def test_the_table_covers_what_the_contract_names(rt):
    assert {c.C for c in CASES} >= {64, 256, 512, 1024} and {c.cls for c in CASES} >= {7, 101} and {c.n for c in CASES} >= {1, 3}
    assert {c.p for c in CASES} == {0.0, 0.5, 0.75}
    assert {(c.H, c.W, c.maxpool) for c in CASES} == {(2, 2, 0), (4, 4, 0), (2, 8, 0), (5, 5, 1), (9, 9, 1), (5, 9, 1)}
    long_ = [c for c in CASES if c.n == 34]
    assert long_
    for c in long_:
        chunks = rt.head_backward_plan(c.n, c.C, c.cls)[1]
        assert chunks >= 3 and c.n % (-(-c.n // chunks)) != 0


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    d, ref = hb.exact_inputs(c)
    hb.check_exactness_condition(c, d, ref)
    x, w, b, g = (d[k].cuda() for k in ("x", "w", "b", "g"))
    out, z = rt.head_train(x, w, b, c.maxpool, c.head, (c.seed, c.p), z=torch.full((c.n, c.C), NAN, device="cuda"),
                           out=torch.full((c.n, c.cls), NAN, device="cuda"))
    if accumulate:
        dx, dw, db = d["dx0"].cuda(), d["dw0"].cuda(), d["db0"].cuda()
    else:
        dx, dw, db = (torch.full(s, NAN, device="cuda") for s in ((c.n, c.H, c.W, c.C), (c.cls, c.C), (c.cls,)))
    rt.head_backward(g, x, w, z, c.maxpool, c.head, (c.seed, c.p), dx=dx, accumulate_dx=accumulate, dw=dw, db=db, accumulate_w=accumulate,
                     scratch=nan_bytes(rt.head_backward_plan(c.n, c.C, c.cls)[0]))
    torch.cuda.synchronize()
    base = {"dX": d["dx0"].double(), "dW": d["dw0"].double(), "db": d["db0"].double()} if accumulate else {}
    mm = exact.Mismatches()
    for name, got in (("out", out), ("z", z), ("dX", dx), ("dW", dw), ("db", db)):
        mm.check(got.cpu(), ref[name] + base.get(name, 0.0), "%s %s" % (hb.case_id(c), name))
    mm.raise_if_any()
    if c.p == 0.0:
        assert bool((z != 0).any(dim=1).all())
    else:
        assert torch.equal(z.cpu() != 0, ref["keep"] & (ref["pooled"] != 0)), "the mask implied by z"


def test_each_gradient_is_optional(rt):
    c = CASES[5]
    d, ref = hb.exact_inputs(c)
    x, w, b, g = (d[k].cuda() for k in ("x", "w", "b", "g"))
    _, z = rt.head_train(x, w, b, c.maxpool, c.head, (c.seed, c.p))
    drop = (c.seed, c.p)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, False, True)):
        dx, dw, db = rt.head_backward(g, x, w, z, c.maxpool, c.head, drop, want_dx=want[0], want_dw=want[1], want_db=want[2])
        torch.cuda.synchronize()
        for name, got, asked in (("dX", dx, want[0]), ("dW", dw, want[1]), ("db", db, want[2])):
            assert (got is not None) == asked, (want, name)
            if asked:
                exact.assert_exact(got.cpu(), ref[name], "%s alone %s" % (name, want))


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", [CASES[1], CASES[6]], ids=[IDS[1], IDS[6]])
def test_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    """x and dx are the middle slices of three-times-wider buffers; every buffer is a carve of a guarded arena whose sentinels (NaN) must
    be intact afterwards, the channels beside the slices included"""
    d, ref = hb.exact_inputs(c)
    n, H, W, C, cls = c.n, c.H, c.W, c.C, c.cls
    sbytes = rt.head_backward_plan(n, C, cls)[0]
    px = n * H * W
    A = arena.Arena.for_sizes([px * 3 * C * 4] * 2 + [cls * C * 4] * 2 + [cls * 4] * 2 + [n * cls * 4] * 2 + [n * C * 4, sbytes])
    xb, dxb = A.empty("x", (n, H, W, 3 * C)), A.empty("dx", (n, H, W, 3 * C))
    xb[..., C:2 * C] = d["x"].cuda()
    w, b, g = A.put("w", d["w"].cuda()), A.put("b", d["b"].cuda()), A.put("g", d["g"].cuda())
    z, out = A.empty("z", (n, C)), A.empty("out", (n, cls))
    if accumulate:
        dxb[..., C:2 * C] = d["dx0"].cuda()
        dw, db = A.put("dw", d["dw0"].cuda()), A.put("db", d["db0"].cuda())
    else:
        dw, db = A.empty("dw", (cls, C)), A.empty("db", (cls,))
    scratch = A.carve("scratch", sbytes)
    drop = (c.seed, c.p)
    rt.head_train(xb, w, b, c.maxpool, c.head, drop, x_coff=C, c=C, z=z, out=out)
    rt.head_backward(g, xb, w, z, c.maxpool, c.head, drop, x_coff=C, c=C, dx=dxb, dx_coff=C, accumulate_dx=accumulate, dw=dw, db=db,
                     accumulate_w=accumulate, scratch=scratch)
    torch.cuda.synchronize()
    base = (lambda name: d[name].double()) if accumulate else (lambda name: 0.0)
    mm = exact.Mismatches()
    mm.check(out.cpu(), ref["out"], "out")
    mm.check(z.cpu(), ref["z"], "z")
    mm.check(dxb[..., C:2 * C].cpu(), ref["dX"] + base("dx0"), "dX")
    mm.check(dw.cpu(), ref["dW"] + base("dw0"), "dW")
    mm.check(db.cpu(), ref["db"] + base("db0"), "db")
    mm.raise_if_any()
    assert A.untouched(dxb[..., :C]) and A.untouched(dxb[..., 2 * C:]), "dx's neighbour slices were written"
    assert A.untouched(xb[..., :C]) and A.untouched(xb[..., 2 * C:])
    A.check()


@pytest.mark.parametrize("c", [CASES[6], CASES[7], CASES[11]], ids=[IDS[6], IDS[7], IDS[11]])
def test_ties_go_to_the_first_maximum(rt, c):
    """x with whole windows of zeros, whole channels of zeros and values 0 .. 2 that repeat inside and across overlapping windows; dX must
    EQUAL torch's max_pool2d autograd (the first maximum in row-major window order; an all-zero window pays its top-left pixel)"""
    c = c._replace(p=0.0)
    d, ref = hb.exact_inputs(c, True)
    hb.check_exactness_condition(c, d, ref)
    assert float((d["x"] == 0).float().mean()) >= 0.5
    x, w, b, g = (d[k].cuda() for k in ("x", "w", "b", "g"))
    # torch's rule itself, in both memory layouts and on both devices: the routing of ones through max_pool2d
    routes = []
    for dev in ("cpu", "cuda"):
        for fmt in (torch.contiguous_format, torch.channels_last):
            xt = d["x"].to(dev).permute(0, 3, 1, 2).contiguous(memory_format=fmt).requires_grad_(True)
            F.max_pool2d(xt, 3, 2, ceil_mode=True).sum().backward()
            routes.append(xt.grad.cpu().contiguous())
    assert all(torch.equal(routes[0], r) for r in routes[1:]), "torch routes ties differently in some layout or device"
    assert float(routes[0][:, :, 0, 0].min()) >= 1.0, "window (0, 0) is all zero: its gradient goes to pixel (0, 0)"
    _, z = rt.head_train(x, w, b, 1, c.head, (c.seed, 0.0))
    dx, _, _ = rt.head_backward(g, x, w, z, 1, c.head, (c.seed, 0.0), dx=torch.full(d["x"].shape, NAN, device="cuda"), want_dw=False, want_db=False)
    torch.cuda.synchronize()
    exact.assert_exact(dx.cpu(), ref["dX"], "dX under ties")
    # and the same through the routing: dX = route * (g . w) / nwin
    v = (d["g"].double() @ d["w"].double()) / hb.nwin(c)
    assert torch.equal(dx.cpu().double(), routes[0].double().permute(0, 2, 3, 1) * v[:, None, None, :])
