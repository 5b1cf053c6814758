"""The stride-2 fusion convs' backward on normal-distributed data: a derived error bound against fp64, run-to-run bit equality from
differently pre-filled scratch, and one capture / replay.

The bound is derived, not measured (tests/test_gpu_conv_bwd.py has the argument): every output element is a sum of m exact-product
terms accumulated in fp32 in some fixed order, so

    |got - ref64| <= gamma_{m+1} * sum |terms|,    gamma_m = m u / (1 - m u),  u = 2^-24

with m = Co ceil(k / 2)^2 for dX (the largest of the four phases: 16 or 9 taps) and m = n OH OW for dW and db, and sum |terms| from
the fp64 reference run on absolute values (tests/conv_bwd_s2.py).  No tolerance here is tuned against the kernel.
"""
import pytest
import torch

import offk_amd  # noqa: F401

from . import conv_bwd_s2 as cs

pytestmark = pytest.mark.gpu
CASES = cs.cases()
IDS = [cs.case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def filled_bytes(n, value):
    return torch.full(((n + 3) // 4,), value, device="cuda").view(torch.uint8)[:n]


def run(rt, c, x, g, w, relu_in, fill):
    """dX (masked by x where relu_in), dW, db from scratch buffers pre-filled with `fill`"""
    pad = cs.FORMS[c.k]
    dbytes, wbytes, _ = rt.conv2d_s2_backward_plan(c.n, c.H, c.W, c.ci, c.co, c.k)
    dx = rt.conv2d_s2_backward_data(g, w, pad, scratch=filled_bytes(dbytes, fill))
    if relu_in:
        rt.relu_backward(dx, x, out=dx)
    dw, db = rt.conv2d_s2_backward_weight(x, g, c.k, pad, relu_in=relu_in, scratch=filled_bytes(wbytes, fill))
    torch.cuda.synchronize()
    return dx, dw, db


@pytest.mark.parametrize("relu_in", [False, True], ids=["plain", "relu_in"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_within_the_derived_bound_and_reproducible(rt, c, relu_in):
    c = cs.resolve(rt.conv2d_s2_backward_plan, c)
    inp, ref = cs.cached(c, "normal", relu_in)
    x, g, w = inp["x"].cuda(), inp["g"].cuda(), inp["w"].cuda()
    got = run(rt, c, x, g, w, relu_in, float("nan"))
    pixels = c.n * (c.H // 2) * (c.W // 2)
    terms = {"dX": cs.dx_terms(c), "dW": pixels, "db": pixels}
    worst = {}
    for name, t in zip(("dX", "dW", "db"), got):
        err = (t.cpu().double() - ref[name]).abs()
        bound = cs.gamma(terms[name] + 1) * ref[name + "_abs"]
        assert bool(torch.isfinite(t).all()), name
        assert bool((err[bound == 0] == 0).all()), "%s %s: an element without terms is not 0" % (cs.case_id(c), name)
        worst[name] = float((err / bound.clamp_min(1e-300)).max())
        print("%s %s: largest error %.3e, largest error / bound %.3f" % (cs.case_id(c), name, float(err.max()), worst[name]))
    for name in worst:
        assert worst[name] <= 1.0, "%s %s: error is %.3f of the derived bound" % (cs.case_id(c), name, worst[name])
    again = run(rt, c, x, g, w, relu_in, -3.0)
    for name, a, b in zip(("dX", "dW", "db"), got, again):
        assert torch.equal(a, b), "%s %s: two runs from differently pre-filled scratch differ" % (cs.case_id(c), name)


@pytest.mark.parametrize("c", [CASES[1], CASES[7]], ids=[IDS[1], IDS[7]])
def test_capture_and_replay(rt, c):
    """relu_backward -> data -> weight on one stream, captured once, replayed twice: equal to the eager results bit for bit"""
    inp, _ = cs.cached(c, "normal", False)
    pad = cs.FORMS[c.k]
    x, gy, w = inp["x"].cuda(), inp["g"].cuda(), inp["w"].cuda()
    y = torch.randn(gy.shape, generator=torch.Generator().manual_seed(7)).cuda()       # the stored output whose ReLU is undone
    dbytes, wbytes, _ = rt.conv2d_s2_backward_plan(c.n, c.H, c.W, c.ci, c.co, c.k)

    def buffers():
        return dict(g=torch.full_like(gy, float("nan")), dx=torch.full_like(x, float("nan")), dw=torch.full_like(w, float("nan")),
                    db=torch.full((c.co,), float("nan"), device="cuda"), sd=filled_bytes(dbytes, float("nan")), sw=filled_bytes(wbytes, float("nan")))

    def chain(b):
        rt.relu_backward(gy, y, out=b["g"])
        rt.conv2d_s2_backward_data(b["g"], w, pad, dx=b["dx"], scratch=b["sd"])
        rt.conv2d_s2_backward_weight(x, b["g"], c.k, pad, dw=b["dw"], db=b["db"], scratch=b["sw"])

    eager = buffers()
    chain(eager)
    torch.cuda.synchronize()
    cap = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(cap)
    for _ in range(2):
        for k in ("g", "dx", "dw", "db"):
            cap[k].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in ("g", "dx", "dw", "db"):
            assert torch.equal(cap[k], eager[k]), "replay differs from the eager run in %s" % k
    assert bool(torch.isfinite(eager["dw"]).all()) and bool((eager["g"] == 0).any())
