"""The heads' training entries on normal data and the real map forms: 14x14x256 with max-pool (the 28-head), 7x7x512 (the 14-head),
7x7x1024 (the 7-head), n = 3 and 5, p = 0.8 (RGB_OFF.py:782-793, 843-847).  Every output must lie within gamma_k * sum |terms| of
the fp64 reference (torch ops on the CPU from the same fp32 inputs and the numpy mask), gamma_k = k u / (1 - k u), u = 2^-24, with k the
number of rounded operations in the longest chain behind one element -- derived below from the kernels' sums, not fitted:

  out  k = nwin + C + 4.  pooled: nwin - 1 adds of the windows (a window's maximum is exact), the rounded constant 1.f / nwin and the
       multiply by it: nwin + 1; the multiply by keep * scale: 1 (scale itself is the reference's fp32 constant); the Linear: no chain
       of it is longer than C fused multiply-adds and adds (a thread's share of the products, the wavefront and block reduction), and
       the bias add: C + 1; one more for the product terms' own rounding inside z.  Sum of |terms|: sum_c |w| z + |b| (x >= 0).
  dW   k = n_img + 1, db the same, against a reference built from the DEVICE's own z (z's error is out's business): a chunk is a chain
       of ceil(n_img / chunks) fused multiply-adds, the chunks are added in order (chunks - 1 adds), together at most n_img; one spare.
  dX   k = classes + 5.  dz: a group's ceil(classes / 8) fused multiply-adds and the 7 adds of the eight groups -- 20 operations at 101
       classes, never more than `classes` from 9 classes on --; the multiply by keep * scale, the rounded constant 1.f / nwin and the
       multiply by it: 3; a pixel is the first maximum of at most four windows and the first add (to zero) is exact: 3.  The longest
       chain at 101 classes is therefore 20 + 3 + 3 = 26 operations; k = classes + 5 = 106 is the contract's figure and covers it.
The sums of |terms| are the reference's (tests/head_bwd.py).  Also here: the mask implied by z, bit-equality from NaN-filled and
-3-filled scratch, and graph capture."""
import pytest
import torch

import offk_amd  # noqa: F401

from . import arena
from . import head_bwd as hb
from .featmaps import rt  # noqa: F401

pytestmark = pytest.mark.gpu
FORMS = {"head28": (14, 14, 1, 256, 0), "head14": (7, 7, 0, 512, 1), "head7": (7, 7, 0, 1024, 2)}
CASES = [hb.Case(H, W, mp, C, 101, n, 0.8, head, 100 + 7 * head + n) for (H, W, mp, C, head) in FORMS.values() for n in (3, 5)]
IDS = [hb.case_id(c) for c in CASES]


_CACHE = {}


def normal_inputs(c):
    """post-ReLU normal x (about half zeros, as the stage outputs the heads read), w and b at nn.Linear's scale, normal g; the reference once"""
    if c not in _CACHE:
        gen = torch.Generator().manual_seed(c.seed)
        x = torch.randn(c.n, c.H, c.W, c.C, generator=gen).clamp_(min=0.0)
        k = c.C ** -0.5
        w = (torch.rand(c.cls, c.C, generator=gen) * 2 - 1) * k
        b = (torch.rand(c.cls, generator=gen) * 2 - 1) * k
        g = torch.randn(c.n, c.cls, generator=gen)
        _CACHE[c] = ((x, w, b, g), hb.reference(c, x, w, b, g))
    return _CACHE[c]


def run(rt, c, dev, scratch_fill=float("nan")):
    x, w, b, g = dev
    drop = (c.seed, c.p)
    out, z = rt.head_train(x, w, b, c.maxpool, c.head, drop)
    nbytes = rt.head_backward_plan(c.n, c.C, c.cls)[0]
    scratch = torch.full((nbytes // 4,), scratch_fill, device="cuda").view(torch.uint8)
    dx, dw, db = rt.head_backward(g, x, w, z, c.maxpool, c.head, drop, scratch=scratch)
    torch.cuda.synchronize()
    return out, z, dx, dw, db


def within(got, ref, mag, k, what):
    err = (got.cpu().double() - ref).abs()
    bound = hb.gamma(k) * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print("%s: worst error / bound = %.3f (k = %d)" % (what, worst, k))
    assert bool((err <= bound).all()), "%s: %d elements beyond gamma_%d * sum |terms|, worst ratio %.3f" % (what, int((err > bound).sum()), k, worst)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_within_the_derived_bounds(rt, c):
    (x, w, b, g), ref = normal_inputs(c)
    out, z, dx, dw, db = run(rt, c, tuple(t.cuda() for t in (x, w, b, g)))
    nw = hb.nwin(c)
    assert nw == 49
    within(out, ref["out"], ref["mag_out"], nw + c.C + 4, "out")
    # z: pooled (nwin + 1 operations) and one multiply; its sum of |terms| is z itself (x >= 0)
    within(z, ref["z"], ref["z"].abs(), nw + 2, "z")
    zd, gd = z.cpu().double(), g.double()
    within(dw, gd.t() @ zd, gd.abs().t() @ zd.abs(), c.n + 1, "dW")
    within(db, gd.sum(0), gd.abs().sum(0), c.n + 1, "db")
    within(dx, ref["dX"], ref["mag_dX"], c.cls + 5, "dX")
    # the mask implied by z: pooled > 0 everywhere on this data (a mean of 49 post-ReLU normals), so z != 0 exactly where kept
    assert bool((ref["pooled"] > 0).all())
    assert torch.equal(z.cpu() != 0, ref["keep"]), "the mask implied by z is not synth.head_dropout_keep"
    kept = float(ref["keep"].float().mean())
    assert abs(kept - 0.2) <= 4 * (0.16 / ref["keep"].numel()) ** 0.5
    # dropped channels get no gradient at all, kept ones some
    assert bool((dx.cpu()[:, :, :, ~ref["keep"].any(0)] == 0).all())


@pytest.mark.parametrize("c", [CASES[1], CASES[5]], ids=[IDS[1], IDS[5]])
def test_results_do_not_depend_on_the_scratch(rt, c):
    (x, w, b, g), _ = normal_inputs(c)
    dev = tuple(t.cuda() for t in (x, w, b, g))
    first = run(rt, c, dev, float("nan"))
    second = run(rt, c, dev, -3.0)
    for name, a, b_ in zip(("out", "z", "dX", "dW", "db"), first, second):
        assert arena.same_bits(a, b_), name


@pytest.mark.parametrize("c", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_graph_replay_equals_eager(rt, c):
    (x, w, b, g), _ = normal_inputs(c)
    x, w, b, g = (t.cuda() for t in (x, w, b, g))
    drop = (c.seed, c.p)
    nbytes = rt.head_backward_plan(c.n, c.C, c.cls)[0]
    bufs = {"out": torch.empty(c.n, c.cls, device="cuda"), "z": torch.empty(c.n, c.C, device="cuda"), "dx": torch.empty(c.n, c.H, c.W, c.C, device="cuda"),
            "dw": torch.empty(c.cls, c.C, device="cuda"), "db": torch.empty(c.cls, device="cuda")}
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def launch():
        rt.head_train(x, w, b, c.maxpool, c.head, drop, z=bufs["z"], out=bufs["out"])
        rt.head_backward(g, x, w, bufs["z"], c.maxpool, c.head, drop, dx=bufs["dx"], dw=bufs["dw"], db=bufs["db"], scratch=scratch)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = dict((k, v.clone()) for k, v in bufs.items())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for v in bufs.values():
        v.fill_(float("nan"))
    scratch.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    for k in bufs:
        assert arena.same_bits(eager[k], bufs[k]), k
