"""Exact integer-input tests of the fusion convs' backward (offk_relu_backward, offk_conv2d_backward_data, offk_conv2d_backward_weight).

Inputs are small integers from the project's generator (tests/conv_bwd.py: g, x in [-8, 8] with a quarter exact zeros, w in [-4, 4],
accumulate bases in [-64, 64]).  The test first checks the reference's own condition on the data -- every output's sum of |terms| is
below 2^23 -- under which every partial sum in any order is an integer fp32 holds exactly; dX, dW and db must then EQUAL the fp64
reference (torch's conv2d + autograd on the CPU), with and without accumulate.  No tolerance anywhere in this file: one lost term, one
tap read a row off, one K-tile that straddles an image boundary wrongly is a failure.

The same cases run once more with relu_in = 1 and with x, g and dx as the middle slices of three-times-wider buffers, every buffer
carved from a guarded arena (tests/arena.py) whose sentinels must be intact afterwards; the outer slices hold NaN (x, g) or must keep
their sentinel (dx).

The bodies the two strides share are tests/conv_grad_checks.py's, written against tests/conv_bwd.py's forms; this file keeps the test
names, the parametrize lists and what this stride alone has.
"""
import pytest
import torch

import offk_amd  # noqa: F401

from . import arena
from . import conv_grad_checks as chk
from . import exact
from .conv_bwd import S1 as cb
from .conv_grad_checks import rt  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
CASES = cb.cases()
IDS = [cb.case_id(c) for c in CASES]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    chk.exact_dense(rt, cb, c, accumulate)


def test_bias_gradient_is_optional(rt):
    chk.exact_bias_optional(rt, cb, CASES[0])


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relu_in_and_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    chk.exact_relu_in_slices(rt, cb, c, accumulate)


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
