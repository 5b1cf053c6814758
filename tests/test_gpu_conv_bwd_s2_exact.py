"""Exact integer-input tests of the stride-2 fusion convs' backward (offk_conv2d_s2_backward_data, offk_conv2d_s2_backward_weight).

Inputs are small integers with the stride-1 tests' ranges (tests/conv_bwd.py (S2): g, x in [-8, 8] with a quarter exact zeros, w in
[-4, 4], accumulate bases in [-64, 64]).  The test first checks the reference's own condition on the data -- every output's sum of
|terms|, plus the base, is below 2^23 (the worst case over the table is 65,600 for dX and 12,608 for dW) -- under which every partial
sum in any order is an integer fp32 holds exactly; dX, dW and db must then EQUAL the fp64 reference (torch's conv2d(stride=2) +
autograd on the CPU), with and without accumulate.  No tolerance anywhere in this file: one tap of one phase read a pixel off, one
K-tile that straddles a padded row wrongly, the upper half of a 32-wide ci tile stored, is a failure.

The same cases run once more with relu_in = 1 and with x, g and dx as the middle slices of three-times-wider buffers, every buffer
carved from a guarded arena (tests/arena.py) whose sentinels must be intact afterwards.

The bodies the two strides share are tests/conv_grad_checks.py's, written against tests/conv_bwd.py's forms; this file keeps the test
names, the parametrize lists and what this stride alone has.
"""
import pytest

import offk_amd  # noqa: F401

from . import conv_grad_checks as chk
from .conv_bwd import S2 as cs
from .conv_grad_checks import rt  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = cs.cases()
IDS = [cs.case_id(c) for c in CASES]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense_equals_fp64(rt, c, accumulate):
    chk.exact_dense(rt, cs, c, accumulate)


def test_bias_gradient_is_optional(rt):
    chk.exact_bias_optional(rt, cs, CASES[2])


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_relu_in_and_channel_slices_in_a_guarded_arena(rt, c, accumulate):
    chk.exact_relu_in_slices(rt, cs, c, accumulate)
