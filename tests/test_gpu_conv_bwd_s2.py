"""The stride-2 fusion convs' backward on normal-distributed data: a derived error bound against fp64, run-to-run bit equality from
differently pre-filled scratch, and one capture / replay.

The bound is derived, not measured (tests/test_gpu_conv_bwd.py has the argument): every output element is a sum of m exact-product
terms accumulated in fp32 in some fixed order, so

    |got - ref64| <= gamma_{m+1} * sum |terms|,    gamma_m = m u / (1 - m u),  u = 2^-24

with m = Co ceil(k / 2)^2 for dX (the largest of the four phases: 16 or 9 taps) and m = n OH OW for dW and db, and sum |terms| from
the fp64 reference run on absolute values (tests/conv_bwd.py (S2)).  No tolerance here is tuned against the kernel.

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


@pytest.mark.parametrize("relu_in", [False, True], ids=["plain", "relu_in"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_within_the_derived_bound_and_reproducible(rt, c, relu_in):
    chk.within_the_derived_bound_and_reproducible(rt, cs, c, relu_in)


@pytest.mark.parametrize("c", [CASES[1], CASES[7]], ids=[IDS[1], IDS[7]])
def test_capture_and_replay(rt, c):
    chk.capture_and_replay(rt, cs, c)
