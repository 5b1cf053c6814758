"""The fusion convs' backward on normal-distributed data: a derived error bound against fp64, run-to-run bit equality from differently
pre-filled scratch, and one capture / replay.

The bound is derived, not measured.  Every output element is a sum of n exact-product terms accumulated in fp32 (FMA chains on the
fp32 matrix pipe, split-K slabs added in a fixed order): for ANY order of such a sum

    |got - ref64| <= gamma_{n+1} * sum |terms|,    gamma_m = m u / (1 - m u),  u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; the products are not rounded inside an FMA, n + 1 leaves one
rounding to spare), with n = Co k^2 for dX and n_img H W for dW and db, and sum |terms| from the fp64 reference run on absolute
values (tests/conv_bwd.py).  No tolerance here is tuned against the kernel.

The bodies the two strides share are tests/conv_grad_checks.py's, written against tests/conv_bwd.py's forms; this file keeps the test
names, the parametrize lists and what this stride alone has.
"""
import pytest

import offk_amd  # noqa: F401

from . import conv_grad_checks as chk
from .conv_bwd import S1 as cb
from .conv_grad_checks import rt  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = cb.cases()
IDS = [cb.case_id(c) for c in CASES]


@pytest.mark.parametrize("relu_in", [False, True], ids=["plain", "relu_in"])
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_within_the_derived_bound_and_reproducible(rt, c, relu_in):
    chk.within_the_derived_bound_and_reproducible(rt, cb, c, relu_in)


@pytest.mark.parametrize("c", [CASES[2], CASES[10]], ids=[IDS[2], IDS[10]])
def test_capture_and_replay(rt, c):
    chk.capture_and_replay(rt, cb, c)
