"""Shared by the tests of the heads' training entries (offk_head_train / offk_head_backward): the fp64 reference of one head -- torch ops
on the CPU, built from the same fp32 inputs and the numpy mask (synth.head_dropout_keep) -- and the integer inputs of the exact tests.
A reference is computed once per case and shared (lru_cache); nobody writes into it."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import synth

from . import exact

Case = collections.namedtuple("Case", "H W maxpool C cls n p head seed")
U = 2.0 ** -24


def case_id(c):
    return "%dx%d%s_c%d_k%d_n%d_p%g" % (c.H, c.W, "max" if c.maxpool else "avg", c.C, c.cls, c.n, c.p)


def nwin(c):
    return ((c.H - 2) // 2 + 1) * ((c.W - 2) // 2 + 1) if c.maxpool else c.H * c.W


def scale32(p):
    """the entry's scale: (float)(1.0 / (1.0 - p))"""
    return float(np.float32(1.0 / (1.0 - p)))


def keep_of(c):
    return torch.from_numpy(synth.head_dropout_keep(c.seed, c.head, c.n, c.C, c.p))


def gamma(k):
    return k * U / (1.0 - k * U)


def pooled64(xd, maxpool):
    """xd: fp64 [n, C, H, W] -> the head's pooled vector [n, C] (RGB_OFF.py:782-784, 789-790, 843-844)"""
    return (F.max_pool2d(xd, 3, 2, ceil_mode=True) if maxpool else xd).mean(dim=(2, 3))


def reference(c, x, w, b, g):
    """fp64 forward and backward of the head on fp32 inputs x [n, H, W, C], w [cls, C], b [cls], g [n, cls]:
    dict out, z, dX [n, H, W, C], dW, db, plus the sums of |terms| behind out and dX (mag_out, mag_dX)."""
    keep, s = keep_of(c).double(), scale32(c.p)
    xd = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pooled = pooled64(xd, c.maxpool)
    z = pooled * keep * s
    out = z @ wd.t() + bd
    out.backward(g.double())
    r = {"out": out.detach(), "z": z.detach(), "pooled": pooled.detach(), "dX": xd.grad.permute(0, 2, 3, 1).contiguous(), "dW": wd.grad,
         "db": bd.grad, "keep": keep.bool()}
    # sums of absolute terms: out through |x| (post-ReLU data: x itself where x >= 0), |w|, |b|; dX by routing |g| . |w| the same way
    xa = x.double().abs().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    pa = pooled64(xa, c.maxpool)
    r["mag_out"] = ((pa * keep * s) @ w.double().abs().t() + b.double().abs()).detach()
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    (mag_dx,) = torch.autograd.grad(pooled64(xr, c.maxpool), xr, grad_outputs=(g.double().abs() @ w.double().abs()) * keep * s)
    r["mag_dX"] = mag_dx.permute(0, 2, 3, 1).contiguous()
    return r


# ---- integer inputs of the exact tests ---------------------------------------------------------------------------------------------
_X, _W, _B, _G, _DX0, _DW0, _DB0 = range(7)
# (H, W, maxpool): window counts 4, 16, 16 (mean) and 4, 16, 8 (max-pool, every border window clipped): 1 / nwin is exact
EXACT_CASES = [
    Case(2, 2, 0, 64, 7, 1, 0.0, 0, 11),
    Case(4, 4, 0, 256, 101, 3, 0.5, 1, 12),
    Case(2, 8, 0, 512, 7, 3, 0.75, 2, 13),
    Case(4, 4, 0, 1024, 101, 1, 0.5, 2, 14),
    Case(2, 8, 0, 64, 101, 3, 0.75, 1, 15),
    Case(5, 5, 1, 64, 101, 3, 0.5, 0, 16),
    Case(9, 9, 1, 256, 7, 1, 0.75, 0, 17),
    Case(5, 9, 1, 512, 101, 3, 0.0, 1, 18),
    Case(9, 9, 1, 1024, 7, 3, 0.5, 2, 19),
    Case(5, 5, 1, 256, 101, 1, 0.0, 0, 20),
    # n_img = 34: the smallest whose plan has >= 3 chunks with a shorter last one (12 + 12 + 10; tests/test_head_bwd_abi.py)
    Case(2, 2, 0, 64, 7, 34, 0.5, 1, 21),
    Case(5, 5, 1, 128, 101, 34, 0.75, 0, 22),
]


@functools.lru_cache(maxsize=None)
def exact_inputs(c, zeros=False):
    """x in 0 .. 4 (post-ReLU: RGB_OFF.py:780), w in -2 .. 2, b in -3 .. 3, g in -4 .. 4, accumulate bases in -64 .. 64; zeros: x for the
    tie test -- most of it 0, whole windows of 0, values 0 .. 2 so that maxima repeat inside and across overlapping windows."""
    st = lambda kind: exact.stream(c.seed, kind)       # noqa: E731
    x = exact.ints(st(_X), (c.n, c.H, c.W, c.C), 0, 4)
    if zeros:
        x = exact.ints(st(_X), (c.n, c.H, c.W, c.C), 0, 2) * (exact.ints(st(_X) + 1, (c.n, c.H, c.W, c.C), 0, 2) == 0).float()
        x[:, :3, :3, :] = 0.0                          # window (0, 0) is all zero in every channel
        x[:, :, :, 0:c.C:5] = 0.0                      # whole channels of zeros: every window ties at 0
    d = {"x": x, "w": exact.ints(st(_W), (c.cls, c.C), -2, 2), "b": exact.ints(st(_B), (c.cls,), -3, 3),
         "g": exact.ints(st(_G), (c.n, c.cls), -4, 4), "dx0": exact.ints(st(_DX0), (c.n, c.H, c.W, c.C), -64, 64),
         "dw0": exact.ints(st(_DW0), (c.cls, c.C), -64, 64), "db0": exact.ints(st(_DB0), (c.cls,), -64, 64)}
    ref = reference(c, d["x"], d["w"], d["b"], d["g"])
    return d, ref


def check_exactness_condition(c, d, ref):
    """The reference's own condition on the data, not a tolerance: every value is a multiple of 1 / nwin (a power of two) and every
    output's sum of |terms| plus the accumulate base, in units of 1 / nwin, stays below 2^23 -- then every partial sum in any order is
    exact in fp32."""
    nw = nwin(c)
    assert nw & (nw - 1) == 0, "window count must be a power of two"
    s = scale32(c.p)
    assert s in (1.0, 2.0, 4.0)
    za = ref["z"].abs()
    caps = {"out": float(ref["mag_out"].max()), "dX": float(ref["mag_dX"].max()) + 64, "dW": float((d["g"].double().abs().t() @ za).max()) + 64,
            "db": float(d["g"].double().abs().sum(0).max()) + 64}
    for name, cap in caps.items():
        assert cap * nw < 2.0 ** 23, (case_id(c), name, cap)
    for name in ("out", "z", "dX", "dW", "db"):
        v = ref[name] * nw
        assert torch.equal(v, v.round()), (case_id(c), name)
