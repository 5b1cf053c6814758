"""Cases, inputs and fp64 references of the fusion convs' backward (tests/test_gpu_conv_bwd_exact.py, tests/test_gpu_conv_bwd.py,
tests/test_gpu_fusion_conv_module.py).  Like tests/arena.py it has no tests of its own.

The references are torch's: torch.nn.functional.conv2d + autograd on the CPU in fp64, never the code under test.  A reference is
computed once per case, shared by every test that needs it and never written to.  Besides the gradients it holds, per output element,
the sum of the absolute values of its terms (the same autograd call on absolute values): the exactness condition of the integer tests
and the scale of the derived error bound of the normal-data tests.
"""
import collections

import torch
import torch.nn.functional as F

from . import exact

U = 2.0 ** -24                 # unit roundoff of fp32
LIMIT = float(2 ** 23)         # integer tests: every output's sum of |terms| (the accumulate base included) stays below this

# (n, H, W, Ci, Co) per kernel size: odd sizes, maps that are no multiple of the 32-position K-tile, 1 .. 13 channel tiles, more than one
# image per chunk; 1x1x1 and 2x2 maps for the 3x3 (all halo / every tap partly outside)
SHAPES = {
    1: [(1, 7, 7, 64, 64), (3, 14, 14, 256, 64), (5, 14, 14, 64, 256), (2, 7, 7, 512, 128), (2, 7, 7, 256, 1024), (1, 5, 3, 128, 128)],
    3: [(1, 7, 7, 64, 64), (3, 14, 14, 64, 64), (2, 7, 7, 128, 512), (2, 7, 7, 832, 256), (5, 7, 7, 256, 256), (2, 5, 3, 128, 128),
        (1, 1, 1, 64, 64), (1, 2, 2, 64, 64)],
}
# per kernel size, one more case whose n comes from the plan: >= 3 chunks, the last one shorter (n = None until chunked_n fills it in)
CHUNKED = {1: (None, 7, 7, 64, 64), 3: (None, 7, 7, 64, 64)}
# the 13 distinct shapes of the 22 stride-1 fusion convs: (H, Ci, Co, k)
FUSION_SHAPES = [(14, 64, 64, 1), (14, 64, 64, 3), (14, 64, 256, 1), (14, 256, 64, 1), (7, 128, 128, 1), (7, 128, 128, 3), (7, 128, 512, 1),
                 (7, 512, 128, 1), (7, 128, 512, 3), (7, 832, 256, 3), (7, 256, 256, 1), (7, 256, 256, 3), (7, 256, 1024, 1)]

Case = collections.namedtuple("Case", "k n H W ci co")


def cases():
    out = []
    for k in (1, 3):
        out += [Case(k, *s) for s in SHAPES[k]] + [Case(k, *CHUNKED[k])]
    return out


def case_id(c):
    return "k%d_n%s_%dx%d_%dto%d" % (c.k, "plan" if c.n is None else c.n, c.H, c.W, c.ci, c.co)


def chunked_n(plan, c):
    """The smallest n at which the plan cuts the weight gradient of `c` into >= 3 chunks with a shorter last one.
    plan = runtime.conv2d_backward_plan; chunks hold ceil(n / chunks) images each (include/offk.h)."""
    for n in range(3, 200):
        chunks = plan(n, c.H, c.W, c.ci, c.co, c.k)[2]
        ipc = -(-n // chunks)
        if chunks >= 3 and n - (chunks - 1) * ipc < ipc:
            return n
    raise AssertionError("no n below 200 gives >= 3 chunks with a short last one for %s" % (c,))


def gamma(m):
    """gamma_m = m u / (1 - m u): the bound of m roundings (Higham, Accuracy and Stability, lemma 3.1)"""
    return m * U / (1.0 - m * U)


def _seed(c, kind, what):
    return exact.stream(0x3B0 + c.k, kind, 0) * 4099 + (c.n * 131 + c.H * 17 + c.W * 5 + c.ci * 3 + c.co) * 16 + what


def int_inputs(c):
    """g, x in [-8, 8] with about a quarter exact zeros, w in [-4, 4], accumulate bases in [-64, 64]: channels-last fp32 on the CPU"""
    def sparse(what, shape):
        return exact.ints(_seed(c, 1, what), shape, -8, 8) * (exact.ints(_seed(c, 2, what), shape, 0, 3) != 0).float()
    d = {"x": sparse(0, (c.n, c.H, c.W, c.ci)), "g": sparse(1, (c.n, c.H, c.W, c.co)),
         "w": exact.ints(_seed(c, 3, 2), (c.co, c.ci, c.k, c.k), -4, 4)}
    d["dx0"] = exact.ints(_seed(c, 4, 3), (c.n, c.H, c.W, c.ci), -64, 64)
    d["dw0"] = exact.ints(_seed(c, 4, 4), (c.co, c.ci, c.k, c.k), -64, 64)
    d["db0"] = exact.ints(_seed(c, 4, 5), (c.co,), -64, 64)
    return d


def normal_inputs(c):
    gen = torch.Generator().manual_seed(_seed(c, 5, 0) & 0x7FFFFFFF)
    return {"x": torch.randn(c.n, c.H, c.W, c.ci, generator=gen), "g": torch.randn(c.n, c.H, c.W, c.co, generator=gen),
            "w": torch.randn(c.co, c.ci, c.k, c.k, generator=gen) * 0.05}


def reference(c, inp, relu_in):
    """fp64 on the CPU: dX (with relu_in: behind the mask of x, as the autograd of conv(relu(x)) gives it), dW, db, and for each the sum of
    the absolute values of its terms (dX_abs, dW_abs, db_abs).  Channels-last like the inputs."""
    pad = (c.k - 1) // 2

    def grads(x, g, w, mask_x):
        x = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = w.double().clone().requires_grad_(True)
        b = torch.zeros(c.co, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(torch.relu(x) if mask_x else x, w, b, padding=pad)
        y.backward(g.double().permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1).contiguous(), w.grad, b.grad

    dx, dw, db = grads(inp["x"], inp["g"], inp["w"], relu_in)
    xin = torch.relu(inp["x"]) if relu_in else inp["x"]
    # absolute values: no mask inside (|in(x)| is the operand), the mask of x applied to dX_abs afterwards
    dxa, dwa, dba = grads(xin.abs(), inp["g"].abs(), inp["w"].abs(), False)
    if relu_in:
        dxa = dxa * (inp["x"] > 0).double()
    return {"dX": dx, "dW": dw, "db": db, "dX_abs": dxa, "dW_abs": dwa, "db_abs": dba}


_REF = {}


def cached(c, kind, relu_in):
    """(inputs, reference) of a case with kind = "int" | "normal": computed once"""
    key = (c, kind, bool(relu_in))
    if key not in _REF:
        ikey = (c, kind, "inputs")
        if ikey not in _REF:
            _REF[ikey] = int_inputs(c) if kind == "int" else normal_inputs(c)
        _REF[key] = (_REF[ikey], reference(c, _REF[ikey], relu_in))
    return _REF[key]


def check_caps(c, inp, ref):
    """the integer tests' condition on the data: every output's sum of |terms|, plus the largest accumulate base, below 2^23"""
    for name, base in (("dX", "dx0"), ("dW", "dw0"), ("db", "db0")):
        cap = float(ref[name + "_abs"].max()) + float(inp[base].abs().max())
        assert cap < LIMIT, "%s %s: sum of |terms| %.0f is not below 2^23: these inputs do not make the result exact" % (case_id(c), name, cap)
