"""Cases, inputs and fp64 references of the two stride-2 fusion convs' backward (tests/test_conv_bwd_s2_abi.py,
tests/test_gpu_conv_bwd_s2_exact.py, tests/test_gpu_conv_bwd_s2.py, tests/test_gpu_fusion_conv_s2_module.py).  No tests of its own.

As in tests/conv_bwd.py the references are torch's: torch.nn.functional.conv2d(stride=2) + autograd on the CPU in fp64, once on the
values and once on absolute values (the sum of |terms| of every output element), never the code under test.  A reference is computed
once per case, shared and never written to.  H and W are the INPUT map's size; g is [n, H / 2, W / 2, co].
"""
import torch
import torch.nn.functional as F

from . import exact
from .conv_bwd import LIMIT, U, Case, gamma  # noqa: F401  (re-exported: the tests take them from here)

FORMS = {7: 3, 5: 2}           # kernel size -> padding; stride 2
# (n, H, W, Ci, Co): the real shape; a half ci tile with two co tiles / a half ci tile; non-square with an OW that is no multiple of any
# tile; a 1x1 output (every tap partly outside)
SHAPES = {
    7: [(1, 28, 28, 320, 64), (3, 14, 14, 96, 128), (2, 6, 10, 64, 64), (1, 2, 2, 32, 64)],
    5: [(1, 14, 14, 1056, 128), (3, 14, 14, 96, 64), (2, 6, 4, 160, 64), (1, 2, 2, 32, 64)],
}
# per kernel size, one more case whose n comes from the plan: >= 3 chunks, the last one shorter (n = None until chunked_n fills it in)
CHUNKED = {7: (None, 6, 10, 64, 64), 5: (None, 6, 4, 32, 64)}
# the two real convs: (key, Ci, Co, k, H)
REAL = [("motion_conv_trans_28", 320, 64, 7, 28), ("motion_conv_trans_14", 1056, 128, 5, 14)]


def cases():
    out = []
    for k in (7, 5):
        out += [Case(k, *s) for s in SHAPES[k]] + [Case(k, *CHUNKED[k])]
    return out


def case_id(c):
    return "k%ds2_n%s_%dx%d_%dto%d" % (c.k, "plan" if c.n is None else c.n, c.H, c.W, c.ci, c.co)


def chunked_n(plan, c):
    """The smallest n at which the plan cuts the weight gradient of `c` into >= 3 chunks with a shorter last one.
    plan = runtime.conv2d_s2_backward_plan; chunks hold ceil(n / chunks) images each (include/offk.h)."""
    for n in range(3, 200):
        chunks = plan(n, c.H, c.W, c.ci, c.co, c.k)[2]
        ipc = -(-n // chunks)
        if chunks >= 3 and n - (chunks - 1) * ipc < ipc:
            return n
    raise AssertionError("no n below 200 gives >= 3 chunks with a short last one for %s" % (c,))


def resolve(plan, c):
    """the plan-chosen case, its property asserted"""
    if c.n is not None:
        return c
    n = chunked_n(plan, c)
    chunks = plan(n, c.H, c.W, c.ci, c.co, c.k)[2]
    ipc = -(-n // chunks)
    assert chunks >= 3 and 0 < n - (chunks - 1) * ipc < ipc, (n, chunks, ipc)
    return c._replace(n=n)


def dx_terms(c):
    """terms of the longest dX sum: Co x the largest phase's taps"""
    return c.co * ((c.k + 1) // 2) ** 2


def _seed(c, kind, what):
    return exact.stream(0x3B2 + c.k, kind, 0) * 4099 + (c.n * 131 + c.H * 17 + c.W * 5 + c.ci * 3 + c.co) * 16 + what


def int_inputs(c):
    """g, x in [-8, 8] with about a quarter exact zeros, w in [-4, 4], accumulate bases in [-64, 64]: channels-last fp32 on the CPU"""
    def sparse(what, shape):
        return exact.ints(_seed(c, 1, what), shape, -8, 8) * (exact.ints(_seed(c, 2, what), shape, 0, 3) != 0).float()
    d = {"x": sparse(0, (c.n, c.H, c.W, c.ci)), "g": sparse(1, (c.n, c.H // 2, c.W // 2, c.co)),
         "w": exact.ints(_seed(c, 3, 2), (c.co, c.ci, c.k, c.k), -4, 4)}
    d["dx0"] = exact.ints(_seed(c, 4, 3), (c.n, c.H, c.W, c.ci), -64, 64)
    d["dw0"] = exact.ints(_seed(c, 4, 4), (c.co, c.ci, c.k, c.k), -64, 64)
    d["db0"] = exact.ints(_seed(c, 4, 5), (c.co,), -64, 64)
    return d


def normal_inputs(c):
    gen = torch.Generator().manual_seed(_seed(c, 5, 0) & 0x7FFFFFFF)
    return {"x": torch.randn(c.n, c.H, c.W, c.ci, generator=gen), "g": torch.randn(c.n, c.H // 2, c.W // 2, c.co, generator=gen),
            "w": torch.randn(c.co, c.ci, c.k, c.k, generator=gen) * 0.05}


def reference(c, inp, relu_in):
    """fp64 on the CPU: dX (with relu_in: behind the mask of x), dW, db, and for each the sum of the absolute values of its terms"""
    def grads(x, g, w, mask_x):
        x = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = w.double().clone().requires_grad_(True)
        b = torch.zeros(c.co, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(torch.relu(x) if mask_x else x, w, b, stride=2, padding=FORMS[c.k])
        y.backward(g.double().permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1).contiguous(), w.grad, b.grad

    dx, dw, db = grads(inp["x"], inp["g"], inp["w"], relu_in)
    xin = torch.relu(inp["x"]) if relu_in else inp["x"]
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
