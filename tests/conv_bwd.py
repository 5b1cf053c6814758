"""Cases, inputs and fp64 references of the fusion convs' backward, both strides: one `Form` per stride, S1 (1x1 and 3x3, stride 1) and S2
(7x7 and 5x5, stride 2), the two rows the library's own table of conv backward entries has per arithmetic.  The tests bind the form they
are about (`from .conv_bwd import S1 as cb`, `from .conv_bwd import S2 as cs`) and everything that differs between the strides -- kernel
sizes, shape tables, the seed base, the id format, the size of g, the length of the longest dX sum, the names of the runtime's plan and
compute functions -- is a field or a method of it.  tests/conv_grad_checks.py holds the GPU test bodies written against a form.  Like
tests/arena.py this module has no tests of its own.

The references are torch's: torch.nn.functional.conv2d + autograd on the CPU in fp64, never the code under test.  A reference is
computed once per case, shared by every test that needs it and never written to.  Besides the gradients it holds, per output element,
the sum of the absolute values of its terms (the same autograd call on absolute values): the exactness condition of the integer tests
and the scale of the derived error bound of the normal-data tests.  H and W are the INPUT map's size; g is [n, H / stride, W / stride, co].
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from offk_amd import synth

from . import exact

U = 2.0 ** -24                 # unit roundoff of fp32
LIMIT = float(2 ** 23)         # integer tests: every output's sum of |terms| (the accumulate base included) stays below this

Case = collections.namedtuple("Case", "k n H W ci co")


def gamma(m):
    """gamma_m = m u / (1 - m u): the bound of m roundings (Higham, Accuracy and Stability, lemma 3.1)"""
    return m * U / (1.0 - m * U)


def wide_ints(seed, shape, one_in=32):
    """sparse (one in `one_in`) odd integers of 17 significant bits, either sign: bit 16, seven random bits, bit 8, seven random bits,
    bit 0 -- the leading plane takes bits 16 .. 9, the middle one bits 8 .. 1, the last one bit 0.  The weight-gradient tests take one in
    thirty-two (about five wide terms per output, sum of |terms| near 2^22), the data-gradient tests pass their own density."""
    hi = exact.ints(exact.stream(seed, 1, 0), shape, 0, 127)
    lo = exact.ints(exact.stream(seed, 2, 0), shape, 0, 127)
    sign = exact.ints(exact.stream(seed, 3, 0), shape, 0, 1) * 2 - 1
    on = (exact.ints(exact.stream(seed, 4, 0), shape, 0, one_in - 1) == 0).float()
    return (65536 + hi * 512 + 256 + lo * 2 + 1) * sign * on


class Form:
    """One stride of the fusion convs' backward.  The names of the runtime functions are strings: the runtime is looked at on the GPU only."""
    Case, LIMIT, U, gamma = Case, LIMIT, U, staticmethod(gamma)

    def __init__(self, stride, ks, seed_base, id_format, shapes, chunked, worst, worst_seed, entries, **tables):
        self.stride, self.ks, self.seed_base, self.id_format = stride, ks, seed_base, id_format
        self.FORMS = dict((k, (k - 1) // 2) for k in ks)           # kernel size -> padding
        self.SHAPES, self.CHUNKED = shapes, chunked
        self.WORST, self.worst_seed = worst, worst_seed            # the data gradient's worst-case shapes (k, n, H, W, ci, co); g's seed
        self.plan, self.data, self.weight, self.data_plan_split, self.weight_plan_split = entries
        self.__dict__.update(tables)                               # FUSION_SHAPES (S1), REAL (S2)
        self._ref = {}

    def cases(self):
        out = []
        for k in self.ks:
            out += [Case(k, *s) for s in self.SHAPES[k]] + [Case(k, *self.CHUNKED[k])]
        return out

    def case_id(self, c):
        return self.id_format % (c.k, "plan" if c.n is None else c.n, c.H, c.W, c.ci, c.co)

    def out_hw(self, c):
        """(OH, OW): the size of g's map"""
        return c.H // self.stride, c.W // self.stride

    def dx_terms(self, c):
        """terms of the longest dX sum: Co x the taps of the largest phase (stride 1: all k k of them)"""
        return c.co * (-(-c.k // self.stride)) ** 2

    def chunked_n(self, plan, c):
        """The smallest n at which the plan cuts the weight gradient of `c` into >= 3 chunks with a shorter last one.
        plan = the runtime's function named self.plan; chunks hold ceil(n / chunks) images each (include/offk.h)."""
        for n in range(3, 200):
            chunks = plan(n, c.H, c.W, c.ci, c.co, c.k)[2]
            ipc = -(-n // chunks)
            if chunks >= 3 and n - (chunks - 1) * ipc < ipc:
                return n
        raise AssertionError("no n below 200 gives >= 3 chunks with a short last one for %s" % (c,))

    def resolve(self, plan, c):
        """the plan-chosen case, its property asserted"""
        if c.n is not None:
            return c
        n = self.chunked_n(plan, c)
        chunks = plan(n, c.H, c.W, c.ci, c.co, c.k)[2]
        ipc = -(-n // chunks)
        assert chunks >= 3 and 0 < n - (chunks - 1) * ipc < ipc, (n, chunks, ipc)
        return c._replace(n=n)

    def _seed(self, c, kind, what):
        return exact.stream(self.seed_base + c.k, kind, 0) * 4099 + (c.n * 131 + c.H * 17 + c.W * 5 + c.ci * 3 + c.co) * 16 + what

    def int_inputs(self, c):
        """g, x in [-8, 8] with about a quarter exact zeros, w in [-4, 4], accumulate bases in [-64, 64]: channels-last fp32 on the CPU"""
        def sparse(what, shape):
            return exact.ints(self._seed(c, 1, what), shape, -8, 8) * (exact.ints(self._seed(c, 2, what), shape, 0, 3) != 0).float()
        d = {"x": sparse(0, (c.n, c.H, c.W, c.ci)), "g": sparse(1, (c.n,) + self.out_hw(c) + (c.co,)),
             "w": exact.ints(self._seed(c, 3, 2), (c.co, c.ci, c.k, c.k), -4, 4)}
        d["dx0"] = exact.ints(self._seed(c, 4, 3), (c.n, c.H, c.W, c.ci), -64, 64)
        d["dw0"] = exact.ints(self._seed(c, 4, 4), (c.co, c.ci, c.k, c.k), -64, 64)
        d["db0"] = exact.ints(self._seed(c, 4, 5), (c.co,), -64, 64)
        return d

    def normal_inputs(self, c):
        gen = torch.Generator().manual_seed(self._seed(c, 5, 0) & 0x7FFFFFFF)
        return {"x": torch.randn(c.n, c.H, c.W, c.ci, generator=gen), "g": torch.randn((c.n,) + self.out_hw(c) + (c.co,), generator=gen),
                "w": torch.randn(c.co, c.ci, c.k, c.k, generator=gen) * 0.05}

    def worst_inputs(self, shape, pattern, signs):
        """the data gradient's g [n, OH, OW, co] and w [co, ci, k, k] on one worst-case mantissa; signs "alternating" flips g ONLY, along co
        (flipping both operands along co would cancel nothing)"""
        c = Case(*shape)
        g = synth.make_adversarial((c.n,) + self.out_hw(c) + (c.co,), pattern, signs, seed=self.worst_seed, relu=(pattern == 0x7FFFFF), k_axis=-1)
        w = synth.make_adversarial((c.co, c.ci, c.k, c.k), pattern, "same", seed=self.worst_seed + 1) * np.float32(2.0 ** -4)
        return g, w

    def reference(self, c, inp, relu_in):
        """fp64 on the CPU: dX (with relu_in: behind the mask of x, as the autograd of conv(relu(x)) gives it), dW, db, and for each the sum
        of the absolute values of its terms (dX_abs, dW_abs, db_abs).  Channels-last like the inputs."""
        def grads(x, g, w, mask_x):
            x = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
            w = w.double().clone().requires_grad_(True)
            b = torch.zeros(c.co, dtype=torch.float64, requires_grad=True)
            y = F.conv2d(torch.relu(x) if mask_x else x, w, b, stride=self.stride, padding=self.FORMS[c.k])
            y.backward(g.double().permute(0, 3, 1, 2))
            return x.grad.permute(0, 2, 3, 1).contiguous(), w.grad, b.grad

        dx, dw, db = grads(inp["x"], inp["g"], inp["w"], relu_in)
        xin = torch.relu(inp["x"]) if relu_in else inp["x"]
        # absolute values: no mask inside (|in(x)| is the operand), the mask of x applied to dX_abs afterwards
        dxa, dwa, dba = grads(xin.abs(), inp["g"].abs(), inp["w"].abs(), False)
        if relu_in:
            dxa = dxa * (inp["x"] > 0).double()
        return {"dX": dx, "dW": dw, "db": db, "dX_abs": dxa, "dW_abs": dwa, "db_abs": dba}

    def cached(self, c, kind, relu_in):
        """(inputs, reference) of a case with kind = "int" | "normal": computed once"""
        key = (c, kind, bool(relu_in))
        if key not in self._ref:
            ikey = (c, kind, "inputs")
            if ikey not in self._ref:
                self._ref[ikey] = self.int_inputs(c) if kind == "int" else self.normal_inputs(c)
            self._ref[key] = (self._ref[ikey], self.reference(c, self._ref[ikey], relu_in))
        return self._ref[key]

    def check_caps(self, c, inp, ref):
        """the integer tests' condition on the data: every output's sum of |terms|, plus the largest accumulate base, below 2^23"""
        for name, base in (("dX", "dx0"), ("dW", "dw0"), ("db", "db0")):
            cap = float(ref[name + "_abs"].max()) + float(inp[base].abs().max())
            assert cap < LIMIT, "%s %s: sum of |terms| %.0f is not below 2^23: these inputs do not make the result exact" % (self.case_id(c), name, cap)

    def lone_taps(self, c):
        """[k, k] bool: the only taps the smallest map feeds (a 1x1 map under a 3x3: the centre; a 2x2 map under stride 2, one output
        pixel: (pad, pad) .. (pad + 1, pad + 1)), or None for every other case"""
        if (c.H, c.W) != (self.stride, self.stride) or c.k == 1:
            return None
        pad = self.FORMS[c.k]
        inner = torch.zeros(c.k, c.k, dtype=torch.bool)
        inner[pad:pad + self.stride, pad:pad + self.stride] = True
        return inner


# (n, H, W, Ci, Co) per kernel size: odd sizes, maps that are no multiple of the 32-position K-tile, 1 .. 13 channel tiles, more than one
# image per chunk; 1x1x1 and 2x2 maps for the 3x3 (all halo / every tap partly outside).  CHUNKED: per kernel size, one more case whose n
# comes from the plan: >= 3 chunks, the last one shorter (n = None until chunked_n fills it in)
S1 = Form(
    1, (1, 3), 0x3B0, "k%d_n%s_%dx%d_%dto%d",
    shapes={
        1: [(1, 7, 7, 64, 64), (3, 14, 14, 256, 64), (5, 14, 14, 64, 256), (2, 7, 7, 512, 128), (2, 7, 7, 256, 1024), (1, 5, 3, 128, 128)],
        3: [(1, 7, 7, 64, 64), (3, 14, 14, 64, 64), (2, 7, 7, 128, 512), (2, 7, 7, 832, 256), (5, 7, 7, 256, 256), (2, 5, 3, 128, 128),
            (1, 1, 1, 64, 64), (1, 2, 2, 64, 64)],
    },
    chunked={1: (None, 7, 7, 64, 64), 3: (None, 7, 7, 64, 64)},
    worst=[(3, 2, 5, 3, 64, 64), (1, 2, 5, 3, 64, 128)], worst_seed=31,
    entries=("conv2d_backward_plan", "conv2d_backward_data", "conv2d_backward_weight", "conv2d_backward_data_plan_split",
             "conv2d_backward_plan_split"),
    # the 13 distinct shapes of the 22 stride-1 fusion convs: (H, Ci, Co, k)
    FUSION_SHAPES=[(14, 64, 64, 1), (14, 64, 64, 3), (14, 64, 256, 1), (14, 256, 64, 1), (7, 128, 128, 1), (7, 128, 128, 3), (7, 128, 512, 1),
                   (7, 512, 128, 1), (7, 128, 512, 3), (7, 832, 256, 3), (7, 256, 256, 1), (7, 256, 256, 3), (7, 256, 1024, 1)])

# (n, H, W, Ci, Co): the real shape; a half ci tile with two co tiles / a half ci tile; non-square with an OW that is no multiple of any
# tile; a 1x1 output (every tap partly outside)
S2 = Form(
    2, (7, 5), 0x3B2, "k%ds2_n%s_%dx%d_%dto%d",
    shapes={
        7: [(1, 28, 28, 320, 64), (3, 14, 14, 96, 128), (2, 6, 10, 64, 64), (1, 2, 2, 32, 64)],
        5: [(1, 14, 14, 1056, 128), (3, 14, 14, 96, 64), (2, 6, 4, 160, 64), (1, 2, 2, 32, 64)],
    },
    chunked={7: (None, 6, 10, 64, 64), 5: (None, 6, 4, 32, 64)},
    worst=[(7, 2, 6, 10, 64, 64), (5, 2, 6, 4, 96, 64)], worst_seed=21,
    entries=("conv2d_s2_backward_plan", "conv2d_s2_backward_data", "conv2d_s2_backward_weight", "conv2d_s2_backward_plan_split",
             "conv2d_s2_backward_weight_plan_split"),
    # the two real convs: (key, Ci, Co, k, H)
    REAL=[("motion_conv_trans_28", 320, 64, 7, 28), ("motion_conv_trans_14", 1056, 128, 5, 14)])
