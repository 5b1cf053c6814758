"""What the range tests share (tests/test_range_cases.py on the CPU, tests/test_gpu_scale_equivariance.py and
tests/test_gpu_train_ranges.py on the GPU): the wide draw, the exact power-of-two scaling, the table of degrees and the reach of a planted
non-finite value.  A helper module like tests/arena.py: no tests of its own, numpy and torch only.

Scale equivariance.  Every kernel of the library is built from +, x, fma, max(., 0) and the truncating cut into bf16 planes; its only
constants multiply (1 / nwin, 1 / (1 - p), the Winograd matrices) or are weights and biases.  Each of these commutes with a multiplication
by 2^a as long as no intermediate comes near 2^+-126: 2^a (u + v) = 2^a u + 2^a v with the SAME rounding (the rounding of a binary format
depends on the significand alone), 2^a max(u, 0) = max(2^a u, 0), and the cut masks significand bits.  So an output whose reference
formula has integer degree d in an operand class is multiplied by exactly 2^(a d) when that class is -- bit for bit, no tolerance."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from offk_amd import synth

SWEEP = (-24, 24)              # the scales that move every operand past fp16's range and the planes past 2^-30 (a = +1 shows neither)
SANITY = 1
BASE_LO, BASE_HI = 2.0 ** -90, 2.0 ** 90


# ---- the draw ----

def wide(shape, seed, relu=False, lo=-12, hi=4):
    """fp32 values (numpy) +-2^e (1 + mant / 2^23): 23 random mantissa bits, random signs, e uniform over the hi - lo octaves [2^lo, 2^hi),
    three in ten exact zeros; relu: the negatives are zeros too.  A function of (shape, seed, relu, lo, hi) alone."""
    n = int(np.prod(shape))
    bits = synth.raw_u64(0x51DE + 7919 * int(seed), 0, n)
    mant = (bits & np.uint64(0x7FFFFF)).astype(np.uint32)
    sign = ((bits >> np.uint64(23)) & np.uint64(1)).astype(np.uint32)
    e = ((bits >> np.uint64(24)) % np.uint64(hi - lo)).astype(np.int64) + lo
    zero = ((bits >> np.uint64(40)) % np.uint64(10)) < np.uint64(3)
    v = ((sign << np.uint32(31)) | ((e + 127).astype(np.uint32) << np.uint32(23)) | mant).view(np.float32).copy()
    v[zero] = 0.0
    if relu:
        v[v < 0] = 0.0
    return v.reshape(shape)


def wide_t(shape, seed, **kw):
    return torch.from_numpy(wide(shape, seed, **kw))


def scale(t, a):
    """t * 2^a, exactly (numpy or torch, any float type): asserts that the result times 2^-a is the input again, bit for bit"""
    if torch.is_tensor(t):
        out = t * (2.0 ** a)
        back = out * (2.0 ** -a)
        assert out.dtype == t.dtype and torch.equal(back, t) and bool(((back == 0) == (out == 0)).all()), "scaling by 2^%d is not exact here" % a
        return out
    t = np.asarray(t)
    with np.errstate(over="ignore", under="ignore"):
        out = np.ldexp(t, a)
        back = np.ldexp(out, -a)
    assert out.dtype == t.dtype and np.array_equal(back, t) and np.array_equal(back == 0, out == 0), "scaling by 2^%d is not exact here" % a
    return out


def base_in_range(t):
    """the condition on the base run: every non-zero |output| in [2^-90, 2^90], no non-finite value"""
    t = t.detach().double().cpu() if torch.is_tensor(t) else torch.from_numpy(np.asarray(t, dtype=np.float64))
    nz = t[t != 0].abs()
    return bool(torch.isfinite(t).all()) and (nz.numel() == 0 or (float(nz.min()) >= BASE_LO and float(nz.max()) <= BASE_HI))


def same_values(got, base, a_times_degree):
    """got == base * 2^(a degree) in value (0.0 == -0.0), no non-finite value on either side"""
    want = scale(base.detach().cpu(), a_times_degree)
    got = got.detach().cpu()
    return bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()) and torch.equal(got, want)


# ---- degrees ----
# entry -> output -> operand class -> integer degree, read off the reference formula (multilinear apart from sign masks, which a positive
# scale leaves alone).  Classes: "x" feature maps / layer input, "w" weights, "b" biases, "g" the incoming gradient, "old" what an
# accumulating call adds to.  A class that is missing does not enter the output (degree 0 and not an operand of that entry's formula).
# The forward entries are affine in (x, b): they have a degree only when x and the bias are scaled TOGETHER, written "x+b".
degrees = {
    # y = conv(in(x), w) + b (+ res) (then max(., 0)): res is scaled with x and b
    "conv2d_nhwc": {"y": {"x+b": 1, "w+b": 1}},
    "relu_backward": {"out": {"g": 1, "x": 0, "old": 1}},                                  # x: the mask operand y
    "conv2d_backward_data": {"dX": {"g": 1, "w": 1, "x": 0, "old": 1}},
    "conv2d_backward_weight": {"dW": {"x": 1, "g": 1, "w": 0, "old": 1}, "db": {"x": 0, "g": 1, "w": 0, "old": 1}},
    "conv2d_s2_backward_data": {"dX": {"g": 1, "w": 1, "x": 0, "old": 1}},
    "conv2d_s2_backward_weight": {"dW": {"x": 1, "g": 1, "w": 0, "old": 1}, "db": {"x": 0, "g": 1, "w": 0, "old": 1}},
    # out = (pool(x) keep / (1 - p)) w^T + b
    "head_train": {"out": {"x+b": 1, "w+b": 1}, "z": {"x+b": 1, "w+b": 0}},
    # dX = route(g w keep / (1 - p)) (the route: the max-pool's argmax, unchanged by a positive scale of x), dW = g^T z, db = sum g
    "head_backward": {"dX": {"g": 1, "w": 1, "x": 0, "old": 1}, "dW": {"g": 1, "x": 1, "w": 0, "old": 1}, "db": {"g": 1, "x": 0, "w": 0, "old": 1}},
    # unit = [G ; sobel(D) ; tdiff(D)] with G = max(Wg x + bg, 0), D = Wd x + bd; training: times keep / (1 - p)
    "off_units": {"unit": {"x+b": 1}, "G": {"x+b": 1}, "D": {"x+b": 1}},
    "off_units_train": {"unit": {"x+b": 1}, "G": {"x+b": 1}, "D": {"x+b": 1}},
    # dWg, dWd = (gradient behind the mask)^T x, dbg, dbd = its sum; dX = W^T (gradient behind the mask)
    "off_units_backward": {"dW": {"x+b": 1, "g": 1, "old": 1}, "db": {"x+b": 0, "g": 1, "old": 1}},
    "off_units_backward_feats": {"dX": {"x+b": 0, "g": 1, "old": 1}},
    # the inference forward: every layer is affine in (its input, its bias), so the whole net has degree 1 in (maps, all biases) and
    # degree 1 in (first-layer weights, all biases)
    "forward": {"logits": {"x+b": 1, "w1+b": 1}, "regions": {"x+b": 1, "w1+b": 1}},
}


# ---- fp64 references of the fusion convs (torch on the CPU; Inf and NaN spread by IEEE rules) ----

def conv_ref64(x, w, b, g, stride, pad, relu_in=False, relu=False, res=None):
    """x [n, H, W, Ci], w [Co, Ci, k, k], b [Co], g [n, OH, OW, Co] (channels-last, any float type) -> dict y, dX, dW, db in fp64,
    channels-last: y = conv(in(x), w) + b (+ res) (max(., 0) with relu), the gradients those of sum(y * g) WITHOUT the output's ReLU mask
    (the backward entries take g behind it)"""
    xd = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    wd = w.double().clone().requires_grad_(True)
    bd = b.double().clone().requires_grad_(True)
    lin = F.conv2d(torch.relu(xd) if relu_in else xd, wd, bd, stride=stride, padding=pad)
    lin.backward(g.double().permute(0, 3, 1, 2))
    y = lin.detach()
    if res is not None:
        y = y + res.double().permute(0, 3, 1, 2)
    if relu:
        y = torch.relu(y)
    return {"y": y.permute(0, 2, 3, 1).contiguous(), "dX": xd.grad.permute(0, 2, 3, 1).contiguous(), "dW": wd.grad, "db": bd.grad}


Plant = collections.namedtuple("Plant", "inputs operand index value")      # inputs: dict x, w, b, g (+ what the entry's ref needs)

CONV_ENTRIES = {"conv2d_backward_data": ("dX",), "conv2d_backward_weight": ("dW", "db"), "conv2d_s2_backward_data": ("dX",),
                "conv2d_s2_backward_weight": ("dW", "db"), "conv2d_nhwc": ("y",)}


def _entry_ref(entry, inp):
    if entry == "relu_backward":
        g, y = inp["g"].double(), inp["x"].double()
        return {"out": g * (y > 0)}
    if entry in CONV_ENTRIES:
        r = conv_ref64(inp["x"], inp["w"], inp["b"], inp["g"], inp["stride"], inp["pad"], relu_in=inp.get("relu_in", False))
        return dict((k, r[k]) for k in CONV_ENTRIES[entry])
    raise KeyError(entry)


def planted(plant):
    inp = dict(plant.inputs)
    t = inp[plant.operand].clone()
    t[plant.index] = plant.value
    inp[plant.operand] = t
    return inp


def _positive(shape, seed):
    return torch.from_numpy(1.0 + np.abs(wide(tuple(shape), seed, lo=-1, hi=0))).double()


def reach(entry, plant, ieee=False):
    """dict output -> bool mask: the output elements that depend, by the operation's definition, on the value at one index of one operand:
    ref(planted) != ref(clean) on the fp64 torch CPU reference.

    ieee=True plants plant.value itself into plant.inputs and lets Inf and NaN spread by IEEE rules (NaN != anything).  For the
    convolutions that is MORE than the definition: torch's CPU kernels materialise the zero padding, so an Inf in g comes out as 0 * Inf
    = NaN in every tap whose x lies outside the map -- terms the sum of include/offk.h does not have.  The default therefore asks the
    same reference for the dependence itself: every operand is replaced by values in [1, 2.5) (no zero, no cancellation, no mask: every
    term of every sum is positive), the planted element is tripled, and an output changes exactly where the element enters its sum.
    An element that enters a sum reaches it whatever the other factor is (0 * Inf = NaN on the device as in IEEE), so this is the set a
    planted non-finite value must come out of."""
    if ieee:
        clean = _entry_ref(entry, plant.inputs)
        dirty = _entry_ref(entry, planted(plant))
    else:
        sur = dict((k, _positive(v.shape, 900 + i) if torch.is_tensor(v) else v) for i, (k, v) in enumerate(sorted(plant.inputs.items())))
        clean = _entry_ref(entry, sur)
        dirty = _entry_ref(entry, planted(Plant(sur, plant.operand, plant.index, 3.0 * float(sur[plant.operand][plant.index]))))
    return dict((k, dirty[k] != clean[k]) for k in clean)
