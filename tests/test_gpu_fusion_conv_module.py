"""FusionConv2d (off_module.py): trainable fusion convs on liboffk, checked as stacks against the same stack of nn.Conv2d in fp64 on the CPU.

Two stacks at n = 2, 14 x 14, loss = (y * r).sum():
  * chain 28b (RGB_OFF.py:670-676): 256 -> 64 1x1 + ReLU, 64 -> 64 3x3 + ReLU, 64 -> 256 1x1 + residual + ReLU -- six parameter gradients
    and the input gradient (two paths join at x: conv1 and the residual);
  * a 28a-style head (RGB_OFF.py:657-667): a relu_in conv 64 -> 64 1x1 + ReLU and the branch conv 64 -> 256 1x1, both from the same pre-ReLU
    input -- four parameter gradients and the input gradient.

The bound is derived per layer and carried through the stack in fp64 on absolute values (class Bounds below): a layer computes
fl(sum of n exact products of its computed inputs), so its error is at most (the inputs' error bounds pushed through |W| or |a|) +
gamma_{n+1} * sum |computed terms|; a ReLU passes an error bound on unchanged (it is 1-Lipschitz), and its backward mask is the reference's
wherever the pre-activation lies farther from zero than its own bound -- elsewhere the device may take the other branch and the bound of
that element's masked gradient is |g| + its bound; a join adds its two bounds and one rounding.  Nothing in it comes from the code under
test.  Such a worst-case bound (every rounding aligned) grows by about sqrt(n) per layer against the typical error; carried through a
three-layer FORWARD of normal data it leaves a percent of the ReLU masks undecided and is then larger than the gradients themselves
(measured on the CPU: chain 28b, bound of c1.weight 400 against values of 57).  So the stacks are checked three ways, each with a bound
that means something:
  1. normal data everywhere, link by link: every layer's output and gradients against fp64 of THAT layer from the device's own inputs, within
     the one-layer bound, and bit-equal to what the layer produced inside the stack -- every link of the chain held to gamma_{n+1};
  2. end to end against the fp64 stack with an integer forward (exact in fp32, asserted by its caps, so every mask is the reference's) and
     a normal-distributed r: the gradients are real-valued and their bounds compose through the backward only;
  3. integers everywhere: torch.equal to the fp64 stack, after the caps (every sum of |terms| below 2^24) are asserted.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

import offk_amd  # noqa: F401

from .conv_bwd import S1 as cb
from . import exact

pytestmark = pytest.mark.gpu
N, HW = 2, 14


@pytest.fixture(scope="module")
def FusionConv2d():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd.off_module import FusionConv2d
    return FusionConv2d


# ---- the two stacks: the same code drives FusionConv2d on the device and nn.Conv2d in fp64 on the CPU -----------------------------
SPECS = {
    "chain28b": [("c1", 256, 64, 1, dict(relu=True)), ("c2", 64, 64, 3, dict(relu=True)), ("c3", 64, 256, 1, dict(relu=True))],
    "head28a": [("c1", 64, 64, 1, dict(relu=True, relu_in=True)), ("br", 64, 256, 1, dict())],
}
CIN = {"chain28b": 256, "head28a": 64}


class Stack(nn.Module):
    def __init__(self, kind, make):
        super().__init__()
        self.kind = kind
        self.flags = {}
        self.trace = None          # a dict: every FusionConv2d call leaves (x, res, y) there, y keeping its gradient
        for name, ci, co, k, fl in SPECS[kind]:
            self.add_module(name, make(ci, co, k, fl))
            self.flags[name] = fl

    def layer(self, name, x, res=None):
        m, fl = getattr(self, name), self.flags[name]
        if type(m) is nn.Conv2d:                      # the reference: post(conv(in(x)) + b + res)
            z = m(torch.relu(x) if fl.get("relu_in") else x)
            z = z if res is None else z + res
            return torch.relu(z) if fl.get("relu") else z
        y = m(x, res)
        if self.trace is not None:
            y.retain_grad()
            self.trace[name] = (x, res, y)
        return y

    def forward(self, x):
        if self.kind == "chain28b":
            return (self.layer("c3", self.layer("c2", self.layer("c1", x)), res=x),)
        return self.layer("c1", x), self.layer("br", x)


def make_pair(FusionConv2d, kind, params):
    """(device stack of FusionConv2d, fp64 CPU stack of nn.Conv2d) holding the same parameter values, loaded through state_dict"""
    dev = Stack(kind, lambda ci, co, k, fl: FusionConv2d(ci, co, k, padding=(k - 1) // 2, **fl))
    ref = Stack(kind, lambda ci, co, k, fl: nn.Conv2d(ci, co, k, padding=(k - 1) // 2))
    dev.load_state_dict(params)
    ref.load_state_dict(params)            # the keys are nn.Conv2d's
    return dev.cuda(), ref.double()


def params_for(kind, integer):
    gen = torch.Generator().manual_seed(0x28B if kind == "chain28b" else 0x28A)
    out = {}
    for i, (name, ci, co, k, _) in enumerate(SPECS[kind]):
        if integer:
            out[name + ".weight"] = exact.sparse_signs(exact.stream(0x5C, 1, i), (co, ci, k, k))
            out[name + ".bias"] = exact.ints(exact.stream(0x5C, 2, i), (co,), -2, 2)
        else:
            out[name + ".weight"] = torch.randn(co, ci, k, k, generator=gen) / (ci * k * k) ** 0.5
            out[name + ".bias"] = torch.randn(co, generator=gen) * 0.1
    return out


def data_for(kind, integer, integer_r=None):
    """x and the loss weights r; integer_r=False with integer=True: the integer forward with a normal-distributed r"""
    shape = (N, CIN[kind], HW, HW)
    outs = [(N, 256, HW, HW)] if kind == "chain28b" else [(N, 64, HW, HW), (N, 256, HW, HW)]
    gen = torch.Generator().manual_seed(0x5E)
    x = exact.ints(exact.stream(0x5D, 1, 0), shape, -3, 3) if integer else torch.randn(shape, generator=gen)
    if integer if integer_r is None else integer_r:
        rs = [exact.ints(exact.stream(0x5D, 2, i), s, -2, 2) for i, s in enumerate(outs)]
    else:
        rs = [torch.randn(s, generator=gen) for s in outs]
    return x, rs


def run_stack(stack, x, rs):
    """one forward / backward round: (outputs, {name: gradient}) with the input gradient under "x" """
    x = x.clone().requires_grad_(True)
    for p in stack.parameters():
        p.grad = None
    ys = stack(x)
    sum((y * r).sum() for y, r in zip(ys, rs)).backward()
    grads = {"x": x.grad}
    grads.update((k, p.grad) for k, p in stack.named_parameters())
    return [y.detach() for y in ys], grads


def on_device(x, rs):
    cl = torch.channels_last
    return x.cuda().contiguous(memory_format=cl), [r.cuda().contiguous(memory_format=cl) for r in rs]


# ---- the composed bound -----------------------------------------------------------------------------------------------------------
class Bounds:
    """Values (fp64) and elementwise error bounds of one stack, layer by layer.  `caps` collects the largest sum of |terms| of every
    output (the integer run's exactness condition); `unstable` / `masked` count the ReLU pre-activations within their own bound of zero."""

    def __init__(self, ref, exact_forward=False):
        self.ref, self.rec, self.caps, self.err, self.unstable, self.masked = ref, {}, {}, {}, 0, 0
        self.exact_forward = exact_forward     # integer operands: the forward is exact once its caps are below 2^24 (asserted here)

    def forward(self, name, x, Ex, res=None, Eres=None):
        m, fl = getattr(self.ref, name), self.ref.flags[name]
        W, b, pad = m.weight.detach(), m.bias.detach(), m.padding[0]
        a = torch.relu(x) if fl.get("relu_in") else x
        Ea = Ex                                                                   # ReLU is 1-Lipschitz
        if fl.get("relu_in"):
            assert not bool((Ex > 0).any()), "a relu_in layer of these stacks reads the exact stack input: its mask is the reference's"
        K = W[0].numel()
        z = F.conv2d(a, W, b, padding=pad) + (0 if res is None else res)
        S = F.conv2d(a.abs() + Ea, W.abs(), b.abs(), padding=pad) + (0 if res is None else res.abs() + Eres)
        Ez = F.conv2d(Ea, W.abs(), None, padding=pad) + (0 if res is None else Eres) + cb.gamma(K + 2) * S
        self.caps[name + ".z"] = float(S.max())
        if self.exact_forward:
            assert bool((a == a.round()).all()) and bool((W == W.round()).all()) and bool((b == b.round()).all()), "integer operands"
            assert float(S.max()) < exact.LIMIT, "%s: sum of |terms| %.0f is not below 2^24" % (name, float(S.max()))
            Ez = torch.zeros_like(z)
        # (Ez == 0: the device holds z itself and takes the reference's branch, at z == 0 too)
        unstable = ((z.abs() <= Ez) & (Ez > 0)) if fl.get("relu") else torch.zeros_like(z, dtype=torch.bool)
        if fl.get("relu"):
            self.unstable, self.masked = self.unstable + int(unstable.sum()), self.masked + z.numel()
        self.rec[name] = dict(x=x, a=a, Ea=Ea, z=z, W=W, pad=pad, fl=fl, unstable=unstable)
        return (torch.relu(z) if fl.get("relu") else z), Ez

    def backward(self, name, gy, Egy):
        """-> (dx, Edx, gz, Egz); the parameter gradients' values and bounds go to self.err[name + ".weight" / ".bias"]"""
        r = self.rec[name]
        a, Ea, W, pad, fl = r["a"], r["Ea"], r["W"], r["pad"], r["fl"]
        mask = (r["z"] > 0).double() if fl.get("relu") else 1.0
        gz, Egz = gy * mask, torch.where(r["unstable"], gy.abs() + Egy, Egy * mask)
        P = gz.shape[0] * gz.shape[2] * gz.shape[3]

        def cw(g, v):
            return conv2d_weight(v, W.shape, g, padding=pad)

        def ct(g):
            return F.conv_transpose2d(g, W.abs(), padding=pad)
        Sw = cw(gz.abs() + Egz, a.abs() + Ea)
        self.err[name + ".weight"] = (cw(gz, a), cw(Egz, a.abs() + Ea) + cw(gz.abs(), Ea) + cb.gamma(P + 1) * Sw)
        Sb = (gz.abs() + Egz).sum((0, 2, 3))
        self.err[name + ".bias"] = (gz.sum((0, 2, 3)), Egz.sum((0, 2, 3)) + cb.gamma(P + 1) * Sb)
        Sx = ct(gz.abs() + Egz)
        da, Eda = F.conv_transpose2d(gz, W, padding=pad), ct(Egz) + cb.gamma(W.shape[0] * W.shape[2] * W.shape[3] + 1) * Sx
        self.caps.update({name + ".dW": float(Sw.max()), name + ".db": float(Sb.max()), name + ".dx": float(Sx.max())})
        if fl.get("relu_in"):
            mx = (r["x"] > 0).double()
            da, Eda = da * mx, Eda * mx
        return da, Eda, gz, Egz

    def join(self, name, a, Ea, b, Eb):
        """autograd's fp32 sum of two gradients"""
        self.caps[name] = float((a.abs() + b.abs()).max())
        return a + b, Ea + Eb + cb.U * (a.abs() + b.abs() + Ea + Eb)


def bounds_of(ref, x, rs, exact_forward=False):
    """the Bounds object of a whole stack: B.err = {gradient name: (fp64 value, elementwise bound)}"""
    B = Bounds(ref, exact_forward)
    x = x.double()
    zero = torch.zeros_like(x)
    if ref.kind == "chain28b":
        t1, E1 = B.forward("c1", x, zero)
        t2, E2 = B.forward("c2", t1, E1)
        _y, _Ey = B.forward("c3", t2, E2, res=x, Eres=zero)
        g = rs[0].double()
        d2, Ed2, gres, Egres = B.backward("c3", g, torch.zeros_like(g))
        d1, Ed1, _, _ = B.backward("c2", d2, Ed2)
        dx, Edx, _, _ = B.backward("c1", d1, Ed1)
        B.err["x"] = B.join("x", dx, Edx, gres, Egres)
    else:
        B.forward("c1", x, zero)
        B.forward("br", x, zero)
        dxa, Ea, _, _ = B.backward("c1", rs[0].double(), torch.zeros_like(rs[0].double()))
        dxb, Eb, _, _ = B.backward("br", rs[1].double(), torch.zeros_like(rs[1].double()))
        B.err["x"] = B.join("x", dxa, Ea, dxb, Eb)
    return B


def within(got, val, bound, what):
    err = (got.detach().cpu().double() - val).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((err > 0).any()) else 0.0
    print("%s: largest error %.3e, largest error / bound %.3f" % (what, float(err.max()), ratio))
    assert bool((err <= bound).all()), "%s: error is %.3f of the derived bound" % (what, ratio)


@pytest.mark.parametrize("kind", ["chain28b", "head28a"])
def test_every_link_within_its_one_layer_bound(FusionConv2d, kind):
    """1. of the module docstring: normal data; each layer against fp64 of that layer from the device's own inputs"""
    dev, ref = make_pair(FusionConv2d, kind, params_for(kind, False))
    x, rs = data_for(kind, False)
    xd, rd = on_device(x, rs)
    dev.trace = {}
    ys, g = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    assert len(g) == (7 if kind == "chain28b" else 5) and all(v is not None for v in g.values())
    for y in ys:
        assert y.is_contiguous(memory_format=torch.channels_last)
    to_input = {}            # what each layer sends to the stack input
    for name, (xi, res, y) in dev.trace.items():
        m = getattr(dev, name)
        gy = y.grad
        xs = xi.detach().clone().requires_grad_(True)
        rr = None if res is None else res.detach().clone().requires_grad_(True)
        m.weight.grad = m.bias.grad = None
        y2 = m(xs, rr)
        y2.backward(gy)
        torch.cuda.synchronize()
        # the layer alone is the layer inside the stack, bit for bit
        assert torch.equal(y2.detach(), y.detach()), name
        assert torch.equal(m.weight.grad, g[name + ".weight"]) and torch.equal(m.bias.grad, g[name + ".bias"]), name
        to_input[name] = (xs.grad, None if rr is None else rr.grad)
        # fp64 of this one layer from the device's own inputs (exact operands: no incoming error)
        B = Bounds(ref)
        x64 = xs.detach().cpu().double()
        r64 = None if rr is None else rr.detach().cpu().double()
        yr, Ez = B.forward(name, x64, torch.zeros_like(x64), r64, None if r64 is None else torch.zeros_like(r64))
        within(y2, yr, Ez, "%s %s y" % (kind, name))
        g64 = gy.cpu().double()
        dx, Edx, gz, Egz = B.backward(name, g64, torch.zeros_like(g64))
        assert B.unstable <= 0.005 * max(B.masked, 1), "more than 0.5 %% of the masks undecided within a one-layer bound: %d of %d" % (B.unstable, B.masked)
        within(xs.grad, dx, Edx, "%s %s dx" % (kind, name))
        if rr is not None:
            within(rr.grad, gz, Egz, "%s %s dres" % (kind, name))
        for pn in (".weight", ".bias"):
            within(getattr(m, pn[1:]).grad, B.err[name + pn][0], B.err[name + pn][1], "%s %s%s" % (kind, name, pn))
    # the join at the stack input is autograd's fp32 sum of the two links that reach it
    parts = (to_input["c1"][0], to_input["c3"][1]) if kind == "chain28b" else (to_input["c1"][0], to_input["br"][0])
    assert torch.equal(g["x"], parts[0] + parts[1])


@pytest.mark.parametrize("kind", ["chain28b", "head28a"])
def test_stack_gradients_within_the_composed_bound(FusionConv2d, kind):
    """2. of the module docstring: integer forward (exact, so every mask is the reference's), normal-distributed r"""
    dev, ref = make_pair(FusionConv2d, kind, params_for(kind, True))
    x, rs = data_for(kind, True, integer_r=False)
    ys_ref, g_ref = run_stack(ref, x.double(), [r.double() for r in rs])
    B = bounds_of(ref, x, rs, exact_forward=True)
    assert B.unstable == 0
    for name, (val, _bound) in B.err.items():            # the hand-written backward of Bounds is autograd's
        assert torch.allclose(val, g_ref[name], rtol=1e-10, atol=1e-9), name
    xd, rd = on_device(x, rs)
    ys, g = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    for y, yr in zip(ys, ys_ref):
        assert torch.equal(y.cpu().double(), yr), "the integer forward is exact"
    for name in sorted(g):
        assert g[name] is not None, name
        within(g[name], g_ref[name], B.err[name][1], "%s %s" % (kind, name))
        assert float(B.err[name][1].max()) < 0.05 * float(g_ref[name].abs().max()), "%s: a bound that says nothing" % name


@pytest.mark.parametrize("kind", ["chain28b", "head28a"])
def test_stack_on_integers_equals_fp64(FusionConv2d, kind):
    dev, ref = make_pair(FusionConv2d, kind, params_for(kind, True))
    x, rs = data_for(kind, True)
    B = bounds_of(ref, x, rs)
    for name, cap in B.caps.items():
        assert cap < exact.LIMIT, "%s %s: sum of |terms| %.0f is not below 2^24" % (kind, name, cap)
    ys_ref, g_ref = run_stack(ref, x.double(), [r.double() for r in rs])
    xd, rd = on_device(x, rs)
    ys, g = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    for i, (y, yr) in enumerate(zip(ys, ys_ref)):
        mm.check(y.cpu(), yr, "%s output %d" % (kind, i))
    for name in sorted(g):
        mm.check(g[name].cpu(), g_ref[name], "%s grad %s" % (kind, name))
    mm.raise_if_any()
    for name in g:
        assert torch.equal(g[name].cpu().double(), g_ref[name]), name


def test_frozen_layer_launches_no_weight_gradient(FusionConv2d):
    dev, _ = make_pair(FusionConv2d, "chain28b", params_for("chain28b", False))
    x, rs = data_for("chain28b", False)
    xd, rd = on_device(x, rs)
    before = FusionConv2d.weight_grad_launches
    _, g_all = run_stack(dev, xd, rd)
    assert FusionConv2d.weight_grad_launches - before == 3
    for p in dev.c2.parameters():
        p.requires_grad_(False)
    before = FusionConv2d.weight_grad_launches
    _, g = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    assert FusionConv2d.weight_grad_launches - before == 2, "the frozen conv ran its weight gradient"
    assert g["c2.weight"] is None and g["c2.bias"] is None
    for name in ("x", "c1.weight", "c1.bias", "c3.weight", "c3.bias"):
        assert torch.equal(g[name], g_all[name]), name          # the gradient still flows THROUGH the frozen conv, bit for bit


def test_optimizer_step_is_seen_without_a_rebind(FusionConv2d):
    dev, _ = make_pair(FusionConv2d, "chain28b", params_for("chain28b", False))
    x, rs = data_for("chain28b", False)
    xd, rd = on_device(x, rs)
    opt = torch.optim.SGD(dev.parameters(), lr=0.05)
    y1, _ = run_stack(dev, xd, rd)
    opt.step()
    y2, g2 = run_stack(dev, xd, rd)
    fresh = Stack("chain28b", lambda ci, co, k, fl: FusionConv2d(ci, co, k, padding=(k - 1) // 2, **fl))
    fresh.load_state_dict(dev.state_dict())
    y3, g3 = run_stack(fresh.cuda(), xd, rd)
    torch.cuda.synchronize()
    assert not torch.equal(y1[0], y2[0]), "the step changed nothing"
    assert torch.equal(y2[0], y3[0])
    for name in g2:
        assert torch.equal(g2[name], g3[name]), name
