"""FusionConv2d at stride 2 (off_module.py): the two stage openers as trainable modules on liboffk, checked as stacks against the same
stack of nn.Conv2d in fp64 on the CPU.  loss = (y * r).sum().

  * open28 (RGB_OFF.py:657-659): 320 -> 64 7x7 / 2 / 3, then the relu_in conv 64 -> 64 1x1 + ReLU that reads it, n = 2 at 28 x 28;
  * open14 (RGB_OFF.py:762): 96 -> 128 5x5 / 2 / 2 + ReLU (a half ci tile), n = 2 at 14 x 14.

Integers everywhere: output, input gradient and every parameter gradient are torch.equal to the fp64 stack, after the caps (every sum
of |terms| below 2^24) are asserted from the reference.  Normal data, link by link as in tests/test_gpu_fusion_conv_module.py: every
layer's output and gradients against fp64 of THAT layer from the device's own inputs, within the one-layer bound

    |got - ref64| <= (what an undecided ReLU mask can move) + gamma_{m+1} * sum |terms|

with m = Ci k^2 + 1 (forward, the bias included), n OH OW (dW, db), Co ceil(k / stride)^2 (dX).  A ReLU's backward mask is the
reference's wherever the pre-activation lies farther from zero than its own bound; elsewhere the device may take the other branch and
that element's gradient may be off by |gy|.  Nothing in the bound comes from the code under test.
"""
import pytest
import torch
import torch.nn as nn

import offk_amd  # noqa: F401

from . import exact
from .conv_grad_checks import one_layer, within

pytestmark = pytest.mark.gpu
N = 2
# kind -> (map size, [(name, ci, co, k, stride, flags)])
SPECS = {
    "open28": (28, [("t", 320, 64, 7, 2, dict()), ("c1", 64, 64, 1, 1, dict(relu_in=True, relu=True))]),
    "open14": (14, [("t", 96, 128, 5, 2, dict(relu=True))]),
}
KINDS = sorted(SPECS)


@pytest.fixture(scope="module")
def FusionConv2d():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd.off_module import FusionConv2d
    return FusionConv2d


class Stack(nn.Module):
    """the layers in sequence; the same code drives FusionConv2d on the device and nn.Conv2d in fp64 on the CPU"""

    def __init__(self, kind, make):
        super().__init__()
        self.kind, self.flags, self.trace = kind, {}, None
        for name, ci, co, k, stride, fl in SPECS[kind][1]:
            self.add_module(name, make(ci, co, k, stride, fl))
            self.flags[name] = fl

    def forward(self, x):
        for name, fl in self.flags.items():
            m = getattr(self, name)
            if type(m) is nn.Conv2d:                      # the reference: post(conv(in(x)) + b)
                z = m(torch.relu(x) if fl.get("relu_in") else x)
                y = torch.relu(z) if fl.get("relu") else z
            else:
                y = m(x)
            if self.trace is not None:
                y.retain_grad()
                self.trace[name] = (x, y)
            x = y
        return x


def make_pair(FusionConv2d, kind, params):
    dev = Stack(kind, lambda ci, co, k, s, fl: FusionConv2d(ci, co, k, stride=s, padding=(k - 1) // 2, **fl))
    ref = Stack(kind, lambda ci, co, k, s, fl: nn.Conv2d(ci, co, k, stride=s, padding=(k - 1) // 2))
    dev.load_state_dict(params)
    ref.load_state_dict(params)            # the keys are nn.Conv2d's
    return dev.cuda(), ref.double()


def params_for(kind, integer):
    gen = torch.Generator().manual_seed(0x52A + len(kind))
    out = {}
    for i, (name, ci, co, k, _s, _fl) in enumerate(SPECS[kind][1]):
        if integer:
            out[name + ".weight"] = exact.sparse_signs(exact.stream(0x5F, 1, i), (co, ci, k, k))
            out[name + ".bias"] = exact.ints(exact.stream(0x5F, 2, i), (co,), -2, 2)
        else:
            out[name + ".weight"] = torch.randn(co, ci, k, k, generator=gen) / (ci * k * k) ** 0.5
            out[name + ".bias"] = torch.randn(co, generator=gen) * 0.1
    return out


def data_for(kind, integer):
    HW, layers = SPECS[kind]
    out_hw = HW
    for l in layers:
        out_hw //= l[4]
    shape, oshape = (N, layers[0][1], HW, HW), (N, layers[-1][2], out_hw, out_hw)
    gen = torch.Generator().manual_seed(0x5E2)
    if integer:
        return exact.ints(exact.stream(0x60, 1, 0), shape, -3, 3), exact.ints(exact.stream(0x60, 2, 0), oshape, -2, 2)
    return torch.randn(shape, generator=gen), torch.randn(oshape, generator=gen)


def run_stack(stack, x, r):
    """one forward / backward round: (output, {name: gradient}) with the input gradient under "x" """
    x = x.clone().requires_grad_(True)
    for p in stack.parameters():
        p.grad = None
    y = stack(x)
    (y * r).sum().backward()
    grads = {"x": x.grad}
    grads.update((k, p.grad) for k, p in stack.named_parameters())
    return y.detach(), grads


def on_device(*ts):
    return [t.cuda().contiguous(memory_format=torch.channels_last) for t in ts]


@pytest.mark.parametrize("kind", KINDS)
def test_every_link_within_its_one_layer_bound(FusionConv2d, kind):
    dev, ref = make_pair(FusionConv2d, kind, params_for(kind, False))
    x, r = data_for(kind, False)
    xd, rd = on_device(x, r)
    dev.trace = {}
    y, g = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    assert all(v is not None for v in g.values())
    assert y.is_contiguous(memory_format=torch.channels_last)
    names = list(dev.trace)
    for i, name in enumerate(names):
        xi, yi = dev.trace[name]
        m = getattr(dev, name)
        dxi = g["x"] if i == 0 else dev.trace[names[i - 1]][1].grad      # the gradient this layer sent to its input
        out, _caps, (unstable, masked) = one_layer(getattr(ref, name), dev.flags[name], xi.detach().cpu().double(), yi.grad.cpu().double())
        assert unstable <= 0.005 * max(masked, 1), "more than 0.5 %% of the masks undecided within a one-layer bound: %d of %d" % (unstable, masked)
        within(yi, out["y"][0], out["y"][1], "%s %s y" % (kind, name))
        within(dxi, out["dx"][0], out["dx"][1], "%s %s dx" % (kind, name))
        within(m.weight.grad, out["weight"][0], out["weight"][1], "%s %s.weight" % (kind, name))
        within(m.bias.grad, out["bias"][0], out["bias"][1], "%s %s.bias" % (kind, name))
    # and the same bits on a second round
    y2, g2 = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    assert torch.equal(y, y2) and all(torch.equal(g[k], g2[k]) for k in g)


@pytest.mark.parametrize("kind", KINDS)
def test_stack_on_integers_equals_fp64(FusionConv2d, kind):
    dev, ref = make_pair(FusionConv2d, kind, params_for(kind, True))
    x, r = data_for(kind, True)
    ref.trace = {}
    y_ref, g_ref = run_stack(ref, x.double(), r.double())
    for name, (xi, yi) in ref.trace.items():
        _out, caps, _ = one_layer(getattr(ref, name), ref.flags[name], xi.detach(), yi.grad)
        for what, cap in caps.items():
            assert cap < exact.LIMIT, "%s %s %s: sum of |terms| %.0f is not below 2^24" % (kind, name, what, cap)
    xd, rd = on_device(x, r)
    y, g = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    mm.check(y.cpu(), y_ref, "%s output" % kind)
    for name in sorted(g):
        assert g[name] is not None, name
        mm.check(g[name].cpu(), g_ref[name], "%s grad %s" % (kind, name))
    mm.raise_if_any()
    for name in g:
        assert torch.equal(g[name].cpu().double(), g_ref[name]), name


def test_frozen_stride2_layer_launches_no_weight_gradient(FusionConv2d):
    dev, _ = make_pair(FusionConv2d, "open28", params_for("open28", False))
    x, r = data_for("open28", False)
    xd, rd = on_device(x, r)
    before = FusionConv2d.weight_grad_launches
    _, g_all = run_stack(dev, xd, rd)
    assert FusionConv2d.weight_grad_launches - before == 2
    for p in dev.t.parameters():
        p.requires_grad_(False)
    before = FusionConv2d.weight_grad_launches
    _, g = run_stack(dev, xd, rd)
    torch.cuda.synchronize()
    assert FusionConv2d.weight_grad_launches - before == 1, "the frozen stride-2 conv ran its weight gradient"
    assert g["t.weight"] is None and g["t.bias"] is None
    for name in ("x", "c1.weight", "c1.bias"):
        assert torch.equal(g[name], g_all[name]), name          # the gradient still flows THROUGH the frozen conv, bit for bit


@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_step_is_seen_without_a_rebind(FusionConv2d, kind):
    dev, _ = make_pair(FusionConv2d, kind, params_for(kind, False))
    x, r = data_for(kind, False)
    xd, rd = on_device(x, r)
    opt = torch.optim.SGD(dev.parameters(), lr=0.05)
    y1, g1 = run_stack(dev, xd, rd)
    opt.step()
    y2, g2 = run_stack(dev, xd, rd)
    fresh = Stack(kind, lambda ci, co, k, s, fl: FusionConv2d(ci, co, k, stride=s, padding=(k - 1) // 2, **fl))
    fresh.load_state_dict(dev.state_dict())
    y3, g3 = run_stack(fresh.cuda(), xd, rd)
    torch.cuda.synchronize()
    assert not torch.equal(y1, y2), "the step changed nothing"
    assert not torch.equal(g1["x"], g2["x"]), "the backward still read the old weight"
    assert torch.equal(y2, y3)
    for name in g2:
        assert torch.equal(g2[name], g3[name]), name
