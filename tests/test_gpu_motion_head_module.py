"""MotionHead (off_module.py) inside a small net where the head's input also feeds the next stage:

    y0 = c0(x)            FusionConv2d(64, 64, 3, padding=1, relu=True)
    logits = head(y0)     MotionHead(64, 101)          -- cross-entropy on it
    y1 = c1(y0)           FusionConv2d(64, 64, 3, padding=1)   -- a sum on it
    loss = cross_entropy(logits, target) + y1.sum()

"avg7": a 7x7 map, the mean; "max14": a 14x14 map, MaxPool(3, 2, ceil) then the mean -- 49 windows both, n = 2.  Checked against
nn.Conv2d, the numpy mask (synth.head_dropout_keep) and nn.Linear in fp64 on the CPU.

What can be equal is: on integer inputs the convolutions' outputs y0 and y1 and the gradients that do not pass through the head
(c1.weight, c1.bias) are torch.equal to fp64.  The head's mean is a multiply by 1.f / 49, which no arithmetic has exactly, and the
cross-entropy's gradient is a softmax, so the logits and every gradient behind the head are checked, on integers and on normal data
alike, link by link against fp64 of THAT link from the device's own inputs (as tests/test_gpu_fusion_conv_s2_module.py does):
  logits            gamma_{nwin + C + 4} sum |terms|                                       (tests/test_gpu_head_bwd.py)
  head.weight, bias gamma_{n + nwin + 3}: the weight gradient's own n + 1 operations and z's nwin + 2, z being the reference's here
  y0.grad           the head's dX (gamma_{classes + 5} sum |terms|) plus c1's dX (its one-layer bound) plus the one rounded add of the two
  c0, c1            their one-layer bounds from y0.grad and y1.grad
(the exact equality of the head on power-of-two window counts is tests/test_gpu_head_bwd_exact.py's).
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import offk_amd  # noqa: F401

from . import exact
from . import head_bwd as hb
from .conv_grad_checks import one_layer, within

pytestmark = pytest.mark.gpu
N, C, CLS, SEED = 2, 64, 101, 31
KINDS = {"avg7": (7, False, 1), "max14": (14, True, 0)}          # map size, maxpool, head_index


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import off_module
    return off_module


class Net(nn.Module):
    def __init__(self, mods, kind, drop_p):
        super().__init__()
        _hw, maxpool, head_index = KINDS[kind]
        self.c0 = mods.FusionConv2d(C, C, 3, padding=1, relu=True)
        self.head = mods.MotionHead(C, CLS, maxpool=maxpool, head_index=head_index, drop_p=drop_p)
        self.c1 = mods.FusionConv2d(C, C, 3, padding=1)

    def forward(self, x, target, seed=SEED):
        y0 = self.c0(x)
        logits = self.head(y0, drop_seed=seed)
        y1 = self.c1(y0)
        for t in (y0, logits, y1):
            if t.requires_grad:
                t.retain_grad()
        self.trace = (y0, logits, y1)
        return F.cross_entropy(logits, target) + y1.sum()


def params_for(integer):
    gen = torch.Generator().manual_seed(0x4EAD)
    out = {}
    for i, name in enumerate(("c0", "c1")):
        if integer:
            out[name + ".weight"] = exact.sparse_signs(exact.stream(0x71, 1, i), (C, C, 3, 3))
            out[name + ".bias"] = exact.ints(exact.stream(0x71, 2, i), (C,), -2, 2)
        else:
            out[name + ".weight"] = torch.randn(C, C, 3, 3, generator=gen) / (C * 9) ** 0.5
            out[name + ".bias"] = torch.randn(C, generator=gen) * 0.1
    if integer:
        out["head.weight"] = exact.ints(exact.stream(0x71, 3, 0), (CLS, C), -1, 1) * 0.0078125       # 2^-7: tame logits
        out["head.bias"] = exact.ints(exact.stream(0x71, 4, 0), (CLS,), -2, 2)
    else:
        out["head.weight"] = (torch.rand(CLS, C, generator=gen) * 2 - 1) / C ** 0.5
        out["head.bias"] = (torch.rand(CLS, generator=gen) * 2 - 1) / C ** 0.5
    return out


def data_for(kind, integer):
    hw = KINDS[kind][0]
    gen = torch.Generator().manual_seed(0x4EAE)
    x = exact.ints(exact.stream(0x72, 1, 0), (N, C, hw, hw), -3, 3) if integer else torch.randn(N, C, hw, hw, generator=gen)
    return x, torch.tensor([3, 77])


def run_net(net, x, target, seed=SEED):
    x = x.clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    loss = net(x, target, seed)
    loss.backward()
    grads = {"x": x.grad}
    grads.update((k, p.grad) for k, p in net.named_parameters())
    return loss.detach(), grads


def make(mods, kind, integer, drop_p):
    net = Net(mods, kind, drop_p)
    net.load_state_dict(params_for(integer))
    x, target = data_for(kind, integer)
    return net.cuda(), x.cuda().contiguous(memory_format=torch.channels_last), target.cuda()


def fp64_conv(net, name):
    m = getattr(net, name)
    ref = nn.Conv2d(C, C, 3, padding=1).double()
    ref.load_state_dict({"weight": m.weight.detach().cpu().double(), "bias": m.bias.detach().cpu().double()})
    return ref


def check_links(net, kind, g, drop_p, integer):
    """every link of the net against fp64 of that link from the device's own inputs"""
    hw, maxpool, head_index = KINDS[kind]
    y0, logits, y1 = net.trace
    c = hb.Case(hw, hw, int(maxpool), C, CLS, N, drop_p, head_index, SEED)
    y0_rows = y0.detach().cpu().permute(0, 2, 3, 1).contiguous()
    w, b = net.head.weight.detach().cpu(), net.head.bias.detach().cpu()
    ghead = logits.grad.cpu()
    ref = hb.reference(c, y0_rows, w, b, ghead)
    nw = hb.nwin(c)
    assert nw == 49
    within(logits, ref["out"], hb.gamma(nw + C + 4) * ref["mag_out"], "%s logits" % kind)
    gd, zd = ghead.double(), ref["z"]
    within(net.head.weight.grad, ref["dW"], hb.gamma(N + nw + 3) * (gd.abs().t() @ zd.abs()), "%s head.weight" % kind)
    within(net.head.bias.grad, ref["db"], hb.gamma(N + nw + 3) * gd.abs().sum(0), "%s head.bias" % kind)
    # c1, from y0 and y1.grad
    out1, caps1, _ = one_layer(fp64_conv(net, "c1"), dict(), y0.detach().cpu().double(), y1.grad.cpu().double())
    if integer:
        assert max(caps1.values()) < exact.LIMIT
        assert torch.equal(y1.detach().cpu().double(), out1["y"][0]) and torch.equal(net.c1.weight.grad.cpu().double(), out1["weight"][0])
        assert torch.equal(net.c1.bias.grad.cpu().double(), out1["bias"][0])
    within(y1, *out1["y"], "%s c1 y" % kind)
    within(net.c1.weight.grad, *out1["weight"], "%s c1.weight" % kind)
    within(net.c1.bias.grad, *out1["bias"], "%s c1.bias" % kind)
    # y0.grad = the head's dX + c1's dX, one rounded add
    dxh, bh = ref["dX"].permute(0, 3, 1, 2), hb.gamma(CLS + 5) * ref["mag_dX"].permute(0, 3, 1, 2)
    dxc, bc = out1["dx"]
    within(y0.grad, dxh + dxc, bh + bc + hb.U * (dxh.abs() + dxc.abs() + bh + bc), "%s y0.grad" % kind)
    # c0, from x and y0.grad
    out0, caps0, (unstable, masked) = one_layer(fp64_conv(net, "c0"), dict(relu=True), net.x_in.detach().cpu().double(), y0.grad.cpu().double())
    if integer:       # pre-activations are exact (many are exactly 0, which one_layer counts as undecided): y0 itself must be equal
        assert caps0["z"] < exact.LIMIT and torch.equal(y0.detach().cpu().double(), out0["y"][0])
    else:
        assert unstable <= 0.005 * masked, "more than 0.5 %% of the masks undecided within a one-layer bound: %d of %d" % (unstable, masked)
    within(y0, *out0["y"], "%s c0 y" % kind)
    within(g["x"], *out0["dx"], "%s c0 dx" % kind)
    within(net.c0.weight.grad, *out0["weight"], "%s c0.weight" % kind)
    within(net.c0.bias.grad, *out0["bias"], "%s c0.bias" % kind)


@pytest.mark.parametrize("integer", [True, False], ids=["integers", "normal"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_net_against_fp64(mods, kind, integer):
    drop_p = 0.5 if integer else 0.8
    net, x, target = make(mods, kind, integer, drop_p)
    net.train()
    net.x_in = x
    loss, g = run_net(net, x, target)
    torch.cuda.synchronize()
    assert all(v is not None for v in g.values()) and bool(torch.isfinite(loss))
    check_links(net, kind, g, drop_p, integer)
    # the same seed gives the same bits, the module's own counter another mask
    loss2, g2 = run_net(net, x, target)
    assert torch.equal(loss, loss2) and all(torch.equal(g[k], g2[k]) for k in g)
    net.head.drop_seed = 0
    a = net.head(net.trace[0].detach())
    b_ = net.head(net.trace[0].detach())
    a1 = net.head(net.trace[0].detach(), drop_seed=1)
    torch.cuda.synchronize()
    assert net.head.drop_seed == 2 and torch.equal(a, a1) and not torch.equal(a, b_)


def test_frozen_head_launches_no_weight_gradient(mods):
    net, x, target = make(mods, "avg7", False, 0.8)
    net.train()
    before = mods.MotionHead.weight_grad_launches
    _, g_all = run_net(net, x, target)
    assert mods.MotionHead.weight_grad_launches - before == 1
    for p in net.head.parameters():
        p.requires_grad_(False)
    before = mods.MotionHead.weight_grad_launches
    _, g = run_net(net, x, target)
    torch.cuda.synchronize()
    assert mods.MotionHead.weight_grad_launches == before, "the frozen head ran its weight gradient"
    assert g["head.weight"] is None and g["head.bias"] is None
    for name in ("x", "c0.weight", "c0.bias", "c1.weight"):
        assert torch.equal(g[name], g_all[name]), name            # the gradient still flows THROUGH the frozen head, bit for bit
    # only the bias trainable: still one launch, and the same bias gradient
    net.head.bias.requires_grad_(True)
    _, g = run_net(net, x, target)
    assert mods.MotionHead.weight_grad_launches == before + 1
    assert g["head.weight"] is None and torch.equal(g["head.bias"], g_all["head.bias"])


def test_optimizer_step_is_seen_without_a_rebind(mods):
    net, x, target = make(mods, "max14", False, 0.8)
    net.train()
    opt = torch.optim.SGD(net.head.parameters(), lr=0.5)
    l1, g1 = run_net(net, x, target)
    opt.step()
    l2, g2 = run_net(net, x, target)
    fresh = Net(mods, "max14", 0.8)
    fresh.load_state_dict(net.state_dict())
    l3, g3 = run_net(fresh.cuda().train(), x, target)
    torch.cuda.synchronize()
    assert not torch.equal(l1, l2), "the step changed nothing"
    assert not torch.equal(g1["x"], g2["x"]), "the backward still read the old weight"
    assert torch.equal(l2, l3)
    for name in g2:
        assert torch.equal(g2[name], g3[name]), name


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_eval_mode(mods, kind):
    from offk_amd import runtime
    net, x, target = make(mods, kind, False, 0.8)
    net.eval()
    hw, maxpool, head_index = KINDS[kind]
    with torch.no_grad():
        y0 = net.c0(x)
        logits = net.head(y0)
        want = runtime.head(y0.permute(0, 2, 3, 1).contiguous(), net.head.weight.detach(), net.head.bias.detach(), maxpool)
    torch.cuda.synchronize()
    assert torch.equal(logits, want), "eval without grad is K5 itself"
    # eval with grad: the training entries without a mask, within the forward bound, and no seed is drawn
    seed_before = net.head.drop_seed
    out = net.head(y0)
    assert out.requires_grad and net.head.drop_seed == seed_before
    c = hb.Case(hw, hw, int(maxpool), C, CLS, N, 0.0, head_index, 0)
    ref = hb.reference(c, y0.cpu().permute(0, 2, 3, 1).contiguous(), net.head.weight.detach().cpu(), net.head.bias.detach().cpu(),
                       torch.zeros(N, CLS))
    within(out, ref["out"], hb.gamma(hb.nwin(c) + C + 4) * ref["mag_out"], "%s eval logits" % kind)
    within(logits, ref["out"], hb.gamma(hb.nwin(c) + C + 4) * ref["mag_out"], "%s K5 logits" % kind)


def test_reference_state_dict_loads(mods):
    class Heads(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc_action_motion_28 = mods.MotionHead(256, 101, maxpool=True, head_index=0)
            self.fc_action_motion_14 = mods.MotionHead(512, 101, head_index=1)
            self.fc_action_motion = mods.MotionHead(1024, 101, head_index=2)

    gen = torch.Generator().manual_seed(5)
    sd = {}
    for name, ci in (("fc_action_motion_28", 256), ("fc_action_motion_14", 512), ("fc_action_motion", 1024)):
        sd[name + ".weight"] = torch.randn(101, ci, generator=gen)
        sd[name + ".bias"] = torch.randn(101, generator=gen)
    h = Heads()
    assert sorted(h.state_dict()) == sorted(sd)
    h.load_state_dict(sd, strict=True)
    h = h.cuda().train()
    x = torch.randn(2, 256, 14, 14, generator=gen).clamp_(min=0).cuda().contiguous(memory_format=torch.channels_last)
    out = h.fc_action_motion_28(x, drop_seed=9)
    out.sum().backward()
    torch.cuda.synchronize()
    assert out.shape == (2, 101) and h.fc_action_motion_28.weight.grad.shape == (101, 256)
    c = hb.Case(14, 14, 1, 256, 101, 2, 0.8, 0, 9)
    ref = hb.reference(c, x.cpu().permute(0, 2, 3, 1).contiguous(), sd["fc_action_motion_28.weight"], sd["fc_action_motion_28.bias"], torch.ones(2, 101))
    within(out, ref["out"], hb.gamma(49 + 256 + 4) * ref["mag_out"], "loaded 28-head logits")
