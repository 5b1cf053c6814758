"""The Python side of the weight state machine: OFFSubNetwork re-pushes a parameter when its (data_ptr, _version) tag moves, OFFUnits
binds its parameters in place and re-binds a re-allocated one.  One test per WRITER, one key per group of tests/weight_updates.py in
each: after the write, the next forward must give the bits of a fresh module loaded with the module's new values.

The writers: p.mul_() under no_grad; an SGD step in which only that parameter has a gradient; p.data = new_tensor; a parent module's
load_state_dict; the module's own load_state_dict; p.data.mul_() followed by mark_weights_dirty(); p.data.mul_() under
OFFK_ALWAYS_PUSH=1.  (p.data.mul_() with neither remedy is the documented blind spot of mark_weights_dirty's docstring and is not
asserted either way.)  The frozen Sobel weight of the Flow variant has no gradient, so the SGD writer leaves it out.
The writers that scale in place (mul_) keep the Sobel weight in its four-tap form; it becomes a dense nine-tap weight only under the
three writers that take new values: p.data = new_tensor and the two load_state_dict ones.

Wall time of this module on an MI355X (first run): 21.0 s for its 28 items, the slowest 2.1 s.
"""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import off_module, spec, synth

from . import weight_updates as wu
from .arena import same_bits
from .featmaps import rt  # noqa: F401
from .forward import dev

pytestmark = pytest.mark.gpu

MODULES = [pytest.param("rgb", "fp32", id="rgb-fp32"), pytest.param("rgb", "f32split", id="rgb-f32split"), pytest.param("flow", "fp32", id="flow-fp32")]
VARIANT = {"rgb": spec.VARIANT_RGB, "flow": spec.VARIANT_FLOW}


def one_key_per_group(variant):
    """The LAST key of every group: the 7x7 sites, the tail of fusion@7 (a first key would do; the last ones sit behind every image)."""
    return [wu.keys_of(variant, g)[-1] for g in wu.groups(variant)]


def feats():
    return [dev(f) for f in synth.make_features(wu.B, wu.L, 2)]


def param(net, key):
    mod, attr = key.rsplit(".", 1)
    m = net
    for part in mod.split("."):
        m = getattr(m, part)
    return getattr(m, attr)


def torch_weights(w):
    return dict((k, torch.from_numpy(np.ascontiguousarray(v))) for k, v in w.items())


def new_net(name, prec, state):
    net = off_module.OFFSubNetwork(spec.NUM_CLASSES, wu.B, wu.L, name, consensus=False, precision=prec).cuda()
    net.load_state_dict(state)
    return net


def outputs(net, x):
    out = [o.detach().clone() for o in net(x)]
    torch.cuda.synchronize()
    return out


def check_writer(name, prec, write, skip=()):
    """For one key per group: write(net, key, new values), then net(feats) against a fresh module holding net's state -- equal bits --
    and against net's forward before the write -- the heads of feeds(key) differ."""
    variant = VARIANT[name]
    w0 = synth.make_weights(variant)
    x = feats()
    net = new_net(name, prec, torch_weights(w0))
    before = outputs(net, x)
    for key in one_key_per_group(variant):
        if wu.group(key) in skip:
            continue
        new = torch.from_numpy(wu.perturbed(key, param(net, key).detach().cpu().numpy()))
        write(net, key, new)
        got = outputs(net, x)
        state = dict((k, v.detach().clone()) for k, v in net.state_dict().items())
        want = outputs(new_net(name, prec, state), x)
        assert all(same_bits(a, b) for a, b in zip(got, want)), key
        moved = set(n for n, a, b in zip(wu.HEAD_ORDER, got, before) if not same_bits(a, b))
        assert moved == wu.feeds(key), (key, sorted(moved))
        before = got


@pytest.mark.parametrize("name,prec", MODULES)
def test_in_place_mul_under_no_grad(rt, name, prec):
    def write(net, key, _new):
        with torch.no_grad():
            param(net, key).mul_(1.5)
    check_writer(name, prec, write)


@pytest.mark.parametrize("name,prec", MODULES)
def test_sgd_step_on_one_parameter(rt, name, prec):
    def write(net, key, new):
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1.0)
        p = param(net, key)
        p.grad = (p.detach() - new.to(p.device))               # lr 1: the step lands on `new`
        opt.step()
        opt.zero_grad(set_to_none=True)
    check_writer(name, prec, write, skip=("sobel",))


@pytest.mark.parametrize("name,prec", MODULES)
def test_data_replaced_by_a_new_tensor(rt, name, prec):
    def write(net, key, new):
        param(net, key).data = new.cuda()
    check_writer(name, prec, write)


@pytest.mark.parametrize("name,prec", MODULES)
def test_parent_module_load_state_dict(rt, name, prec):
    def write(net, key, new):
        parent = torch.nn.Sequential(net)                       # never reaches net.load_state_dict
        sd = dict((k, v.detach().clone()) for k, v in parent.state_dict().items())
        sd["0." + key] = new
        parent.load_state_dict(sd)
    check_writer(name, prec, write)


@pytest.mark.parametrize("name,prec", MODULES)
def test_own_load_state_dict(rt, name, prec):
    def write(net, key, new):
        sd = dict((k, v.detach().clone()) for k, v in net.state_dict().items())
        sd[key] = new
        net.load_state_dict(sd)
    check_writer(name, prec, write)


@pytest.mark.parametrize("name,prec", MODULES)
def test_data_mul_then_mark_weights_dirty(rt, name, prec):
    def write(net, key, _new):
        param(net, key).data.mul_(1.5)
        net.mark_weights_dirty()
    check_writer(name, prec, write)


@pytest.mark.parametrize("name,prec", MODULES)
def test_data_mul_under_always_push(rt, name, prec, monkeypatch):
    monkeypatch.setenv("OFFK_ALWAYS_PUSH", "1")

    def write(net, key, _new):
        param(net, key).data.mul_(1.5)
    check_writer(name, prec, write)


# ---- OFFUnits: parameters bound in place ---------------------------------------------------------------------------------------------
def new_units(name, prec, state):
    units = off_module.OFFUnits(wu.B, wu.L, name, precision=prec).cuda()
    units.load_state_dict(state)
    return units.eval()


def check_units_writer(name, prec, write, only=None):
    variant = VARIANT[name]
    w0 = torch_weights(synth.make_weights(variant))
    x = feats()
    units = new_units(name, prec, w0)
    before = outputs(units, x)
    own = set(units.state_dict())
    for key in one_key_per_group(variant):
        if key not in own or (only is not None and wu.group(key) not in only) or (only is None and wu.group(key) == "sobel"):
            continue
        new = torch.from_numpy(wu.perturbed(key, param(units, key).detach().cpu().numpy()))
        write(units, key, new)
        got = outputs(units, x)
        state = dict((k, v.detach().clone()) for k, v in units.state_dict().items())
        want = outputs(new_units(name, prec, state), x)
        assert all(same_bits(a, b) for a, b in zip(got, want)), key
        assert not all(same_bits(a, b) for a, b in zip(got, before)), key
        before = got


UNITS = [pytest.param("rgb", "fp32", id="rgb-fp32"), pytest.param("rgb", "f32split", id="rgb-f32split"), pytest.param("flow", "fp32", id="flow-fp32")]


@pytest.mark.parametrize("name,prec", UNITS)
def test_units_in_place_mul_and_sgd_step(rt, name, prec):
    def mul(units, key, _new):
        with torch.no_grad():
            param(units, key).mul_(1.5)

    def sgd(units, key, new):
        opt = torch.optim.SGD([p for p in units.parameters() if p.requires_grad], lr=1.0)
        p = param(units, key)
        p.grad = (p.detach() - new.to(p.device))
        opt.step()
        opt.zero_grad(set_to_none=True)
    check_units_writer(name, prec, mul)
    check_units_writer(name, prec, sgd)


@pytest.mark.parametrize("name,prec", UNITS)
def test_units_data_replaced_and_state_dicts_loaded(rt, name, prec):
    def data(units, key, new):
        param(units, key).data = new.cuda()

    def own(units, key, new):
        sd = dict((k, v.detach().clone()) for k, v in units.state_dict().items())
        sd[key] = new
        units.load_state_dict(sd)

    def parent(units, key, new):
        p = torch.nn.Sequential(units)
        sd = dict((k, v.detach().clone()) for k, v in p.state_dict().items())
        sd["0." + key] = new
        p.load_state_dict(sd)
    for write in (data, own, parent):
        check_units_writer(name, prec, write)


def test_units_sobel_weight_loaded_after_a_forward(rt):
    """The Flow variant's Sobel weight is frozen but travels in checkpoints: one loaded after the first forward must reach the handle."""
    def own(units, key, new):
        sd = dict((k, v.detach().clone()) for k, v in units.state_dict().items())
        sd[key] = new
        units.load_state_dict(sd)

    def data(units, key, new):
        param(units, key).data = new.cuda()
    for write in (own, data):
        check_units_writer("flow", "fp32", write, only=("sobel",))
