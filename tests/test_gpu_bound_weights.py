"""Weights bound in place (offk_bind_weight) across an update: the six arrays of bindings in the handle (bnd_*), which offk_set_weight
clears silently, beside the copies of tests/test_gpu_weight_updates.py.

A handle with a contraction weight bound runs the register-staged units kernel, whose bits are not those of a handle that holds copies,
so the reference here is always a handle FRESHLY BOUND to fresh tensors (clones holding the values in question), never a set handle.
RGB variant, B = 1, L = 3, the configurations `default` (fused units) and `unfused_units` (K1 + K2) of test_gpu_weight_updates.py, both
arithmetic modes; one site of each map size (3a, 3c, 5a) and all six unit kinds.  Every assertion is on equal bits:

  * in-place update: bind, forward, write the bound tensor in place on the same stream with no library call, forward;
  * re-bind: the same key bound to another tensor;
  * set replaces a binding: offk_set_weight on a bound key, after which a write to the old tensor changes nothing -- against a handle
    that binds the remaining keys and sets this one;
  * partial binding: motion_conv_gen_3c.weight alone bound, everything else set;
  * the training side: the first and the third property through offk_off_units_train + offk_off_units_backward -- G / D, the unit
    channels of the fusion buffers, dG / dD and the whole flat gradient buffer.

Wall time of this module on an MI355X (first run): 12.1 s for its 40 items, the slowest 1.2 s.
"""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import weight_updates as wu
from .arena import same_bits
from .units_grad import random_views
from .featmaps import rt  # noqa: F401
from .forward import HANDLE_PRECISIONS, dev
from .weight_updates import CONFIGS, differing, feats, run

pytestmark = pytest.mark.gpu

RGB = spec.VARIANT_RGB
BOUND_CONFIGS = ("default", "unfused_units")
SITES = ("3a", "3c", "5a")                        # 28x28, 14x14, 7x7
UNIT_KEYS = [k for k in wu.keys(RGB) if k.startswith(spec.UNIT_PARAM_PREFIXES)]
DROP = (5, 0.5)
CASES = [pytest.param(c, p, s, id="%s-%s-%s" % (c, p, s)) for c in BOUND_CONFIGS for p in HANDLE_PRECISIONS for s in SITES]


def site_keys(site):
    return [k for k in UNIT_KEYS if k.rsplit(".", 1)[0].endswith("_" + site)]


class Bound:
    """A fresh handle holding `w`: the keys of `bind` bound to clones of their values (self.t), every other key set."""

    def __init__(self, rt, config, prec, w, bind, training=False):
        with pytest.MonkeyPatch.context() as mp:
            for k, v in CONFIGS[config][0].items():
                mp.setenv(k, v)
            self.h = rt.OffForward(wu.B, wu.L, RGB, consensus=False, precision=prec, training=training)
        bind = set(bind)
        assert self.h.load_state_dict(dict((k, v) for k, v in w.items() if k not in bind), strict=False) == sorted(bind, key=list(w).index)
        self.t = dict((k, dev(w[k]).clone()) for k in bind)
        for k, t in self.t.items():
            self.h.bind_weight(k, t)
        assert self.h.missing_weights()[0] == 0


def train_run(b, views):
    """offk_off_units_train + offk_off_units_backward: name -> a copy of every region they leave and of the flat gradient buffer."""
    b.h.off_units_train(feats(), *DROP)
    flat, _got = b.h.off_units_backward(feats(), views, *DROP)
    snap = {"grads": flat.clone()}
    # (the unit channels alone: the carried-over channels behind them are the fusion stages' to write, and these calls run none)
    for name, ch, units in [("fusion_28", 320, 2), ("fusion_14", 1056, 5), ("fusion_7", 832, 2)]:
        snap[name] = b.h.region(name, ch)[:, :spec.UNIT_CH * units].clone()
    for s in spec.SITE_NAMES:
        for reg, ch in (("G_", 128), ("D_", 32), ("dG_", 128), ("dD_", 32)):
            snap[reg + s] = b.h.region(reg + s, ch).clone()
    torch.cuda.synchronize()
    return snap


def moved_heads(a, b):
    return set(n for n in wu.HEAD_ORDER if not same_bits(a[n], b[n]))


@pytest.mark.parametrize("config,prec,site", CASES)
def test_in_place_update_and_rebind(rt, config, prec, site):
    w0 = synth.make_weights(RGB)
    a = Bound(rt, config, prec, w0, UNIT_KEYS)
    base = run(a.h)
    for k in site_keys(site):
        new = wu.perturbed(k, w0[k])
        fresh = Bound(rt, config, prec, wu.with_key(w0, k, new), UNIT_KEYS)
        want = run(fresh.h)
        a.t[k].copy_(dev(new))                                  # in place, this stream, no library call
        got = run(a.h)
        assert differing(got, want) == [], k
        assert moved_heads(got, base) == wu.feeds(k), k
        a.t[k].copy_(dev(w0[k]))
        assert differing(run(a.h), base) == [], k
        other = dev(new).clone()                                # the same key bound to another tensor
        a.h.bind_weight(k, other)
        assert differing(run(a.h), want) == [], k
        a.h.bind_weight(k, a.t[k])
        assert differing(run(a.h), base) == [], k


@pytest.mark.parametrize("config,prec,site", CASES)
def test_set_weight_replaces_a_binding(rt, config, prec, site):
    w0 = synth.make_weights(RGB)
    for k in site_keys(site):
        a = Bound(rt, config, prec, w0, UNIT_KEYS)
        base = run(a.h)
        new = wu.perturbed(k, w0[k])
        a.h.set_weight(k, new)
        got = run(a.h)
        a.t[k].mul_(3.0)                                        # the old tensor: nobody reads it any more
        assert differing(run(a.h), got) == [], k
        fresh = Bound(rt, config, prec, wu.with_key(w0, k, new), [u for u in UNIT_KEYS if u != k])
        assert differing(got, run(fresh.h)) == [], k
        assert moved_heads(got, base) == wu.feeds(k), k


@pytest.mark.parametrize("config,prec", [pytest.param(c, p, id="%s-%s" % (c, p)) for c in BOUND_CONFIGS for p in HANDLE_PRECISIONS])
def test_partial_binding(rt, config, prec):
    k = "motion_conv_gen_3c.weight"
    w0 = synth.make_weights(RGB)
    new = wu.perturbed(k, w0[k])
    a = Bound(rt, config, prec, w0, [k])
    base = run(a.h)
    a.t[k].copy_(dev(new))
    got = run(a.h)
    fresh = Bound(rt, config, prec, wu.with_key(w0, k, new), [k])
    assert differing(got, run(fresh.h)) == []
    assert moved_heads(got, base) == wu.feeds(k)
    a.t[k].copy_(dev(w0[k]))
    assert differing(run(a.h), base) == []


@pytest.mark.parametrize("config,prec,site", CASES)
def test_training_side_follows_bound_weights(rt, config, prec, site):
    w0 = synth.make_weights(RGB)
    _bufs, views = random_views(wu.B * (wu.L - 1))
    a = Bound(rt, config, prec, w0, UNIT_KEYS, training=True)
    base = train_run(a, views)
    for k in site_keys(site):
        new = wu.perturbed(k, w0[k])
        want = train_run(Bound(rt, config, prec, wu.with_key(w0, k, new), UNIT_KEYS, training=True), views)
        a.t[k].copy_(dev(new))
        got = train_run(a, views)
        assert differing(got, want) == [], k
        assert differing(got, base) != [], k
        a.t[k].copy_(dev(w0[k]))
        assert differing(train_run(a, views), base) == [], k
        # set replaces the binding, on a handle of its own
        b = Bound(rt, config, prec, w0, UNIT_KEYS, training=True)
        b.h.set_weight(k, new)
        got = train_run(b, views)
        b.t[k].mul_(3.0)
        assert differing(train_run(b, views), got) == [], k
        want = train_run(Bound(rt, config, prec, wu.with_key(w0, k, new), [u for u in UNIT_KEYS if u != k], training=True), views)
        assert differing(got, want) == [], k
