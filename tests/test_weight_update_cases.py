"""The case table of tests/weight_updates.py against the reference's key list and the fp64 oracle (no GPU).

The GPU tests assert "exactly the heads in feeds(key) change their bits"; that is only a statement about the library if the
table is right and if the perturbation moves each of those heads by more than an fp32 forward can round away.  Both are
conditions on the table and on the inputs, so they are proved here, with the oracle as the arbiter.
"""
import json
import os

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

from . import weight_updates as wu

FEATURE_CONFIG = 2          # the synth.make_features stream the GPU tests use as well
MIN_MOVE = 1e-3             # of the head's max |logit|: three orders above fp32 rounding of a logit


def _oracle(feats, w, variant):
    with torch.no_grad():
        out = orc.off_forward(feats, dict((k, torch.from_numpy(v).double()) for k, v in w.items()), wu.B, wu.L, variant, orc.SLICE_FLAT,
                              consensus=False)
    return [o.reshape(wu.B * (wu.L - 1), -1) for o in out]


_BASE = {}


def base(variant):
    """(feature maps, synth weights, the oracle's three logits on them) in fp64, once per variant and never written to."""
    if variant not in _BASE:
        feats = [torch.from_numpy(f).double() for f in synth.make_features(wu.B, wu.L, FEATURE_CONFIG)]
        w0 = synth.make_weights(variant)
        _BASE[variant] = (feats, w0, _oracle(feats, w0, variant))
    return _BASE[variant]


@pytest.mark.parametrize("variant", wu.VARIANTS, ids=wu.VARIANT_TAGS.get)
def test_keys_and_groups_cover_the_reference_state_dict(variant, golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))[wu.VARIANT_TAGS[variant]]
    want = {k for k in ref if "motion" in k or "sobel" in k}
    got = wu.keys(variant)
    assert len(got) == len(set(got)) and set(got) == want
    for k in got:
        assert wu.group(k) in wu.GROUPS, k
        assert wu.feeds(k) <= set(wu.HEAD_ORDER) and wu.feeds(k), k
    assert sum(len(wu.keys_of(variant, g)) for g in wu.groups(variant)) == len(got)      # the groups partition the keys
    for g in wu.GROUPS:
        assert bool(wu.keys_of(variant, g)) == (g in wu.groups(variant)), g


def test_the_perturbation_moves_every_element():
    for variant in wu.VARIANTS:
        w0 = synth.make_weights(variant)
        for k, v in w0.items():
            d = wu.delta(k, v.shape)
            assert d.shape == v.shape and np.all(d != 0) and np.all(d * 8 == np.round(d * 8)), k
            w1 = wu.perturbed(k, v)
            assert w1.dtype == np.float32 and np.all(w1 != v), k
            assert np.array_equal(w1, wu.perturbed(k, v)), k
    sob = wu.perturbed(spec.SOBEL_KEY, synth.make_weights(spec.VARIANT_FLOW)[spec.SOBEL_KEY])
    assert np.all(sob != 0)                                                              # a dense nine-tap weight


_CASES = [pytest.param(v, g, id="%s-%s" % (wu.VARIANT_TAGS[v], g)) for v in wu.VARIANTS for g in wu.groups(v)]


@pytest.mark.parametrize("variant,grp", _CASES)
def test_feeds_is_what_the_oracle_says(variant, grp):
    """One key perturbed: the heads of the fp64 oracle that differ are exactly feeds(key), and each of them moves by at least
    MIN_MOVE of its max |logit| (else: enlarge that key's d in weight_updates._d_scale)."""
    feats, w0, ref = base(variant)
    for k in wu.keys_of(variant, grp):
        out = _oracle(feats, wu.with_key(w0, k), variant)
        moved = set()
        for name, a, b in zip(wu.HEAD_ORDER, out, ref):
            rel = ((a - b).abs().max() / b.abs().max()).item()
            if rel != 0.0:
                moved.add(name)
                assert rel >= MIN_MOVE, (k, name, rel)
        assert moved == wu.feeds(k), (k, sorted(moved))


class _FakeUnitsRuntime:
    """Stands in for runtime.OffForward behind OFFUnits on a machine without a GPU: records what is copied and what is bound."""

    def __init__(self, *a, **kw):
        self.device = torch.device(kw.get("device", "cpu"))
        self.set, self.bound = [], []

    def set_weight(self, key, value):
        self.set.append(key)

    def bind_weight(self, key, tensor):
        self.bound.append(key)


def test_off_units_push_a_sobel_weight_loaded_after_the_first_forward(monkeypatch):
    """OFFUnits binds its trainable tensors and COPIES the frozen Sobel weight of the Flow variant; a checkpoint loaded after the first
    forward (its own load_state_dict or a parent's, or .data replaced) must send the copy again, and nothing else may."""
    from offk_amd import off_module
    monkeypatch.setattr(off_module.runtime, "OffForward", _FakeUnitsRuntime)
    units = off_module.OFFUnits(wu.B, wu.L, "flow")
    params = [units._param(k) for k in units.param_keys]
    rt = units._handle("cpu", params)
    assert rt.set == [spec.SOBEL_KEY] and rt.bound == units.param_keys
    del rt.set[:], rt.bound[:]
    units._handle("cpu", params)
    assert rt.set == [] and rt.bound == []
    dense = torch.from_numpy(wu.perturbed(spec.SOBEL_KEY, synth.make_weights(spec.VARIANT_FLOW)[spec.SOBEL_KEY]))
    sd = dict((k, v.detach().clone()) for k, v in units.state_dict().items())
    sd[spec.SOBEL_KEY] = dense
    units.load_state_dict(sd)
    units._handle("cpu", params)
    assert rt.set == [spec.SOBEL_KEY] and rt.bound == []          # (load_state_dict copies in place: nothing is re-bound)
    del rt.set[:]
    units.sobel_edge_diagonal.conv.weight.data = dense.clone()
    units._handle("cpu", params)
    assert rt.set == [spec.SOBEL_KEY] and rt.bound == []
    # an in-place write through .data moves neither half of the tag (OFFSubNetwork's documented blind spot); OFFK_ALWAYS_PUSH=1 is the remedy
    del rt.set[:]
    units.sobel_edge_diagonal.conv.weight.data.mul_(2.0)
    monkeypatch.setenv("OFFK_ALWAYS_PUSH", "1")
    units._handle("cpu", params)
    assert rt.set == [spec.SOBEL_KEY] and rt.bound == []
