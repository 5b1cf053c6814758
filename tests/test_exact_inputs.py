"""The integer inputs of tests/exact.py on the CPU: what the exact GPU tests (tests/test_gpu_exact.py) stand on.

1. The generator restated on torch int64 is synth's own (bits and dropout keep mask), and the value sets are the documented ones.
2. The exactness condition holds for every shape the GPU tests use: the largest per-element sum of absolute terms of every output is
   below 2^23 for the six parameter gradients (an accumulate call doubles them) and below 2^24 for everything else.  A condition
   of the inputs, not a tolerance.  The largest sums grow with the row count; at B = 64, L = 7 (asserted on the device by the
   full-size GPU case from its own reference) the worst is the depthwise-tap gradient at site 3b, 4.0e6 of 8.4e6.
3. exact.unit_reference agrees with the oracle the rest of the suite trusts (oracle.off_oracle.off_unit, its autograd through
   unit_param_grads_from_dm, and x.grad) in fp64 on the same inputs with zero difference.
4. assert_exact sees one wrong element, a NaN, a wrong shape and an all-zero reference, and does not see a signed zero.
"""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

from . import exact


def test_generator_is_synths_own():
    for seed, start, n in ((0, 0, 1000), (exact.stream(1, 0, 3), 12345, 4097), (synth.dropout_stream(21, 8), 0, 513), (0xFFFFFFFFFFFF, 7, 64)):
        want = synth.raw_u64(seed, start, n)
        got = exact.raw_bits(seed, start, n).numpy().view(np.uint64)
        assert np.array_equal(got, want), seed
    for si, P, H in ((0, 2, 28), (4, 3, 14), (8, 5, 7)):
        want = synth.dropout_keep(21, si, P, H, exact.DROP_P)
        assert np.array_equal(exact.keep_mask_torch(21, si, P, H, "cpu").numpy(), want)
        assert np.array_equal(exact.keep_mask(21, si, P, H).numpy(), want)
        assert 0.45 < want.mean() < 0.55
    assert 1.0 / (1.0 - exact.DROP_P) == 2.0 and synth.dropout_threshold(exact.DROP_P) == 1 << 15


@pytest.mark.parametrize("variant", [spec.VARIANT_RGB, spec.VARIANT_FLOW])
def test_value_sets(variant):
    s = exact.SiteInputs(1, 2, 3, variant)
    sets = lambda t: set(t.unique().tolist())   # noqa: E731
    plain = synth.make_weights(variant)
    assert s.x.dtype == torch.float32 and tuple(s.x.shape) == (6, 320, 28, 28) and tuple(s.dm.shape) == (4, 160, 28, 28)
    assert sets(s.x) == {-2.0, -1.0, 0.0, 1.0, 2.0} and sets(s.dm) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert sets(s.wg) == {-1.0, 0.0, 1.0} and sets(s.wd) == {-1.0, 0.0, 1.0}
    assert sets(s.bg) <= set(float(v) for v in range(-3, 4)) and sets(s.bd) <= set(float(v) for v in range(-3, 4))
    assert 0.2 < float((s.wd != 0).float().mean()) < 0.3                     # about a quarter nonzero
    assert abs(float((s.wd > 0).float().mean()) - float((s.wd < 0).float().mean())) < 0.03
    if variant == spec.VARIANT_RGB:
        assert sets(s.tap) == {-1.0, 0.0, 1.0} and sets(s.tb) <= {-1.0, 0.0, 1.0}
    else:
        assert s.tb is None and torch.equal(s.tap, torch.from_numpy(plain[spec.SOBEL_KEY]))
    # another seed, other values; the same seed, the same
    assert not torch.equal(s.x, exact.SiteInputs(1, 2, 3, variant, seed=2).x)
    assert torch.equal(s.x, exact.SiteInputs(1, 2, 3, variant).x)
    w = exact.weights(variant, [exact.SiteInputs(si, 1, 2, variant) for si in range(spec.NUM_SITES)])
    assert list(w) == list(plain) and w["motion_conv_gen_3b.weight"].dtype == np.float32
    assert np.array_equal(w["motion_conv_gen_3b.weight"], s.wg.numpy())
    assert np.array_equal(w["motion_conv_trans_28.weight"], plain["motion_conv_trans_28.weight"])


@pytest.fixture(scope="module", params=exact.SHAPES, ids=exact.IDS)
def case(request):
    B, L, variant, slice_mode = request.param
    sites = [exact.SiteInputs(si, B, L, variant) for si in range(spec.NUM_SITES)]
    refs = [exact.unit_reference(s, B, L, variant, slice_mode) for s in sites]
    return request.param, sites, refs


def test_condition_holds(case):
    (B, L, variant, _slice), _sites, refs = case
    worst = {}
    for (name, _C, _H), (out, cap) in zip(spec.SITES, refs):
        assert set(cap) == set(out) and len(out) == (13 if variant == spec.VARIANT_RGB else 11)
        exact.check_caps(cap, name)
        assert cap["G"] <= 4e3 and cap["D"] <= 4e3 and cap["M_train"] <= 4e3
        for k, c in cap.items():
            if c / (exact.LIMIT_ACC if k in exact.PARAM_OUTPUTS else exact.LIMIT) > worst.get("share", 0.0):
                worst = {"share": c / (exact.LIMIT_ACC if k in exact.PARAM_OUTPUTS else exact.LIMIT), "site": name, "output": k, "sum": c}
        # every value is an integer, and none of the outputs is trivial
        for k, t in out.items():
            assert t.dtype == torch.float64 and bool((t == t.round()).all()) and bool((t != 0).any()), (name, k)
    print("B = %d, L = %d: largest sum of |terms| %.0f (%s at %s), %.4f of its limit" % (B, L, worst["sum"], worst["output"], worst["site"], worst["share"]))


@pytest.mark.parametrize("shape", exact.SOBEL_SHAPES, ids=exact.SOBEL_IDS)
def test_condition_holds_with_a_dense_sobel_weight(shape):
    """Flow shapes (exact.SOBEL_SHAPES) with exact.dense_sobel in place of the fixed four-tap kernel (K2's nine-tap path, tests/test_gpu_sobel_taps.py):
    nine terms per S element instead of four, the same 2^24 / 2^23 limits; and the reference is still the oracle's."""
    B, L, variant, slice_mode = shape
    sob = exact.dense_sobel()
    assert set(sob.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert torch.equal(sob, exact.dense_sobel()) and not torch.equal(sob, exact.dense_sobel(seed=2))
    sites = [exact.SiteInputs(si, B, L, variant, sobel=sob) for si in range(spec.NUM_SITES)]
    w = exact.weights(variant, sites)
    assert np.array_equal(w[spec.SOBEL_KEY], sob.numpy())
    wt = dict((k, torch.from_numpy(v).double()) for k, v in w.items())
    for s in sites:
        out, cap = exact.unit_reference(s, B, L, variant, slice_mode)
        assert len(out) == 11
        exact.check_caps(cap, s.name)
        assert cap["M"] <= 4e3 and cap["M_train"] <= 4e3
        for k, t in out.items():
            assert bool((t == t.round()).all()) and bool((t != 0).any()), (s.name, k)
        with torch.no_grad():
            m_eval = orc.off_unit(s.x.double(), wt, s.name, B, L, variant, slice_mode)
        exact.assert_exact(m_eval.permute(0, 2, 3, 1).reshape(-1, 160), out["M"], s.name + " M")


def test_reference_is_the_oracles(case):
    (B, L, variant, slice_mode), sites, refs = case
    P = B * (L - 1)
    w = {}
    for s in sites:
        w.update((k, v.double()) for k, v in s.params().items())
    if variant == spec.VARIANT_FLOW:
        w[spec.SOBEL_KEY] = sites[0].tap.double()
    feats = [s.x.double() for s in sites]
    drops = [s.keep.double() * 2.0 for s in sites]
    dms = [s.dm.double() for s in sites]
    grads = orc.unit_param_grads_from_dm(feats, w, B, L, variant, slice_mode, dms, drops)
    assert len(grads) == (54 if variant == spec.VARIANT_RGB else 36)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])   # noqa: E731
    for s, x, (out, _cap) in zip(sites, feats, refs):
        with torch.no_grad():
            m_eval = orc.off_unit(x, w, s.name, B, L, variant, slice_mode)
        xg = x.clone().requires_grad_(True)
        m_train = orc.off_unit(xg, w, s.name, B, L, variant, slice_mode, drops[s.si])
        m_train.backward(dms[s.si])
        assert tuple(m_eval.shape) == (P, 160, s.H, s.H)
        exact.assert_exact(rows(m_eval), out["M"], s.name + " M")
        exact.assert_exact(rows(m_train.detach()), out["M_train"], s.name + " M_train")
        exact.assert_exact(rows(xg.grad), out["dX"], s.name + " dX")
        for short, key in exact.PARAM_KEYS.items():
            if short in out:
                exact.assert_exact(grads[key % s.name], out[short], s.name + " " + short)
        # G and D, as the kernels store them
        with torch.no_grad():
            g = torch.relu(torch.nn.functional.conv2d(x, w["motion_conv_gen_%s.weight" % s.name], w["motion_conv_gen_%s.bias" % s.name]))
            d = torch.nn.functional.conv2d(orc.spatial_frames(x, B, L, slice_mode), w["motion_spatial_down_%s.weight" % s.name],
                                           w["motion_spatial_down_%s.bias" % s.name])
        exact.assert_exact(rows(g), out["G"], s.name + " G")
        exact.assert_exact(rows(d), out["D"], s.name + " D")
        # dGpre and dD: the bias gradients are their column sums
        exact.assert_exact(out["dG"].sum(0), out["gen_b"], s.name)
        exact.assert_exact(out["dD"].sum(0), out["down_b"], s.name)


def test_dx_rows_are_the_rows_of_the_whole(case):
    (B, L, variant, slice_mode), sites, refs = case
    s, (out, _cap) = sites[7], refs[7]
    idx = torch.tensor([0, 5, 48, 49, B * L * 49 - 1])
    part, _ = exact.unit_reference(s, B, L, variant, slice_mode, dx_rows=idx)
    assert torch.equal(part["dX"], out["dX"][idx])


def test_assert_exact_sees_what_it_has_to():
    ref = torch.arange(-6, 6, dtype=torch.float64).reshape(3, 4)
    exact.assert_exact(ref.float(), ref)
    neg = ref.float().clone()
    neg[1, 2] = -0.0                                  # ref[1, 2] == 0: a signed zero is not a difference
    assert float(ref[1, 2]) == 0.0
    exact.assert_exact(neg, ref)
    exact.assert_exact(ref.bfloat16(), ref)
    one = ref.float().clone()
    one[2, 3] += 1.0
    with pytest.raises(AssertionError, match=r"1 of 12 elements differ.*\(2, 3\): got 6.0, reference 5.0"):
        exact.assert_exact(one, ref, "one")
    nan = ref.float().clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="1 of 12"):
        exact.assert_exact(nan, ref)
    with pytest.raises(AssertionError, match="shape"):
        exact.assert_exact(ref.float().reshape(4, 3), ref)
    with pytest.raises(AssertionError, match="all zero"):
        exact.assert_exact(torch.zeros(3), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(AssertionError, match="fp64"):
        exact.assert_exact(ref.float(), ref.float())
    with pytest.raises(AssertionError, match="not below"):
        exact.check_caps({"gen_w": float(2 ** 23)})
    assert exact.check_caps({"gen_w": float(2 ** 22), "dX": float(2 ** 22)}) == 0.5
    mm = exact.Mismatches()
    mm.check(ref.float(), ref, "same")
    mm.raise_if_any()
    mm.check(one, ref, "one")
    mm.check(nan, ref, "nan")
    with pytest.raises(AssertionError, match=r"(?s)2 tensors differ.*one: 1 of 12.*nan: 1 of 12"):
        mm.raise_if_any()
