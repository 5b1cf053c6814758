"""The integer inputs of tests/exact_fusion.py on the CPU: what the exact fusion-stage GPU tests (tests/test_gpu_exact_fusion.py) stand on.

For every case the GPU file uses (the chain cases, the between forms, the forward shapes):

1. Caps and non-degeneracy.  Every cap -- direct form, and for the chains' 3x3 the Winograd-domain caps in units of 1/4 -- is below
   2^24; in every tensor behind a ReLU the share of zeroed elements lies in 5 % .. 95 %; every checked tensor takes at least 8 values.
2. Order independence, without any kernel: the same computation in fp32 torch CPU ops with the channels as given and with the channels
   permuted, and the chains' 3x3 through an explicit F(2x2, 3x3) restatement in fp32, equal the fp64 reference value for value.
3. Split-fp32 emulation: on sampled output elements of every contraction synth.split_terms drops nothing and synth.emulate_split_dot
   gives exactly the fp64 dot.
4. Sensitivity: one dropped product -- a (pixel, channel, tap) term of c2, a K-element of c3, a point of an A-transform -- is a
   difference assert_exact reports.  The smallest term is an integer >= 1 (>= 1/4 in the Winograd domain).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import exact
from . import exact_fusion as ef

CHAIN_CASES = ef.chain_cases()
BETWEEN_CASES = sorted(set((cin, phases, gemm, n) for cin, phases, gemm, _prec in ef.BETWEEN_FORMS for n in ef.BETWEEN_N))
_CACHE = {}


def chain_case(n, kind, hand):
    """(inputs, out, cap direct, cap F(2x2, 3x3)) of one chain case, computed once"""
    key = ("chain", n, kind, hand)
    if key not in _CACHE:
        c = ef.ChainInputs(n, kind, hand)
        out, cap = c.reference("direct")
        _out, cap_w = c.reference("wino")
        _CACHE[key] = (c, out, cap, cap_w)
    return _CACHE[key]


def between_case(cin, phases, gemm, n):
    key = ("between", cin, phases, gemm, n)
    if key not in _CACHE:
        b = ef.BetweenInputs(n, cin, phases, gemm)
        _CACHE[key] = (b,) + b.reference()
    return _CACHE[key]


def forward_case(B, L):
    key = ("forward", B, L)
    if key not in _CACHE:
        sites = [exact.SiteInputs(si, B, L, spec.VARIANT_RGB) for si in range(spec.NUM_SITES)]
        w = ef.forward_weights(spec.VARIANT_RGB, sites)
        out, cap = ef.forward28_reference(sites, w, B, L, spec.VARIANT_RGB, form="direct")
        _out, cap_w = ef.forward28_reference(sites, w, B, L, spec.VARIANT_RGB, form="wino")
        _CACHE[key] = (sites, w, out, cap, cap_w)
    return _CACHE[key]


def integers(t):
    return bool((t == t.round()).all())


# ---- 1. caps and non-degeneracy --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n,kind,hand", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_chain_conditions(name, n, kind, hand):
    c, out, cap, cap_w = chain_case(n, kind, hand)
    d, w = ef.check_caps(cap, name), ef.check_caps(cap_w, name + " F(2x2, 3x3)")
    print("chain %s: largest cap / 2^24 direct %.2e (%s), F(2x2, 3x3) %.2e" % (name, d, max(cap, key=cap.get), w))
    assert cap_w["t2"] >= cap["t2"] and cap_w["t1"] == cap["t1"] and cap_w["y"] == cap["y"]
    ef.check_nondegenerate(out, ("t1", "t2", "y"), (), name)
    assert all(integers(t) and t.dtype == torch.float64 for t in out.values())
    assert tuple(out["y"].shape) == (n, 14, 14, 256) and tuple(out["t2"].shape) == (n, 14, 14, 64)
    if hand == "seam":
        assert bool((c.x[:, :6] == 0).all()) and bool((c.x[:, 8:] == 0).all()) and bool((c.x[:, 6:8] != 0).any())
    if hand == "border":
        assert bool((c.x[:, 1:13, 1:13] == 0).all()) and all(bool((e != 0).any()) for e in (c.x[:, 0], c.x[:, 13], c.x[:, :, 0], c.x[:, :, 13]))
    if kind == "res_other":
        assert c.res is not c.x and not torch.equal(c.res, c.x)
    # x is signed exactly where the chain takes a ReLU on the way in
    assert bool((c.x < 0).any()) == c.relu_in


def test_chain_weights_are_shared():
    a, b, h = ef.ChainInputs(1, "28a"), ef.ChainInputs(9, "plain"), ef.ChainInputs(1, "28a", "border")
    assert all(torch.equal(getattr(a, k), getattr(b, k)) and torch.equal(getattr(a, k), getattr(h, k)) for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    assert not torch.equal(a.x[0], b.x[0])
    w3m, b3m = a.merged()
    assert tuple(w3m.shape) == (256, 128) and torch.equal(w3m[:, :64], a.w3) and torch.equal(w3m[:, 64:], a.wb) and torch.equal(b3m, a.b3 + a.bb)
    with pytest.raises(AssertionError):
        ef.assert_weight_bits(torch.tensor([256.0]))
    with pytest.raises(AssertionError):
        ef.assert_weight_bits(torch.tensor([0.5]))
    ef.assert_weight_bits(torch.tensor([-255.0, 0.0, 255.0]))


@pytest.mark.parametrize("cin,phases,gemm,n", BETWEEN_CASES)
def test_between_conditions(cin, phases, gemm, n):
    b, out, cap = between_case(cin, phases, gemm, n)
    name = "between Cin %d phases %d gemm %d n %d" % (cin, phases, gemm, n)
    print("%s: largest cap / 2^24 %.2e (%s)" % (name, ef.check_caps(cap, name), max(cap, key=cap.get)))
    ef.check_nondegenerate(out, ("x", "t"), ("V",), name)
    assert all(integers(t) and t.dtype == torch.float64 for t in out.values())
    assert tuple(out["x"].shape) == (n, 7, 7, cin) and tuple(out["V"].shape) == (121, n, cin)


@pytest.mark.parametrize("B,L", ef.FORWARD_SHAPES)
def test_forward_conditions(B, L):
    """fusion@28 on the units' integer outputs: caps of both forms through sb_28 (F(2x2, 3x3): what the fp32 handle's chains run)."""
    _sites, w, out, cap, cap_w = forward_case(B, L)
    name = "forward B %d L %d" % (B, L)
    through_sa = lambda c: max(c[k] for k in ef.THROUGH_SA) / exact.LIMIT   # noqa: E731
    print("%s: largest cap / 2^24 through sa_28 direct %.2e, F(2x2, 3x3) %.2e; through sb_28 direct %.2e, F(2x2, 3x3) %.2e"
          % (name, through_sa(cap), through_sa(cap_w), ef.check_caps(cap, name), ef.check_caps(cap_w, name + " F(2x2, 3x3)")))
    ef.check_nondegenerate(out, ("a_t1", "a_t2", "sa", "b_t1", "b_t2", "sb"), ("x0",), name)
    assert bool((out["x0"] < 0).any()) and all(integers(t) for t in out.values())
    for key in ef.INTEGER_CONVS:
        assert set(np.unique(w[key + ".weight"])) == {-1.0, 0.0, 1.0}, key
    plain = synth.make_weights(spec.VARIANT_RGB)
    assert np.array_equal(w["motion_conv1_trans_28c.weight"], plain["motion_conv1_trans_28c.weight"])


# ---- 2. order independence -------------------------------------------------------------------------------------------------------

def fixed_perm(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).permutation(n))


@pytest.mark.parametrize("name,n,kind,hand", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_chain_order_independence(name, n, kind, hand):
    c, out, _cap, _cap_w = chain_case(n, kind, hand)
    args = (c.x, c.w1, c.b1, c.w2, c.b2, c.w3, c.b3, (c.wb, c.bb) if c.wb is not None else None, c.res, c.relu_in)
    perm = (fixed_perm(c.Cin, 5), fixed_perm(64, 6))
    mm = exact.Mismatches()
    for what, kw in (("as given", {}), ("permuted", {"perm": perm}), ("F(2x2, 3x3)", {"wino": True}), ("F(2x2, 3x3) permuted", {"wino": True, "perm": perm})):
        got = ef.chain_fp32(*args, **kw)
        for k in ("t1", "t2", "y"):
            assert got[k].dtype == torch.float32
            mm.check(got[k], out[k], "%s fp32 %s: %s" % (name, what, k))
    mm.raise_if_any()
    if c.wb is not None:          # the merged form of the fp32 kernel: one contraction over [t2 | x]
        w3m, b3m = c.merged()
        y = torch.relu(torch.cat((out["t2"], c.x.double()), 3) @ w3m.double().t() + b3m.double())
        exact.assert_exact(y, out["y"], name + " merged c3")


@pytest.mark.parametrize("cin,phases,gemm,n", BETWEEN_CASES)
def test_between_order_independence(cin, phases, gemm, n):
    b, out, _cap = between_case(cin, phases, gemm, n)
    mm = exact.Mismatches()
    for what, perm in (("as given", None), ("permuted", fixed_perm(cin, 7))):
        x, t, V = ef.between_fp32(b.M, b.bias, phases, b.w1, b.b1, perm=perm)
        for k, got in (("x", x), ("t", t), ("V", V)):
            assert got.dtype == torch.float32
            mm.check(got, out[k], "between fp32 %s: %s" % (what, k))
    mm.raise_if_any()


@pytest.mark.parametrize("B,L", ef.FORWARD_SHAPES)
def test_forward_order_independence(B, L):
    """The 7x7 / stride 2 conv and both chains in fp32, channels as given and permuted, the 3x3 convs direct and in F(2x2, 3x3) form."""
    sites, w, out, _cap, _cap_w = forward_case(B, L)
    P = B * (L - 1)
    f28 = torch.cat([exact.unit_reference(s, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT)[0]["M"].view(P, 28, 28, exact.UNIT) for s in sites[:2]], 3).float()
    t = lambda k: torch.from_numpy(w[k])   # noqa: E731
    m = lambda k: t(k).reshape(t(k).shape[0], -1)   # noqa: E731
    mm = exact.Mismatches()
    for what, p320, permuted, wino in (("as given", torch.arange(320), False, False), ("permuted", fixed_perm(320, 8), True, False),
                                       ("F(2x2, 3x3)", torch.arange(320), False, True)):
        x0 = F.conv2d(f28[..., p320].permute(0, 3, 1, 2), t("motion_conv_trans_28.weight")[:, p320], t("motion_conv_trans_28.bias"), stride=2,
                      padding=3).permute(0, 2, 3, 1)
        mm.check(x0, out["x0"], "forward fp32 %s: x0" % what)
        pa = {"wino": wino, "perm": (fixed_perm(64, 9), fixed_perm(64, 10)) if permuted else None}
        a = ef.chain_fp32(x0, m("motion_conv1_trans_28a.weight"), t("motion_conv1_trans_28a.bias"), t("motion_conv2_trans_28a.weight"),
                          t("motion_conv2_trans_28a.bias"), m("motion_conv3_trans_28a.weight"), t("motion_conv3_trans_28a.bias"),
                          (m("motion_conv_branch_28a.weight"), t("motion_conv_branch_28a.bias")), None, True, **pa)
        pb = {"wino": wino, "perm": (fixed_perm(256, 11), fixed_perm(64, 12)) if permuted else None}
        b = ef.chain_fp32(a["y"], m("motion_conv1_trans_28b.weight"), t("motion_conv1_trans_28b.bias"), t("motion_conv2_trans_28b.weight"),
                          t("motion_conv2_trans_28b.bias"), m("motion_conv3_trans_28b.weight"), t("motion_conv3_trans_28b.bias"), None, a["y"], False, **pb)
        for k, got in (("a_t1", a["t1"]), ("a_t2", a["t2"]), ("sa", a["y"]), ("b_t1", b["t1"]), ("b_t2", b["t2"]), ("sb", b["y"])):
            mm.check(got, out[k], "forward fp32 %s: %s" % (what, k))
    mm.raise_if_any()


# ---- 3. split-fp32 emulation -----------------------------------------------------------------------------------------------------

def split_is_exact(w, x, what):
    """8 sampled rows of x (of those that are not all zero: the hand-made x) against 8 sampled rows of w: nothing dropped, the emulated
    split dot is the fp64 dot"""
    g = np.random.default_rng(len(what) + w.shape[0] + x.shape[0])
    x = x[(x != 0).any(1)]
    xs = x[g.choice(x.shape[0], 8, replace=False)].float().numpy()
    ws = w[g.choice(w.shape[0], 8, replace=False)].float().numpy()
    ref, dropped, _mag = synth.split_terms(ws, xs)
    assert not dropped.any(), what
    assert bool(ref.any()), what
    assert np.array_equal(synth.emulate_split_dot(ws, xs).astype(np.float64), ref), what


def patches(t1):
    """im2col of the 3x3 / pad 1 conv: [n * 196, 64 * 9] in w2's own (ci, dy, dx) order"""
    return F.unfold(t1.permute(0, 3, 1, 2), 3, padding=1).transpose(1, 2).reshape(-1, t1.shape[3] * 9)


@pytest.mark.parametrize("name,n,kind,hand", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_chain_split_emulation(name, n, kind, hand):
    c, out, _cap, _cap_w = chain_case(n, kind, hand)
    xin = torch.relu(c.x) if c.relu_in else c.x
    split_is_exact(c.w1, xin.reshape(-1, c.Cin), name + " c1")
    split_is_exact(c.w2.reshape(64, 576), patches(out["t1"]), name + " c2")
    split_is_exact(c.w3, out["t2"].reshape(-1, 64), name + " c3")
    if c.wb is not None:
        split_is_exact(c.wb, c.x.reshape(-1, 64), name + " branch")


@pytest.mark.parametrize("cin,phases,gemm,n", [c for c in BETWEEN_CASES if c[2]])
def test_between_split_emulation(cin, phases, gemm, n):
    b, out, _cap = between_case(cin, phases, gemm, n)
    split_is_exact(b.w1, out["x"].reshape(-1, cin), "between 1x1")


@pytest.mark.parametrize("B,L", ef.FORWARD_SHAPES)
def test_forward_split_emulation(B, L):
    """The activations of the forward case reach five digits: top and middle plane, both kept against an 8-bit weight."""
    _sites, w, out, _cap, _cap_w = forward_case(B, L)
    m = lambda k: torch.from_numpy(w[k]).reshape(w[k].shape[0], -1)   # noqa: E731
    assert float(out["sa"].max()) > 256
    split_is_exact(m("motion_conv1_trans_28a.weight"), torch.relu(out["x0"]).reshape(-1, 64), "28a c1")
    split_is_exact(m("motion_conv2_trans_28a.weight"), patches(out["a_t1"]), "28a c2")
    split_is_exact(m("motion_conv3_trans_28a.weight"), out["a_t2"].reshape(-1, 64), "28a c3")
    split_is_exact(m("motion_conv_branch_28a.weight"), out["x0"].reshape(-1, 64), "28a branch")
    split_is_exact(m("motion_conv1_trans_28b.weight"), out["sa"].reshape(-1, 256), "28b c1")
    split_is_exact(m("motion_conv2_trans_28b.weight"), patches(out["b_t1"]), "28b c2")
    split_is_exact(m("motion_conv3_trans_28b.weight"), out["b_t2"].reshape(-1, 64), "28b c3")


# ---- 4. sensitivity --------------------------------------------------------------------------------------------------------------

def first_where(mask):
    return tuple(int(i) for i in mask.nonzero()[0])


@pytest.mark.parametrize("kind", ["28a", "res"])
def test_one_dropped_product_is_seen(kind):
    c, out, _cap, _cap_w = chain_case(5, kind, None)
    w2, w3 = c.w2.double(), c.w3.double()
    # c2: one (pixel, channel, tap) term of an output the ReLU passes
    tp = F.pad(out["t1"], (0, 0, 1, 1, 1, 1))
    pre2 = ef.conv3x3(out["t1"], w2) + c.b2.double()
    img, y, x, co = first_where(pre2 > 0)
    ci, dy, dx = first_where((w2[co] != 0) & (tp[img, y:y + 3, x:x + 3].permute(2, 0, 1) != 0))
    term = float(w2[co, ci, dy, dx] * tp[img, y + dy, x + dx, ci])
    assert abs(term) >= 1 and term == round(term)
    t2 = out["t2"].clone()
    t2[img, y, x, co] = max(float(pre2[img, y, x, co]) - term, 0.0)
    with pytest.raises(AssertionError, match="1 of %d elements differ" % t2.numel()):
        exact.assert_exact(t2.float(), out["t2"], "c2 without one term")
    # ... and one Winograd-domain product U V of the same output: a multiple of 1/4
    u = torch.einsum("pa,ab,qb->pq", torch.from_numpy(ef.W2_G), w2[co, ci], torch.from_numpy(ef.W2_G))
    ty, tx = y // 2, x // 2
    v = torch.from_numpy(ef.W2_BT) @ tp[img, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4, ci] @ torch.from_numpy(ef.W2_BT).t()
    at = torch.from_numpy(ef.W2_AT)
    seen = 0
    for p in range(4):
        for q in range(4):
            lost = float(at[y % 2, p] * at[x % 2, q] * u[p, q] * v[p, q])
            if lost != 0.0:
                assert abs(lost) >= ef.GRANULE_WINO and lost * 4 == round(lost * 4)
                t2w = out["t2"].clone()
                t2w[img, y, x, co] = max(float(pre2[img, y, x, co]) - lost, 0.0)
                with pytest.raises(AssertionError, match="1 of"):
                    exact.assert_exact(t2w.float(), out["t2"], "c2 without one Winograd-domain product")
                seen += 1
    assert seen > 0
    # c3: one K-element
    row, co = first_where(out["y"].reshape(-1, 256) > 0)
    k = first_where((w3[co] != 0) & (out["t2"].reshape(-1, 64)[row] != 0))[0]
    term = float(w3[co, k] * out["t2"].reshape(-1, 64)[row, k])
    assert abs(term) >= 1
    yy = out["y"].clone().reshape(-1, 256)
    yy[row, co] = max(float(yy[row, co]) - term, 0.0)
    with pytest.raises(AssertionError, match="1 of"):
        exact.assert_exact(yy.float(), out["y"].reshape(-1, 256), "c3 without one K-element")


def test_one_dropped_transform_point_is_seen():
    b, out, _cap = between_case(128, 1, True, 5)
    # x[img, 1, 2, c] (class 0, 0; output row 1, column 2) = sum_ij A^T[1, i] A^T[2, j] M[point (i, j)]: lose one nonzero point
    img, c = first_where(out["x"][:, 1, 2] > 0)
    at = torch.from_numpy(ef._AT[4])
    i, j = next((i, j) for i in range(6) for j in range(6) if at[1, i] * at[2, j] * b.M[ef._mindex(1, 0, 0, i, j), img, c] != 0)
    term = float(at[1, i] * at[2, j] * b.M[ef._mindex(1, 0, 0, i, j), img, c])
    assert abs(term) >= 1
    x = out["x"].clone()
    x[img, 1, 2, c] = max(float(x[img, 1, 2, c]) - term, 0.0)
    with pytest.raises(AssertionError, match="1 of %d elements differ" % x.numel()):
        exact.assert_exact(x.float(), out["x"], "x without one point")
    # and V sees a one-off x through the 1x1 conv wherever w1 is nonzero
    t = torch.relu(x @ b.w1.double().t() + b.b1.double())
    assert not torch.equal(ef.input_transform(t), out["V"])
