"""The integer inputs of tests/exact_wino.py on the CPU: what the exact Winograd GPU tests (tests/test_gpu_exact_wino.py) stand on.

For every case the GPU file uses (the stage-entry cases of the three convs, the forward shapes):

1. The transforms: each (B^T, G, A^T) is a Winograd algorithm in exact fractions; tap_scales are the least integers; the point
   numbering is tests/wino_ref.py's (held to its two earlier spellings by tests/test_forward_checks.py).
2. The direct fp64 reference equals the Winograd restatement value for value; every cap of every exact stage is below 2^24 (printed
   per case); the ReLU zeroes 5 % .. 95 %; at least 8 distinct values.
3. U in fp32 the way the device computes it -- constant times value, both pass orders, plain and fused with a zero addend -- equals
   the exact U; U has at most 8 significant bits wherever a split-fp32 GEMM reads it (3x3, 5x5 / 2; F(5, 4): fp32 only, <= 24 bits).
4. Order independence: the restatement in fp32 torch CPU ops, channels as given and permuted, equals fp64.
5. Sensitivity (3x3, 5x5 / 2): a dropped (point, phase) product, a dropped 32-channel K-tile at one point and a shifted class offset of
   the point numbering each change at least one output.
6. F(5x5, 4x4): V and M exact in units of 1/16, the output transform's cap in units of 1/4096 far above 2^24 (why it gets a bound), and
   the bound is concrete: it is smaller than what a lost (point, phase) product moves an output by.
"""
from fractions import Fraction as Fr
from itertools import product

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec

from . import exact
from . import exact_wino as ew
from .wino_ref import mindex as _mindex

_CACHE = {}
CASES = [(k,) + c for k in (3, 5, 7) for c in ew.conv_cases(k)]
CASE_IDS = ["k%d-%s" % (c[0], c[1]) for c in CASES]
EXACT_CASES = [c for c in CASES if c[0] != 7]
EXACT_IDS = ["k%d-%s" % (c[0], c[1]) for c in EXACT_CASES]


def conv_case(k, ci, co, n, signed, hand):
    key = (k, ci, co, n, signed, hand)
    if key not in _CACHE:
        _CACHE[key] = ew.ConvInputs(k, ci, co, n, signed, hand)
    return _CACHE[key]


def forward_case(B, L):
    key = ("forward", B, L)
    if key not in _CACHE:
        sites = [exact.SiteInputs(si, B, L, spec.VARIANT_RGB) for si in range(spec.NUM_SITES)]
        w = ew.forward_weights(spec.VARIANT_RGB, sites)
        _CACHE[key] = (sites, w) + ew.forward_reference(sites, w, B, L, spec.VARIANT_RGB)
    return _CACHE[key]


def fixed_perm(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).permutation(n))


# ---- 1. the transforms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("npts", [6, 5, 8])
def test_transforms_are_winograd_algorithms(npts):
    """A^T [(G g) (.) (B^T d)] = the correlation y[o] = sum_u g[u] d[o + u], in exact fractions, on a basis of g and d"""
    outs, taps = ew.OUTPUTS[npts], ew.TAPS[npts]
    assert outs + taps - 1 == npts
    bt = [[Fr(float(v)) for v in row] for row in ew.BT[npts]]
    at = [[Fr(float(v)) for v in row] for row in ew.AT[npts]]
    g = [[Fr(v) for v in row] for row in ew.G[npts]]
    for u, i in product(range(taps), range(npts)):
        gg = [Fr(int(t == u)) for t in range(taps)]
        dd = [Fr(int(t == i)) for t in range(npts)]
        U = [sum(g[p][t] * gg[t] for t in range(taps)) for p in range(npts)]
        V = [sum(bt[p][t] * dd[t] for t in range(npts)) for p in range(npts)]
        for o in range(outs):
            assert sum(at[o][p] * U[p] * V[p] for p in range(npts)) == sum(gg[t] * dd[o + t] for t in range(taps)), (npts, u, i, o)


def test_tap_scales_are_the_least_integers():
    """Computed from G: every column a tap lands in becomes integer, and no proper divisor of the scale does that in every class."""
    assert ew.tap_scales(3) == [24, 12, 6] and ew.tap_scales(5) == [24, 24, 12, 12, 6] and ew.tap_scales(7) == [90, 45, 45, 45, 45, 45, 45]
    for k in (3, 5, 7):
        sc, classes = ew.tap_scales(k), ((8,) if k == 7 else (6, 5))
        seen = set()
        for a in ((0,) if k == 3 else (0, 1)):
            for u, kh in ew.phase_taps(k, a):
                seen.add(kh)
                clears = lambda d: all((Fr(row[u]) * d).denominator == 1 for npts in classes for row in ew.G[npts])   # noqa: E731
                assert clears(sc[kh])
                assert not any(clears(d) for d in range(1, sc[kh]) if sc[kh] % d == 0), (k, kh)
        assert seen == set(range(k))             # every tap belongs to exactly one phase


def test_point_numbering_is_the_shared_one():
    for phases in (1, 4):
        seen = set()
        for cy, cx, ny, nx, _oy, _ox in ew.classes():
            for i in range(ny):
                for j in range(nx):
                    assert ew.mindex(phases, cy, cx, i, j) == _mindex(phases, cy, cx, i, j)
                    seen.add(ew.mindex(phases, cy, cx, i, j))
        assert seen == set(range(121))
    # the live (point, phase) products: 400 of 484 and 225 of 256
    assert sum(ew.live_product(5, ny, nx, i, j, a, b) for _cy, _cx, ny, nx, _oy, _ox in ew.classes() for i in range(ny) for j in range(nx)
               for a in (0, 1) for b in (0, 1)) == 400
    assert sum(ew.live_product(7, 8, 8, p, q, a, b) for p in range(8) for q in range(8) for a in (0, 1) for b in (0, 1)) == 225


def test_single_tap_weights():
    w = ew.single_tap_weights(3, 64, 32, 3, 8, 3)
    assert tuple(w.shape) == (64, 32, 3, 3) and int((w != 0).sum()) == 512
    assert int((w != 0).any(3).any(2).sum(1).min()) == 8                       # eight distinct input channels per output channel
    sc = torch.tensor(ew.tap_scales(3), dtype=torch.float32)
    c = w / (sc[:, None] * sc[None, :])
    assert bool((c == c.round()).all()) and float(c.abs().max()) == 3 and bool((w < 0).any()) and bool((w > 0).any())
    live = ew.single_tap_weights(3, 256, 832, 3, 4, 3, live_ci=range(320))
    assert bool((live[:, 320:] == 0).all()) and bool((live[:, :320] != 0).any(3).any(2).any(0).all())
    with pytest.raises(AssertionError, match="not used"):
        ew.single_tap_weights(3, 64, 320, 7, 2, 3)
    assert ew.significant_bits([0.0, 96.0, 255.0, 432.0]) == 8 and ew.significant_bits([2025.0]) == 11 and ew.significant_bits([0.75]) == 2


# ---- 2. direct = Winograd restatement, caps, non-degeneracy ----------------------------------------------------------------------------

def forms_of(k):
    return ew.FORMS3 if k == 3 else ew.FORMS3[:2]


@pytest.mark.parametrize("k,name,ci,co,n,signed,hand", EXACT_CASES, ids=EXACT_IDS)
def test_exact_case_conditions(k, name, ci, co, n, signed, hand):
    c = conv_case(k, ci, co, n, signed, hand)
    worst, zero = {}, []
    for form, flags, with_res in forms_of(k):
        res = c.res if with_res else None
        y, pre, cdir = ew.direct_reference(c.x, c.w, c.bias, k, flags, res)
        out, cap = ew.f43_reference(c.x, c.w, c.bias, k, flags, res)
        exact.assert_exact(out["y"], y, "%s %s: restatement against direct" % (name, form))
        exact.assert_exact(out["pre"], pre, "%s %s: pre-epilogue" % (name, form))
        assert torch.equal(out["pool"], ew.tile_sums(y))
        ew.check_caps(dict(cap, direct=cdir), "%s %s" % (name, form))
        for s, v in cap.items():
            worst[s] = max(worst.get(s, 0.0), v / exact.LIMIT)
        assert all(bool((t == t.round()).all()) for t in (out["M"], out["y"]))
        if flags and hand is None:
            ew.check_nondegenerate({"y": y}, ("y",), (), "%s %s" % (name, form))
            zero.append(float((y == 0).double().mean()))
        elif hand is None:
            ew.check_nondegenerate({"y": y}, (), ("y",), "%s %s" % (name, form))
    print("k %d %s (%d taps): largest cap / 2^24 %s; the ReLU zeroes %s" % (k, name, c.taps, " ".join("%s %.2e" % kv for kv in worst.items()),
                                                                             " ".join("%.2f" % z for z in zero)))
    assert bool((c.x < 0).any()) == signed
    m = ew.hand_mask(k, hand) if hand else None
    if hand:
        assert bool((c.x[:, m == 0] == 0).all()) and bool((c.x[:, m == 1] != 0).any())
    if hand == "seam" and k == 3:
        assert float(m.sum()) == 2 * 7 + 2 * 7 - 4 and bool(m[3].all()) and bool(m[:, 4].all()) and m[0, 0] == 0
    if hand == "seam" and k == 5:
        assert bool(m[6:10].all()) and bool(m[:, 6:10].all()) and m[5, 5] == 0 and m[10, 10] == 0
    if hand in ("odd", "even"):
        a = 1 if hand == "odd" else 0
        assert float(m.sum()) == 49 and bool(m[a::2, a::2].all())


@pytest.mark.parametrize("B,L", ew.FORWARD_SHAPES)
def test_forward_conditions(B, L):
    """x1 and x2 of the forward on the units' integer outputs: direct = restatement (asserted inside forward_reference), caps, the ReLU's
    share, weight bits, where the weights live."""
    _sites, w, out, cap = forward_case(B, L)
    name = "forward B %d L %d" % (B, L)
    worst = ew.check_caps(cap, name)
    print("%s: largest cap / 2^24 %.2e; %s; unit outputs reach %.0f; the ReLU zeroes x1 %.2f x2 %.2f"
          % (name, worst, " ".join("%s %.2e" % (k, v / exact.LIMIT) for k, v in cap.items() if k[0] == "x"), float(out["f7"].abs().max()),
             float((out["x1"] == 0).double().mean()), float((out["x2"] == 0).double().mean())))
    ew.check_nondegenerate(out, ("x1", "x2"), ("x1_pre", "x2_pre"), name)
    assert tuple(out["x1"].shape) == (B * (L - 1), 7, 7, 128) and tuple(out["x2"].shape) == (B * (L - 1), 7, 7, 256)
    for key, (k, live, taps) in ew.FORWARD_CONVS.items():
        wt = torch.from_numpy(w[key + ".weight"])
        assert bool((wt[:, live:] == 0).all()) and bool((wt[:, :live] != 0).any(3).any(2).any(0).all())
        assert int((wt != 0).any(3).any(2).sum(1).min()) == taps == int((wt != 0).any(3).any(2).sum(1).max())
        b = w[key + ".bias"]
        assert np.array_equal(b, np.round(b)) and np.abs(b).max() <= 3 and np.abs(b).max() > 0


# ---- 3. U in fp32, the way the device computes it ---------------------------------------------------------------------------------------

def u_checks(w, k, what, split):
    """Every class and phase: the fp32 weight transform of the single taps, both pass orders, plain and fused, against the exact U;
    returns the largest number of significant bits of U."""
    bits = 0
    z = torch.zeros(())
    for a, b in (((0, 0),) if k == 3 else product((0, 1), (0, 1))):
        g = ew.phase_kernel(w, k, a, b)
        o, c, u, v = (g != 0).nonzero(as_tuple=True)
        val = g[o, c, u, v]
        assert val.dtype == torch.float32
        for ny, nx in (((8, 8),) if k == 7 else product((6, 5), (6, 5))):
            ue = ew.exact_u(g, ny, nx)
            want = ue[:, :, o, c].permute(2, 0, 1)
            bits = max(bits, ew.significant_bits(ue.numpy()))
            ga = torch.from_numpy(ew.g_float(ny).astype(np.float32))[:, u].t()          # [taps, ny]: the fp32 constants of column u
            gb = torch.from_numpy(ew.g_float(nx).astype(np.float32))[:, v].t()
            forms = {"columns first": (val[:, None] * ga)[:, :, None] * gb[:, None, :],
                     "rows first": ga[:, :, None] * (val[:, None] * gb)[:, None, :],
                     "columns first, fused": torch.addcmul(z, torch.addcmul(z, val[:, None], ga)[:, :, None], gb[:, None, :]),
                     "rows first, fused": torch.addcmul(z, ga[:, :, None], torch.addcmul(z, val[:, None], gb)[:, None, :])}
            for form, got in forms.items():
                assert got.dtype == torch.float32
                assert torch.equal(got.double(), want), "%s phase (%d, %d) class %d x %d: fp32 U (%s) is not the exact U" % (what, a, b, ny, nx, form)
    if split:
        assert bits <= 8, "%s: U has %d significant bits" % (what, bits)
    assert bits <= 24
    return bits


@pytest.mark.parametrize("k,ci,co", [(k, ci, co) for k in (3, 5, 7) for ci, co in ew.SHAPES[k]])
def test_u_fp32_is_exact(k, ci, co):
    c = conv_case(k, ci, co, 1, False, None)
    bits = u_checks(c.w, k, "k %d %d -> %d" % (k, ci, co), split=k != 7)
    print("k %d %d -> %d: U has at most %d significant bits" % (k, ci, co, bits))
    assert (bits > 8) == (k == 7)              # F(5, 4): 45 x 45 = 2025 is 11 bits; its stage entry runs fp32 GEMMs only


def test_u_fp32_is_exact_forward_weights():
    _sites, w, _out, _cap = forward_case(1, 2)
    for key, (k, _live, _taps) in ew.FORWARD_CONVS.items():
        u_checks(torch.from_numpy(w[key + ".weight"]), k, key, split=True)


# ---- 4. order independence ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,name,ci,co,n,signed,hand", CASES, ids=CASE_IDS)
def test_order_independence(k, name, ci, co, n, signed, hand):
    """fp32 torch CPU ops, channels as given and permuted: 3x3 and 5x5 / 2 every stage against fp64; 7x7 / 2: M (exact), not y."""
    c = conv_case(k, ci, co, n, signed, hand)
    mm = exact.Mismatches()
    if k == 7:
        ref, _cap = ew.f54_reference(c.x, c.w, c.bias)
        for what, perm in (("as given", None), ("permuted", fixed_perm(ci, 5))):
            got, _ = ew.f54_reference(c.x, c.w, c.bias, dtype=torch.float32, perm=perm)
            mm.check(got["M"], ref["M"], "%s fp32 %s: M" % (name, what))
    else:
        flags, res = (ew.RELU_PRE | ew.RELU_POST, c.res) if k == 3 else (ew.RELU_PRE, None)
        ref, _cap = ew.f43_reference(c.x, c.w, c.bias, k, flags, res)
        for what, perm in (("as given", None), ("permuted", fixed_perm(ci, 5))):
            got, _ = ew.f43_reference(c.x, c.w, c.bias, k, flags, res, dtype=torch.float32, perm=perm)
            for s in ("M", "pre", "y", "pool"):
                assert got[s].dtype == torch.float32
                mm.check(got[s], ref[s], "%s fp32 %s: %s" % (name, what, s))
    mm.raise_if_any()


@pytest.mark.parametrize("B,L", ew.FORWARD_SHAPES)
def test_forward_order_independence(B, L):
    _sites, w, out, _cap = forward_case(B, L)
    mm = exact.Mismatches()
    for name, key, src in (("x1", "motion_conv_trans_14", "f14"), ("x2", "motion_conv_trans", "f7")):
        k, live, _taps = ew.FORWARD_CONVS[key]
        wt, bt = torch.from_numpy(w[key + ".weight"])[:, :live], torch.from_numpy(w[key + ".bias"])
        for what, perm in (("as given", None), ("permuted", fixed_perm(live, 6))):
            got, _ = ew.f43_reference(out[src].float(), wt, bt, k, ew.RELU_PRE, dtype=torch.float32, perm=perm)
            mm.check(got["y"], out[name], "forward fp32 %s: %s" % (what, name))
    mm.raise_if_any()


# ---- 5. sensitivity ----------------------------------------------------------------------------------------------------------------

def differs(c, k, ref, mutate):
    got, _ = ew.f43_reference(c.x, c.w, c.bias, k, mutate=mutate)
    try:
        exact.assert_exact(got["y"], ref, "mutated")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("k", [3, 5])
def test_lost_terms_are_seen(k):
    """On the smallest shape at n = 1.  Every live (point, phase) product has a nonzero term in some output (y is linear in M here: no
    ReLU); the restatement run WITHOUT a product -- 3x3: each of the 121; 5x5 / 2: an inner point, a last-row, a last-column and the
    corner point of every class and phase, which is every K group -- without a K-tile at an inner point of every class and phase, and
    with each class offset of each table shifted by one differs from the reference in at least one output."""
    ci, co = ew.SHAPES[k][0]
    c = conv_case(k, ci, co, 1, False, None)
    out, _cap = ew.f43_reference(c.x, c.w, c.bias, k)
    ref = out["y"]
    phases = 1 if k == 3 else 4
    products = 0
    for cy, cx, ny, nx, _oy, _ox in ew.classes():
        cls = 2 * cy + cx
        at_y, at_x = torch.from_numpy(ew.AT[ny]), torch.from_numpy(ew.AT[nx])
        for ph in range(phases):
            ends = {(1, 1), (ny - 1, 1), (1, nx - 1), (ny - 1, nx - 1)}
            for i in range(ny):
                for j in range(nx):
                    if not ew.live_product(k, ny, nx, i, j, ph >> 1, ph & 1):
                        assert bool((out["Mph"][(cls, ph)][i, j] == 0).all())
                        continue
                    products += 1
                    assert bool((out["Mph"][(cls, ph)][i, j] != 0).any()) and bool((at_y[:, i] != 0).any()) and bool((at_x[:, j] != 0).any())
                    if k == 3 or (i, j) in ends:
                        assert differs(c, k, ref, {"drop_product": (cls, i, j, ph)}), "a lost product goes unseen: class %d point (%d, %d) phase %d" % (cls, i, j, ph)
            assert differs(c, k, ref, {"drop_ktile": (cls, 1, 1, ph, 0)}), "a lost K-tile goes unseen: class %d phase %d" % (cls, ph)
    assert products == (121 if k == 3 else 400)
    for table in (("off1",) if k == 3 else ("offA", "offB", "offC")):
        for cls in (1, 2, 3):
            offs = dict(ew.OFFSETS)
            shift = -1 if (table, cls) == ("off1", 3) else 1               # (off1[3] + 1 would leave the 121 points)
            offs[table] = tuple(v + (shift if q == cls else 0) for q, v in enumerate(offs[table]))
            assert differs(c, k, ref, {"offsets": offs}), "a shifted %s[%d] goes unseen" % (table, cls)
    assert not differs(c, k, ref, {})


def test_lost_ktile_is_seen_at_the_widest_conv():
    """832 -> 256: one 32-channel K-tile at one of the 121 points (1/26 of one point's contribution)"""
    c = conv_case(3, 832, 256, 1, False, None)
    ref, _cap = ew.f43_reference(c.x, c.w, c.bias, 3)
    for k0 in (0, 416, 800):
        assert differs(c, 3, ref["y"], {"drop_ktile": (3, 2, 2, 0, k0)})


# ---- 6. F(5x5, 4x4): exact through M, a derived bound behind it -----------------------------------------------------------------------

SEVEN = [c for c in CASES if c[0] == 7]


@pytest.mark.parametrize("k,name,ci,co,n,signed,hand", SEVEN, ids=[c[1] for c in SEVEN])
def test_f54_conditions(k, name, ci, co, n, signed, hand):
    c = conv_case(7, ci, co, n, False, None)
    assert set(c.x.unique().tolist()) == {0.0, 1.0} and 0.10 < float(c.x.mean()) < 0.15
    out, cap = ew.f54_reference(c.x, c.w, c.bias)
    y, _pre, cdir = ew.direct_reference(c.x, c.w, c.bias, 7)
    assert torch.equal(out["y"], y), "the restatement is not the direct conv"        # (fp64 holds the 1/4096 granule of these magnitudes exactly)
    assert bool((out["M"] * 16 == (out["M"] * 16).round()).all())
    worst = ew.check_caps({"V": cap["V"], "M": cap["M"], "direct": cdir}, name)
    assert cap["y"] > 16 * exact.LIMIT            # the output transform cannot be exact: the granule is 1/4096, the terms reach 16 M
    relu = torch.relu(y)
    ew.check_nondegenerate({"y": relu}, ("y",), (), name)
    # the bound is concrete: without any one live (point, phase) product some output leaves it
    count, guard = ew.product_reach(out["Mph"], out["bound_terms"])
    live = torch.tensor([[[ew.live_product(7, 8, 8, p, q, ph >> 1, ph & 1) for q in range(8)] for p in range(8)] for ph in range(4)])
    assert int(live.sum()) == 225 and bool((guard[~live] == 0).all())
    print("7x7 / 2 %s (%d taps): V %.2e M %.2e of 2^24 in units of 1/16 (largest %.2e), y %.0f x 2^24 in units of 1/4096; largest bound %.2e; "
          "a lost (point, phase) product / bound at its best output: min %.0f, median %.0f; outputs with one product: %d; the ReLU zeroes %.2f"
          % (name, c.taps, cap["V"] / exact.LIMIT, cap["M"] / exact.LIMIT, worst, cap["y"] / exact.LIMIT, float((ew.GAMMA_K_F54 * out["bound_terms"]).max()),
             float(guard[live].min()), float(guard[live].median()), int((count == 1).sum()), float((relu == 0).double().mean())))
    assert float(guard[live].min()) > 100.0
