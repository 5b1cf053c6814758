"""Exact integer-input tests of the Winograd convolutions: winograd.hip (F(4, 3) x F(3, 3) on 7x7 maps, the polyphase 5x5 / stride 2
form), winograd7.hip (the polyphase F(5x5, 4x4) form of the 7x7 / stride 2 conv) and the handle's Winograd launches.

Until this module these kernels were held to a tolerance alone (2e-4 of the largest magnitude, a multiple of 2^-24 sum |w x| on
heavy-tailed data), which cannot see a lost term: a skipped (point, phase) product, a wrong class offset of the point numbering, a
32-channel K-tile dropped at one of 121 points.  Here the weights are the single scaled taps of tests/exact_wino.py, so that U = G g G^T
is an integer the fp32 weight transform computes exactly, and every stage (V, M, Y) is a sum of integers below 2^24 -- asserted on the
CPU by tests/test_exact_wino_inputs.py together with the sensitivity of the reference to each such fault.

  1. offk_winograd_conv3x3 == fp64: five shapes, n = 1, 5, 67, x in 0..3 and -3..3, the plain / ReLU / 14b (ReLU, residual, ReLU)
     epilogues, the per-tile pool sums, channel slices inside a guarded arena, x on the F(4, 3) / F(3, 3) seam and on the border.
  2. offk_winograd_conv5x5s2 == fp64: three shapes, n = 1, 5, 67, slices, x with one live phase (odd / even) and on the seam.
  3. offk_winograd_conv7x7s2: V and M are exact (CPU file), A^T runs from 1/16 to 16, so Y is held to the derived bound
     |got - ref| <= gamma_k (|A|^T |M| |A| + |bias|) per element and nothing else.  k = 6 + 6 + 1, counted from wino7_output_kernel:
     at5x8's longest chains are s[0] (seven terms, six additions) and s[4] (one addition, four fmaf, one addition) -- the products
     inside an fmaf are not rounded and every coefficient is a power of two -- so a term passes at most 6 roundings per pass, twice, and
     the bias add is one more; max(., 0) rounds nothing and is 1-Lipschitz.  No measured slack.
  4. offk_forward on exact.SiteInputs with single-tap motion_conv_trans_14 / motion_conv_trans: x1 in xu_14 and x2 in xv_7 == fp64 in
     fp32 and split-fp32 handles under the polyphase form forced on, without wino_mid, without the persistent GEMM, and direct.

No tolerance anywhere in parts 1, 2 and 4.  Outputs are filled with NaN (or carved from the arena's NaN sentinel) before every launch.
"""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec

from . import exact
from . import exact_wino as ew
from .arena import Arena
from .featmaps import rt  # noqa: F401

pytestmark = pytest.mark.gpu
NAN = float("nan")
_REF = {}


def dev(t):
    return None if t is None else t.cuda()


def conv_case(k, ci, co, n, signed, hand):
    """(inputs, pre-epilogue fp64 reference of the direct form): computed once, never written to; the caps of the Winograd stages (with
    the residual where the conv has one) and of the direct form are checked first"""
    key = (k, ci, co, n, signed, hand)
    if key not in _REF:
        c = ew.ConvInputs(k, ci, co, n, signed, hand)
        _y, pre, cdir = ew.direct_reference(c.x, c.w, c.bias, k, 0, c.res)
        out, cap = ew.f43_reference(c.x, c.w, c.bias, k, 0, c.res)
        assert torch.equal(out["pre"], pre), "the Winograd restatement is not the direct conv"
        ew.check_caps(dict(cap, direct=cdir), str(key))
        _REF[key] = (c, pre)
    return _REF[key]


def forms_of(k):
    return ew.FORMS3 if k == 3 else ew.FORMS3[:2]


def reference(c, pre, flags, with_res):
    """(y, pool) of one form in fp64; the pool sums stay below 2^24 as well"""
    y = ew.epilogue(pre, flags, c.res.double() if with_res else None)
    assert float(ew.tile_sums(y.abs()).max()) < exact.LIMIT
    return y, ew.tile_sums(y)


def run_case(rt, k, name, ci, co, n, signed, hand):
    c, pre = conv_case(k, ci, co, n, signed, hand)
    H = 7 if k == 3 else 14
    x, w, b = dev(c.x), dev(c.w), dev(c.bias)
    wp = rt.pack_conv_weight(w)
    mm = exact.Mismatches()
    for form, flags, with_res in forms_of(k):
        ref, pool_ref = reference(c, pre, flags, with_res)
        y = torch.full((n, 7, 7, co), NAN, device="cuda")
        if k == 3:
            pool = torch.full((4 * n, co), NAN, device="cuda")
            rt.winograd_conv3x3(x, w, b, res=dev(c.res) if with_res else None, flags=flags, y=y, want_pool=True, w_packed=wp, pool=pool)
            torch.cuda.synchronize()
            mm.check(pool.cpu(), pool_ref, "3x3 %s %s: pool_part" % (name, form))
        else:
            rt.winograd_conv5x5s2(x, w, b, flags=flags, y=y, w_packed=wp)
            torch.cuda.synchronize()
        mm.check(y.cpu(), ref, "%dx%d %s %s" % (k, k, name, form))
    if hand is None:
        # the last form again with the input at channel 32 of a wider buffer and the output at channel 64, every buffer carved from a guarded arena
        form, flags, with_res = forms_of(k)[-1]
        ref, _pool = reference(c, pre, flags, with_res)
        sizes = [n * H * H * (ci + 64) * 4, n * 49 * (co + 96) * 4, co * 4, n * 49 * co * 4]
        ar = Arena.for_sizes(sizes)
        xw = ar.empty("x", (n, H, H, ci + 64))
        xw[..., 32:32 + ci] = x
        yw = ar.empty("y", (n, 7, 7, co + 96))
        ba = ar.put("bias", b)
        if k == 3:
            rt.winograd_conv3x3(xw, w, ba, res=ar.put("res", dev(c.res)) if with_res else None, flags=flags, x_coff=32, y=yw, y_coff=64, w_packed=wp)
        else:
            rt.winograd_conv5x5s2(xw, w, ba, flags=flags, x_coff=32, y=yw, y_coff=64, w_packed=wp)
        torch.cuda.synchronize()
        mm.check(yw[..., 64:64 + co].cpu(), ref, "%dx%d %s %s at x_coff 32, y_coff 64" % (k, k, name, form))
        ar.check()
        assert ar.untouched(yw[..., :64]) and ar.untouched(yw[..., 64 + co:]), "the output's neighbour channels were written"
        assert ar.untouched(xw[..., :32]) and ar.untouched(xw[..., 32 + ci:]) and torch.equal(xw[..., 32:32 + ci], x)
    mm.raise_if_any()


# ---- 1. offk_winograd_conv3x3 ------------------------------------------------------------------------------------------------------

CASES3 = ew.conv_cases(3)


@pytest.mark.parametrize("name,ci,co,n,signed,hand", CASES3, ids=[c[0] for c in CASES3])
def test_winograd_conv3x3_exact(rt, name, ci, co, n, signed, hand):
    """Every form of the epilogue and the per-tile sums, value for value: n = 1 (one image), 5 (a partial 64-row GEMM tile), 67 (one past
    a tile); (32, 64) is the smallest shape the entry takes, the other four are the forward's."""
    run_case(rt, 3, name, ci, co, n, signed, hand)


# ---- 2. offk_winograd_conv5x5s2 ----------------------------------------------------------------------------------------------------

CASES5 = ew.conv_cases(5)


@pytest.mark.parametrize("name,ci,co,n,signed,hand", CASES5, ids=[c[0] for c in CASES5])
def test_winograd_conv5x5s2_exact(rt, name, ci, co, n, signed, hand):
    """The polyphase form: 400 live (point, phase) products in four K groups.  'odd' / 'even': one live phase -- with the skipped
    phase-points a wrong slot or kmul of a group shows here and nowhere else; 'seam': phase rows and columns 3 and 4."""
    run_case(rt, 5, name, ci, co, n, signed, hand)


# ---- 3. offk_winograd_conv7x7s2: the derived output-transform bound ------------------------------------------------------------------

CASES7 = ew.conv_cases(7)


def seven_case(ci, co, n):
    key = (7, ci, co, n)
    if key not in _REF:
        c = ew.ConvInputs(7, ci, co, n)
        out, cap = ew.f54_reference(c.x, c.w, c.bias)
        y, _pre, cdir = ew.direct_reference(c.x, c.w, c.bias, 7)
        assert torch.equal(out["y"], y), "the F(5x5, 4x4) restatement is not the direct conv"
        ew.check_caps({"V": cap["V"], "M": cap["M"], "direct": cdir}, str(key))           # the premise: M is exact on the device
        count, guard = ew.product_reach(out["Mph"], out["bound_terms"])
        _REF[key] = (c, y, ew.GAMMA_K_F54 * out["bound_terms"], count, guard)
    return _REF[key]


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("name,ci,co,n,signed,hand", CASES7, ids=[c[0] for c in CASES7])
def test_winograd_conv7x7s2_output_transform_bound(rt, name, ci, co, n, signed, hand, relu):
    """|got - ref| <= gamma_13 (|A|^T |M_ref| |A| + |bias|) at every element (n = 8: 72 GEMM rows, past the 64-row tile).  Without any one
    of the 225 live (point, phase) products some output misses the bound by the printed factor; where an output has a single product
    behind it, nothing but the bias add rounds and it must be the fp32 nearest to the reference."""
    c, y, bound, count, guard = seven_case(ci, co, n)
    ref = torch.relu(y) if relu else y
    got = torch.full((n, 14, 14, co), NAN, device="cuda")
    rt.winograd_conv7x7s2(dev(c.x), dev(c.w), dev(c.bias), flags=ew.RELU_PRE if relu else 0, y=got)
    torch.cuda.synchronize()
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    live = guard > 0
    print("7x7 / 2 %s relu %d: largest |got - ref| / bound %.3f (largest error %.2e, largest bound %.2e); a lost (point, phase) product would "
          "miss the bound by a factor >= %.0f; %d outputs with a single product"
          % (name, relu, float((err / bound.clamp_min(1e-300)).max()), float(err.max()), float(bound.max()), float(guard[live].min()), int((count == 1).sum())))
    assert int(live.sum()) == 225 and float(guard[live].min()) > 100.0
    bad = err > bound
    assert not bool(bad.any()), "%d of %d elements outside the derived bound; first %s: got %r, reference %r, bound %r" % (
        int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist()), float(got[bad][0]), float(ref[bad][0]), float(bound[bad][0]))
    one = count == 1
    assert torch.equal(got[one], ref[one].float().double())


# ---- 4. the forward ------------------------------------------------------------------------------------------------------------------

def forward_case(B, L):
    key = ("forward", B, L)
    if key not in _REF:
        sites = [exact.SiteInputs(si, B, L, spec.VARIANT_RGB) for si in range(spec.NUM_SITES)]
        w = ew.forward_weights(spec.VARIANT_RGB, sites)
        out, cap = ew.forward_reference(sites, w, B, L, spec.VARIANT_RGB)
        ew.check_caps(cap, str(key))
        ew.check_nondegenerate(out, ("x1", "x2"), ("x1_pre", "x2_pre"), str(key))
        _REF[key] = (sites, w, out)
    return _REF[key]


@pytest.mark.parametrize("env", list(ew.FORWARD_ENVS))
@pytest.mark.parametrize("prec", ["fp32", "f32split"])
@pytest.mark.parametrize("B,L", ew.FORWARD_SHAPES)
def test_forward_winograd_convs_exact(rt, monkeypatch, B, L, prec, env):
    """offk_forward through the handle's own weight table and launches: motion_conv_trans_14 (5x5 / 2, single taps on the 800 unit
    channels of fusion_14, 8 per output channel) and motion_conv_trans (3x3, on the 320 unit channels of fusion_7, 4 per output channel);
    the carried-over channels meet a zero U.  xu_14[..., 128:] == relu(x1) and xv_7[..., 256:] == relu(x2), the fp64 references built from
    exact.unit_reference's M of the five 14-sites and the two 7-sites.  Split-fp32 handles read the plane image of U."""
    sites, w, out = forward_case(B, L)
    P = B * (L - 1)
    for k, v in ew.FORWARD_ENVS[env].items():
        monkeypatch.setenv(k, v)                                    # (read once, at offk_create)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, consensus=False, precision=prec)
    for k in ew.FORWARD_ENVS[env]:
        monkeypatch.delenv(k, raising=False)
    assert h.load_state_dict(w) == []
    h.region("xu_14", 256).fill_(NAN)
    h.region("xv_7", 512).fill_(NAN)
    h.set_profiling(2)
    h.forward([s.x.cuda() for s in sites])
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    starts = lambda sub: any(n.startswith(sub) for n in names)   # noqa: E731
    if env == "direct":
        assert not any("[winograd" in n for n in names), names
    else:
        assert starts("motion_conv_trans [winograd") and starts("motion_conv_trans_14 [winograd") == (P >= 2), names
        assert any("[winograd: between]" in n for n in names) == (env != "wino-nomid"), names
    mm = exact.Mismatches()
    what = "forward B %d L %d %s %s: " % (B, L, prec, env)
    mm.check(h.region("xu_14", 256).view(P, 7, 7, 256)[..., 128:].cpu(), out["x1"], what + "x1 in xu_14")
    mm.check(h.region("xv_7", 512).view(P, 7, 7, 512)[..., 256:].cpu(), out["x2"], what + "x2 in xv_7")
    mm.raise_if_any()
