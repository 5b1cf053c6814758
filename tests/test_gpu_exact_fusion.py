"""Exact integer-input tests of the fusion stage: the three kernels of the fusion@28 bottleneck chains and wino_mid.hip.

tests/test_gpu_exact.py holds the units, the direct convs and the batched GEMM to fp64 value for value; until this module every
other fusion-stage kernel was held to a tolerance, which finds a wrong pixel and not a lost term (a K-step skipped for one lane
group, a halo row read one slot off, the masked (row, dy) pair of the direct 3x3 on the wrong row, a ReLU on the wrong plane word
show at 1e-3 .. 1e-5 of the maximum on random data).  Here the inputs are the small integers of tests/exact_fusion.py -- their
exactness caps, non-degeneracy, order independence in fp32 and exactness under the split-fp32 cut are asserted on the CPU by
tests/test_exact_fusion_inputs.py -- and every result must equal the fp64 reference: exact.assert_exact through a Mismatches, no
tolerance anywhere in this file.  Every output is filled with NaN before the launch, or with the -3.0 sentinel where a channel slice
of a wider buffer is written.

  a. offk_bottleneck_chain14 (chain_fused.hip, the fp32 pipe with the direct 3x3): the merged 28a form reading channels 64.. of a
     128-channel buffer, the residual forms (res = x, res in a buffer of its own, no residual), a 256-channel slice of a 352-channel
     buffer; n = 1 (two half-image blocks), 5 (odd), 9 (past the 8-image block); x nonzero only at the half-image seam / the border.
  b. offk_bottleneck_chain14_split (chain_split.hip) on the same cases, the branch as a 1x1 of its own: equal to fp64 AND to a.
  c. the chains as offk_forward runs them, from the units' integer outputs on: chain_fused.hip's F(2x2, 3x3) form (no stage entry
     reaches it) in an fp32 handle, chain_split.hip on the handle's pre-cut plane images in a split-fp32 handle.
  d. offk_winograd_between / _ex in the eight forms of test_winograd_between_vs_fp64.

Not covered here: the whole Winograd convs (tests/test_gpu_exact_wino.py: single scaled taps make their 1/6, 1/12, 1/24 and 1/3 exact) and
the heads (1/49 is not exact in binary).
"""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec

from . import exact
from . import exact_fusion as ef
from .featmaps import rt  # noqa: F401

pytestmark = pytest.mark.gpu
NAN, SENTINEL = float("nan"), -3.0
CHAIN_CASES = ef.chain_cases()
CHAIN_IDS = [c[0] for c in CHAIN_CASES]
_REF = {}


def chain_case(n, kind, hand):
    """(inputs, fp64 reference) of a chain case: computed once, shared by a. and b., never written to; the caps are checked first"""
    key = (n, kind, hand)
    if key not in _REF:
        c = ef.ChainInputs(n, kind, hand)
        out, cap = c.reference("direct")            # (both stage entries run the direct 3x3)
        ef.check_caps(cap, str(key))
        ef.check_nondegenerate(out, ("t1", "t2", "y"), (), str(key))
        _REF[key] = (c, out["y"])
    return _REF[key]


def dev(t):
    return None if t is None else t.cuda()


def x_view(c):
    """x on the device as the case's kernel sees it: the 28a kinds read channels 64.. of a 128-channel buffer whose other half is NaN
    (the forward's [t2 | x0]), the others a buffer of their own -> (buffer, x_coff)"""
    if c.Cin == 64:
        buf = torch.full((c.n, 14, 14, 128), NAN, device="cuda")
        buf[..., 64:] = c.x.cuda()
        return buf, 64
    return c.x.cuda(), 0


def residual(c, xbuf):
    return None if c.res is None else xbuf if c.res is c.x else c.res.cuda()


def out_buffer(n, sliced):
    """(y, y_coff): a NaN-filled [n, 14, 14, 256], or channels [64, 320) of a 352-channel buffer of sentinels"""
    if sliced:
        return torch.full((n, 14, 14, 352), SENTINEL, device="cuda"), 64
    return torch.full((n, 14, 14, 256), NAN, device="cuda"), 0


def run_fp32(rt, c, sliced=False):
    """offk_bottleneck_chain14; the branch of 28a merged into c3's K (K3 = 128) -> (buffer, the 256 channels written)"""
    xbuf, coff = x_view(c)
    y, ycoff = out_buffer(c.n, sliced)
    w3, b3 = c.merged() if c.wb is not None else (c.w3, c.b3)
    rt.bottleneck_chain14(xbuf, dev(c.w1), dev(c.b1), dev(c.w2), dev(c.b2), dev(w3), dev(b3), res=residual(c, xbuf), relu_in=c.relu_in,
                          x_coff=coff, y=y, y_coff=ycoff)
    torch.cuda.synchronize()
    return y, y[..., ycoff:ycoff + 256]


def run_split(rt, c, sliced=False):
    """offk_bottleneck_chain14_split; the branch of 28a as its own 1x1 on the pre-ReLU input"""
    xbuf, coff = x_view(c)
    y, ycoff = out_buffer(c.n, sliced)
    rt.bottleneck_chain14_split(xbuf, dev(c.w1), dev(c.b1), dev(c.w2), dev(c.b2), dev(c.w3), dev(c.b3), res=residual(c, xbuf),
                                branch=(dev(c.wb), dev(c.bb)) if c.wb is not None else None, relu_in=c.relu_in, x_coff=coff, y=y, y_coff=ycoff)
    torch.cuda.synchronize()
    return y, y[..., ycoff:ycoff + 256]


def sentinels_unchanged(buf):
    return bool(torch.all(buf[..., :64] == SENTINEL)) and bool(torch.all(buf[..., 320:] == SENTINEL))


# ---- a. offk_bottleneck_chain14 --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n,kind,hand", CHAIN_CASES, ids=CHAIN_IDS)
def test_chain14_exact(rt, name, n, kind, hand):
    """The merged 28a form (Cin = 64, relu_in, K3 = 128, signed x at channel 64 of a 128-channel buffer), the residual form (Cin = 256,
    K3 = 64, res = x), the same with the residual elsewhere, and Cin = 64 without either."""
    c, ref = chain_case(n, kind, hand)
    mm = exact.Mismatches()
    _buf, y = run_fp32(rt, c)
    mm.check(y.cpu(), ref, "chain14 %s" % name)
    if kind == "res":
        buf, y = run_fp32(rt, c, sliced=True)
        mm.check(y.cpu(), ref, "chain14 %s into channels 64..319 of 352" % name)
        assert sentinels_unchanged(buf)
    mm.raise_if_any()


# ---- b. offk_bottleneck_chain14_split ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,n,kind,hand", CHAIN_CASES, ids=CHAIN_IDS)
def test_chain14_split_exact(rt, name, n, kind, hand):
    """The branch form (Cin = 64, signed x, the branch on the pre-ReLU input), the residual form (res = x; res a different buffer), Cin =
    64 without branch or residual, output into a slice: equal to fp64, and to offk_bottleneck_chain14 on the equivalent case (the
    branch folded into w3)."""
    c, ref = chain_case(n, kind, hand)
    mm = exact.Mismatches()
    _buf, y = run_split(rt, c)
    mm.check(y.cpu(), ref, "chain14_split %s" % name)
    _buf, ya = run_fp32(rt, c)
    mm.check(ya.cpu(), ref, "chain14 %s" % name)
    same = torch.equal(y, ya)
    if kind in ("res", "28a"):
        buf, ys = run_split(rt, c, sliced=True)
        mm.check(ys.cpu(), ref, "chain14_split %s into channels 64..319 of 352" % name)
        assert sentinels_unchanged(buf)
    mm.raise_if_any()
    assert same, "chain14_split and chain14 differ on %s" % name


# ---- c. the chains as the forward runs them -----------------------------------------------------------------------------------------

def forward_case(B, L):
    key = ("forward", B, L)
    if key not in _REF:
        sites = [exact.SiteInputs(si, B, L, spec.VARIANT_RGB) for si in range(spec.NUM_SITES)]
        w = ef.forward_weights(spec.VARIANT_RGB, sites)
        out, cap = ef.forward28_reference(sites, w, B, L, spec.VARIANT_RGB, form="direct")
        _out, cap_w = ef.forward28_reference(sites, w, B, L, spec.VARIANT_RGB, form="wino")
        ef.check_nondegenerate(out, ("a_t1", "a_t2", "sa", "b_t1", "b_t2", "sb"), ("x0",), str(key))
        _REF[key] = (sites, w, out, cap, cap_w)
    return _REF[key]


CHAIN_GATE = 2      # OFFK_CHAIN=<pairs>: "a number > 1" moves the gate; 2 is the lowest an fp32 handle can have


@pytest.mark.parametrize("prec", ["fp32", "f32split"])
@pytest.mark.parametrize("B,L", ef.FORWARD_SHAPES)
def test_forward_chains_exact(rt, monkeypatch, B, L, prec):
    """offk_forward on the integer maps of exact.SiteInputs, integer unit parameters (exact.weights) and sparse integer weights for
    motion_conv_trans_28 and the convs of chains 28a and 28b (ef.forward_weights) at P = 1, 4, 9 -- below the 12-pair gate, so the 7x7 /
    stride 2 conv runs direct.  The x0 half of xt_28 (channels 64..127), sa_28 and sb_28 equal the fp64 reference built from
    exact.unit_reference's M of the two 28-sites, the 7x7 conv and chain_reference.

    fp32 handle: the chain gate opened to its lowest value (OFFK_CHAIN=2 at offk_create: the switch takes a pair count > 1, and 1 means
    'on, from the default 72 pairs'), so P = 4 and 9 run chain_fused.hip in its F(2x2, 3x3) form, held to the Winograd-domain caps; at
    P = 1 an fp32 handle has no chained form and the same tensors are checked behind the three convs per chain.  Split-fp32 handle:
    chain_split.hip from the first pair on.  The caps stay below 2^24 through chain 28b in both forms (largest: b_t2 in the F(2x2, 3x3)
    form, 7.1e-2 of the limit), so sb_28 is checked as well."""
    sites, w, out, cap, cap_w = forward_case(B, L)
    P = B * (L - 1)
    chained = prec == "f32split" or P >= CHAIN_GATE
    wino_form = prec == "fp32" and chained
    ef.check_caps(cap_w if wino_form else cap, "forward B %d L %d %s" % (B, L, prec))
    if prec == "fp32":
        monkeypatch.setenv("OFFK_CHAIN", str(CHAIN_GATE))          # (read once, at offk_create)
    h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, consensus=False, precision=prec)
    monkeypatch.delenv("OFFK_CHAIN", raising=False)
    assert h.load_state_dict(w) == []
    for name, ch in (("xt_28", 128), ("sa_28", 256), ("sb_28", 256)):
        h.region(name, ch).fill_(NAN)
    h.set_profiling(2)
    h.forward([s.x.cuda() for s in sites])
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    starts = lambda sub: any(n.startswith(sub) for n in names)   # noqa: E731
    assert not starts("motion_conv_trans_28 [winograd"), names
    if chained:
        assert starts("chain_28a") and starts("chain_28b") and starts("chain_28c") and not starts("motion_conv2_trans_28a"), names
    else:
        assert starts("motion_conv2_trans_28a") and starts("motion_conv2_trans_28b") and not starts("chain_28"), names
    mm = exact.Mismatches()
    what = "forward B %d L %d %s: " % (B, L, prec)
    mm.check(h.region("xt_28", 128).view(P, 14, 14, 128)[..., 64:].cpu(), out["x0"], what + "x0 in xt_28")
    mm.check(h.region("sa_28", 256).view(P, 14, 14, 256).cpu(), out["sa"], what + "sa_28")
    mm.check(h.region("sb_28", 256).view(P, 14, 14, 256).cpu(), out["sb"], what + "sb_28")
    mm.raise_if_any()


# ---- d. offk_winograd_between / _ex ---------------------------------------------------------------------------------------------------

def between_case(cin, phases, gemm, n):
    key = ("between", cin, phases, gemm, n)
    if key not in _REF:
        b = ef.BetweenInputs(n, cin, phases, gemm)
        out, cap = b.reference()
        ef.check_caps(cap, str(key))
        ef.check_nondegenerate(out, ("x", "t"), ("V",), str(key))
        _REF[key] = (b, out)
    return _REF[key]


@pytest.mark.parametrize("cin,phases,gemm,prec", ef.BETWEEN_FORMS)
@pytest.mark.parametrize("n", ef.BETWEEN_N)
def test_winograd_between_exact(rt, cin, phases, gemm, n, prec):
    """V is exact; the stored x is exact in channels [32, 32 + cin) of a wider buffer whose sentinel columns stay; the call without an
    x store gives a bit-equal V."""
    b, out = between_case(cin, phases, gemm, n)
    xbuf = torch.full((n, 7, 7, cin + 64), SENTINEL, device="cuda")
    V = torch.full((121, n, cin), NAN, device="cuda")
    rt.winograd_between(dev(b.M), dev(b.bias), phases, dev(b.w1), dev(b.b1), x=xbuf, x_coff=32, precision=prec, V=V)
    torch.cuda.synchronize()
    mm = exact.Mismatches()
    what = "winograd between Cin %d phases %d gemm %d n %d %s: " % (cin, phases, gemm, n, prec)
    mm.check(V.cpu(), out["V"], what + "V")
    mm.check(xbuf[..., 32:32 + cin].cpu(), out["x"], what + "x")
    mm.raise_if_any()
    assert bool(torch.all(xbuf[..., :32] == SENTINEL)) and bool(torch.all(xbuf[..., 32 + cin:] == SENTINEL))
    V2 = torch.full((121, n, cin), NAN, device="cuda")
    rt.winograd_between(dev(b.M), dev(b.bias), phases, dev(b.w1), dev(b.b1), precision=prec, V=V2)          # no x store
    torch.cuda.synchronize()
    assert torch.equal(V, V2)
