"""Exact integer inputs for the fusion stage: the bottleneck chains of fusion@28 and what sits between two Winograd convs at 7x7
(tests/test_exact_fusion_inputs.py, tests/test_gpu_exact_fusion.py).

Every part of a chain is closed over the integers (1x1, ReLU, 3x3, ReLU, 1x1, bias, residual, ReLU); in chain_fused.hip's
F(2x2, 3x3) form of the 3x3 the transforms B and A hold only +-1 and G holds 1 and 1/2, so every Winograd-domain value is a multiple
of 1/4.  Between two Winograd convs at 7x7 the output transform A (1, 2, 4, 8), the input transform B (1 .. 5), a 1x1 conv, biases and
ReLUs are closed too.  tests/exact.py's argument then holds: where the sum of the absolute values of an output's terms, in units of
its smallest granule, is below 2^24, every partial sum in any order is a number fp32 holds, and the kernel must equal fp64 value for
value.  The split-fp32 mode is exact under the same condition for ANY fp32 activation as long as the weights have at most 8
significant bits (asserted here): such a weight is its own top bf16 plane, and w_h x_h, w_h x_m, w_h x_l are all among the six kept
products.

This module holds the inputs, the fp64 references with their caps (the largest per-element sum of absolute terms), the condition
checks (check_caps, check_nondegenerate) and the case lists both test files walk.  No tests of its own; CPU tensors.

Largest cap / 2^24 per group, measured by tests/test_exact_fusion_inputs.py (which prints it per case); the F(2x2, 3x3) figures are
in units of 1/4:
  chains, direct 3x3 form      1.31e-4  (y of the Cin = 256 residual chains at n = 5 and 9; Cin = 64: 6.25e-5)
  chains, F(2x2, 3x3) form     1.24e-3  (t2 of the Cin = 256 chains at n = 9; Cin = 64: 5.51e-4)
  between                      8.23e-4  (V at Cin = 256 with the 1x1 conv, n = 5; without a 1x1 conv 1.75e-4)
  forward through sa_28        direct 6.16e-4, F(2x2, 3x3) 6.64e-3  (B = 2, L = 3 and B = 3, L = 4)
  forward through sb_28        direct 6.70e-3, F(2x2, 3x3) 7.13e-2  (b_t2, the 3x3 conv of chain 28b): below 1 with room, so the
                               forward cases check sb_28 as well
"""
import numpy as np
import torch
import torch.nn.functional as F

from offk_amd import spec

from . import exact
from .wino_ref import AT as _AT, BT as _BT, between_reference as _between_reference, mindex as _mindex

# kinds of tensor for exact.stream, clear of exact's own _X .. _DM (0 .. 7) and of tests/exact_units.py's 8 .. 15
(_CX, _CW1, _CB1, _CW2, _CB2, _CW3, _CB3, _CWB, _CBB, _CRES, _BM, _BBIAS, _BW1, _BB1, _FW, _FB) = range(16, 32)

WEIGHT_BITS = 8          # |w| < 2^8: the weight is its own top bf16 plane
GRANULE_WINO = 0.25      # G w G^T of an integer w: multiples of 1/4

# ---- F(2x2, 3x3) as chain_fused.hip states it (points 0, 1, -1, inf) -------------------------------------------------------------
W2_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
W2_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
W2_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def sparse(seed, shape, every):
    """fp32 tensor in {-1, 0, 1} with 2 of `every` nonzero (exact.sparse_signs is every = 8)."""
    r = exact.ints(seed, shape, 0, every - 1)
    return (r == 1).to(torch.float32) - (r == 0).to(torch.float32)


def assert_weight_bits(*tensors):
    """The split-fp32 condition: integers of at most 8 significant bits."""
    for t in tensors:
        if t is not None:
            assert bool((t == t.round()).all()) and float(t.abs().max()) < 2 ** WEIGHT_BITS


# ---- chains ----------------------------------------------------------------------------------------------------------------------

# kind -> (Cin, signed x, ReLU on the way in, branch, residual)
#   28a        RGB_OFF.py:658-667: c1 on relu(x), the branch 1x1 on the pre-ReLU x (merged into c3's K in the fp32 kernel)
#   res        :670-685: Cin = 256, res = x
#   res_other  the same with the residual in a buffer of its own
#   plain      Cin = 64, neither branch nor residual
CHAIN_KINDS = {"28a": (64, True, True, True, None), "res": (256, False, False, False, "x"), "res_other": (256, False, False, False, "other"),
               "plain": (64, True, True, False, None)}
HAND = ("seam", "border")      # x nonzero only in image rows 6 and 7 / only in rows 0 and 13 and columns 0 and 13
CHAIN_N = (1, 5, 9)            # two half-image blocks; odd; past the fused kernel's 8-image block into a block of one image


def hand_mask(hand):
    m = torch.zeros(14, 14)
    if hand == "seam":
        m[6:8] = 1.0
    else:
        assert hand == "border"
        m[0] = m[13] = 1.0
        m[:, 0] = m[:, 13] = 1.0
    return m


class ChainInputs:
    """Integer inputs of one chain: x [n, 14, 14, Cin] in -3..3 (signed kinds) or 0..3, w1 [64, Cin], w2 [64, 64, 3, 3], w3 [256, 64],
    the branch wb [256, 64] in {-1, 0, 1} with a quarter nonzero, biases in -3..3, other [n, 14, 14, 256] in 0..3 (the residual of
    'res_other'); all fp32.  The weights depend on (seed, Cin) alone: every n and both hand-made x share them."""

    def __init__(self, n, kind, hand=None, seed=1):
        Cin, signed, relu_in, branch, res = CHAIN_KINDS[kind]
        self.n, self.kind, self.hand, self.Cin, self.relu_in = n, kind, hand, Cin, relu_in
        site = 0 if Cin == 64 else 1
        st = lambda k: exact.stream(seed, k, site)   # noqa: E731
        self.x = exact.ints(exact.stream(seed + n, _CX, site), (n, 14, 14, Cin), -3 if signed else 0, 3)
        if hand is not None:
            self.x = self.x * hand_mask(hand)[None, :, :, None]
        self.w1, self.b1 = exact.sparse_signs(st(_CW1), (64, Cin)), exact.ints(st(_CB1), (64,), -3, 3)
        self.w2, self.b2 = exact.sparse_signs(st(_CW2), (64, 64, 3, 3)), exact.ints(st(_CB2), (64,), -3, 3)
        self.w3, self.b3 = exact.sparse_signs(st(_CW3), (256, 64)), exact.ints(st(_CB3), (256,), -3, 3)
        self.wb, self.bb = (exact.sparse_signs(st(_CWB), (256, 64)), exact.ints(st(_CBB), (256,), -3, 3)) if branch else (None, None)
        self.res = None if res is None else self.x if res == "x" else exact.ints(exact.stream(seed + n, _CRES, site), (n, 14, 14, 256), 0, 3)
        assert_weight_bits(self.w1, self.b1, self.w2, self.b2, self.w3, self.b3, self.wb, self.bb)

    def merged(self):
        """c3 and the branch as the fp32 kernel's one contraction over [t2 | x]: (w3 [256, 128], b3 [256])"""
        return torch.cat((self.w3, self.wb), 1), self.b3 + self.bb

    def reference(self, form="direct"):
        br = (self.wb, self.bb) if self.wb is not None else None
        return chain_reference(self.x, self.w1, self.b1, self.w2, self.b2, self.w3, self.b3, br, self.res, self.relu_in, form)


def chain_cases(kinds=tuple(CHAIN_KINDS)):
    """(id, n, kind, hand) of every chain case: seeded inputs at n = 1, 5, 9 for every kind, both hand-made x at n = 1 for the kinds with
    their own x recipe (28a: signed, Cin = 64; res: non-negative, Cin = 256)."""
    out = [("%s-n%d" % (k, n), n, k, None) for k in kinds for n in CHAIN_N]
    return out + [("%s-%s" % (k, h), 1, k, h) for k in kinds if k in ("28a", "res") for h in HAND]


def conv3x3(t, w):
    """3x3 / pad 1 cross-correlation, channels-last: t [n, 14, 14, ci], w [co, ci, 3, 3] -> [n, 14, 14, co]"""
    return F.conv2d(t.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)


def c2_winograd(t1, w2, absolute=False):
    """The 3x3 conv in F(2x2, 3x3) form, in the dtype of t1: 7 x 7 tiles, V = B^T d B, M = sum_ci U V with U = G w G^T, Y = A^T M A.
    absolute: the same with |B|, |U|, |A| on |t1| -- the sum of the absolute terms of the Winograd-domain computation."""
    dt = t1.dtype
    bt, g, at = (torch.from_numpy(m).to(dt) for m in (W2_BT, W2_G, W2_AT))
    n = t1.shape[0]
    u = torch.einsum("pa,oiab,qb->pqoi", g.double(), w2.double(), g.double())       # (multiples of 1/4: exact in every dtype here)
    assert bool((u * 4 == (u * 4).round()).all())
    u = u.to(dt)
    if absolute:
        t1, bt, u, at = t1.abs(), bt.abs(), u.abs(), at.abs()
    tp = F.pad(t1, (0, 0, 1, 1, 1, 1))
    d = tp.unfold(1, 4, 2).unfold(2, 4, 2)                                           # [n, 7, 7, ci, 4, 4]
    v = torch.einsum("pa,nyxiab,qb->nyxpqi", bt, d, bt)
    m = torch.einsum("nyxpqi,pqoi->nyxpqo", v, u)
    y = torch.einsum("rp,nyxpqo,sq->nyrxso", at, m, at)                              # [n, 7, 2, 7, 2, co]
    return y.reshape(n, 14, 14, w2.shape[0])


def chain_reference(x, w1, b1, w2, b2, w3, b3, branch=None, res=None, relu_in=False, form="direct"):
    """fp64 reference of one chain: t1 = relu(c1(in(x))), t2 = relu(c2(t1)), y = relu(c3(t2) + b3 [+ branch(x)] [+ res]); channels-last.
    Returns (out, cap): out name -> fp64 tensor, cap name -> the largest per-element sum of absolute terms.  form 'direct': the terms
    are the products, the biases and the residual; 'wino': for t2 the Winograd-domain computation |A|^T (|U| . |B|^T |t1| |B|) |A|
    + |b2| in units of 1/4.  The VALUES do not depend on the form."""
    assert form in ("direct", "wino")
    x, w1, b1, w2, b2, w3, b3 = (t.double() for t in (x, w1, b1, w2, b2, w3, b3))
    out, cap = {}, {}
    xin = torch.relu(x) if relu_in else x
    out["t1"] = torch.relu(xin @ w1.t() + b1)
    cap["t1"] = float((xin.abs() @ w1.abs().t() + b1.abs()).max())
    t1 = out["t1"]
    out["t2"] = torch.relu(conv3x3(t1, w2) + b2)
    if form == "direct":
        cap["t2"] = float((conv3x3(t1, w2.abs()) + b2.abs()).max())
    else:
        cap["t2"] = float((c2_winograd(t1, w2, absolute=True) + b2.abs()).max()) / GRANULE_WINO
    t2 = out["t2"]
    y, ya = t2 @ w3.t() + b3, t2 @ w3.abs().t() + b3.abs()
    if branch is not None:
        wb, bb = branch[0].double(), branch[1].double()
        y, ya = y + x @ wb.t() + bb, ya + x.abs() @ wb.abs().t() + bb.abs()
    if res is not None:
        y, ya = y + res.double(), ya + res.double().abs()
    out["y"], cap["y"] = torch.relu(y), float(ya.max())
    return out, cap


def chain_fp32(x, w1, b1, w2, b2, w3, b3, branch=None, res=None, relu_in=False, perm=None, wino=False):
    """The same chain in fp32 torch CPU ops.  perm: (perm of Cin, perm of 64): every contraction sums its channels in that order
    (another summation order); wino: c2 through the explicit F(2x2, 3x3) restatement."""
    assert all(t.dtype == torch.float32 for t in (x, w1, b1, w2, b2, w3, b3))
    pi, pm = perm if perm is not None else (torch.arange(w1.shape[1]), torch.arange(64))
    xin = torch.relu(x) if relu_in else x
    t1 = torch.relu(xin[..., pi] @ w1[:, pi].t() + b1)
    c2 = c2_winograd(t1[..., pm], w2[:, pm]) if wino else conv3x3(t1[..., pm], w2[:, pm])
    t2 = torch.relu(c2 + b2)
    y = t2[..., pm] @ w3[:, pm].t() + b3
    if branch is not None:
        y = y + x[..., pi] @ branch[0][:, pi].t() + branch[1]
    if res is not None:
        y = y + res
    return {"t1": t1, "t2": t2, "y": torch.relu(y)}


# ---- between two Winograd convs at 7x7 (wino_mid.hip) ------------------------------------------------------------------------------

# the eight forms of test_winograd_between_vs_fp64, each at n = 1 and 5
BETWEEN_FORMS = [(128, 4, True, "fp32"), (128, 1, True, "fp32"), (256, 1, True, "fp32"), (128, 1, False, "fp32"), (256, 1, False, "fp32"),
                 (128, 4, True, "f32split"), (128, 1, True, "f32split"), (256, 1, True, "f32split")]
BETWEEN_N = (1, 5)


class BetweenInputs:
    """M [121, n, Cin] in {-1, 0, 1} with a quarter nonzero, bias_in [Cin] in -3..3, w1 [Cin, Cin] in {-1, 0, 1} with a quarter
    nonzero and b1 [Cin] in -3..3 (gemm), else None; fp32.  Arithmetic mode does not enter: both modes of a form share their inputs."""

    def __init__(self, n, cin, phases, gemm, seed=1):
        self.n, self.cin, self.phases, self.gemm = n, cin, phases, gemm
        site = (cin // 128) * 4 + phases // 2 + (8 if gemm else 0)         # 4 .. 15, one per (cin, phases, gemm)
        self.M = exact.sparse_signs(exact.stream(seed + n, _BM, site), (121, n, cin))
        self.bias = exact.ints(exact.stream(seed, _BBIAS, site), (cin,), -3, 3)
        self.w1 = exact.sparse_signs(exact.stream(seed, _BW1, site), (cin, cin)) if gemm else None
        self.b1 = exact.ints(exact.stream(seed, _BB1, site), (cin,), -3, 3) if gemm else None
        assert_weight_bits(self.w1, self.b1, self.bias)

    def reference(self):
        return between_reference(self.M, self.bias, self.phases, self.w1, self.b1)


def _classes():
    for cy in (0, 1):
        for cx in (0, 1):
            yield cy, cx, (5 if cy else 6), (5 if cx else 6), (4 if cy else 0), (4 if cx else 0)


def output_transform(M, phases, absolute=False):
    """A^T M A per class, placed as the 7x7 map [n, 7, 7, c], in the dtype of M -- with the transform matrices and the point numbering of
    tests/wino_ref.py.  absolute: |A| on |M|, the sum of the absolute terms."""
    dt = M.dtype
    n, cin = M.shape[1], M.shape[2]
    mat = lambda a: (torch.from_numpy(a).abs() if absolute else torch.from_numpy(a)).to(dt)   # noqa: E731
    x = torch.zeros(n, 7, 7, cin, dtype=dt)
    Ma = M.abs() if absolute else M
    for cy, cx, ny, nx, oy, ox in _classes():
        m = torch.stack([torch.stack([Ma[_mindex(phases, cy, cx, i, j)] for j in range(nx)], 0) for i in range(ny)], 0)      # [ny, nx, n, c]
        y = torch.einsum("oi,ijnc,pj->nopc", mat(_AT[3 if cy else 4]), m, mat(_AT[3 if cx else 4]))
        x[:, oy:oy + y.shape[1], ox:ox + y.shape[2]] = y
    return x


def between_fp32(M, bias, phases, w1, b1, perm=None):
    """The between stage in fp32 torch CPU ops -> (x, t, V)."""
    assert M.dtype == torch.float32
    x = torch.relu(output_transform(M, phases) + bias)
    t = x
    if w1 is not None:
        p = perm if perm is not None else torch.arange(w1.shape[1])
        t = torch.relu(x[..., p] @ w1[:, p].t() + b1)
    return x, t, input_transform(t)


def input_transform(t, absolute=False):
    """V [121, n, c] = B^T d B per class of the zero-padded t [n, 7, 7, c] (phases-1 point numbering), in the dtype of t"""
    dt = t.dtype
    n, c = t.shape[0], t.shape[3]
    tp = F.pad(t.abs() if absolute else t, (0, 0, 1, 1, 1, 1))
    V = torch.zeros(121, n, c, dtype=dt)
    for cy, cx, ny, nx, oy, ox in _classes():
        by, bx = (torch.from_numpy(_BT[k]).to(dt) for k in (ny, nx))
        if absolute:
            by, bx = by.abs(), bx.abs()
        v = torch.einsum("pi,nijc,qj->pqnc", by, tp[:, oy:oy + ny, ox:ox + nx], bx)
        for i in range(ny):
            for j in range(nx):
                V[_mindex(1, cy, cx, i, j)] = v[i, j]
    return V


def between_reference(M, bias, phases, w1, b1):
    """fp64: tests/wino_ref.py's between_reference for x and V, t restated beside it; and the cap pass with |A|, |w1|, |B|.
    Returns (out, cap) over x [n, 7, 7, Cin], t [n, 7, 7, Cmid], V [121, n, Cmid]."""
    f64 = lambda t: None if t is None else t.double().numpy()   # noqa: E731
    x, V = _between_reference(f64(M), f64(bias), phases, f64(w1), f64(b1))
    x, V = torch.from_numpy(x), torch.from_numpy(V)
    out, cap = {"x": x, "V": V}, {}
    cap["x"] = float((output_transform(M.double(), phases, absolute=True) + bias.double().abs()).max())
    if w1 is not None:
        out["t"] = torch.relu(x @ w1.double().t() + b1.double())
        cap["t"] = float((x @ w1.double().abs().t() + b1.double().abs()).max())
    else:
        out["t"] = x
        cap["t"] = cap["x"]
    cap["V"] = float(input_transform(out["t"], absolute=True).max())
    return out, cap


# ---- the fusion@28 stage as the forward runs it: units of the two 28-sites -> 7x7 / stride 2 -> chain 28a [-> chain 28b] --------------

FORWARD_SHAPES = [(1, 2), (2, 3), (3, 4)]            # P = 1, 4, 9: below the 12-pair gate of the polyphase Winograd 7x7 conv
INTEGER_CONVS = ("motion_conv_trans_28", "motion_conv1_trans_28a", "motion_conv2_trans_28a", "motion_conv3_trans_28a", "motion_conv_branch_28a",
                 "motion_conv1_trans_28b", "motion_conv2_trans_28b", "motion_conv3_trans_28b")
# 2 of this many weights nonzero: the unit outputs reach +-100 and every conv multiplies the magnitude, so the stage is kept sparse
# enough for sa_28 to stay far below 2^24 (the 7x7 conv: 15 680 taps, ~30 of them nonzero per output channel)
_EVERY = {"motion_conv_trans_28": 1024, "motion_conv1_trans_28a": 16, "motion_conv2_trans_28a": 64, "motion_conv3_trans_28a": 16,
          "motion_conv_branch_28a": 16, "motion_conv1_trans_28b": 64, "motion_conv2_trans_28b": 64, "motion_conv3_trans_28b": 16}


def forward_weights(variant, sites, seed=1):
    """exact.weights (integer unit parameters, synth's fusion convs and heads) with motion_conv_trans_28 and the convs of chains 28a and
    28b replaced by sparse integers in {-1, 0, 1}, biases in -3..3 (numpy fp32, state_dict keys)."""
    w = exact.weights(variant, sites)
    for i, (key, co, ci, k, _s, _p) in enumerate(c for c in spec.FUSION_CONVS if c[0] in INTEGER_CONVS):
        wt = sparse(exact.stream(seed, _FW, i), (co, ci, k, k), _EVERY[key])
        bt = exact.ints(exact.stream(seed, _FB, i), (co,), -3, 3)
        assert_weight_bits(wt, bt)
        assert w[key + ".weight"].shape == tuple(wt.shape)
        w[key + ".weight"], w[key + ".bias"] = wt.numpy(), bt.numpy()
    return w


def forward28_reference(sites, w, B, L, variant, slice_mode=spec.SLICE_FLAT, form="direct"):
    """fp64 of fusion@28 up to sb_28 on the integer maps of `sites` (all nine exact.SiteInputs; the two 28-sites are read) and the
    weights of forward_weights: fusion_28 = [M_3a | M_3b] from exact.unit_reference, x0 = the 7x7 / stride 2 / pad 3 conv (pre-ReLU),
    chain 28a (branch form) -> sa, chain 28b (res = sa) -> sb.  Returns (out, cap) over x0, sa, sb [P, 14, 14, .], the chains' inner
    tensors as a_t1, a_t2, b_t1, b_t2, and the units' own caps as unit_<site>."""
    P = B * (L - 1)
    out, cap, ms = {}, {}, []
    for s in sites[:2]:
        o, c = exact.unit_reference(s, B, L, variant, slice_mode)
        ms.append(o["M"].view(P, 28, 28, exact.UNIT))
        cap["unit_" + s.name] = max(c["G"], c["D"], c["M"])
    f28 = torch.cat(ms, 3).permute(0, 3, 1, 2)
    t = lambda k: torch.from_numpy(w[k]).double()   # noqa: E731
    wt, bt = t("motion_conv_trans_28.weight"), t("motion_conv_trans_28.bias")
    out["x0"] = F.conv2d(f28, wt, bt, stride=2, padding=3).permute(0, 2, 3, 1).contiguous()
    cap["x0"] = float(F.conv2d(f28.abs(), wt.abs(), bt.abs(), stride=2, padding=3).max())
    m = lambda k: t(k).reshape(t(k).shape[0], -1)   # noqa: E731
    a, ca = chain_reference(out["x0"], m("motion_conv1_trans_28a.weight"), t("motion_conv1_trans_28a.bias"), t("motion_conv2_trans_28a.weight"),
                            t("motion_conv2_trans_28a.bias"), m("motion_conv3_trans_28a.weight"), t("motion_conv3_trans_28a.bias"),
                            (m("motion_conv_branch_28a.weight"), t("motion_conv_branch_28a.bias")), None, True, form)
    b, cb = chain_reference(a["y"], m("motion_conv1_trans_28b.weight"), t("motion_conv1_trans_28b.bias"), t("motion_conv2_trans_28b.weight"),
                            t("motion_conv2_trans_28b.bias"), m("motion_conv3_trans_28b.weight"), t("motion_conv3_trans_28b.bias"),
                            None, a["y"], False, form)
    out.update(a_t1=a["t1"], a_t2=a["t2"], sa=a["y"], b_t1=b["t1"], b_t2=b["t2"], sb=b["y"])
    cap.update(a_t1=ca["t1"], a_t2=ca["t2"], sa=ca["y"], b_t1=cb["t1"], b_t2=cb["t2"], sb=cb["y"])
    return out, cap


THROUGH_SA = ("unit_3a", "unit_3b", "x0", "a_t1", "a_t2", "sa")


# ---- the conditions on the inputs ----------------------------------------------------------------------------------------------

def check_caps(cap, where=""):
    """Every cap below 2^24 (exact.check_caps): a condition on the inputs, not a tolerance.  Returns the largest cap / 2^24."""
    return exact.check_caps(cap, where)


def check_nondegenerate(out, relu_names, value_names, where=""):
    """From the reference alone: in each tensor of relu_names the share of elements the ReLU zeroes lies between 5 % and 95 %; each
    of those and of value_names takes at least 8 distinct values."""
    for name in relu_names:
        share = float((out[name] == 0).double().mean())
        assert 0.05 <= share <= 0.95, "%s %s: the ReLU zeroes %.3f of the elements" % (where, name, share)
    for name in tuple(relu_names) + tuple(value_names):
        assert out[name].unique().numel() >= 8, "%s %s: fewer than 8 distinct values" % (where, name)
