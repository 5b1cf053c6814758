"""Exact integer inputs for the Winograd convolutions: the 3x3 convs on 7x7 maps (F(4, 3) x F(3, 3)), the polyphase 5x5 / stride 2
conv (the same transforms on four phase images) and the polyphase 7x7 / stride 2 conv (F(5x5, 4x4))
(tests/test_exact_wino_inputs.py, tests/test_gpu_exact_wino.py).

The weight transform G holds thirds (F(4, 3), F(3, 3)) and ninths and fifths (F(5, 4)), so an integer kernel does not stay an integer
as it does in the F(2x2, 3x3) chains of tests/exact_fusion.py.  It does with ONE nonzero tap per (co, ci) kernel, scaled by the least
integer that clears the tap's two columns of G (tap_scales, computed from G): every entry of G g G^T then has one nonzero term -- no
cancellation, no contraction can matter -- and is an integer.  Different (co, ci) pairs take different taps, so every tap, channel
and tile is still exercised.  B^T and A^T of F(4, 3) / F(3, 3) are integer, so U, V, M and Y are integers and tests/exact.py's
argument holds stage by stage: where the sum of the absolute terms of a stage is below 2^24, fp32 in any order equals fp64, and the
split-fp32 GEMMs are exact too because every U has at most 8 significant bits (it is its own top bf16 plane).

F(5, 4): B^T holds quarters (V: multiples of 1/16), U is an integer of up to 11 significant bits (45 x 45 = 2025, |c| = 1; the stage
entry of this conv has no split mode, the forward cases stay below its gate), and A^T runs from 1/16 to 16 per axis: in units of its
granule 1/4096 the output-transform cap is several hundred times 2^24 WHATEVER the scale of the inputs, so Y cannot be exact.  With V
and M exact the output transform and the bias add are the only roundings, and Y is held to the derived bound gamma_k (|A|^T |M| |A| +
|bias|) per element (GAMMA_K_F54; counted in tests/test_gpu_exact_wino.py).

This module holds the transforms as matrices (G in exact fractions), the weights, the fp64 references -- direct (F.conv2d) and a
restatement per conv that follows the device's decomposition: tiles, phases, the skipped phase-points, the point numbering -- with
the caps of V, M and Y, and the case lists both test files walk.  No tests of its own; CPU tensors.

Largest cap / 2^24 per group, measured by tests/test_exact_wino_inputs.py (which prints it per case; |c| <= 3 but for F(5, 4)):
  3x3 stage entry        V 1.8e-5, M 1.7e-3, y 1.6e-2, pool 5.8e-3   (8 taps per output channel; the largest at x in -3..3)
  5x5 / 2 stage entry    V 1.8e-5, M 2.7e-3, y 1.3e-2                (8 taps per output channel, 1056 -> 128: 9)
  7x7 / 2 stage entry    V 1.3e-4, M 0.47 in units of 1/16 (1 tap per output channel at 32 -> 64, else 2; |c| = 1);
                         y in units of 1/4096: 367 .. 726 x 2^24 -- not exact, the derived bound instead
  forward, x2 (3x3)      V 6.1e-4, M 4.9e-2, y 0.275   (motion_conv_trans on the 320 unit channels of fusion_7, 4 taps per output channel)
  forward, x1 (5x5 / 2)  V 5.2e-4, M 3.5e-2, y 0.226   (motion_conv_trans_14 on the 800 unit channels of fusion_14, 8 taps per output channel)
The tap counts of the forward: 4 for x2; 8 for x1 -- 128 output channels need 7 taps each to reach all 800 live input channels, and with
per-tap scales 8 taps leave the output transform's cap at 0.23 of the limit at all three shapes (the unit outputs reach +-248).
"""
from fractions import Fraction as Fr
from math import gcd

import numpy as np
import torch
import torch.nn.functional as F

from offk_amd import spec

from . import exact
from .exact_fusion import FORWARD_SHAPES, assert_weight_bits, check_caps, check_nondegenerate  # noqa: F401
from .wino_ref import AT as _AT, BT as _BT, OFFSETS, mindex  # noqa: F401

# kinds of tensor for exact.stream, clear of exact's 0 .. 7, tests/exact_units.py's 8 .. 15 and tests/exact_fusion.py's 16 .. 31
(_WX, _WCH, _WPOS, _WVAL, _WSIGN, _WBIAS, _WRES, _WFW) = range(32, 40)

RELU_PRE, RELU_POST = 2, 4           # the conv flags of the stage entries (offk.h)

# ---- the 1-D transforms as matrices, keyed by the number of points: 6 = F(4, 3), 5 = F(3, 3) (winograd_common.h), 8 = F(5, 4) (winograd7.hip)
OUTPUTS = {6: 4, 5: 3, 8: 5}
TAPS = {6: 3, 5: 3, 8: 4}
BT = {6: _BT[6], 5: _BT[5],
      8: np.array([[-1, 0, 5.25, 0, -5.25, 0, 1, 0], [0, 1, 1, -4.25, -4.25, 1, 1, 0], [0, -1, 1, 4.25, -4.25, -1, 1, 0],
                   [0, 2, 4, -2.5, -5, 0.5, 1, 0], [0, -2, 4, 2.5, -5, -0.5, 1, 0], [0, 0.5, 0.25, -2.5, -1.25, 2, 1, 0],
                   [0, -0.5, 0.25, 2.5, -1.25, -2, 1, 0], [0, -1, 0, 5.25, 0, -5.25, 0, 1]], dtype=np.float64)}
AT = {6: _AT[4], 5: _AT[3],
      8: np.array([[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 0.5, -0.5, 2, -2, 0], [0, 1, 1, 0.25, 0.25, 4, 4, 0],
                   [0, 1, -1, 0.125, -0.125, 8, -8, 0], [0, 1, 1, 0.0625, 0.0625, 16, 16, 1]], dtype=np.float64)}
G = {6: [[Fr(1, 4), 0, 0], [Fr(-1, 6), Fr(-1, 6), Fr(-1, 6)], [Fr(-1, 6), Fr(1, 6), Fr(-1, 6)], [Fr(1, 24), Fr(1, 12), Fr(1, 6)],
         [Fr(1, 24), Fr(-1, 12), Fr(1, 6)], [0, 0, 1]],
     5: [[Fr(1, 2), 0, 0], [Fr(-1, 2), Fr(-1, 2), Fr(-1, 2)], [Fr(-1, 6), Fr(1, 6), Fr(-1, 6)], [Fr(1, 6), Fr(1, 3), Fr(2, 3)], [0, 0, 1]],
     8: [[-1, 0, 0, 0], [Fr(-2, 9)] * 4, [Fr(-2, 9), Fr(2, 9), Fr(-2, 9), Fr(2, 9)], [Fr(32, 45), Fr(16, 45), Fr(8, 45), Fr(4, 45)],
         [Fr(32, 45), Fr(-16, 45), Fr(8, 45), Fr(-4, 45)], [Fr(1, 90), Fr(1, 45), Fr(2, 45), Fr(4, 45)],
         [Fr(1, 90), Fr(-1, 45), Fr(2, 45), Fr(-4, 45)], [0, 0, 0, 1]]}
GRANULE = {3: 1.0, 5: 1.0, 7: 1.0 / 16}       # of V and M (B^T of F(5, 4) holds quarters); Y of the 7x7: 1 / 4096, not exact


def _lcm(values):
    out = 1
    for v in values:
        out = out * v // gcd(out, v)
    return out


def g_float(npts):
    return np.array([[float(Fr(v)) for v in row] for row in G[npts]], dtype=np.float64)


def g_integer(npts):
    """(L G as an integer matrix in fp64, L): L the lcm of all denominators of G"""
    L = _lcm(Fr(v).denominator for row in G[npts] for v in row)
    return np.array([[float(Fr(v) * L) for v in row] for row in G[npts]], dtype=np.float64), L


def column_scale(npts, u):
    """the least integer that makes column u of G integer"""
    return _lcm(Fr(row[u]).denominator for row in G[npts])


def phase_taps(k, a):
    """[(u, kh)]: the taps of phase a of a k-tap axis, kh the tap of the conv, u its place in the phase kernel.
    k = 3: one phase, u = kh.  k = 5 (stride 2, pad 2): kh = 2 u + a.  k = 7 (stride 2, pad 3): kh = 2 u - 1 + a (winograd7.hip)."""
    if k == 3:
        return [(u, u) for u in range(3)]
    if k == 5:
        return [(u, 2 * u + a) for u in range(3) if 2 * u + a < 5]
    assert k == 7
    return [(u, 2 * u - 1 + a) for u in range(4) if 2 * u - 1 + a >= 0]


def tap_scales(k):
    """Per axis, for each tap kh of a k-tap conv: the least integer that clears the columns of G the tap lands in (every class)."""
    classes = (8,) if k == 7 else (6, 5)
    out = [0] * k
    for a in ((0,) if k == 3 else (0, 1)):
        for u, kh in phase_taps(k, a):
            out[kh] = _lcm(column_scale(c, u) for c in classes)
    assert all(out)
    return out


def phase_kernel(w, k, a, b):
    """[co, ci, R, R]: the kernel of phase (a, b), zero where the phase has no tap"""
    R = 4 if k == 7 else 3
    g = torch.zeros(w.shape[0], w.shape[1], R, R, dtype=w.dtype)
    for u, kh in phase_taps(k, a):
        for v, kw in phase_taps(k, b):
            g[:, :, u, v] = w[:, :, kh, kw]
    return g


def exact_u(g, ny, nx):
    """U = G g G^T [ny, nx, co, ci] in exact arithmetic: integer-scaled G in fp64, then an exact division"""
    gy, ly = g_integer(ny)
    gx, lx = g_integer(nx)
    ul = torch.einsum("pa,ocab,qb->pqoc", torch.from_numpy(gy), g.double(), torch.from_numpy(gx))
    assert float(ul.abs().max()) < 2.0 ** 52
    assert bool((ul % (ly * lx) == 0).all()), "G g G^T is not an integer: the kernel is not a single scaled tap"
    return ul / (ly * lx)


def significant_bits(t):
    """the largest number of significant bits of an element of t"""
    m, _e = np.frexp(np.abs(np.asarray(t, dtype=np.float64)))
    m = m[m != 0]
    for bits in range(1, 54):
        if np.all(m * 2.0 ** bits == np.round(m * 2.0 ** bits)):
            return bits
    return 54


# ---- weights ---------------------------------------------------------------------------------------------------------------------

def _order(seed, n):
    """a seeded permutation of 0 .. n - 1"""
    return torch.argsort(exact.ints(seed, (n,), 0, (1 << 20) - 1).long() * n + torch.arange(n))


def single_tap_weights(seed, co, ci, k, taps_per_co, cmax, live_ci=None, cover=True):
    """[co, ci, k, k] fp32: every output channel takes taps_per_co distinct input channels (of live_ci when given), each with ONE
    nonzero tap sign * c * scale(kh) * scale(kw), c in 1 .. cmax.  Asserts that every tap position occurs and -- cover -- that every
    (live) input channel is used by some output channel."""
    live = torch.arange(ci) if live_ci is None else torch.as_tensor(list(live_ci))
    nl, kk = live.numel(), k * k
    assert taps_per_co <= nl
    st = lambda kind: exact.stream(seed, kind, k)   # noqa: E731
    idx = torch.arange(co * taps_per_co)
    ch = live[_order(st(_WCH), nl)[idx % nl]]                                        # consecutive: distinct inside an output channel
    pos = _order(st(_WPOS), kk)[(idx + idx // kk) % kk]
    c = exact.ints(st(_WVAL), (idx.numel(),), 1, cmax)
    sign = exact.ints(st(_WSIGN), (idx.numel(),), 0, 1) * 2 - 1
    sc = torch.tensor(tap_scales(k), dtype=torch.float32)
    kh, kw = pos // k, pos % k
    w = torch.zeros(co, ci, k, k)
    w[idx // taps_per_co, ch, kh, kw] = sign * c * sc[kh] * sc[kw]
    assert int((w != 0).sum()) == idx.numel() and int((w != 0).sum((2, 3)).max()) == 1
    assert bool((w != 0).any(1).any(0).all()), "a tap position does not occur"
    used = (w != 0).any(3).any(2).any(0)
    if cover:
        assert bool(used[live].all()), "an input channel is not used: co * taps_per_co = %d < %d" % (idx.numel(), nl)
    assert int(used.sum()) == int(used[live].sum())
    return w


# ---- the point numbering of winograd_common.h: wino_ref.mindex and OFFSETS ----------------------------------------------------------
def classes():
    for cy in (0, 1):
        for cx in (0, 1):
            yield cy, cx, (5 if cy else 6), (5 if cx else 6), (4 if cy else 0), (4 if cx else 0)


def live_product(k, npy, npx, p, q, a, b):
    """False where the device skips the (point, phase) product: the transform of a phase kernel with a zero tap vanishes at a point.
    5x5 / 2: phase a = 1 has taps u = 0, 1 only -- zero at the last point ('infinity'); 7x7 / 2: phase a = 0 has no tap u = 0 -- zero at
    point 0."""
    if k == 5:
        return not (a == 1 and p == npy - 1) and not (b == 1 and q == npx - 1)
    if k == 7:
        return not (a == 0 and p == 0) and not (b == 0 and q == 0)
    return True


# ---- references ------------------------------------------------------------------------------------------------------------------

def epilogue(pre, flags, res):
    y = torch.relu(pre) if flags & RELU_PRE else pre
    if res is not None:
        y = y + res
    return torch.relu(y) if flags & RELU_POST else y


def direct_reference(x, w, bias, k, flags=0, res=None):
    """fp64: post(pre(conv + bias) + res), channels-last; x [n, H, H, ci], w [co, ci, k, k] -> (y, pre-epilogue conv + bias, cap of the
    direct form)"""
    stride, pad = (1, 1) if k == 3 else (2, k // 2)
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    bd = None if bias is None else bias.double()
    pre = F.conv2d(xd, wd, bd, stride, pad).permute(0, 2, 3, 1).contiguous()
    cap = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), stride, pad).permute(0, 2, 3, 1)
    rd = None if res is None else res.double()
    if rd is not None:
        cap = cap + rd.abs()
    return epilogue(pre, flags, rd), pre, float(cap.max())


def tile_sums(y):
    """pool_part of offk_winograd_conv3x3: [4 n, co], row = img * 4 + class, the sum of the stored values of the tile"""
    n, co = y.shape[0], y.shape[3]
    out = torch.zeros(n, 4, co, dtype=y.dtype)
    for cy, cx, ny, nx, oy, ox in classes():
        out[:, 2 * cy + cx] = y[:, oy:oy + ny - 2, ox:ox + nx - 2].sum((1, 2))
    return out.reshape(4 * n, co)


def f43_reference(x, w, bias, k, flags=0, res=None, dtype=torch.float64, perm=None, mutate=None):
    """The 3x3 conv on 7x7 maps (k = 3) or the 5x5 / stride 2 / pad 2 conv on 14x14 maps (k = 5, polyphase) as winograd.hip runs it:
    per class (cy, cx) of the 7 = 4 + 3 cut and per phase V = B^T d B of the window that starts one sample up / left of the tile,
    M[point] += V U^T over the phases whose product is not skipped, M stored under wino_mindex, Y = A^T M A per class, then the
    epilogue.  Returns (out, cap): out = y [n, 7, 7, co], pre (before the epilogue), M [121, n, co], Mph ((class, phase) -> that phase's own
    products [ny, nx, n, co]), pool [4 n, co]; cap = the largest
    per-element sum of absolute terms of V (|B| on |d|), M (|U| on |V|), y (|A| on |M|, + |bias| + |res|) and pool.
    dtype / perm: the same in another dtype with the input channels in another order.  mutate (the sensitivity checks): 'drop_product'
    (cls, i, j, phase), 'drop_ktile' (cls, i, j, phase, first channel), 'offsets' (another table for the OUTPUT side's numbering)."""
    assert k in (3, 5)
    phases = 1 if k == 3 else 4
    mutate = mutate or {}
    n, co, ci = x.shape[0], w.shape[0], w.shape[1]
    p = torch.arange(ci) if perm is None else perm
    xd, wd = x.to(dtype)[..., p], w.double()[:, p]
    M, Mabs = torch.zeros(121, n, co, dtype=dtype), torch.zeros(121, n, co, dtype=dtype)
    cap, Mph = {"V": 0.0}, {}
    mat = lambda a: torch.from_numpy(a).to(dtype)   # noqa: E731
    for cy, cx, ny, nx, oy, ox in classes():
        cls = 2 * cy + cx
        pts = [mindex(phases, cy, cx, i, j) for i in range(ny) for j in range(nx)]
        for ph in range(phases):
            a, b = ph >> 1, ph & 1
            X = xd if phases == 1 else xd[:, a::2, b::2]
            U = exact_u(phase_kernel(wd, k, a, b), ny, nx)
            d = F.pad(X, (0, 0, 1, 1, 1, 1))[:, oy:oy + ny, ox:ox + nx]
            V = torch.einsum("pi,nijc,qj->pqnc", mat(BT[ny]), d, mat(BT[nx]))
            Vabs = torch.einsum("pi,nijc,qj->pqnc", mat(BT[ny]).abs(), d.abs(), mat(BT[nx]).abs())
            cap["V"] = max(cap["V"], float(Vabs.max()))
            live = torch.tensor([[live_product(k, ny, nx, i, j, a, b) for j in range(nx)] for i in range(ny)])
            assert bool((U[~live] == 0).all()), "a skipped product is not identically zero"
            if "drop_product" in mutate and mutate["drop_product"][0] == cls and mutate["drop_product"][3] == ph:
                live[mutate["drop_product"][1], mutate["drop_product"][2]] = False
            U = (U * live[:, :, None, None]).to(dtype)
            m = torch.einsum("pqnc,pqoc->pqno", V, U)
            if "drop_ktile" in mutate and mutate["drop_ktile"][0] == cls and mutate["drop_ktile"][3] == ph:
                _c, i, j, _ph, k0 = mutate["drop_ktile"]
                kt = (p >= k0) & (p < k0 + 32)                      # (the K-tile in the device's channel order)
                m[i, j] -= V[i, j][:, kt] @ U[i, j][:, kt].t()
            Mph[(cls, ph)] = m
            M[pts] += m.reshape(ny * nx, n, co)
            Mabs[pts] += torch.einsum("pqnc,pqoc->pqno", V.abs(), U.abs()).reshape(ny * nx, n, co)
    cap["M"] = float(Mabs.max())
    y, yabs = torch.zeros(n, 7, 7, co, dtype=dtype), torch.zeros(n, 7, 7, co, dtype=dtype)
    offs = mutate.get("offsets", OFFSETS)
    for cy, cx, ny, nx, oy, ox in classes():
        pts = [mindex(phases, cy, cx, i, j, offs) for i in range(ny) for j in range(nx)]
        m = M[pts].reshape(ny, nx, n, co)
        t = torch.einsum("oi,ijnc,pj->nopc", mat(AT[ny]), m, mat(AT[nx]))
        y[:, oy:oy + t.shape[1], ox:ox + t.shape[2]] = t
        yabs[:, oy:oy + t.shape[1], ox:ox + t.shape[2]] = torch.einsum("oi,ijnc,pj->nopc", mat(AT[ny]).abs(), m.abs(), mat(AT[nx]).abs())
    if bias is not None:
        y, yabs = y + bias.to(dtype), yabs + bias.to(dtype).abs()
    r = None if res is None else res.to(dtype)
    if r is not None:
        yabs = yabs + r.abs()
    out = {"pre": y, "M": M, "Mph": Mph, "y": epilogue(y, flags, r)}
    out["pool"] = tile_sums(out["y"])
    cap["y"], cap["pool"] = float(yabs.max()), float(tile_sums(out["y"].abs()).max())
    return out, cap


def f54_reference(x, w, bias, flags=0, dtype=torch.float64, perm=None):
    """The 7x7 / stride 2 / pad 3 conv on 28x28 maps as winograd7.hip runs it: four 14x14 phase images, 3 x 3 tiles of 5 x 5 outputs,
    V = B^T d B of the 8 x 8 window that starts two samples up / left of the tile, M[p, q] += V U^T over the phases whose product is not
    skipped, Y = A^T M A, the valid 14 x 14 kept.  Returns (out, cap): out = y [n, 14, 14, co], M [8, 8, n, 3, 3, co], Mph (the four
    phases' own M, the products a lost (point, phase) takes away), bound_terms = |A|^T |M| |A| + |bias| [n, 14, 14, co] (what the derived
    bound multiplies); cap = V and M in units of 1/16 (exact below 2^24), y in units of 1/4096 (for the record: far above)."""
    n, co, ci = x.shape[0], w.shape[0], w.shape[1]
    p = torch.arange(ci) if perm is None else perm
    xd, wd = x.to(dtype)[..., p], w.double()[:, p]
    mat = lambda a: torch.from_numpy(a).to(dtype)   # noqa: E731
    bt, at = mat(BT[8]), mat(AT[8])
    M, Mabs, Mph, capV = 0, 0, [], 0.0
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        U = exact_u(phase_kernel(wd, 7, a, b), 8, 8)
        d = F.pad(xd[:, a::2, b::2], (0, 0, 2, 2, 2, 2)).unfold(1, 8, 5).unfold(2, 8, 5)        # [n, 3, 3, ci, 8, 8]
        V = torch.einsum("pi,nyxcij,qj->pqnyxc", bt, d, bt)
        capV = max(capV, float(torch.einsum("pi,nyxcij,qj->pqnyxc", bt.abs(), d.abs(), bt.abs()).max()))
        live = torch.tensor([[live_product(7, 8, 8, i, j, a, b) for j in range(8)] for i in range(8)])
        assert bool((U[~live] == 0).all()), "a skipped product is not identically zero"
        U = U.to(dtype)
        Mph.append(torch.einsum("pqnyxc,pqoc->pqnyxo", V, U))
        M = M + Mph[-1]
        Mabs = Mabs + torch.einsum("pqnyxc,pqoc->pqnyxo", V.abs(), U.abs())
    fold = lambda t: t.reshape(n, 15, 15, co)[:, :14, :14]   # noqa: E731
    y = fold(torch.einsum("rp,pqnyxo,sq->nyrxso", at, M, at))
    terms = fold(torch.einsum("rp,pqnyxo,sq->nyrxso", at.abs(), M.abs(), at.abs()))
    if bias is not None:
        y, terms = y + bias.to(dtype), terms + bias.to(dtype).abs()
    out = {"y": torch.relu(y) if flags & (RELU_PRE | RELU_POST) else y, "M": M, "Mph": Mph, "bound_terms": terms}
    return out, {"V": capV / GRANULE[7], "M": float(Mabs.max()) / GRANULE[7], "y": float(terms.max()) * 4096.0}


def product_reach(Mph, bound_terms):
    """What losing ONE (point, phase) product would do.  Returns (count, guard): count [n, 14, 14, co], the number of products with a
    nonzero term A^T[r, p] A^T[s, q] M_phase[p, q] in the output; guard [4, 8, 8], per product the largest over the outputs of |its
    term| / (gamma_k bound_terms) -- above 1: the derived bound cannot hold without it (0: a skipped product)."""
    n, co = bound_terms.shape[0], bound_terms.shape[3]
    at = torch.from_numpy(AT[8]).abs()
    bound = F.pad(GAMMA_K_F54 * bound_terms, (0, 0, 0, 1, 0, 1), value=float("inf")).reshape(n, 3, 5, 3, 5, co)
    count = torch.zeros(n, 3, 5, 3, 5, co, dtype=torch.int64)
    guard = torch.zeros(4, 8, 8, dtype=torch.float64)
    for ph, m in enumerate(Mph):
        for p in range(8):
            for q in range(8):
                c = torch.einsum("r,s,nyxo->nyrxso", at[:, p], at[:, q], m[p, q].abs().double())
                count += c != 0
                guard[ph, p, q] = float(torch.where(c != 0, c / bound, torch.zeros(())).max())
    return count.reshape(n, 15, 15, co)[:, :14, :14], guard


# the roundings on the longest path of wino7_output_kernel (counted in tests/test_gpu_exact_wino.py): 6 + 6 + 1
K_F54 = 13
GAMMA_K_F54 = K_F54 * 2.0 ** -24 / (1 - K_F54 * 2.0 ** -24)


# ---- the stage-entry cases -------------------------------------------------------------------------------------------------------

SHAPES = {3: [(32, 64), (128, 128), (128, 512), (256, 256), (832, 256)], 5: [(32, 64), (64, 64), (1056, 128)], 7: [(32, 64), (64, 128), (320, 64)]}
N67 = {3: [(32, 64), (832, 256)], 5: [(32, 64), (64, 64)]}      # n = 67: one past a 64-row GEMM tile (WG_BM = 64)
HAND = {3: ("seam", "border"), 5: ("odd", "even", "seam")}
CMAX = {3: 3, 5: 3, 7: 1}       # |c| of a tap; F(5, 4): U reaches 90 x 90 and V 240 in units of 1/16 -- c = 1 keeps M's cap a third of 2^24


def taps_per_co(k, ci, co):
    """3x3 and 5x5 / 2: 8, or what reaches every input channel (1056 -> 128: 9).  7x7 / 2: 1 (32 -> 64) or 2 -- more taps would take M's cap
    past 2^24, so 320 -> 64 reaches 128 of its 320 input channels (the others multiply a zero U)."""
    if k == 7:
        return 1 if ci == 32 else 2
    return max(8, -(-ci // co))


def hand_mask(k, hand):
    H = 7 if k == 3 else 14
    m = torch.zeros(H, H)
    r = torch.arange(H)
    if hand == "border":
        m[0] = m[H - 1] = 1.0
        m[:, 0] = m[:, H - 1] = 1.0
    elif hand == "seam":                # rows / columns 3 and 4 of the 7x7 (phase) map: what both the F(4, 3) and the F(3, 3) window read
        s = ((r == 3) | (r == 4)) if k == 3 else ((r >= 6) & (r <= 9))
        m[s] = 1.0
        m[:, s] = 1.0
    else:
        keep = (r % 2 == 1) if hand == "odd" else (r % 2 == 0)          # one live phase
        m[keep[:, None] & keep[None, :]] = 1.0
    return m


class ConvInputs:
    """One stage-entry case: x [n, H, H, ci] (k = 3: 7x7, 5: 14x14, in 0..3 or -3..3; 7: 28x28 in {0, 1}, one in 8 nonzero), w of
    single_tap_weights, bias [co] in -3..3, res [n, 7, 7, co] in 0..3 (k = 3); fp32.  The weights depend on (k, ci, co) alone."""

    def __init__(self, k, ci, co, n, signed=False, hand=None, seed=1):
        self.k, self.ci, self.co, self.n, self.signed, self.hand = k, ci, co, n, signed, hand
        site = SHAPES[k].index((ci, co))
        H = {3: 7, 5: 14, 7: 28}[k]
        xs = exact.stream(seed + n + (100 if signed else 0) + 256 * k, _WX, site)
        if k == 7:
            self.x = (exact.ints(xs, (n, H, H, ci), 0, 7) == 0).to(torch.float32)
        else:
            self.x = exact.ints(xs, (n, H, H, ci), -3 if signed else 0, 3)
        if hand is not None:
            self.x = self.x * hand_mask(k, hand)[None, :, :, None]
        self.taps = taps_per_co(k, ci, co)
        self.w = single_tap_weights(seed + 16 * site, co, ci, k, self.taps, CMAX[k], cover=co * self.taps >= ci)
        self.bias = exact.ints(exact.stream(seed + 256 * k, _WBIAS, site), (co,), -3, 3)
        self.res = exact.ints(exact.stream(seed + n, _WRES, site), (n, 7, 7, co), 0, 3) if k == 3 else None


def conv_cases(k):
    """(id, ci, co, n, signed, hand) of every stage-entry case of the k x k conv"""
    ns = (1, 3, 8) if k == 7 else (1, 5)
    out = [("%dx%d-n%d" % (ci, co, n), ci, co, n, False, None) for ci, co in SHAPES[k] for n in ns]
    if k == 7:
        return out
    out += [("%dx%d-n67" % s, s[0], s[1], 67, False, None) for s in N67[k]]
    out += [("%dx%d-n5-signed" % s, s[0], s[1], 5, True, None) for s in SHAPES[k]]
    return out + [("%dx%d-%s" % (s[0], s[1], h), s[0], s[1], 1, False, h) for s in (SHAPES[k][0], SHAPES[k][-1]) for h in HAND[k]]


# the forms of the 3x3 entry: (name, flags, residual)
FORMS3 = (("plain", 0, False), ("relu", RELU_PRE, False), ("14b", RELU_PRE | RELU_POST, True))


# ---- the forward: x1 = motion_conv_trans_14 (5x5 / 2) and x2 = motion_conv_trans (3x3) on the units' integer outputs ------------------

FORWARD_CONVS = {"motion_conv_trans_14": (5, 800, 8), "motion_conv_trans": (3, 320, 4)}         # key -> (k, live input channels, taps per output channel)
# the environments of the forward test, each set before the handle is created
FORWARD_ENVS = {"wino": {"OFFK_WINOGRAD_5X5": "2"}, "wino-nomid": {"OFFK_WINOGRAD_5X5": "2", "OFFK_WINO_MID": "0"},
                "wino-nogemm": {"OFFK_WINOGRAD_5X5": "2", "OFFK_WINO_GEMM": "0"}, "direct": {"OFFK_WINOGRAD": "0"}}


def forward_weights(variant, sites, seed=1):
    """exact.weights with motion_conv_trans_14 and motion_conv_trans replaced: single scaled taps on the unit channels of fusion_14 /
    fusion_7 (0..799 / 0..319), zero on the channels the stage in front carries over, integer biases (numpy fp32, state_dict keys)."""
    w = exact.weights(variant, sites)
    for i, (key, co, ci, k, _s, _p) in enumerate(c for c in spec.FUSION_CONVS if c[0] in FORWARD_CONVS):
        kk, live, taps = FORWARD_CONVS[key]
        assert kk == k
        wt = single_tap_weights(seed + 512 + i, co, ci, k, taps, CMAX[k], live_ci=range(live))
        bt = exact.ints(exact.stream(seed, _WFW, i), (co,), -3, 3)
        assert w[key + ".weight"].shape == tuple(wt.shape) and bool((wt[:, live:] == 0).all())
        w[key + ".weight"], w[key + ".bias"] = wt.numpy(), bt.numpy()
    return w


def forward_inputs(sites, B, L, variant, slice_mode=spec.SLICE_FLAT):
    """The unit channels of fusion_14 [P, 14, 14, 800] and fusion_7 [P, 7, 7, 320] in fp64, from exact.unit_reference's M of the five
    14-sites and the two 7-sites; and the units' own caps."""
    P = B * (L - 1)
    maps, cap = {}, {}
    for name, idx, H in (("f14", range(2, 7), 14), ("f7", range(7, 9), 7)):
        ms = []
        for si in idx:
            o, c = exact.unit_reference(sites[si], B, L, variant, slice_mode)
            ms.append(o["M"].view(P, H, H, exact.UNIT))
            cap["unit_" + sites[si].name] = max(c["G"], c["D"], c["M"])
        maps[name] = torch.cat(ms, 3)
    return maps, cap


def forward_reference(sites, w, B, L, variant, slice_mode=spec.SLICE_FLAT):
    """fp64 of x1 and x2 as the forward stores them: out x1 = relu(motion_conv_trans_14(fusion_14)) [P, 7, 7, 128], x2 =
    relu(motion_conv_trans(fusion_7)) [P, 7, 7, 256], their pre-ReLU values, the maps; cap: the units', the direct form's (x1_direct,
    x2_direct) and the Winograd stages' (x1_V, x1_M, x1_y, ...).  The direct and the Winograd values are asserted equal."""
    maps, cap = forward_inputs(sites, B, L, variant, slice_mode)
    out = dict(maps)
    for name, key, src in (("x1", "motion_conv_trans_14", "f14"), ("x2", "motion_conv_trans", "f7")):
        k, live, _taps = FORWARD_CONVS[key]
        wt, bt = torch.from_numpy(w[key + ".weight"])[:, :live], torch.from_numpy(w[key + ".bias"])
        y, pre, cdir = direct_reference(maps[src], wt, bt, k, RELU_PRE)
        ow, cw = f43_reference(maps[src], wt, bt, k, RELU_PRE)
        assert torch.equal(ow["y"], y) and torch.equal(ow["pre"], pre)
        out[name], out[name + "_pre"] = y, pre
        cap[name + "_direct"] = cdir
        cap.update((name + "_" + s, cw[s]) for s in ("V", "M", "y"))
    return out, cap
