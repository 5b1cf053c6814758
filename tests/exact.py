"""Exact integer inputs for the OFF units, the direct convs and the batched GEMM (tests/test_exact_inputs.py, tests/test_gpu_exact.py).

The OFF unit and its backward are closed over the integers: 1x1 convs, bias, ReLU, a subtraction, a depthwise 3x3, a dropout
multiplier that is exactly 2 at p = 0.5, and in the backward the transposes, the weight and bias sums and dX.  Feed small integers
everywhere: if, for every output element, the sum of the absolute values of its terms stays below 2^24, every partial sum in any
order is an integer fp32 holds exactly -- FMA chains, the fp32 matrix pipe, split-K slabs, fixed-order reductions alike -- and the
kernel must equal an fp64 reference value for value.  The split-fp32 mode is exact under the same condition: its cut truncates into
three bf16 planes, an integer of at most 8 significant bits is its own top plane, a 12-bit one is top + middle, all of whose
products are kept.  No summation order, ReLU-kink decision or roundoff model enters; one lost term out of 350 000 is a failure.

This module holds
  * the inputs: a seeded integer recipe on the project's own counter-based generator (synth.raw_u64, restated on torch int64 so
    that the full-size case can draw on the device; tests/test_exact_inputs.py checks the two are the same function),
  * unit_reference: fp64 of one unit and of its whole backward, with the largest per-element sum of absolute terms of every output
    (the exactness condition, measured on the data),
  * assert_exact, and Mismatches: the same over many tensors with one report at the end.
Like tests/arena.py it has no tests of its own.  Everything here works on CPU and on device tensors.
"""
import numpy as np
import torch

from offk_amd import spec, synth

LIMIT = float(2 ** 24)        # every output: sum of |terms| below this
LIMIT_ACC = float(2 ** 23)    # what an accumulate=1 call doubles (the six parameter gradients)
DROP_P = 0.5                  # keep multiplier 1 / (1 - p) = 2 exactly
GEN, DOWN, UNIT = spec.GEN_CH, spec.DOWN_CH, spec.UNIT_CH
PARAM_OUTPUTS = ("gen_w", "gen_b", "down_w", "down_b", "tap_w", "tap_b")

# (B, L, variant, slice mode): the smallest shapes that reach each temporal-step count (K2's and the fused kernel's third group from
# L = 14, K2b's third step from L = 15) and several K1b chunk lengths
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP),
          (2, 8, spec.VARIANT_FLOW, spec.SLICE_FLAT), (2, 13, spec.VARIANT_RGB, spec.SLICE_PER_CLIP), (2, 14, spec.VARIANT_FLOW, spec.SLICE_FLAT),
          (1, 15, spec.VARIANT_RGB, spec.SLICE_FLAT), (5, 9, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP)]
IDS = ["b1l2_rgb_flat", "b2l3_rgb_flat", "b3l4_rgb_clip", "b2l8_flow_flat", "b2l13_rgb_clip", "b2l14_flow_flat", "b1l15_rgb_flat",
       "b5l9_flow_clip"]
FULL_SIZE = (64, 7, spec.VARIANT_RGB, spec.SLICE_FLAT)
# the Flow shapes run again with a dense Sobel weight (dense_sobel): both slice modes, one and several strips per map at every site
SOBEL_SHAPES = [(2, 3, spec.VARIANT_FLOW, spec.SLICE_FLAT), (3, 4, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP), (2, 8, spec.VARIANT_FLOW, spec.SLICE_FLAT)]
SOBEL_IDS = ["b2l3_flow_flat", "b3l4_flow_clip", "b2l8_flow_flat"]


# ---- the project's counter-based generator (synth.raw_u64: splitmix64 finaliser on seed, index) on torch int64 ----------------
_MASK64 = (1 << 64) - 1
_GOLD, _M1, _M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_CHUNK = 1 << 24


def _s64(u):
    """the int64 with the bits of the unsigned 64-bit u"""
    u &= _MASK64
    return u - (1 << 64) if u >> 63 else u


def _lsr(z, k):
    """logical shift right of an int64 tensor (torch's >> is arithmetic)"""
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix(z):
    z = (z ^ _lsr(z, 30)) * _s64(_M1)          # (int64 products wrap: the low 64 bits, as in uint64)
    z = (z ^ _lsr(z, 27)) * _s64(_M2)
    return z ^ _lsr(z, 31)


def _mix_int(z):
    z = ((z ^ (z >> 30)) * _M1) & _MASK64
    z = ((z ^ (z >> 27)) * _M2) & _MASK64
    return z ^ (z >> 31)


def raw_bits(seed, start, count, device="cpu"):
    """synth.raw_u64(seed, start, count) as an int64 tensor holding the same 64 bits."""
    base = _mix_int((int(seed) * _GOLD + _GOLD) & _MASK64)
    idx = torch.arange(start + 1, start + 1 + count, dtype=torch.int64, device=device)
    return _mix(idx * _s64(_GOLD) + _s64(base))


def _field(seed, count, device):
    """the upper 24 bits of each draw, as non-negative int64 (synth.uniform_values' field), chunked to bound the temporaries"""
    out = torch.empty(count, dtype=torch.int64, device=device)
    for o in range(0, count, _CHUNK):
        n = min(_CHUNK, count - o)
        out[o:o + n] = _lsr(raw_bits(seed, o, n, device), 40)
    return out


def ints(seed, shape, lo, hi, device="cpu"):
    """fp32 tensor of integers in lo..hi (field mod (hi - lo + 1): uniform to 2^-21)."""
    n = int(np.prod(shape))
    return (_field(seed, n, device) % (hi - lo + 1) + lo).to(torch.float32).reshape(shape)


def sparse_signs(seed, shape, device="cpu"):
    """fp32 tensor in {-1, 0, 1} with a quarter nonzero: field mod 8 -> 0: -1, 1: +1, else 0."""
    r = _field(seed, int(np.prod(shape)), device) % 8
    return ((r == 1).to(torch.float32) - (r == 0).to(torch.float32)).reshape(shape)


def stream(seed, kind, site=0):
    """one generator stream per (seed, kind of tensor, site); clear of synth's own (feature_seed, make_weights, dropout_stream << 8)"""
    return (0xE8AC7 << 24) | ((int(seed) & 0xFFF) << 12) | (int(kind) << 4) | int(site)


_X, _WG, _BG, _WD, _BD, _TAP, _TB, _DM = range(8)
_SOBEL = 16          # (8 .. 15: the conv and GEMM inputs of tests/exact_units.py)


def dense_sobel(seed=1, device="cpu"):
    """A Sobel weight [32, 1, 3, 3] of integers in -1..1 with every tap in use, corners and centre included: what a checkpoint whose
    sobel_edge_diagonal.conv.weight is not the fixed kernel of util.py:61 sends down K2's nine-tap, no-bias path."""
    w = ints(stream(seed, _SOBEL), (DOWN, 1, 3, 3), -1, 1, device)
    assert bool((w != 0).reshape(DOWN, 9).any(0).all())
    return w


def keep_mask(seed, site_index, pairs, H, device="cpu"):
    """synth.dropout_keep(seed, site_index, pairs, H, DROP_P) -- the project's own keep function -- as a bool tensor [P, 32, H, H];
    on a device: the same integer function evaluated there (keep_mask_torch)."""
    if torch.device(device).type == "cpu":
        return torch.from_numpy(synth.dropout_keep(seed, site_index, pairs, H, DROP_P))
    return keep_mask_torch(seed, site_index, pairs, H, device)


def keep_mask_torch(seed, site_index, pairs, H, device):
    """synth.dropout_keep's integer function on torch int64 (tests/test_exact_inputs.py: equal to synth's, on the CPU)"""
    hw, q = H * H, DOWN // 4
    x = raw_bits(synth.dropout_stream(seed, site_index), 0, pairs * hw * q, device).reshape(pairs, hw, q)
    thr = synth.dropout_threshold(DROP_P)
    keep = torch.stack([((x >> (16 * c)) & 0xFFFF) >= thr for c in range(4)], dim=-1)        # (bits 48..63 survive the arithmetic shift)
    return keep.reshape(pairs, H, H, DOWN).permute(0, 3, 1, 2).contiguous()


class SiteInputs:
    """Integer inputs of one site: x [N, C, H, H] in -2..2, wg [128, C, 1, 1] in -1..1, bg [128] in -3..3, wd [32, C, 1, 1] in -1..1 with
    a quarter nonzero, bd [32] in -3..3, tap [32, 1, 3, 3] in -1..1 and tb [32] in -1..1 (RGB; Flow: the fixed diagonal Sobel, tb None),
    dm [P, 160, H, H] in -2..2, keep [P, 32, H, H] bool (p = 0.5, drop_seed); all fp32.
    sobel (Flow only): the weight that stands in for the fixed kernel, the same tensor at all nine sites as in the reference
    (dense_sobel)."""

    def __init__(self, si, B, L, variant, seed=1, drop_seed=21, device="cpu", sobel=None):
        name, C, H = spec.SITES[si]
        N, P = B * L, B * (L - 1)
        self.si, self.name, self.C, self.H, self.variant = si, name, C, H, variant
        self.x = ints(stream(seed, _X, si), (N, C, H, H), -2, 2, device)
        self.wg = ints(stream(seed, _WG, si), (GEN, C, 1, 1), -1, 1, device)
        self.bg = ints(stream(seed, _BG, si), (GEN,), -3, 3, device)
        self.wd = sparse_signs(stream(seed, _WD, si), (DOWN, C, 1, 1), device)
        self.bd = ints(stream(seed, _BD, si), (DOWN,), -3, 3, device)
        if variant == spec.VARIANT_RGB:
            self.tap = ints(stream(seed, _TAP, si), (DOWN, 1, 3, 3), -1, 1, device)
            self.tb = ints(stream(seed, _TB, si), (DOWN,), -1, 1, device)
        elif sobel is not None:
            assert tuple(sobel.shape) == (DOWN, 1, 3, 3)
            self.tap, self.tb = sobel.to(device=device, dtype=torch.float32).contiguous(), None
        else:
            k = torch.tensor(spec.DIAG_SOBEL, dtype=torch.float32, device=device)
            self.tap, self.tb = k.expand(DOWN, 1, 3, 3).contiguous(), None
        assert sobel is None or variant == spec.VARIANT_FLOW
        self.dm = ints(stream(seed, _DM, si), (P, UNIT, H, H), -2, 2, device)
        self.keep = keep_mask(drop_seed, si, P, H, device)

    def params(self):
        """state_dict key -> tensor of this site's unit parameters (Flow: without the shared Sobel weight)"""
        d = {"motion_conv_gen_%s.weight" % self.name: self.wg, "motion_conv_gen_%s.bias" % self.name: self.bg,
             "motion_spatial_down_%s.weight" % self.name: self.wd, "motion_spatial_down_%s.bias" % self.name: self.bd}
        if self.variant == spec.VARIANT_RGB:
            d["motion_spatial_grad_%s.weight" % self.name] = self.tap
            d["motion_spatial_grad_%s.bias" % self.name] = self.tb
        return d


def weights(variant, sites):
    """A full state_dict (numpy fp32): the integer unit parameters of `sites` (nine SiteInputs), the fusion convs and heads as
    synth.make_weights leaves them -- nothing here reads those.  Flow: the Sobel weight the sites hold (the fixed kernel, or theirs)."""
    w = synth.make_weights(variant)
    if variant == spec.VARIANT_FLOW:
        assert all(torch.equal(s.tap, sites[0].tap) for s in sites)
        w[spec.SOBEL_KEY] = sites[0].tap.cpu().numpy()
    for s in sites:
        for k, v in s.params().items():
            assert w[k].shape == tuple(v.shape), k
            w[k] = v.cpu().numpy()
    return w


PARAM_KEYS = {"gen_w": "motion_conv_gen_%s.weight", "gen_b": "motion_conv_gen_%s.bias", "down_w": "motion_spatial_down_%s.weight",
              "down_b": "motion_spatial_down_%s.bias", "tap_w": "motion_spatial_grad_%s.weight", "tap_b": "motion_spatial_grad_%s.bias"}


def down_rows(B, L, slice_mode):
    """r(n) of every frame n: its row among the P sliced frames, -1 outside the spatial slice."""
    N, P = B * L, B * (L - 1)
    if slice_mode == spec.SLICE_FLAT:
        return [n if n < P else -1 for n in range(N)]
    return [(n // L) * (L - 1) + n % L if n % L < L - 1 else -1 for n in range(N)]


def _dw(Dp, tap, H):
    """depthwise 3x3 cross-correlation, channels-last: Dp [P, H + 2, H + 2, 32] zero-padded, tap [3, 3, 32] -> [P, H, H, 32]"""
    out = None
    for i in range(3):
        for j in range(3):
            t = Dp[:, i:i + H, j:j + H] * tap[i, j]
            out = t if out is None else out + t
    return out


def _dw_t(dSp, tap, H):
    """its transpose: dD[y, x] = sum_ij tap[i, j] dS[y - i + 1, x - j + 1]; dSp zero-padded"""
    out = None
    for i in range(3):
        for j in range(3):
            t = dSp[:, 2 - i:2 - i + H, 2 - j:2 - j + H] * tap[i, j]
            out = t if out is None else out + t
    return out


def _pad(t):
    return torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))


def unit_reference(inp, B, L, variant, slice_mode, dx_rows=None):
    """fp64 reference of one OFF unit (eval and training mode at p = 0.5) and of its whole backward on the integer inputs `inp`.

    Returns (out, cap): out name -> fp64 tensor, cap name -> the largest per-element sum of absolute terms of that output (a float).
    Everything is channels-last, rows in the library's order: G / dGpre [N*HW, 128]; D / dD [P*HW, 32]; M / M_train [P*HW, 160] =
    [S | T], the unit's channels of its fusion buffer (M_train: S times the dropout multiplier); gen_w [128, C, 1, 1], gen_b [128],
    down_w [32, C, 1, 1], down_b [32], tap_w [32, 1, 3, 3], tap_b [32] (RGB only) for the cotangent inp.dm of the TRAINING forward;
    dX [N*HW, C] -- or, with dx_rows (an index tensor of rows), those rows alone.
    Every output's terms: the products (or the two operands of a difference) that the kernel producing it sums, taken on the exact
    values of its inputs."""
    x = inp.x.double()
    dev_ = x.device
    N, P, C, H = B * L, B * (L - 1), inp.C, inp.H
    HW = H * H
    X = x.permute(0, 2, 3, 1).reshape(N * HW, C)
    wg, bg = inp.wg.double().reshape(GEN, C), inp.bg.double()
    wd, bd = inp.wd.double().reshape(DOWN, C), inp.bd.double()
    tap = inp.tap.double().reshape(DOWN, 3, 3).permute(1, 2, 0)          # [3, 3, 32]
    rows = down_rows(B, L, slice_mode)
    frames = torch.tensor([n for n, r in sorted(enumerate(rows), key=lambda nr: nr[1]) if r >= 0], dtype=torch.long, device=dev_)
    assert frames.numel() == P
    Xs = X.view(N, HW, C)[frames].reshape(P * HW, C)
    out, cap = {}, {}

    def keep_(name, val, absval):
        out[name] = val
        cap[name] = float(absval.max())

    # forward
    pre = X @ wg.t() + bg
    keep_("G", torch.relu(pre), X.abs() @ wg.abs().t() + bg.abs())
    G = out["G"]
    D = Xs @ wd.t() + bd
    keep_("D", D, Xs.abs() @ wd.abs().t() + bd.abs())
    D4 = D.view(P, H, H, DOWN)
    tb = inp.tb.double() if inp.tb is not None else torch.zeros(DOWN, dtype=torch.float64, device=dev_)
    S = _dw(_pad(D4), tap, H) + tb
    S_abs = _dw(_pad(D4.abs()), tap.abs(), H) + tb.abs()
    mult = inp.keep.permute(0, 2, 3, 1).double() * (1.0 / (1.0 - DROP_P))          # [P, H, H, 32] of 0 / 2
    G5 = G.view(B, L, HW, GEN)
    T = (G5[:, 1:] - G5[:, :-1]).reshape(P * HW, GEN)
    T_abs = (G5[:, 1:] + G5[:, :-1]).reshape(P * HW, GEN)                         # (G >= 0)
    keep_("M", torch.cat((S.reshape(P * HW, DOWN), T), 1), torch.cat((S_abs.reshape(P * HW, DOWN), T_abs), 1))
    keep_("M_train", torch.cat(((S * mult).reshape(P * HW, DOWN), T), 1), torch.cat(((S_abs * mult).reshape(P * HW, DOWN), T_abs), 1))

    # backward of the training forward
    dm = inp.dm.double().permute(0, 2, 3, 1)                                       # [P, H, H, 160]
    dS = dm[..., :DOWN] * mult
    dT = dm[..., DOWN:].reshape(B, L - 1, HW, GEN)
    z = torch.zeros(B, 1, HW, GEN, dtype=torch.float64, device=dev_)
    mask = (pre > 0).double()
    dG = (torch.cat((z, dT), 1) - torch.cat((dT, z), 1)).reshape(N * HW, GEN) * mask
    dG_abs = (torch.cat((z, dT), 1).abs() + torch.cat((dT, z), 1).abs()).reshape(N * HW, GEN) * mask
    keep_("dG", dG, dG_abs)
    dD = _dw_t(_pad(dS), tap, H).reshape(P * HW, DOWN)
    keep_("dD", dD, _dw_t(_pad(dS.abs()), tap.abs(), H))
    keep_("gen_w", (dG.t() @ X).reshape(GEN, C, 1, 1), dG.abs().t() @ X.abs())
    keep_("gen_b", dG.sum(0), dG.abs().sum(0))
    keep_("down_w", (dD.t() @ Xs).reshape(DOWN, C, 1, 1), dD.abs().t() @ Xs.abs())
    keep_("down_b", dD.sum(0), dD.abs().sum(0))
    if variant == spec.VARIANT_RGB:
        Dp, Dpa, dSa = _pad(D4), _pad(D4.abs()), dS.abs()
        tw = torch.stack([torch.stack([(dS * Dp[:, i:i + H, j:j + H]).sum((0, 1, 2)) for j in range(3)]) for i in range(3)])
        twa = torch.stack([torch.stack([(dSa * Dpa[:, i:i + H, j:j + H]).sum((0, 1, 2)) for j in range(3)]) for i in range(3)])
        keep_("tap_w", tw.permute(2, 0, 1).reshape(DOWN, 1, 3, 3), twa)
        keep_("tap_b", dS.sum((0, 1, 2)), dSa.sum((0, 1, 2)))
    # dX[frame n] = dGpre[n] Wg + dD[r(n)] Wd, the second term inside the slice only
    r_of = torch.tensor(rows, dtype=torch.long, device=dev_)
    idx = torch.arange(N * HW, device=dev_) if dx_rows is None else dx_rows.to(dev_)
    f, px = idx // HW, idx % HW
    r = r_of[f]
    inside = r >= 0
    a = torch.zeros(idx.numel(), UNIT, dtype=torch.float64, device=dev_)
    a[:, :GEN] = dG[idx]
    a[inside, GEN:] = dD[(r * HW + px)[inside]]
    wcat = torch.cat((wg, wd))
    keep_("dX", a @ wcat, a.abs() @ wcat.abs())
    return out, cap


def check_caps(cap, where=""):
    """The exactness condition: a condition of the inputs, not a tolerance.  Returns the largest cap over its limit's share
    (max cap / limit, below 1)."""
    worst = 0.0
    for name, c in cap.items():
        limit = LIMIT_ACC if name in PARAM_OUTPUTS else LIMIT
        assert c < limit, "%s %s: sum of |terms| %.0f is not below %.0f: these inputs do not make the result exact" % (where, name, c, limit)
        worst = max(worst, c / limit)
    return worst


def assert_exact(got, ref, what=""):
    """got (any float dtype) equals the fp64 reference at every element: equal shapes, got.double() == ref everywhere (a signed zero is
    not a difference), a reference that is not all zero.  On failure: the count and the first few indices with both values."""
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, reference %s" % (what, tuple(got.shape), tuple(ref.shape))
    assert ref.dtype == torch.float64, "%s: the reference must be fp64" % what
    assert bool((ref != 0).any()), "%s: the reference is all zero" % what
    g = got.detach().double()
    if g.device != ref.device:
        g = g.to(ref.device)
    bad = ~(g == ref)                       # (a NaN is a difference)
    nbad = int(bad.sum())
    if nbad:
        where = bad.nonzero()[:8].cpu()
        lines = ["%s: got %r, reference %r" % (tuple(int(i) for i in ix), float(g[tuple(ix)]), float(ref[tuple(ix)])) for ix in where]
        raise AssertionError("%s: %d of %d elements differ from the fp64 reference; first: %s" % (what, nbad, bad.numel(), "; ".join(lines)))


class Mismatches:
    """assert_exact over many tensors, all of them looked at before anything is raised: the report of a lost tile then names every
    tensor it reached (the gen- and the down-weight gradient of one channel slab, say), not only the first."""

    def __init__(self):
        self.found = []

    def check(self, got, ref, what=""):
        try:
            assert_exact(got, ref, what)
        except AssertionError as e:
            self.found.append(str(e))

    def raise_if_any(self):
        assert not self.found, "%d tensors differ from the fp64 reference:\n%s" % (len(self.found), "\n".join(self.found))
