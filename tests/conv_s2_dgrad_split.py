"""What the tests of the stride-2 fusion convs' split-fp32 data gradient share (tests/test_conv_s2_dgrad_split_abi.py on the CPU,
tests/test_gpu_conv_s2_dgrad_split.py on the GPU): the per-phase operands of csrc/conv_dgrad_s2_split.hip in its K order and the CPU model
of its arithmetic; the inequality both files assert of them is tests/split_bound.py's.  A helper module like tests/conv_wgrad_split.py: numpy only, no torch, no tests of its own.

The K order is the one include/offk.h states for offk_conv2d_s2_backward_data_split.  An input pixel is (2a + r, 2b + s); per axis and phase
bit r the taps are the kernel elements k0 + 2 t (k0 = (r + pad) & 1, t = 0 .. ntap - 1), and tap t reads g at a + d0 - t with
d0 = (r + pad - k0) / 2.  K of phase (r, s) = (tap = th * nw + tw, co): the taps th major, inside a tap all Co output channels (in MFMA steps
of 32; Co % 64 == 0, so no step straddles a tap); a tap that leaves the map at a pixel contributes zeros.  The conv weight takes the role
of `w` and g the role of `x` of synth.emulate_split_dot(form="units")."""
import numpy as np

from offk_amd import synth

FORMS = {7: 3, 5: 2}           # kernel size -> padding; stride 2
PHASES = ((0, 0), (0, 1), (1, 0), (1, 1))


def axis(k, r):
    """(ntap, k0, d0) of phase bit r along one axis"""
    pad = FORMS[k]
    k0 = (r + pad) & 1
    return (k - k0 + 1) // 2, k0, (r + pad - k0) // 2


def phase_taps(k, r, s):
    return axis(k, r)[0] * axis(k, s)[0]


def operands(g, w, r, s):
    """g [n, OH, OW, Co], w [Co, Ci, k, k] -> (Wm [Ci, taps * Co], Gm [n * OH * OW, taps * Co]): the two operand matrices of phase (r, s) in the
    kernel's K order; dx[:, r::2, s::2, :] = Gm @ Wm.T"""
    g = np.asarray(g, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    n, OH, OW, Co = g.shape
    Ci, k = w.shape[1], w.shape[2]
    nh, kh0, dh0 = axis(k, r)
    nw, kw0, dw0 = axis(k, s)
    Wm = np.zeros((Ci, nh * nw, Co), dtype=np.float32)
    Gm = np.zeros((n, OH, OW, nh * nw, Co), dtype=np.float32)
    for th in range(nh):
        for tw in range(nw):
            t = th * nw + tw
            Wm[:, t, :] = w[:, :, kh0 + 2 * th, kw0 + 2 * tw].T
            dh, dw = dh0 - th, dw0 - tw                        # output pixel (a, b) reads g at (a + dh, b + dw)
            a_lo, a_hi = max(0, -dh), min(OH, OH - dh)
            b_lo, b_hi = max(0, -dw), min(OW, OW - dw)
            if a_lo < a_hi and b_lo < b_hi:
                Gm[:, a_lo:a_hi, b_lo:b_hi, t, :] = g[:, a_lo + dh:a_hi + dh, b_lo + dw:b_hi + dw, :]
    return Wm.reshape(Ci, -1), Gm.reshape(n * OH * OW, -1)


def _assemble(parts, n, OH, OW, Ci, dtype):
    out = np.zeros((n, 2 * OH, 2 * OW, Ci), dtype=dtype)
    for (r, s), p in zip(PHASES, parts):
        out[:, r::2, s::2, :] = np.asarray(p).reshape(n, OH, OW, Ci)
    return out


def direct(g, w):
    """dx [n, H, W, Ci] in fp64: the operands summed directly"""
    n, OH, OW, _ = np.shape(g)
    parts = []
    for r, s in PHASES:
        Wm, Gm = operands(g, w, r, s)
        parts.append(Gm.astype(np.float64) @ Wm.astype(np.float64).T)
    return _assemble(parts, n, OH, OW, np.shape(w)[1], np.float64)


def emulate(g, w, skip=None):
    """dx [n, H, W, Ci] (fp32) as the kernel computes it: per phase synth.emulate_split_dot(form="units") over K in steps of 32, the weight as
    `w`, g as `x`.  skip: index into synth.SPLIT_PRODUCTS of a product to leave out."""
    n, OH, OW, _ = np.shape(g)
    parts = []
    for r, s in PHASES:
        Wm, Gm = operands(g, w, r, s)
        parts.append(synth.emulate_split_dot(Wm, Gm, form="units", skip=skip))
    return _assemble(parts, n, OH, OW, np.shape(w)[1], np.float32)


def terms(g, w):
    """(ref64, dropped64, sum |g w|), each [n, H, W, Ci]: synth.split_terms with the weight as w"""
    n, OH, OW, _ = np.shape(g)
    per = [synth.split_terms(*operands(g, w, r, s)) for r, s in PHASES]
    return tuple(_assemble([p[i] for p in per], n, OH, OW, np.shape(w)[1], np.float64) for i in range(3))
