"""What the tests of the stride-1 fusion convs' split-fp32 data gradient share (tests/test_conv_dgrad_split_abi.py on the CPU,
tests/test_gpu_conv_dgrad_split.py on the GPU): the operands of csrc/conv_dgrad_split.hip in its K order and the CPU model of its arithmetic;
the inequality both files assert of them is tests/split_bound.py's.  A helper module like tests/conv_s2_dgrad_split.py: numpy only, no torch, no tests of its own.

The K order is the one include/offk.h states for offk_conv2d_backward_data_split:
    dx[n, h, w, ci] = sum_{kh, kw, co} g[n, h + pad - kh, w + pad - kw, co] * w[co, ci, kh, kw],   pad = (k - 1) / 2,
K index = tap * Co + co with tap = kh * k + kw: the taps kh major, inside a tap all Co output channels (in MFMA steps of 32; Co % 64 == 0,
so no step straddles a tap); a tap whose g pixel leaves the map at a pixel contributes zeros.  The conv weight takes the role of `w` and
g the role of `x` of synth.emulate_split_dot(form="units")."""
import numpy as np

from offk_amd import synth



def operands(g, w):
    """g [n, H, W, Co], w [Co, Ci, k, k] -> (Wm [Ci, k k Co], Gm [n H W, k k Co]): the two operand matrices in the kernel's K order;
    dx = Gm @ Wm.T"""
    g = np.asarray(g, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    n, H, W, Co = g.shape
    Ci, k = w.shape[1], w.shape[2]
    pad = (k - 1) // 2
    Wm = np.zeros((Ci, k * k, Co), dtype=np.float32)
    Gm = np.zeros((n, H, W, k * k, Co), dtype=np.float32)
    for kh in range(k):
        for kw in range(k):
            t = kh * k + kw
            Wm[:, t, :] = w[:, :, kh, kw].T
            dh, dw = pad - kh, pad - kw                        # pixel (h, w) reads g at (h + dh, w + dw)
            a_lo, a_hi = max(0, -dh), min(H, H - dh)
            b_lo, b_hi = max(0, -dw), min(W, W - dw)
            if a_lo < a_hi and b_lo < b_hi:
                Gm[:, a_lo:a_hi, b_lo:b_hi, t, :] = g[:, a_lo + dh:a_hi + dh, b_lo + dw:b_hi + dw, :]
    return Wm.reshape(Ci, -1), Gm.reshape(n * H * W, -1)


def _shape(g, w):
    n, H, W, _ = np.shape(g)
    return n, H, W, np.shape(w)[1]


def direct(g, w):
    """dx [n, H, W, Ci] in fp64: the operands summed directly"""
    Wm, Gm = operands(g, w)
    return (Gm.astype(np.float64) @ Wm.astype(np.float64).T).reshape(_shape(g, w))


def emulate(g, w, skip=None):
    """dx [n, H, W, Ci] (fp32) as the kernel computes it: synth.emulate_split_dot(form="units") over K in steps of 32, the weight as `w`,
    g as `x`.  skip: index into synth.SPLIT_PRODUCTS of a product to leave out."""
    Wm, Gm = operands(g, w)
    return np.asarray(synth.emulate_split_dot(Wm, Gm, form="units", skip=skip), dtype=np.float32).reshape(_shape(g, w))


def terms(g, w):
    """(ref64, dropped64, sum |g w|), each [n, H, W, Ci]: synth.split_terms with the weight as w"""
    return tuple(np.asarray(p, dtype=np.float64).reshape(_shape(g, w)) for p in synth.split_terms(*operands(g, w)))
