"""What the tests of the stride-2 fusion convs' split-fp32 weight gradient share (tests/test_conv_s2_wgrad_split_abi.py on the CPU,
tests/test_gpu_conv_s2_wgrad_split.py on the GPU): the K layout of csrc/conv_wgrad_s2_split.hip in numpy and the CPU model of its CHUNKED
arithmetic; the inequality both files assert of them is tests/split_bound.py's.  A helper module like tests/conv_wgrad_split.py: no tests of its own, no torch.

The K order is the one include/offk.h states for offk_conv2d_s2_backward_weight_split.  K runs over the OUTPUT pixels, real pixels only:
q = (img * OH + oh) * OW + ow with OH = H / 2, OW = W / 2, PP = OH * OW positions per image, images back to back.  Tap (kh, kw) pairs g at q
with X_(kh, kw)[q] = in(x)[img, 2 oh + kh - pad, 2 ow + kw - pad], a zero where the row or the column leaves the map.  A chunk is the
positions of ceil(n / chunks) whole images; its MFMA step t holds the 32 positions from the chunk's first on (the last step padded with
zeros).  A block runs synth.emulate_split_dot(form="units") over its chunk with g in the role of w; the reduce kernel adds the chunks'
partials in chunk order in fp32."""
import numpy as np

from offk_amd import synth

KT = 32                                   # positions per MFMA step
PADS = {7: 3, 5: 2}


def geometry(H, W):
    """(OW, PP): positions per output row and per image; H, W the INPUT map"""
    return W // 2, (H // 2) * (W // 2)


def chunk_bounds(n, H, W, chunks):
    """[(first position, end position)] of the chunks: ceil(n / chunks) whole images each, the last one what is left"""
    _, PP = geometry(H, W)
    ipc = -(-n // chunks)
    assert chunks == -(-n // ipc), "the plan leaves no chunk empty"
    return [(b * PP, min(n, b + ipc) * PP) for b in range(0, n, ipc)]


def operands(g, x, k, relu_in=False):
    """g [n, H/2, W/2, Co], x [n, H, W, Ci] -> (G [Q, Co], {(kh, kw): X [Q, Ci]}): per tap the pair of operand matrices in the kernel's
    position order, Q = n * PP; X of a tap is in(x) at the tap's pixel, zeros where it lies outside the map."""
    g = np.asarray(g, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    if relu_in:
        x = np.maximum(x, np.float32(0))
    n, H, W, Ci = x.shape
    OH, OW = H // 2, W // 2
    assert g.shape[:3] == (n, OH, OW) and H % 2 == 0 and W % 2 == 0
    pad = PADS[k]
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    G = np.ascontiguousarray(g.reshape(n * OH * OW, -1))
    taps = {}
    for kh in range(k):
        for kw in range(k):
            taps[(kh, kw)] = np.ascontiguousarray(xp[:, kh:kh + 2 * OH:2, kw:kw + 2 * OW:2].reshape(n * OH * OW, Ci))
    return G, taps


def emulate_chunked(G, taps, bounds, k, skip=None):
    """dW [Co, Ci, k, k] (fp32) as the kernel and the reduce compute it: per chunk synth.emulate_split_dot(form="units") over its positions in
    steps of 32 (g as w), the chunks' partials added in chunk order.  skip: index into synth.SPLIT_PRODUCTS of a product to leave out."""
    Co, Ci = G.shape[1], taps[(0, 0)].shape[1]
    xs = np.concatenate([taps[(kh, kw)] for kh in range(k) for kw in range(k)], axis=1)       # [Q, k k Ci]: the taps share g
    total = None
    for qb, qe in bounds:
        part = synth.emulate_split_dot(np.ascontiguousarray(G[qb:qe].T), np.ascontiguousarray(xs[qb:qe].T), form="units", skip=skip)
        total = part if total is None else total + part                                      # fp32, chunk order
    return np.ascontiguousarray(total.reshape(k, k, Ci, Co).transpose(3, 2, 0, 1))


def terms(G, taps, k):
    """(ref64, dropped64, sum|g x|), each [Co, Ci, k, k]: synth.split_terms with g as w"""
    Co, Ci = G.shape[1], taps[(0, 0)].shape[1]
    xs = np.concatenate([taps[(kh, kw)] for kh in range(k) for kw in range(k)], axis=1)
    out = synth.split_terms(np.ascontiguousarray(G.T), np.ascontiguousarray(xs.T))
    return tuple(np.ascontiguousarray(t.reshape(k, k, Ci, Co).transpose(3, 2, 0, 1)) for t in out)
