"""What the tests of the fusion convs' split-fp32 weight gradient share (tests/test_conv_wgrad_split_abi.py on the CPU,
tests/test_gpu_conv_wgrad_split.py on the GPU): the K layout of csrc/conv_wgrad_split.hip in numpy and the CPU model of its CHUNKED
arithmetic; the inequality both files assert of them is tests/split_bound.py's.  A helper module like tests/wgrad_split.py: no tests of its own, no torch.

The K order is the one include/offk.h states for offk_conv2d_backward_weight_split.  K runs over positions q:
  k = 1: the pixels, q = (img * H + h) * W + w, PP = H * W per image;
  k = 3: pitch = 8 * ceil((W + 1) / 8) positions per row (W pixels, then zeros), PP = (H + 1) * pitch per image (H rows, then a row of
         zeros), q = img * PP + h * pitch + w, zeros outside [0, n * PP); tap (kh, kw) pairs g at q with x at q + (kh - 1) pitch + (kw - 1).
A chunk is the positions of ceil(n / chunks) whole images; its MFMA step t holds the 32 positions from the chunk's first on (the last step
padded with zeros).  A block runs synth.emulate_split_dot(form="units") over its chunk with g in the role of w; the reduce kernel adds the
chunks' partials in chunk order in fp32."""
import numpy as np

from offk_amd import synth

KT = 32                                   # positions per MFMA step


def geometry(H, W, k):
    """(pitch, PP): positions per row and per image"""
    if k == 1:
        return W, H * W
    pitch = 8 * ((W + 1 + 7) // 8)
    return pitch, (H + 1) * pitch


def chunk_bounds(n, H, W, k, chunks):
    """[(first position, end position)] of the chunks: ceil(n / chunks) whole images each, the last one what is left"""
    _, PP = geometry(H, W, k)
    ipc = -(-n // chunks)
    assert chunks == -(-n // ipc), "the plan leaves no chunk empty"
    return [(b * PP, min(n, b + ipc) * PP) for b in range(0, n, ipc)]


def _positions(t, k):
    """[n, H, W, C] -> [n * PP, C] in position order, pad positions zeros"""
    t = np.asarray(t, dtype=np.float32)
    n, H, W, C = t.shape
    if k == 1:
        return t.reshape(n * H * W, C)
    pitch, PP = geometry(H, W, k)
    out = np.zeros((n, H + 1, pitch, C), dtype=np.float32)
    out[:, :H, :W] = t
    return out.reshape(n * PP, C)


def operands(g, x, k, relu_in=False):
    """g [n, H, W, Co], x [n, H, W, Ci] -> (G [Q, Co], {(kh, kw): X [Q, Ci]}): per tap the pair of operand matrices in the kernel's position
    order, Q = n * PP; pad positions are zeros and X of a tap is x shifted by the tap with zeros outside the map."""
    g = np.asarray(g, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    if relu_in:
        x = np.maximum(x, np.float32(0))
    W = x.shape[2]
    pitch, _ = geometry(x.shape[1], W, k)
    G, X = _positions(g, k), _positions(x, k)
    Q = G.shape[0]
    taps = {}
    for kh in range(k):
        for kw in range(k):
            s = (kh - (k - 1) // 2) * pitch + (kw - (k - 1) // 2)
            sh = np.zeros_like(X)
            lo, hi = max(0, -s), min(Q, Q - s)
            if lo < hi:
                sh[lo:hi] = X[lo + s:hi + s]
            taps[(kh, kw)] = sh
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
