"""What the tests of the split-fp32 weight gradient share (tests/test_wgrad_split_abi.py on the CPU, tests/test_gpu_wgrad_split.py on the
GPU): the CPU model of csrc/units_wgrad_split.hip's CHUNKED arithmetic; the inequality both files assert of it is tests/split_bound.py's.  A
helper module like tests/arena.py: no tests of its own, no torch.

The kernel's contraction index runs over K-tiles: 32 pixels of one frame, ceil(HW / 32) tiles per frame, pad pixels zeros.  A block
owns `kpb` consecutive K-tiles (a chunk) and runs synth.emulate_split_dot(form="units") over them -- one 32-k MFMA step per K-tile, a in
the role of w, X in the role of x; the reduce kernel then adds the chunks' partial tiles in chunk order in fp32, starting from 0."""
import numpy as np

from offk_amd import synth

KT = 32                                   # pixels per K-tile


def pad_ktiles(rows):
    """[N, HW, ch] -> [N * ceil(HW / 32) * 32, ch]: every frame padded with zero pixels to whole K-tiles, frames in order."""
    rows = np.asarray(rows, dtype=np.float32)
    n, hw, ch = rows.shape
    tpf = (hw + KT - 1) // KT
    out = np.zeros((n, tpf * KT, ch), dtype=np.float32)
    out[:, :hw] = rows
    return out.reshape(n * tpf * KT, ch)


def emulate_chunked(a, x, kpb, skip=None):
    """dW^T [C, 160] (fp32) of a [K, 160], x [K, C] (K a multiple of 32, K-tile order) as the kernel and the reduce compute it: chunks of kpb
    K-tiles, each in the split arithmetic, added in chunk order.  skip: index into synth.SPLIT_PRODUCTS of a product to leave out."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert a.shape[0] == x.shape[0] and a.shape[0] % KT == 0
    total = np.zeros((x.shape[1], a.shape[1]), dtype=np.float32)
    step = kpb * KT
    for k0 in range(0, a.shape[0], step):
        slab = synth.emulate_split_dot(np.ascontiguousarray(a[k0:k0 + step].T), np.ascontiguousarray(x[k0:k0 + step].T), form="units", skip=skip)
        total = total + slab                       # fp32, chunk order
    return total


def terms(a, x):
    """(ref64, dropped64, sum|a x|) of dW^T [C, 160] = x^T a: synth.split_terms with a as w.  `dropped` is what the planes of THESE operands
    drop: all of a_m x_l + a_l x_m + a_l x_l for fp32 maps, a_l x_m alone where x is fp16-valued (x_l = 0), nothing where it is bf16-valued."""
    return synth.split_terms(np.ascontiguousarray(np.asarray(a, dtype=np.float32).T), np.ascontiguousarray(np.asarray(x, dtype=np.float32).T))
