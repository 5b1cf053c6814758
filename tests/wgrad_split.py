"""What the tests of the split-fp32 weight gradient share (tests/test_wgrad_split_abi.py on the CPU, tests/test_gpu_wgrad_split.py on the
GPU; tests/test_gpu_train_ranges.py): the CPU model of csrc/units_wgrad_split.hip's CHUNKED arithmetic, and below it what the GPU files
share -- the GEMM's operands read back from a handle, and the inequality of tests/split_bound.py asserted of a result with the printed
figures.  A helper module like tests/arena.py: no tests of its own; the model itself is numpy only.

The kernel's contraction index runs over K-tiles: 32 pixels of one frame, ceil(HW / 32) tiles per frame, pad pixels zeros.  A block
owns `kpb` consecutive K-tiles (a chunk) and runs synth.emulate_split_dot(form="units") over them -- one 32-k MFMA step per K-tile, a in
the role of w, X in the role of x; the reduce kernel then adds the chunks' partial tiles in chunk order in fp32, starting from 0."""
import numpy as np
import torch

from offk_amd import spec, synth

from . import split_bound as sb
from .exact import down_rows
from .units_fwd_split import DOWN_W, GEN_W

KT = 32                                   # pixels per K-tile
KPB = [4, 4, 4, 4, 13]                    # K-tiles per block at tests/units_grad.py's SHAPES: max(4, ceil(332 N / 1536))


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


# ---- on the GPU: the operands a handle holds, and the inequality asserted of a result ----

def dw_t(got, si):
    """[C, 160]: the two weight gradients of site si, transposed as emulate_chunked has them"""
    site, C, _H = spec.SITES[si]
    return torch.cat((got[GEN_W % site].reshape(128, C), got[DOWN_W % site].reshape(32, C))).t().contiguous()


def site_operands(h, B, L, slice_mode, si, x):
    """The GEMM's own operands of site si in K-tile order on the host: a [K, 160] from the dG_ / dD_ regions (the dD part at row r(f),
    zeros outside the slice) and X [K, C] from the map (any dtype, any layout), frames padded to whole K-tiles."""
    site, C, H = spec.SITES[si]
    HW, N, P = H * H, B * L, B * (L - 1)
    a = torch.zeros(N, HW, 160, device="cuda")
    a[..., :128] = h.region("dG_" + site, 128).view(N, HW, 128)
    dD = h.region("dD_" + site, 32).view(P, HW, 32)
    for n, r in enumerate(down_rows(B, L, slice_mode)):
        if r >= 0:
            a[n, :, 128:] = dD[r]
    xr = x.float().permute(0, 2, 3, 1).reshape(N, HW, C)
    return pad_ktiles(a.cpu().numpy()), pad_ktiles(xr.cpu().numpy())


def check_inequality(tag, got, a, x, kpb, got32=None, max_cols=None):
    """Asserts, per element and none excluded, |got - ref64| <= |dropped64| + A 2^-24 sum|a x| + 2^-24 |ref64|, A = max(1, 2 c_acc), for got
    [C, 160] on the operands (a, x).  c_acc: the chunked emulation on the same operands -- on all C channel columns, or (max_cols) on a
    sample of them: the first and last 32 and a stride between; every column is a contraction of its own, so a sampled column's emulation
    is what the full run gives for it.  Prints the emulated and the measured accumulation constants (the latter on all elements) and the
    errors against fp64, beside them the default entry's when given."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    ref, dropped, mag = terms(a, x)
    assert got.shape == ref.shape
    C = x.shape[1]
    cols = np.arange(C)
    if max_cols is not None and C > max_cols:
        cols = np.unique(np.concatenate((cols[:32], cols[-32:], cols[::max(1, C // (max_cols - 64))])))
    c_emu = sb.c_acc(emulate_chunked(a, x[:, cols], kpb), ref[cols], dropped[cols], mag[cols])
    A = max(1.0, 2.0 * c_emu)
    unit = np.maximum(sb.EPS * mag, 1e-300)
    err = np.abs(got - ref)
    c_gpu = float((np.abs(got - (ref - dropped)) / unit).max())
    line = "%s: c_acc emulated %.3f (%d of %d columns) -> A %.3f | gpu accumulation %.3f | dropped (exact) max %.3f | err max %.3e rms %.3e" % (
        tag, c_emu, len(cols), C, A, c_gpu, float((np.abs(dropped) / unit).max()), float(err.max()), float(np.sqrt((err ** 2).mean())))
    if got32 is not None:
        e32 = np.abs(np.asarray(got32.detach().cpu(), dtype=np.float64) - ref)
        line += " | default entry: err max %.3e rms %.3e" % (float(e32.max()), float(np.sqrt((e32 ** 2).mean())))
    print(line)
    zero = mag == 0
    assert not got[zero].any(), "%s: %d elements with sum|a x| = 0 are not exactly 0" % (tag, int((got[zero] != 0).sum()))
    over = sb.excess_map(got, ref, dropped, mag, A)
    assert float(over.max()) <= 0.0, "%s: element %d misses the limit by %.3e (err %.3e)" % (tag, int(over.argmax()), float(over.max()),
                                                                                            float(err.reshape(-1)[over.argmax()]))
    return c_emu, c_gpu
