"""What the tests of the split-fp32 units forward share (tests/test_units_fwd_split_abi.py on the CPU, tests/test_gpu_units_fwd_split.py on
the GPU): the CPU model of csrc/units_fwd_split.hip's arithmetic; the inequality both files assert of it is tests/split_bound.py's.  A helper
module like tests/wgrad_split.py: no tests of its own, no torch.

The kernel's contraction index is the channel: one 32-k MFMA step per 32 consecutive channels over the whole C, in increasing order, no
chunks -- synth.emulate_split_dot(form="units") over the whole C as it stands; then v = (A1 + A2) + bias in fp32, G = max(v, 0) for
the 128 gen outputs, D = v for the 32 down outputs."""
import numpy as np

from offk_amd import synth

GEN = 128


def emulate(w, x, bias=None, skip=None):
    """v [M, 160] (fp32, before the ReLU) of x [M, C] rows and w [160, C] = [Wg ; Wd] as the kernel computes it.  skip: index into
    synth.SPLIT_PRODUCTS of a product to leave out."""
    v = synth.emulate_split_dot(np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32), form="units", skip=skip)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float32)[None, :]       # one fp32 add
    return v


def outputs(v):
    """(G, D) of the pre-activation v [M, 160]"""
    return np.maximum(v[:, :GEN], np.float32(0)), v[:, GEN:]


def terms(w, x, bias=None):
    """(ref64, dropped64, magnitude) of v [M, 160] = x w^T (+ bias): synth.split_terms; with a bias the reference includes it and the magnitude
    is sum|w x| + |b|.  `dropped` is what the planes of THESE operands drop: all of w_m x_l + w_l x_m + w_l x_l for fp32 maps, w_l x_m alone
    where x is fp16-valued (x_l = 0), nothing where it is bf16-valued."""
    ref, dropped, mag = synth.split_terms(np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32))
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)[None, :]
        ref, mag = ref + b, mag + np.abs(b)
    return ref, dropped, mag


def as_map_form(x, form):
    """fp32 values a map of that form can hold: "f32" as they are, "bf16" truncated to the leading plane, "f16" rounded to fp16."""
    if form == "bf16":
        return (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    if form == "f16":
        return x.astype(np.float16).astype(np.float32)
    return x
