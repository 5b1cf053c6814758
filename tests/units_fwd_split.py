"""What the tests of the split-fp32 units forward share (tests/test_units_fwd_split_abi.py on the CPU, tests/test_gpu_units_fwd_split.py on
the GPU; tests/test_gpu_train_ranges.py): the CPU model of csrc/units_fwd_split.hip's arithmetic, the names of the four parameters of a
site's stacked reduce, and below them what the GPU files share -- the inequality of tests/split_bound.py asserted of the G_ / D_ regions a
handle holds, with the printed figures.  A helper module like tests/wgrad_split.py: no tests of its own; the model itself is numpy only.

The kernel's contraction index is the channel: one 32-k MFMA step per 32 consecutive channels over the whole C, in increasing order, no
chunks -- synth.emulate_split_dot(form="units") over the whole C as it stands; then v = (A1 + A2) + bias in fp32, G = max(v, 0) for
the 128 gen outputs, D = v for the 32 down outputs."""
import numpy as np

from offk_amd import spec, synth

from . import split_bound as sb
from .exact import down_rows

GEN = 128
GEN_W, DOWN_W, GEN_B, DOWN_B = "motion_conv_gen_%s.weight", "motion_spatial_down_%s.weight", "motion_conv_gen_%s.bias", "motion_spatial_down_%s.bias"


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


# ---- on the GPU: the inequality asserted of what a handle holds ----

def sample(n, max_rows):
    rows = np.arange(n)
    if max_rows is not None and n > max_rows:
        rows = np.unique(np.concatenate((rows[:32], rows[-32:], rows[::max(1, n // (max_rows - 64))])))
    return rows


def check_site(tag, h, B, L, slice_mode, si, x, w160, bias, max_rows=None, default=None):
    """Asserts the inequality for G_<site> (every row) and D_<site> (every row of the slice) on the operands (w160, x rows).  c_acc: the
    emulation on all rows, or (max_rows) on a sample of them: the first and last 32 and a stride between; every row is a contraction of
    its own, so a sampled row's emulation is what the full run gives for it.  Returns (emulated c_acc, measured accumulation constant)."""
    site, C, H = spec.SITES[si]
    HW, N = H * H, B * L
    X = x.float().permute(0, 2, 3, 1).reshape(N * HW, C).cpu().numpy()
    ref, dropped, mag = terms(w160, X, bias)
    rows = sample(N * HW, max_rows)
    c_emu = sb.c_acc(emulate(w160, X[rows], bias), ref[rows], dropped[rows], mag[rows])
    A = max(1.0, 2.0 * c_emu)
    G = h.region("G_" + site, 128).cpu().numpy().astype(np.float64)
    Dg = h.region("D_" + site, 32).view(-1, HW, 32).cpu().numpy().astype(np.float64)
    dr = down_rows(B, L, slice_mode)
    frames = [n for n in range(N) if dr[n] >= 0]
    D = np.stack([Dg[dr[n]] for n in frames]).reshape(-1, 32)
    drows = np.concatenate([np.arange(n * HW, (n + 1) * HW) for n in frames])
    assert sorted(dr[n] for n in frames) == list(range(Dg.shape[0]))
    unit = np.maximum(sb.EPS * mag, 1e-300)
    g, d = slice(0, GEN), slice(GEN, 160)
    over_g = sb.excess_map(G, np.maximum(ref[:, g], 0.0), dropped[:, g], mag[:, g], A)
    over_d = sb.excess_map(D, ref[drows, d], dropped[drows, d], mag[drows, d], A)
    pos = G > 0
    c_gpu = max(float((np.abs(G - (ref - dropped)[:, g]) / unit[:, g])[pos].max()) if pos.any() else 0.0,
                float((np.abs(D - (ref - dropped)[drows, d]) / unit[drows, d]).max()))
    err = np.concatenate((np.abs(G - np.maximum(ref[:, g], 0.0)).reshape(-1), np.abs(D - ref[drows, d]).reshape(-1)))
    line = "%s: c_acc emulated %.3f (%d of %d rows) -> A %.3f | gpu accumulation %.3f | dropped (exact) max %.3f | err max %.3e rms %.3e" % (
        tag, c_emu, len(rows), N * HW, A, c_gpu, float((np.abs(dropped) / unit).max()), float(err.max()), float(np.sqrt((err ** 2).mean())))
    if default is not None:
        G0, D0 = default
        D0 = np.stack([D0.reshape(-1, HW, 32)[dr[n]] for n in frames]).reshape(-1, 32)
        e0 = np.concatenate((np.abs(G0 - np.maximum(ref[:, g], 0.0)).reshape(-1), np.abs(D0 - ref[drows, d]).reshape(-1)))
        line += " | default entry: err max %.3e rms %.3e" % (float(e0.max()), float(np.sqrt((e0 ** 2).mean())))
    print(line)
    assert not G[mag[:, g] == 0].any() and not D[mag[drows, d] == 0].any(), "%s: elements with sum|w x| = 0 are not exactly 0" % tag
    for name, ov in (("G", over_g), ("D", over_d)):
        assert float(ov.max()) <= 0.0, "%s: %s element %d misses the limit by %.3e" % (tag, name, int(ov.argmax()), float(ov.max()))
    return c_emu, c_gpu
