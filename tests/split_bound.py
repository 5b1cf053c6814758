"""The inequality every split-fp32 test asserts, once:

    |got - exact| <= |dropped64| + A 2^-24 magnitude + 2^-24 |ref64| [+ 2^-24 |exact| when accumulating onto a base],
    exact = ref64 (+ base),   A = max(1, 2 c_acc),

with (ref64, dropped64, magnitude) from synth.split_terms on the operands in the kernel's own K order and c_acc the accumulation
constant of the CPU emulation on the same operands (synth.split_c_acc), never of the kernel's output.  The helper modules
(tests/conv_dgrad_split.py, tests/conv_s2_dgrad_split.py, tests/conv_wgrad_split.py, tests/conv_s2_wgrad_split.py, tests/wgrad_split.py,
tests/units_fwd_split.py) build the operands and the emulation of their kernel; what is asserted of them is here.  The CPU tests that
leave out one issued product at a time (tests/test_conv_*_split_abi.py, tests/test_wgrad_split_abi.py, tests/test_units_fwd_split_abi.py)
show that this one copy rejects a lost product.  numpy only, no torch, no tests of its own."""
import numpy as np

from offk_amd import synth

EPS = synth.SPLIT_EPS


def c_acc(emulated, ref, dropped, mag):
    return float(synth.split_c_acc(emulated, ref, dropped, mag).max())


def excess_map(got, ref, dropped, mag, A, base=None):
    """per element |got - exact| - bound: <= 0 where the inequality holds"""
    bound = np.abs(dropped) + A * EPS * mag + EPS * np.abs(ref)
    exact = ref
    if base is not None:
        exact = ref + np.asarray(base, dtype=np.float64)
        bound = bound + EPS * np.abs(exact)
    return np.abs(np.asarray(got, dtype=np.float64) - exact) - bound


def excess(got, ref, dropped, mag, A, base=None):
    return float(excess_map(got, ref, dropped, mag, A, base).max())


def assert_discriminates(what, emulate, ref, dropped, mag, parts=(Ellipsis,)):
    """The inequality holds for the CPU emulation `emulate(None)` with A = max(1, 2 c_acc) of that emulation, what is dropped stays within
    synth.SPLIT_DROP_BOUND and an element without terms is exactly 0; with any one of the six issued products left out (`emulate(skip)`)
    the inequality breaks, in every one of `parts` (index expressions into the output; the whole of it by default)."""
    emu = emulate(None)
    c = c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * c)
    print("%s: emulated c_acc %.3f, A %.3f, dropped max %.3f of %.3f" % (
        what, c, A, float((np.abs(dropped) / np.maximum(EPS * mag, 1e-300)).max()), synth.SPLIT_DROP_BOUND))
    assert excess(emu, ref, dropped, mag, A) <= 0.0
    assert float((np.abs(dropped) - synth.SPLIT_DROP_BOUND * EPS * mag).max()) <= 0.0
    assert np.array_equal(emu[mag == 0], np.zeros(int((mag == 0).sum()), dtype=np.float32))
    for skip in range(len(synth.SPLIT_PRODUCTS)):
        lost = excess_map(emulate(skip), ref, dropped, mag, A)
        for part in parts:
            assert float(lost[part].max()) > 0.0, (skip, synth.SPLIT_PRODUCTS[skip], part)


def planes_used(x):
    """How many bf16 planes the values of x need: 1 (bf16-valued), 2 (fp16-valued, or any value of <= 16 significant bits), 3."""
    _h, m, l = synth.cut3(x)
    return 3 if l.any() else (2 if m.any() else 1)


# SPLIT_PRODUCTS indices a map form does not issue (their x plane does not exist): bf16 maps have x_h only, fp16 maps x_h and x_m
NOT_ISSUED = {1: tuple(i for i, (_a, b) in enumerate(synth.SPLIT_PRODUCTS) if b > 0), 2: tuple(i for i, (_a, b) in enumerate(synth.SPLIT_PRODUCTS) if b > 1),
              3: ()}
