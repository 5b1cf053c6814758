"""CPU checks of offk_off_units_backward_feats_split (the units' feature-map gradient in split-fp32 arithmetic on the bf16 matrix
pipe): the header declares it and the binding has it with the typed entry's argument types under the unchanged ABI version; a
handle-less call fails cleanly without a GPU; the wrappers refuse an unknown `arith` / `feat_grad_arith` without a device; and the
inequality tests/test_gpu_feat_grad_split.py asserts DISCRIMINATES at K = 160: the CPU emulation of the kernel's arithmetic
satisfies it on worst-case mantissas, the same emulation with any one of the six kept plane products left out does not."""
import ctypes
import os
import re

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "offk_off_units_backward_feats_split"
EPS = synth.SPLIT_EPS


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_entry_and_the_binding_has_it():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % NAME, src)
    assert m, NAME
    assert re.sub(r"\s+", " ", m.group(1)) == ("offk_handle* h, void* stream, void* workspace, int grad_dtype, "
                                               "void* const dfeats[OFFK_NUM_SITES], int layout, int accumulate")
    assert NAME in _lib.SIGNATURES
    typed = _lib.SIGNATURES["offk_off_units_backward_feats_typed"]
    assert _lib.SIGNATURES[NAME][0] is typed[0] and list(_lib.SIGNATURES[NAME][1]) == list(typed[1]) and len(typed[1]) == 7
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    doc = src[src.index("split-fp32 arithmetic on the bf16 matrix pipe (additive, opt-in"):src.index("int %s(" % NAME)]
    for needle in ("(2^-21 + 2^-30)", "NaN", "graph replay", "dx32s.to(dtype)", "(old.float() + dx32s).to(dtype)", "NOT bit-equal",
                   "TWO launches", "capturable", "(dX, NCHW, split)", "16-byte aligned"):
        assert needle in doc, needle


def test_symbol_is_exported_and_fails_cleanly_without_a_handle(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME)
    assert built.offk_abi_version() == 10
    arr = (ctypes.c_void_p * 9)()
    assert getattr(built, NAME)(None, None, None, 0, arr, 0, 0) == -1
    assert b"offk_off_units_backward_feats_split: null argument" in built.offk_last_error(None)


def test_unknown_arith_is_refused_without_a_device():
    from offk_amd import off_module, runtime
    assert runtime.FEAT_GRAD_ARITHS == ("fp32", "f32split")
    blank = object.__new__(runtime.OffForward)            # no handle, no device: the check comes before anything touches either
    for bad in ("bf16", "split", None, "FP32"):
        with pytest.raises(ValueError, match="arith must be one of"):
            runtime.OffForward.off_units_backward_feats(blank, arith=bad)
        with pytest.raises(ValueError, match="feat_grad_arith must be one of"):
            off_module.OFFUnits(1, 2, "rgb", feat_grad=True, feat_grad_arith=bad)
    assert off_module.OFFUnits(1, 2).feat_grad_arith == "fp32"
    assert off_module.OFFUnits(1, 2, feat_grad=True, feat_grad_arith="f32split").feat_grad_arith == "f32split"


def gpu_inequality_excess(got, ref, dropped, mag, A):
    """max over elements of |got - ref64| - (|dropped64| + A 2^-24 sum|a w| + 2^-24 |ref64|): <= 0 where the GPU test's inequality holds."""
    return float((np.abs(got.astype(np.float64) - ref) - (np.abs(dropped) + A * EPS * mag + EPS * np.abs(ref))).max())


@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
def test_the_gpu_inequality_discriminates_at_k_160(pattern, signs):
    rows, C, K = 96, 64, 160
    a = synth.make_adversarial((rows, K), pattern, "same", seed=3, relu=(pattern == 0x7FFFFF))
    w = synth.make_adversarial((C, K), pattern, signs, seed=4) * np.float32(2.0 ** -4)
    ref, dropped, mag = synth.split_terms(w, a)
    emu = synth.emulate_split_dot(w, a, form="units")
    A = max(1.0, 2.0 * float(synth.split_c_acc(emu, ref, dropped, mag).max()))
    assert gpu_inequality_excess(emu, ref, dropped, mag, A) <= 0.0
    for skip in range(len(synth.SPLIT_PRODUCTS)):
        lost = synth.emulate_split_dot(w, a, form="units", skip=skip)
        assert gpu_inequality_excess(lost, ref, dropped, mag, A) > 0.0, (skip, synth.SPLIT_PRODUCTS[skip])
