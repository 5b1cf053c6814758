"""CPU checks of offk_off_units_backward_split (the units' backward with the weight-gradient GEMM in split-fp32 arithmetic on the bf16
matrix pipe): the header declares it and the binding has it under the unchanged ABI version; a handle-less call fails cleanly without a
GPU; the wrappers refuse an unknown `arith` / `wgrad_arith` without a device; and the inequality tests/test_gpu_wgrad_split.py asserts
DISCRIMINATES in the chunked form the kernel has: the CPU emulation of the kernel's arithmetic (tests/wgrad_split.py: chunks of four
K-tiles = 128 k in split arithmetic, slabs added in order in fp32) satisfies it on worst-case mantissas, the same emulation with any one
of the issued plane products left out does not -- for fp32 maps (six products), fp16-valued maps (five) and bf16-valued maps (three)."""
import ctypes
import os
import re

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from . import split_bound as sb
from . import wgrad_split as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "offk_off_units_backward_split"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_entry_and_the_binding_has_it():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % NAME, src)
    assert m, NAME
    assert re.sub(r"\s+", " ", m.group(1)) == ("offk_handle* h, void* stream, int feat_dtype, int layout, "
                                               "const void* const feats[OFFK_NUM_SITES], const offk_grad_view gm[OFFK_NUM_SITES], "
                                               "void* workspace, uint64_t drop_seed, double drop_p, float* grads, int accumulate")
    assert NAME in _lib.SIGNATURES
    cl = _lib.SIGNATURES["offk_off_units_backward_cl"]
    res, args = _lib.SIGNATURES[NAME]
    # the _cl entry's arguments with `layout` behind feat_dtype
    assert res is cl[0] and len(args) == 11 and list(args[:3]) == list(cl[1][:3]) and args[3] is ctypes.c_int and list(args[4:]) == list(cl[1][3:])
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    doc = src[src.index("weight gradient in split-fp32 arithmetic on the bf16 matrix pipe (additive, opt-in"):src.index("int %s(" % NAME)]
    for needle in ("(2^-21 + 2^-30)", "NaN", "graph", "NOT bit-equal", "THREE launches", "capturable", "bf16 maps", "fp16 maps", "a_l x_m",
                   "x.float()", "OFFK_PRECISION_F32SPLIT", "OFFK_FEAT_NHWC", "offk_train_workspace_bytes is unchanged", "backward-has-run"):
        assert needle in doc, needle


def test_symbol_is_exported_and_fails_cleanly_without_a_handle(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME)
    assert built.offk_abi_version() == 10
    arr = (ctypes.c_void_p * 9)()
    gv = (_lib.OffkGradView * 9)()
    assert getattr(built, NAME)(None, None, 0, 0, arr, gv, None, 0, 0.0, None, 0) == -1
    assert b"offk_off_units_backward_split: null argument" in built.offk_last_error(None)


def test_the_build_keeps_the_kernel_in_registers(built):
    """build.py's register guard covers the six forms of the GEMM, and refuses one that spills or uses scratch memory."""
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("offk_build", os.path.join(os.path.dirname(_lib.LIB_PATH), "build.py"))
    b = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(b)
    assert "units_wgrad_split.hip" in b.SOURCES and "-fno-slp-vectorize" in b.EXTRA_FLAGS["units_wgrad_split.hip"]
    obj = os.path.join(b.OBJ, "units_wgrad_split.o")
    cos = b._code_objects(obj)
    try:
        kernels = [k for co in cos for k in b.kernel_resources(co)]
    finally:
        for path in cos:
            os.remove(path)
    rows = b.check_register_resident("units_wgrad_split.hip", kernels)
    assert len(rows) == 6 and all(k["vgpr_count"] <= 256 and k["private_segment_fixed_size"] == 0 for k in rows)
    bad = [dict(k) for k in kernels]
    bad[0]["private_segment_fixed_size"] = 256
    with pytest.raises(RuntimeError, match="register guard failed"):
        b.check_register_resident("units_wgrad_split.hip", bad)
    with pytest.raises(RuntimeError, match="expected 6"):
        b.check_register_resident("units_wgrad_split.hip", kernels[:5])


def test_unknown_arith_is_refused_without_a_device():
    from offk_amd import off_module, runtime
    assert runtime.WGRAD_ARITHS == ("fp32", "f32split")
    blank = object.__new__(runtime.OffForward)            # no handle, no device: the check comes before anything touches either
    for bad in ("bf16", "split", None, "FP32"):
        with pytest.raises(ValueError, match="arith must be one of"):
            runtime.OffForward.off_units_backward(blank, None, None, arith=bad)
        with pytest.raises(ValueError, match="wgrad_arith must be one of"):
            off_module.OFFUnits(1, 2, "rgb", wgrad_arith=bad)
    assert off_module.OFFUnits(1, 2).wgrad_arith == "fp32"
    u = off_module.OFFUnits(1, 2, wgrad_arith="f32split")
    assert u.wgrad_arith == "f32split" and u.feat_grad_arith == "fp32"                 # independent of each other
    assert off_module.OFFUnits(1, 2, feat_grad=True, feat_grad_arith="f32split").wgrad_arith == "fp32"
    import inspect
    assert inspect.signature(runtime.OffForward.off_units_backward).parameters["arith"].default == "fp32"


def as_map_form(x, form):
    """fp32 values a map of that form can hold: "f32" as they are, "bf16" truncated to the leading plane, "f16" rounded to fp16."""
    if form == "bf16":
        return (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    if form == "f16":
        return x.astype(np.float16).astype(np.float32)
    return x


@pytest.mark.parametrize("form", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
def test_the_gpu_inequality_discriminates_in_the_chunked_form(pattern, signs, form):
    """K = 4800 (150 K-tiles, 38 chunks of four, the last one short), 160 x 96 outputs.  16-bit forms: the maps carry mantissa 0x7FE000
    (every bit an fp16 has; its truncation 0x7F0000 every bit a bf16 has), so that each plane such a map has is as full as it can be."""
    K, C, kpb = 4800, 96, 4
    a = synth.make_adversarial((K, 160), pattern, "same", seed=3, relu=(pattern == 0x7FFFFF))
    x = as_map_form(synth.make_adversarial((K, C), pattern if form == "f32" else 0x7FE000, signs, seed=4, k_axis=0) * np.float32(2.0 ** -4), form)
    nplanes = {"f32": 3, "f16": 2, "bf16": 1}[form]
    assert sb.planes_used(x) == nplanes and sb.planes_used(a) == 3
    ref, dropped, mag = ws.terms(a, x)
    if form == "bf16":
        assert not dropped.any()                                     # nothing is dropped on bf16 maps
    emu = ws.emulate_chunked(a, x, kpb)
    c = sb.c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * c)
    print("pattern 0x%06X %-11s %-4s maps: emulated c_acc %.3f, A %.3f, dropped max %.3f" % (
        pattern, signs, form, c, A, float((np.abs(dropped) / np.maximum(sb.EPS * mag, 1e-300)).max())))
    assert sb.excess(emu, ref, dropped, mag, A) <= 0.0
    for skip in range(len(synth.SPLIT_PRODUCTS)):
        lost = ws.emulate_chunked(a, x, kpb, skip=skip)
        if skip in sb.NOT_ISSUED[nplanes]:
            # a product the form does not issue adds exact zeros: the three- / five-product kernel computes the six-product values
            assert np.array_equal(lost, emu), (skip, synth.SPLIT_PRODUCTS[skip])
        else:
            assert sb.excess(lost, ref, dropped, mag, A) > 0.0, (skip, synth.SPLIT_PRODUCTS[skip])
