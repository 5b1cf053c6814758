"""CPU checks of offk_off_units_backward_feats_typed (dX in the maps' own 16-bit dtype): the header declares it and states its
contract, the binding has it, the library exports it under the unchanged ABI version, a handle-less call fails cleanly without a
GPU, and its four kernels sit in an object of their own, built with the flags of the other training-side objects, without spills
or scratch, beside an fp32 object that keeps exactly its two kernels."""
import ctypes
import importlib.util
import inspect
import os
import re

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "offk_off_units_backward_feats_typed"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_entry_and_its_contract():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % NAME, src)
    assert m, NAME
    assert re.sub(r"\s+", " ", m.group(1)) == ("offk_handle* h, void* stream, void* workspace, int grad_dtype, "
                                               "void* const dfeats[OFFK_NUM_SITES], int layout, int accumulate")
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    doc = re.sub(r"\s*\n \*\s*", " ", src[src.index("the same gradient in the maps' own 16-bit dtype"):src.index("int %s(" % NAME)])
    for needle in ("enum offk_feat_dtype", "OFFK_FEAT_F32 forwards to offk_off_units_backward_feats", "OFFK_FEAT_BF16", "OFFK_FEAT_F16",
                   "rounded ONCE, to nearest-even", "bit-equal to dx32.to(dtype)", "+-Inf", "subnormal results are kept",
                   "rne16(widen(old) + new)", "bit-equal to (old.float() + dx32).to(dtype)", "A NaN, or the sign of a zero sum",
                   "16-byte aligned", "overlap", "real byte size", "OFFK_ERR_INVALID", "unknown grad_dtype", "capturable",
                   "units:feature-map gradient (dX, NCHW, bf16)"):
        assert needle in doc, needle


def test_binding_has_seven_arguments():
    assert NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 7 and args[3] is ctypes.c_int
    # the untyped entry keeps its six
    assert len(_lib.SIGNATURES["offk_off_units_backward_feats"][1]) == 6


def test_wrapper_takes_a_dtype():
    from offk_amd import runtime
    sig = inspect.signature(runtime.OffForward.off_units_backward_feats)
    assert sig.parameters["dtype"].default is torch.float32


def test_symbol_is_exported_and_fails_cleanly_without_a_handle(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME)
    assert built.offk_abi_version() == 10
    arr = (ctypes.c_void_p * 9)()
    for dt in (_lib.FEAT_BF16, _lib.FEAT_F16):
        assert built.offk_off_units_backward_feats_typed(None, None, None, dt, arr, 0, 0) == -1
        assert b"offk_off_units_backward_feats_typed: null argument" in built.offk_last_error(None)
    # OFFK_FEAT_F32 is the untyped entry, in its own words
    assert built.offk_off_units_backward_feats_typed(None, None, None, _lib.FEAT_F32, arr, 0, 0) == -1
    assert b"offk_off_units_backward_feats: null argument" in built.offk_last_error(None)


def test_kernel_object_holds_the_four_kernels_without_spills(built):
    path = os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "build.py")
    sp = importlib.util.spec_from_file_location("offk_build_feat_grad16", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    assert "units_dx_f16.hip" in mod.SOURCES and mod.EXTRA_FLAGS["units_dx_f16.hip"] == mod.EXTRA_FLAGS["units_bwd.hip"]
    assert mod.INCLUDED_SOURCES["units_dx_f16.hip"] == ("units_dx.hip",)
    cos = mod._code_objects(os.path.join(mod.OBJ, "units_dx_f16.o"))
    try:
        ks = [k for co in cos for k in mod.kernel_resources(co)]
    finally:
        for p in cos:
            os.remove(p)
    # <NCHW, element kind>: 1 = bf16, 2 = fp16 (enum offk_feat_dtype)
    assert sorted(k["name"].split("(")[0] for k in ks) == ["void offk::units_dx16_kernel<false, 1>", "void offk::units_dx16_kernel<false, 2>",
                                                           "void offk::units_dx16_kernel<true, 1>", "void offk::units_dx16_kernel<true, 2>"]
    for k in ks:        # one block of four waves per CU, as the fp32 kernels: nothing in memory
        assert k["vgpr_count"] <= 512 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
