"""CPU checks of the 16-bit feature-map entries of the training side (offk_pw_reduce_typed, offk_off_units_typed,
offk_off_units_train_typed, offk_off_units_backward_typed): the header declares them and the binding has them, the library
exports them under the unchanged ABI version, a handle-less call fails cleanly without a GPU, and the four new kernel
instantiations (K1 and K1b on bf16 / fp16 maps) compile without spills inside the register budget of two blocks per CU."""
import ctypes
import os
import re

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = ("offk_pw_reduce_typed", "offk_off_units_typed", "offk_off_units_train_typed", "offk_off_units_backward_typed")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_typed_training_entries():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    for name in TYPED:
        m = re.search(r"\bint %s\(offk_handle\* h, void\* stream, int feat_dtype, ([^;]*);" % name, src)
        assert m, name
        assert "const void*" in m.group(1), name                 # the maps come as untyped pointers
        assert name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args[2] is ctypes.c_int   # (handle, stream, feat_dtype, ...)
    # the typed signatures are the untyped ones with feat_dtype in front of the maps
    for typed, plain in (("offk_off_units_typed", "offk_off_units"), ("offk_off_units_train_typed", "offk_off_units_train"),
                         ("offk_off_units_backward_typed", "offk_off_units_backward"), ("offk_pw_reduce_typed", "offk_pw_reduce")):
        assert len(_lib.SIGNATURES[typed][1]) == len(_lib.SIGNATURES[plain][1]) + 1
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    # the contract and the alignment are stated beside the declarations
    doc = src[src.index("16-bit feature maps on the training side"):src.index("int offk_pw_reduce_typed(")]
    assert "EQUAL VALUES" in doc and "8-byte aligned" in doc and "same LDS slots" in doc


def test_typed_training_symbols_are_exported(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in TYPED:
        assert hasattr(raw, name), name
    assert built.offk_abi_version() == 10


def test_handleless_calls_fail_with_a_message(built):
    feats = (ctypes.c_void_p * 9)()
    gv = (_lib.OffkGradView * 9)()
    for dt in (_lib.FEAT_F32, _lib.FEAT_BF16, _lib.FEAT_F16, 7):
        assert built.offk_pw_reduce_typed(None, None, dt, 0, None, None, None) == -1
        assert b"bad argument" in built.offk_last_error(None)
        assert built.offk_off_units_typed(None, None, dt, feats, None) == -1
        assert b"null argument" in built.offk_last_error(None)
        assert built.offk_off_units_train_typed(None, None, dt, feats, None, 7, 0.8) == -1
        assert b"null argument" in built.offk_last_error(None)
        assert built.offk_off_units_backward_typed(None, None, dt, feats, gv, None, 7, 0.8, None, 0) == -1
        assert b"null argument" in built.offk_last_error(None)


def _kernels(mod, obj_name, needle):
    obj = os.path.join(mod.OBJ, obj_name)
    cos = mod._code_objects(obj)
    try:
        return [k for co in cos for k in mod.kernel_resources(co) if needle in k["name"]]
    finally:
        for p in cos:
            os.remove(p)


def test_kernels_for_16bit_maps_have_no_spills(built):
    """pw_reduce_kernel<0, 1, FEAT> and pw_wgrad_kernel<FEAT>, FEAT = 1 (bf16), 2 (fp16): no VGPR spills, no private segment, and
    the budget their fp32 siblings are launched under -- __launch_bounds__(256, 2): four waves per block, two blocks per CU, so two
    waves per SIMD and 512 / 2 = 256 registers per wave."""
    import importlib.util
    path = os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "build.py")
    spec = importlib.util.spec_from_file_location("offk_build_f16_train", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    k1 = _kernels(mod, "pw_reduce_f16.o", "offk::pw_reduce_kernel<")
    k1b = _kernels(mod, "units_bwd.o", "offk::pw_wgrad_kernel<")
    names = sorted(k["name"].split("(")[0] for k in k1 + k1b)
    assert names == ["void offk::pw_reduce_kernel<0, 1, 1>", "void offk::pw_reduce_kernel<0, 1, 2>",
                     "void offk::pw_wgrad_kernel<0>", "void offk::pw_wgrad_kernel<1>", "void offk::pw_wgrad_kernel<2>"], names
    # the fp32 forms of K1 stay in their own object, alone
    f32 = sorted(k["name"].split("(")[0] for k in _kernels(mod, "pw_reduce.o", "offk::pw_reduce_kernel<"))
    assert f32 == ["void offk::pw_reduce_kernel<0, 0, 0>", "void offk::pw_reduce_kernel<0, 1, 0>"], f32
    new = [k for k in k1 + k1b if not k["name"].startswith("void offk::pw_wgrad_kernel<0>")]
    assert len(new) == 4
    for k in new:
        assert k["vgpr_count"] <= 256 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
