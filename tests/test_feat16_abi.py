"""CPU checks of the 16-bit feature-map entries (offk_forward_typed and its siblings): the header's enum and the binding agree,
the symbols are exported, a handle-less call fails cleanly without a GPU, and the new units kernel compiles without spills."""
import ctypes
import os
import re

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = ("offk_forward_typed", "offk_forward_parts_typed", "offk_off_units_fused_typed")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_dtype_enum():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    m = re.search(r"enum offk_feat_dtype \{([^}]*)\}", src)
    assert m
    vals = dict((k, int(v)) for k, v in re.findall(r"(OFFK_FEAT_\w+)\s*=\s*(\d+)", m.group(1)))
    assert vals == {"OFFK_FEAT_F32": 0, "OFFK_FEAT_BF16": 1, "OFFK_FEAT_F16": 2}
    assert (_lib.FEAT_F32, _lib.FEAT_BF16, _lib.FEAT_F16) == (0, 1, 2)
    for name in TYPED:
        assert re.search(r"\bint %s\(" % name, src), name
        assert name in _lib.SIGNATURES


def test_typed_symbols_are_exported(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in TYPED:
        assert hasattr(raw, name), name
    assert built.offk_abi_version() == 10


def test_handleless_calls_fail_with_a_message(built):
    feats = (ctypes.c_void_p * 9)()
    parts = (_lib.OffkFeatParts * 9)()
    for dt in (_lib.FEAT_BF16, _lib.FEAT_F16, 7):
        assert built.offk_forward_typed(None, None, dt, feats, None, None, None, None) == -1
        assert b"null argument" in built.offk_last_error(None)
        assert built.offk_forward_parts_typed(None, None, dt, parts, None, None, None, None) == -1
        assert built.offk_off_units_fused_typed(None, None, dt, feats, None) == -1
        assert b"null argument" in built.offk_last_error(None)


def test_units_kernel_for_16bit_maps_has_no_spills(built):
    import importlib.util
    path = os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "build.py")
    spec = importlib.util.spec_from_file_location("offk_build_f16", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    obj = os.path.join(mod.OBJ, "pw_tdiff_f16.o")
    cos = mod._code_objects(obj)
    try:
        ks = [k for co in cos for k in mod.kernel_resources(co) if "pw_tdiff_feat16_kernel" in k["name"]]
    finally:
        for p in cos:
            os.remove(p)
    assert len(ks) == 2                               # bf16 and fp16 forms
    for k in ks:                                      # eight waves per block, one block per CU: 256 registers per wave
        assert k["vgpr_count"] <= 256 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
