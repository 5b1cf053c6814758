"""CPU checks of offk_off_units_backward_feats (the gradient w.r.t. the nine feature maps): the header declares it and the binding
has it, the library exports it under the unchanged ABI version, a handle-less call fails cleanly without a GPU, its kernel sits in
an object of its own, built with the flags of the other training-side objects and without spills, and the wrapper's pure
helpers -- which sites an autograd node's needs_input_grad asks for, which sites a `sites` argument names -- work on the CPU."""
import ctypes
import os
import re

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "offk_off_units_backward_feats"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_entry():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % NAME, src)
    assert m, NAME
    assert re.sub(r"\s+", " ", m.group(1)) == ("offk_handle* h, void* stream, void* workspace, float* const dfeats[OFFK_NUM_SITES], "
                                               "int layout, int accumulate")
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 6
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    doc = src[src.index("gradient w.r.t. the nine feature maps"):src.index("int %s(" % NAME)]
    for needle in ("16-byte aligned", "accumulate", "OFFK_FEAT_NHWC", "captured graph", "capturable", "bit for bit"):
        assert needle in doc, needle
    # the sentence about what train_off.py leaves trainable no longer says "exactly the OFF units' tensors"
    assert "leaves exactly the" not in src


def test_symbol_is_exported_and_fails_cleanly_without_a_handle(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME)
    assert built.offk_abi_version() == 10
    arr = (ctypes.c_void_p * 9)()
    assert built.offk_off_units_backward_feats(None, None, None, arr, 0, 0) == -1
    assert b"offk_off_units_backward_feats: null argument" in built.offk_last_error(None)


def test_kernel_object_has_no_spills(built):
    import importlib.util
    path = os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "build.py")
    sp = importlib.util.spec_from_file_location("offk_build_feat_grad", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    assert "units_dx.hip" in mod.SOURCES and mod.EXTRA_FLAGS["units_dx.hip"] == mod.EXTRA_FLAGS["units_bwd.hip"]
    cos = mod._code_objects(os.path.join(mod.OBJ, "units_dx.o"))
    try:
        ks = [k for co in cos for k in mod.kernel_resources(co)]
    finally:
        for p in cos:
            os.remove(p)
    assert sorted(k["name"].split("(")[0] for k in ks) == ["void offk::units_dx_kernel<false>", "void offk::units_dx_kernel<true>"]
    for k in ks:        # one block of four waves per CU (its LDS): 512 registers per wave are there, none may be in memory
        assert k["vgpr_count"] <= 512 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k


def test_needs_input_grad_to_sites():
    from offk_amd import runtime
    none = (False,) * 9
    assert runtime.feat_grad_sites(none) == []
    assert runtime.feat_grad_sites((True,) * 9) == list(range(9))
    # the module's node: (mod, drop, nine maps, 54 parameters) -- only 5a and 5b un-frozen
    flags = (False, False) + (False,) * 7 + (True, True) + (True,) * 54
    assert runtime.feat_grad_sites(flags, first=2) == [7, 8]
    assert [spec.SITES[i][0] for i in runtime.feat_grad_sites(flags, first=2)] == ["5a", "5b"]
    with pytest.raises(ValueError, match="nine"):
        runtime.feat_grad_sites((True,) * 5)
    assert runtime.feat_grad_sites_mask(None) == [True] * 9
    assert runtime.feat_grad_sites_mask([8, 0]) == [True] + [False] * 7 + [True]
    assert runtime.feat_grad_sites_mask([]) == [False] * 9
    for bad in ([9], [-1], [3, 3]):
        with pytest.raises(ValueError, match="distinct"):
            runtime.feat_grad_sites_mask(bad)


def test_module_node_takes_the_maps_as_inputs_only_with_feat_grad():
    """OFFUnits(feat_grad=True) hands the maps to the autograd node as tensor arguments; the default keeps today's node."""
    from offk_amd import off_module
    seen = {}

    class Stop(Exception):
        pass

    def spy(name):
        def apply(*args):
            seen[name] = args
            raise Stop()
        return apply

    B, L = 1, 2
    feats = [torch.zeros(B * L, C, H, H) for _n, C, H in spec.SITES]
    old = off_module._OFFUnitsFn.apply, off_module._OFFUnitsFeatFn.apply
    off_module._OFFUnitsFn.apply, off_module._OFFUnitsFeatFn.apply = spy("plain"), spy("feat")
    try:
        for fg in (False, True):
            u = off_module.OFFUnits(B, L, "rgb", feat_grad=fg)
            assert u.feat_grad is fg
            u.eval()
            real = torch.Tensor.is_cuda
            with pytest.raises(Stop):
                torch.Tensor.is_cuda = property(lambda self: True)      # no device here: the node is never reached for real
                try:
                    u(feats)
                finally:
                    torch.Tensor.is_cuda = real
    finally:
        off_module._OFFUnitsFn.apply, off_module._OFFUnitsFeatFn.apply = old
    assert isinstance(seen["plain"][1], tuple) and len(seen["plain"][1]) == 9              # the maps inside a tuple: invisible to autograd
    assert all(torch.is_tensor(t) for t in seen["feat"][2:11]) and len(seen["feat"]) == 2 + 9 + 54
    assert off_module.OFFUnits(B, L).feat_grad is False
