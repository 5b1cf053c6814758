"""CPU checks of the channels-last feature-map entries (offk_forward_cl and its siblings): the header and the binding agree, the
symbols are exported, a handle-less call fails cleanly without a GPU, the new units kernel compiles within its resources, and
the layout classifier of the Python wrapper tells NCHW from channels_last maps."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = ("offk_forward_cl", "offk_forward_parts_cl", "offk_off_units_fused_cl")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_entries():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    for name in CL:
        assert re.search(r"\bint %s\(offk_handle\* h, void\* stream, int feat_dtype," % name, src), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    assert _lib.SIGNATURES["offk_forward_cl"] == _lib.SIGNATURES["offk_forward_typed"]
    assert _lib.SIGNATURES["offk_forward_parts_cl"] == _lib.SIGNATURES["offk_forward_parts_typed"]
    assert _lib.SIGNATURES["offk_off_units_fused_cl"] == _lib.SIGNATURES["offk_off_units_fused_typed"]


def test_cl_symbols_are_exported(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in CL:
        assert hasattr(raw, name), name
    assert built.offk_abi_version() == 10


def test_handleless_calls_fail_with_a_message(built):
    feats = (ctypes.c_void_p * 9)()
    parts = (_lib.OffkFeatParts * 9)()
    for dt in (_lib.FEAT_F32, _lib.FEAT_BF16, _lib.FEAT_F16, 7):
        assert built.offk_forward_cl(None, None, dt, feats, None, None, None, None) == -1
        assert b"null argument" in built.offk_last_error(None)
        assert built.offk_forward_parts_cl(None, None, dt, parts, None, None, None, None) == -1
        assert b"null argument" in built.offk_last_error(None)
        assert built.offk_off_units_fused_cl(None, None, dt, feats, None) == -1
        assert b"null argument" in built.offk_last_error(None)


def test_units_kernel_for_channels_last_maps_fits_its_resources(built):
    import importlib.util
    path = os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "build.py")
    sp = importlib.util.spec_from_file_location("offk_build_cl", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    assert "pw_tdiff_cl.hip" in mod.SOURCES and "-fno-slp-vectorize" in mod.EXTRA_FLAGS["pw_tdiff_cl.hip"]
    obj = os.path.join(mod.OBJ, "pw_tdiff_cl.o")
    cos = mod._code_objects(obj)
    try:
        ks = [k for co in cos for k in mod.kernel_resources(co) if "pw_tdiff_cl_kernel" in k["name"]]
        notes = "".join(subprocess.run([mod._llvm_readelf(), "--notes", co], capture_output=True, text=True).stdout for co in cos)
    finally:
        for p in cos:
            os.remove(p)
    assert sorted(k["name"] for k in ks) == ["void offk::pw_tdiff_cl_kernel<%d>(offk::PtParams)" % d for d in (0, 1, 2)]   # fp32, bf16, fp16
    for k in ks:                                      # eight waves per block, one block per CU: 256 registers per wave
        assert k["vgpr_count"] <= 256 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    # LDS: nothing static beside the launch's dynamic 2 x (30 KB weight image + 7 frames x 2 pixel tiles x planes KB); the CU has 160 KB
    static = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        static[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    for k in ks:
        planes = {"<0>": 3, "<1>": 1, "<2>": 2}[re.search(r"<\d>", k["name"]).group(0)]
        dynamic = 2 * (30 * 1024 + 7 * 2 * planes * 1024)
        assert static[k["mangled"]] + dynamic <= 160 * 1024, (k, dynamic)


def _maps(B, L, fmt=torch.contiguous_format, dtype=torch.float32):
    return [torch.zeros(B * L, C, H, H, dtype=dtype).contiguous(memory_format=fmt) for _, C, H in spec.SITES]


def test_layout_classifier_on_cpu_tensors():
    from offk_amd import runtime
    B, L = 1, 2
    nchw = _maps(B, L)
    cl = _maps(B, L, torch.channels_last, torch.float16)
    assert runtime.feat_layout(nchw, B, L) == "nchw"
    assert runtime.feat_layout(cl, B, L) == "cl"
    assert all(tuple(t.shape) == s for t, s in zip(cl, spec.feature_shapes(B, L)))       # logical shape unchanged
    # a mix, in either direction
    with pytest.raises(ValueError, match="one layout"):
        runtime.feat_layout(nchw[:8] + cl[8:], B, L)
    with pytest.raises(ValueError, match="one layout"):
        runtime.feat_layout(cl[:1] + nchw[1:], B, L)
    # lists of channel groups: each group channels_last on its own; a mix inside one map
    parts = [[t[:, :64].contiguous(memory_format=torch.channels_last), t[:, 64:].contiguous(memory_format=torch.channels_last)] for t in cl]
    assert all(p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous() for ps in parts for p in ps)
    assert runtime.feat_layout(parts, B, L) == "cl"
    assert runtime.feat_layout(parts[:4] + cl[4:], B, L) == "cl"
    assert runtime.feat_layout([[t[:, :64].contiguous(), t[:, 64:].contiguous()] for t in nchw], B, L) == "nchw"
    mixed = list(parts)
    mixed[2] = [parts[2][0], parts[2][1].contiguous()]
    with pytest.raises(ValueError, match="one layout"):
        runtime.feat_layout(mixed, B, L)
    # a channels_last tensor of the wrong logical shape (another batch; H and C swapped, what an NHWC-shaped tensor permuted wrongly gives)
    bad = list(cl)
    bad[3] = torch.zeros((B * L + 1,) + tuple(cl[3].shape[1:])).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match=r"feats\[3\].*logical shape"):
        runtime.feat_layout(bad, B, L)
    bad[3] = torch.zeros(B * L, 14, 14, 576).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match=r"feats\[3\].*logical shape"):
        runtime.feat_layout(bad, B, L)
    # neither layout, and not nine maps
    with pytest.raises(ValueError, match="neither"):
        runtime.feat_layout(nchw[:8] + [nchw[8].permute(0, 1, 3, 2)], B, L)
    with pytest.raises(ValueError, match="nine"):
        runtime.feat_layout(cl[:8], B, L)
