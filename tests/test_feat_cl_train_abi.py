"""CPU checks of the channels-last feature-map entries of the training side (offk_pw_reduce_cl, offk_off_units_cl,
offk_off_units_train_cl, offk_off_units_backward_cl): the header declares them and the binding has them, the library exports them
under the unchanged ABI version, a handle-less call fails cleanly without a GPU, the five new kernel instantiations (K1 on
channels-last bf16 / fp16 maps, K1b on channels-last fp32 / bf16 / fp16 maps) sit in code objects of their own without spills inside
the register budget of two blocks per CU, and the training-side layout classifier of the Python wrapper tells NCHW from
channels_last maps whatever the handle's precision."""
import ctypes
import os
import re
import types

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = ("offk_pw_reduce_cl", "offk_off_units_cl", "offk_off_units_train_cl", "offk_off_units_backward_cl")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_declares_the_cl_training_entries():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    for name in CL:
        m = re.search(r"\bint %s\(offk_handle\* h, void\* stream, int feat_dtype, ([^;]*);" % name, src)
        assert m, name
        assert "const void*" in m.group(1), name                 # the maps come as untyped pointers
        assert name in _lib.SIGNATURES
        # argument for argument the _typed entry
        typed = re.search(r"\bint %s\(([^;]*);" % name.replace("_cl", "_typed"), src).group(1)
        assert re.sub(r"\s+", " ", typed) == re.sub(r"\s+", " ", "offk_handle* h, void* stream, int feat_dtype, " + m.group(1)), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_cl", "_typed")], name
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    # the contract, the alignment and the per-call layout are stated beside the declarations
    doc = src[src.index("channels-last feature maps on the training side"):src.index("int offk_pw_reduce_cl(")]
    assert "EQUAL VALUES" in doc and "16-byte aligned" in doc and "cfg.feat_layout" in doc and "2 GiB" in doc


def test_cl_training_symbols_are_exported(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in CL:
        assert hasattr(raw, name), name
    assert built.offk_abi_version() == 10


def test_handleless_calls_fail_with_a_message(built):
    feats = (ctypes.c_void_p * 9)()
    gv = (_lib.OffkGradView * 9)()
    for dt in (_lib.FEAT_F32, _lib.FEAT_BF16, _lib.FEAT_F16, 7):
        assert built.offk_pw_reduce_cl(None, None, dt, 0, None, None, None) == -1
        assert b"offk_pw_reduce_cl: bad argument" in built.offk_last_error(None)
        assert built.offk_off_units_cl(None, None, dt, feats, None) == -1
        assert b"offk_off_units_cl: null argument" in built.offk_last_error(None)
        assert built.offk_off_units_train_cl(None, None, dt, feats, None, 7, 0.8) == -1
        assert b"offk_off_units_train_cl: null argument" in built.offk_last_error(None)
        assert built.offk_off_units_backward_cl(None, None, dt, feats, gv, None, 7, 0.8, None, 0) == -1
        assert b"offk_off_units_backward_cl: null argument" in built.offk_last_error(None)


def _build_module():
    import importlib.util
    path = os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "build.py")
    sp = importlib.util.spec_from_file_location("offk_build_cl_train", path)
    mod = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(mod)
    return mod


def _kernels(mod, obj_name, needle):
    obj = os.path.join(mod.OBJ, obj_name)
    cos = mod._code_objects(obj)
    try:
        return [k for co in cos for k in mod.kernel_resources(co) if needle in k["name"]]
    finally:
        for p in cos:
            os.remove(p)


def test_kernels_for_channels_last_maps_have_no_spills(built):
    """pw_reduce_kernel<0, 1, FEAT | 4>, FEAT = 1 (bf16), 2 (fp16), and pw_wgrad_kernel<FEAT | 4>, FEAT = 0 (fp32), 1, 2 -- 4 is
    kFeatCl, the channels-last loader form: code objects of their own (the existing forms keep theirs, alone), no VGPR spills, no
    private segment, and the budget their NCHW siblings are launched under -- __launch_bounds__(256, 2): four waves per block, two
    blocks per CU, so two waves per SIMD and 512 / 2 = 256 registers per wave."""
    mod = _build_module()
    for src, base in (("pw_reduce_cl.hip", "pw_reduce.hip"), ("units_bwd_cl.hip", "units_bwd.hip")):
        assert src in mod.SOURCES and mod.INCLUDED_SOURCES[src] == (base,)
        assert mod.EXTRA_FLAGS.get(src, []) == mod.EXTRA_FLAGS.get(base, [])        # the flags of the file it derives from
    assert "-fno-slp-vectorize" in mod.EXTRA_FLAGS["units_bwd_cl.hip"]
    k1 = _kernels(mod, "pw_reduce_cl.o", "offk::")
    k1b = _kernels(mod, "units_bwd_cl.o", "offk::")
    names = sorted(k["name"].split("(")[0] for k in k1 + k1b)
    assert names == ["void offk::pw_reduce_kernel<0, 1, 5>", "void offk::pw_reduce_kernel<0, 1, 6>",
                     "void offk::pw_wgrad_kernel<4>", "void offk::pw_wgrad_kernel<5>", "void offk::pw_wgrad_kernel<6>"], names
    for k in k1 + k1b:
        assert k["vgpr_count"] + k["agpr_count"] <= 256 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    # two blocks per CU in LDS as well: the tiles are static, (128 + 160) rows of the padded K-tile each way
    import subprocess
    for obj_name in ("pw_reduce_cl.o", "units_bwd_cl.o"):
        cos = mod._code_objects(os.path.join(mod.OBJ, obj_name))
        try:
            notes = "".join(subprocess.run([mod._llvm_readelf(), "--notes", co], capture_output=True, text=True).stdout for co in cos)
        finally:
            for p in cos:
                os.remove(p)
        sizes = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)]
        assert sizes and all(0 < s <= 80 * 1024 for s in sizes), sizes
    # the existing forms stay in the objects they had, alone
    assert sorted(k["name"].split("(")[0] for k in _kernels(mod, "pw_reduce.o", "offk::pw_reduce_kernel<")) == \
        ["void offk::pw_reduce_kernel<0, 0, 0>", "void offk::pw_reduce_kernel<0, 1, 0>"]
    assert sorted(k["name"].split("(")[0] for k in _kernels(mod, "pw_reduce_f16.o", "offk::pw_reduce_kernel<")) == \
        ["void offk::pw_reduce_kernel<0, 1, 1>", "void offk::pw_reduce_kernel<0, 1, 2>"]
    assert sorted(k["name"].split("(")[0] for k in _kernels(mod, "units_bwd.o", "offk::pw_wgrad_kernel<")) == \
        ["void offk::pw_wgrad_kernel<%d>" % d for d in (0, 1, 2)]


def _maps(B, L, fmt=torch.contiguous_format, dtype=torch.float32):
    return [torch.zeros(B * L, C, H, H, dtype=dtype).contiguous(memory_format=fmt) for _, C, H in spec.SITES]


def test_training_side_layout_classifier_on_cpu_tensors():
    from offk_amd import runtime
    B, L = 1, 2
    nchw = _maps(B, L)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        cl = _maps(B, L, torch.channels_last, dtype)
        assert all(not t.is_contiguous() for t in cl)
        assert runtime.train_feat_layout(cl, B, L) == "cl"
        assert runtime.train_feat_layout(_maps(B, L, dtype=dtype), B, L) == "nchw"
    cl = _maps(B, L, torch.channels_last, torch.float16)
    # a mix, in either direction
    with pytest.raises(ValueError, match="one layout"):
        runtime.train_feat_layout(nchw[:8] + cl[8:], B, L)
    with pytest.raises(ValueError, match="one layout"):
        runtime.train_feat_layout(cl[:1] + nchw[1:], B, L)
    # a channels_last tensor of the wrong logical shape
    bad = list(cl)
    bad[3] = torch.zeros((B * L + 1,) + tuple(cl[3].shape[1:])).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError, match=r"feats\[3\].*logical shape"):
        runtime.train_feat_layout(bad, B, L)
    # no channels_last map among them: "nchw", i.e. the checks such maps always met (NHWC-shaped contiguous maps of an NHWC
    # handle, a transposed view that _check_dev names)
    assert runtime.train_feat_layout([t.permute(0, 2, 3, 1).contiguous() for t in nchw], B, L) == "nchw"
    assert runtime.train_feat_layout(nchw[:8] + [nchw[8].permute(0, 1, 3, 2)], B, L) == "nchw"
    with pytest.raises(ValueError, match="nine"):
        runtime.train_feat_layout(cl[:8], B, L)
    # the handle's precision plays no part -- unlike takes_channels_last, the inference rule, which raises on the fp32 pipe
    for precision in (_lib.PRECISION_FP32, _lib.PRECISION_F32SPLIT):
        for handle_layout in (0, 1):
            h = types.SimpleNamespace(batch=B, length=L, precision=precision, feat_layout=handle_layout)
            assert runtime.OffForward.train_takes_channels_last(h, cl) is True
            assert runtime.OffForward.train_takes_channels_last(h, nchw) is False
    h = types.SimpleNamespace(batch=B, length=L, precision=_lib.PRECISION_FP32, feat_layout=0)
    with pytest.raises(ValueError, match="f32split"):
        runtime.OffForward.takes_channels_last(h, cl)


def test_off_units_module_keeps_channels_last_maps():
    """OFFUnits._as_handed_over: nine channels_last maps of one supported dtype stay as they are; anything else is made contiguous."""
    from offk_amd.off_module import OFFUnits
    B, L = 1, 2
    u = OFFUnits(B, L, "rgb")
    cl = _maps(B, L, torch.channels_last, torch.bfloat16)
    assert u._as_handed_over(cl) is True
    assert u._as_handed_over(_maps(B, L)) is False
    assert u._as_handed_over(_maps(B, L)[:8] + cl[8:]) is False                           # a mix of layouts
    assert u._as_handed_over(cl[:8] + [cl[8].half()]) is False                            # a mix of dtypes
    assert u._as_handed_over(_maps(B, L, torch.channels_last, torch.float64)) is False    # no kernel reads fp64 maps
    assert u._as_handed_over(_maps(B + 1, L, torch.channels_last)) is False               # another batch
