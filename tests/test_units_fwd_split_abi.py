"""CPU checks of offk_off_units_train_split (the units' train forward with the stacked 1x1 reduces K1 in split-fp32 arithmetic on the bf16
matrix pipe): the header declares it and the binding has it under the unchanged ABI version; a handle-less call fails cleanly without a
GPU; build.py's register guard covers the six forms of the GEMM; the wrappers refuse an unknown `arith` / `fwd_arith` without a device;
and the inequality tests/test_gpu_units_fwd_split.py asserts DISCRIMINATES: the CPU emulation of the kernel's arithmetic
(tests/units_fwd_split.py) satisfies it on worst-case mantissas, the same emulation with any one of the issued plane products left out
does not -- for fp32 maps (six products), fp16-valued maps (five) and bf16-valued maps (three)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from . import split_bound as sb
from . import units_fwd_split as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "offk_off_units_train_split"


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
                                               "const void* const feats[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed, double drop_p")
    assert NAME in _lib.SIGNATURES
    cl = _lib.SIGNATURES["offk_off_units_train_cl"]
    res, args = _lib.SIGNATURES[NAME]
    # the _cl entry's arguments with `layout` behind feat_dtype
    assert res is cl[0] and len(args) == 8 and list(args[:3]) == list(cl[1][:3]) and args[3] is ctypes.c_int and list(args[4:]) == list(cl[1][3:])
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)
    doc = src[src.index("1x1 reduces in split-fp32 arithmetic on the bf16 matrix pipe (additive, opt-in"):src.index("int %s(" % NAME)]
    for needle in ("(2^-21 + 2^-30)", "NaN", "graph", "NOT", "bit-equal", "THREE launches", "capturable", "bf16 maps", "fp16 maps", "w_l x_m", "x.float()",
                   "OFFK_PRECISION_F32SPLIT", "OFFK_FEAT_NHWC", "offk_train_workspace_bytes and offk_workspace_bytes are", "unchanged",
                   "offk_off_units_fused", "5,345,280", "must be ordered", "drop_p = 0", "(A1 + A2) + bias", "32 kt + 8 g + e", "units:pw_reduce weight cut (K1, split)",
                   "units:pw_reduce (K1, NCHW, split)"):
        assert needle in doc, needle
    # the sentence the two earlier entries left standing is gone, here and in DESIGN.md
    for path in (os.path.join(ROOT, "include", "offk.h"), os.path.join(ROOT, "DESIGN.md")):
        flat = re.sub(r"[\s*]+", " ", open(path).read())
        assert "a split-fp32 handle runs its training side on the fp32 kernels" not in flat, path
        assert "A split-fp32 handle runs the training side on the fp32 kernels" not in flat, path


def test_symbol_is_exported_and_fails_cleanly_without_a_handle(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, NAME)
    assert built.offk_abi_version() == 10
    arr = (ctypes.c_void_p * 9)()
    assert getattr(built, NAME)(None, None, 0, 0, arr, None, 0, 0.0) == -1
    assert b"offk_off_units_train_split: null argument" in built.offk_last_error(None)


def test_the_build_keeps_the_kernel_in_registers(built):
    """build.py's register guard covers the six forms of the GEMM, and refuses one that spills, uses scratch memory or is missing."""
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("offk_build", os.path.join(os.path.dirname(_lib.LIB_PATH), "build.py"))
    b = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(b)
    src = "units_fwd_split.hip"
    assert src in b.SOURCES and "-fno-slp-vectorize" in b.EXTRA_FLAGS[src]
    assert any(g[0] == src and g[2] == 6 for g in b.REGISTER_RESIDENT_KERNELS)
    cos = b._code_objects(os.path.join(b.OBJ, "units_fwd_split.o"))
    try:
        kernels = [k for co in cos for k in b.kernel_resources(co)]
    finally:
        for path in cos:
            os.remove(path)
    rows = b.check_register_resident(src, kernels)
    assert len(rows) == 6 and all(k["vgpr_count"] <= 256 and k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 for k in rows)
    gemm = [i for i, k in enumerate(kernels) if "units_fwd_split_kernel<" in k["name"]]
    assert len(gemm) == 6 and len(kernels) == 7                       # + the weight pre-pass
    for field in ("private_segment_fixed_size", "vgpr_spill_count"):
        bad = [dict(k) for k in kernels]
        bad[gemm[0]][field] = 256
        with pytest.raises(RuntimeError, match="register guard failed"):
            b.check_register_resident(src, bad)
    with pytest.raises(RuntimeError, match="expected 6"):
        b.check_register_resident(src, [k for i, k in enumerate(kernels) if i != gemm[-1]])


def test_unknown_arith_is_refused_without_a_device():
    from offk_amd import off_module, runtime
    assert runtime.FWD_ARITHS == ("fp32", "f32split")
    blank = object.__new__(runtime.OffForward)            # no handle, no device: the check comes before anything touches either
    for bad in ("bf16", "split", None, "FP32"):
        with pytest.raises(ValueError, match="arith must be one of"):
            runtime.OffForward.off_units_train(blank, None, 0, 0.5, arith=bad)
        with pytest.raises(ValueError, match="arith must be one of"):
            runtime.OffForward.off_units(blank, None, arith=bad)
        with pytest.raises(ValueError, match="fwd_arith must be one of"):
            off_module.OFFUnits(1, 2, "rgb", fwd_arith=bad)
    u = off_module.OFFUnits(1, 2)
    assert (u.fwd_arith, u.wgrad_arith, u.feat_grad_arith) == ("fp32", "fp32", "fp32")
    for i, key in enumerate(("fwd_arith", "wgrad_arith", "feat_grad_arith")):      # independent of each other
        u = off_module.OFFUnits(1, 2, feat_grad=True, **{key: "f32split"})
        assert [u.fwd_arith, u.wgrad_arith, u.feat_grad_arith] == ["f32split" if j == i else "fp32" for j in range(3)]
    assert inspect.signature(runtime.OffForward.off_units_train).parameters["arith"].default == "fp32"
    assert inspect.signature(runtime.OffForward.off_units).parameters["arith"].default == "fp32"
    assert inspect.signature(off_module.OFFUnits.__init__).parameters["fwd_arith"].default == "fp32"


@pytest.mark.parametrize("form", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
@pytest.mark.parametrize("K", [608, 1024])
def test_the_gpu_inequality_discriminates(K, pattern, signs, form):
    """K = 608 (19 steps, odd) and 1024, 160 outputs, 48 rows.  16-bit forms: the maps carry mantissa 0x7FE000 (every bit an fp16 has; its
    truncation 0x7F0000 every bit a bf16 has), so that each plane such a map has is as full as it can be."""
    M = 48
    w = synth.make_adversarial((160, K), pattern, "same", seed=3)
    x = fs.as_map_form(synth.make_adversarial((M, K), pattern if form == "f32" else 0x7FE000, signs, seed=4, relu=(pattern == 0x7FFFFF)) * np.float32(2.0 ** -4), form)
    nplanes = {"f32": 3, "f16": 2, "bf16": 1}[form]
    assert sb.planes_used(x) == nplanes and sb.planes_used(w) == 3
    ref, dropped, mag = fs.terms(w, x)
    if form == "bf16":
        assert not dropped.any()                                     # nothing is dropped on bf16 maps
    emu = fs.emulate(w, x)
    c = sb.c_acc(emu, ref, dropped, mag)
    A = max(1.0, 2.0 * c)
    print("K %4d pattern 0x%06X %-11s %-4s maps: emulated c_acc %.3f, A %.3f, dropped max %.3f" % (
        K, pattern, signs, form, c, A, float((np.abs(dropped) / np.maximum(sb.EPS * mag, 1e-300)).max())))
    assert sb.excess(emu, ref, dropped, mag, A) <= 0.0
    # the ReLU is 1-Lipschitz: the bound of the pre-activation holds for G against max(ref64, 0)
    G, _D = fs.outputs(emu)
    assert sb.excess(G, np.maximum(ref[:, :fs.GEN], 0.0), dropped[:, :fs.GEN], mag[:, :fs.GEN], A) <= 0.0
    for skip in range(len(synth.SPLIT_PRODUCTS)):
        lost = fs.emulate(w, x, skip=skip)
        if skip in sb.NOT_ISSUED[nplanes]:
            # a product the form does not issue adds exact zeros: the three- / five-product kernel computes the six-product values
            assert np.array_equal(lost, emu), (skip, synth.SPLIT_PRODUCTS[skip])
        else:
            assert sb.excess(lost, ref, dropped, mag, A) > 0.0, (skip, synth.SPLIT_PRODUCTS[skip])
