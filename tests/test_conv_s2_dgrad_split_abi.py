"""CPU checks of the stride-2 fusion convs' split-fp32 data gradient (offk_conv2d_s2_backward_data_split /
offk_conv2d_s2_backward_plan_split, csrc/conv_dgrad_s2_split.hip): both symbols exist and are bound under the unchanged ABI version and the
header states the arithmetic; the plan is a pure function with pinned bytes; every refusal tests/test_conv_bwd_s2_abi.py asks of the fp32
data entry is a refusal of the new one, under its own name and before any HIP call (fake pointers, never dereferenced); FusionConv2d's
switch; the helper's operands (tests/conv_s2_dgrad_split.py) summed directly equal the fp64 reference; and the inequality
tests/test_gpu_conv_s2_dgrad_split.py asserts DISCRIMINATES in the kernel's K order: the CPU emulation satisfies it on worst-case mantissas,
the same emulation with any one of the six issued plane products left out does not, in every phase."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

from .conv_bwd import S2 as cs
from . import conv_s2_dgrad_split as ds
from . import split_bound as sb
from . import conv_bwd_s2_abi as fp32_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA, PLAN = "offk_conv2d_s2_backward_data_split", "offk_conv2d_s2_backward_plan_split"

# data_scratch_bytes at n_img = 1, 6, 384: Co Ci k k x 6 + n (H / 2)(W / 2) Co x 6, each region rounded up to 256
PLAN_BYTES = {"motion_conv_trans_28": (6096384, 6472704, 34922496), "motion_conv_trans_14": (20312832, 20500992, 34725888)}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _plan(lib, n, H, W, ci, co, k):
    d = ctypes.c_size_t(0)
    rc = lib.offk_conv2d_s2_backward_plan_split(n, H, W, ci, co, k, k, ctypes.byref(d))
    return rc, d.value


def test_symbols_are_exported_bound_and_declared(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in (DATA, PLAN):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert tuple(getattr(built, name).argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert built.offk_abi_version() == 10
    assert list(_lib.SIGNATURES[DATA][1]) == list(_lib.SIGNATURES["offk_conv2d_s2_backward_data"][1])
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)

    def args(name):
        return re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % name, src).group(1))
    assert args(DATA) == args("offk_conv2d_s2_backward_data"), "the argument list of the fp32 entry, word for word"
    doc = src[src.index("K4b, stride 2: the data gradient in split-fp32 arithmetic"):src.index("int %s(" % DATA)]
    for needle in ("(2^-21 + 2^-30)", "th major, then tw", "steps of 32", "never straddles a tap", "contributes zeros", "no atomics",
                   "OFFK_PRECISION_F32SPLIT", "w_l g_h, w_h g_l, w_m g_m, w_m g_h, w_h g_m", "A1 + A2", "pure host code", "rounded up to 256", "2^-109",
                   "A = max(1, 2 c_acc)", "capturable", "exactly one thread"):
        assert needle in doc, needle


@pytest.mark.parametrize("real", cs.REAL, ids=[r[0] for r in cs.REAL])
def test_plan_is_a_pure_function_with_pinned_bytes(built, real):
    key, ci, co, k, H = real
    for n_img, want in zip((1, 6, 384), PLAN_BYTES[key]):
        first = _plan(built, n_img, H, H, ci, co, k)
        assert first[0] == 0, built.offk_last_error(None)
        assert first[1] == want, (key, n_img, first[1])
        assert first[1] == -(-co * ci * k * k * 6 // 256) * 256 + -(-n_img * (H // 2) ** 2 * co * 6 // 256) * 256
        for _ in range(3):
            assert _plan(built, n_img, H, H, ci, co, k) == first
    assert built.offk_conv2d_s2_backward_plan_split(6, H, H, ci, co, k, k, None) == 0, "the output pointer may be NULL"


def test_plan_rounds_each_region_and_runs_from_the_python_wrapper(built):
    from offk_amd import runtime
    # M = 1: g's planes are 384 bytes, rounded up to 512
    assert _plan(built, 1, 2, 2, 32, 64, 7) == (0, 49 * 64 * 32 * 6 + 512)
    assert _plan(built, 3, 2, 2, 32, 64, 5) == (0, 25 * 64 * 32 * 6 + 1280)
    assert runtime.conv2d_s2_backward_plan_split(6, 28, 28, 320, 64, 7) == _plan(built, 6, 28, 28, 320, 64, 7)[1]
    assert runtime.DGRAD_ARITHS == ("fp32", "f32split")


def test_the_refusal_table_covers_the_fp32_entrys(built):
    assert len([1 for e, _m, _o in fp32_abi.REFUSALS.values() if e == "offk_conv2d_s2_backward_data"]) == 20
    assert _plan(built, fp32_abi.N, fp32_abi.H, fp32_abi.H, fp32_abi.CI, fp32_abi.CO, 5) == (0, fp32_abi.DGRAD_SPLIT_SCRATCH)


@pytest.mark.parametrize("rule", sorted(fp32_abi.DGRAD_SPLIT_REFUSALS))
def test_refusals_name_the_split_entry(built, rule):
    over = fp32_abi.DGRAD_SPLIT_REFUSALS[rule]
    rc = getattr(built, DATA)(*fp32_abi.data_args(**over))
    assert rc == -1, (rule, rc, built.offk_last_error(None))
    assert DATA.encode() + b":" in built.offk_last_error(None), built.offk_last_error(None)


def test_the_unmodified_arguments_are_refused_for_the_scratch_only_and_plan_refusals(built):
    rc = getattr(built, DATA)(*fp32_abi.data_args(scratch_bytes=0))
    assert rc == -1 and b"scratch too small (offk_conv2d_s2_backward_plan_split)" in built.offk_last_error(None)
    for over in (dict(kh=3, kw=3), dict(kw=7), dict(H=13), dict(W=15), dict(ci=48), dict(co=96), dict(n=0)):
        assert built.offk_conv2d_s2_backward_plan_split(*fp32_abi.plan_args(**over)[:8]) == -1
        assert PLAN.encode() + b":" in built.offk_last_error(None)


def test_fusion_conv_switch():
    from offk_amd import runtime
    from offk_amd.off_module import FusionConv2d
    for kw in (dict(kernel_size=7, padding=3), dict(kernel_size=5, padding=2)):
        m = FusionConv2d(64, 64, stride=2, **kw)
        assert m.dgrad_arith == "fp32" and "dgrad_arith" not in repr(m)
        assert repr(m) == repr(FusionConv2d(64, 64, stride=2, dgrad_arith="fp32", **kw))
        assert repr(m).endswith("relu=False, relu_in=False)"), "the default repr is unchanged"
        s = FusionConv2d(64, 64, stride=2, relu=True, dgrad_arith="f32split", **kw)
        assert s.dgrad_arith == "f32split" and s.wgrad_arith == "fp32" and "dgrad_arith=f32split" in repr(s)
        for bad in ("bf16", "split", None, "FP32"):
            with pytest.raises(ValueError, match="dgrad_arith"):
                FusionConv2d(64, 64, stride=2, dgrad_arith=bad, **kw)
    for args, kw in (((64, 64, 3), dict(padding=1)), ((128, 64, 1), dict())):
        assert FusionConv2d(*args, **kw).dgrad_arith == "fp32"
        with pytest.raises(ValueError, match="no split entry"):
            FusionConv2d(*args, dgrad_arith="f32split", **kw)
    assert inspect.signature(runtime.conv2d_s2_backward_data).parameters["arith"].default == "fp32"
    assert inspect.signature(FusionConv2d.__init__).parameters["dgrad_arith"].default == "fp32"
    with pytest.raises(ValueError, match="arith must be one of"):
        runtime.conv2d_s2_backward_data(None, None, 3, arith="bf16")


def test_the_build_lists_the_file_with_the_split_flags(built):
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("offk_build", os.path.join(os.path.dirname(_lib.LIB_PATH), "build.py"))
    b = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(b)
    assert "conv_dgrad_s2_split.hip" in b.SOURCES and "-fno-slp-vectorize" in b.EXTRA_FLAGS["conv_dgrad_s2_split.hip"]
    cos = b._code_objects(os.path.join(b.OBJ, "conv_dgrad_s2_split.o"))
    try:
        kernels = [k for co in cos for k in b.kernel_resources(co)]
    finally:
        for path in cos:
            os.remove(path)
    assert len(kernels) == 3 and all(k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 for k in kernels), "no spills, no private segment"
    assert [r for r in b.REGISTER_RESIDENT_KERNELS if r[0] == "conv_dgrad_s2_split.hip"], "the register-guard row"
    rows = b.check_register_resident("conv_dgrad_s2_split.hip", kernels)
    assert len(rows) == 1 and rows[0]["vgpr_count"] <= 256, "one block of eight waves per CU: two waves per SIMD"
    bad = [dict(k) for k in kernels]
    for k in bad:
        if "conv_s2_dgrad_split_kernel" in k["name"]:
            k["vgpr_spill_count"] = 3
    with pytest.raises(RuntimeError, match="register guard failed"):
        b.check_register_resident("conv_dgrad_s2_split.hip", bad)


@pytest.mark.parametrize("c", cs.cases(), ids=cs.case_id)
def test_the_operands_summed_directly_equal_the_reference(built, c):
    """the helper's K order against the definition: fp64 sums over (tap, co) per phase equal torch's fp64 dX"""
    from offk_amd import runtime
    c = cs.resolve(runtime.conv2d_s2_backward_plan, c)
    inp, ref = cs.cached(c, "int", False)
    assert np.array_equal(ds.direct(inp["g"].numpy(), inp["w"].numpy()), ref["dX"].numpy()), cs.case_id(c)
    for r, s in ds.PHASES:
        Wm, Gm = ds.operands(inp["g"].numpy(), inp["w"].numpy(), r, s)
        taps = ds.phase_taps(c.k, r, s)
        assert Wm.shape == (c.ci, taps * c.co) and Gm.shape == (c.n * (c.H // 2) * (c.W // 2), taps * c.co)
    assert sorted(ds.phase_taps(c.k, r, s) for r, s in ds.PHASES) == ([9, 12, 12, 16] if c.k == 7 else [4, 6, 6, 9])


@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
@pytest.mark.parametrize("shape", cs.WORST, ids=["k7_2x6x10_64to64", "k5_2x6x4_96to64"])
def test_the_gpu_inequality_discriminates_in_the_kernels_k_order(shape, pattern, signs):
    g, w = cs.worst_inputs(shape, pattern, signs)
    ref, dropped, mag = ds.terms(g, w)
    sb.assert_discriminates("k %d pattern 0x%06X %-11s" % (shape[0], pattern, signs), lambda skip: ds.emulate(g, w, skip=skip), ref, dropped, mag,
                            parts=[(slice(None), slice(r, None, 2), slice(s, None, 2)) for r, s in ds.PHASES])      # in every phase
