"""CPU checks of the stride-1 fusion convs' split-fp32 data gradient (offk_conv2d_backward_data_split /
offk_conv2d_backward_data_plan_split / offk_conv2d_backward_data_form_split, csrc/conv_dgrad_split.hip): the symbols exist and are bound
under the unchanged ABI version and the header states the arithmetic; the plan is a pure function with pinned bytes and a pinned block
form; every refusal tests/test_conv_bwd_abi.py asks of the fp32 data entry is a refusal of the new one, under its own name and before any
HIP call (fake pointers, never dereferenced); runtime.conv2d_backward_data's `arith` and FusionConv2d's `bwd_arith`; the helper's
operands (tests/conv_dgrad_split.py) summed directly equal the fp64 reference; and the inequality tests/test_gpu_conv_dgrad_split.py
asserts DISCRIMINATES in the kernel's K order: the CPU emulation satisfies it on worst-case mantissas, the same emulation with any one
of the six issued plane products left out does not."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

from .conv_bwd import S1 as cb
from . import conv_dgrad_split as dg
from . import split_bound as sb
from . import conv_bwd_abi as fp32_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA, PLAN, FORM = "offk_conv2d_backward_data_split", "offk_conv2d_backward_data_plan_split", "offk_conv2d_backward_data_form_split"
SHAPE_IDS = ["%dx%d_%dto%d_k%d" % (s[0], s[0], s[1], s[2], s[3]) for s in cb.FUSION_SHAPES]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _plan(lib, n, H, W, ci, co, k):
    d = ctypes.c_size_t(0)
    rc = lib.offk_conv2d_backward_data_plan_split(n, H, W, ci, co, k, k, ctypes.byref(d))
    return rc, d.value


def _form(lib, n, H, W, ci, co, k):
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.offk_conv2d_backward_data_form_split(n, H, W, ci, co, k, k, ctypes.byref(a), ctypes.byref(b))
    return rc, a.value, b.value


def test_symbols_are_exported_bound_and_declared(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in (DATA, PLAN, FORM):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert tuple(getattr(built, name).argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert built.offk_abi_version() == 10
    assert list(_lib.SIGNATURES[DATA][1]) == list(_lib.SIGNATURES["offk_conv2d_backward_data"][1])
    assert list(_lib.SIGNATURES[PLAN][1]) == list(_lib.SIGNATURES["offk_conv2d_s2_backward_plan_split"][1])
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)

    def args(name):
        return re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % name, src).group(1))
    assert args(DATA) == args("offk_conv2d_backward_data"), "the argument list of the fp32 entry, word for word"
    assert args(PLAN) == "int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes"
    doc = src[src.index("K4b's data gradient in split-fp32 arithmetic"):src.index("int %s(" % DATA)]
    for needle in ("(2^-21 + 2^-30)", "K index = tap * Co + co", "tap = kh * k + kw", "steps of 32", "never straddles a tap", "contributes zeros",
                   "no atomics", "no reduce launch", "OFFK_PRECISION_F32SPLIT", "w_l g_h, w_h g_l, w_m g_m, w_m g_h, w_h g_m", "A1 + A2",
                   "pure host code", "rounded up to 256", "2^-109", "A = max(1, 2 c_acc)", "capturable", "exactly one thread", "three launches",
                   "16-byte aligned", "[tap][32-co step][16-ci tile][plane][lane]", "its row or its image"):
        assert needle in doc, needle


@pytest.mark.parametrize("shape", cb.FUSION_SHAPES, ids=SHAPE_IDS)
def test_plan_is_a_pure_function_with_pinned_bytes(built, shape):
    H, ci, co, k = shape
    for n_img in (1, 6, 384):
        first = _plan(built, n_img, H, H, ci, co, k)
        assert first[0] == 0, built.offk_last_error(None)
        assert first[1] == fp32_abi.round256(co * ci * k * k * 6) + fp32_abi.round256(n_img * H * H * co * 6), (shape, n_img, first[1])
        for _ in range(3):
            assert _plan(built, n_img, H, H, ci, co, k) == first
    assert built.offk_conv2d_backward_data_plan_split(6, H, H, ci, co, k, k, None) == 0, "the output pointer may be NULL"


def test_plan_rounds_each_region_and_runs_from_the_python_wrapper(built):
    from offk_amd import runtime
    assert _plan(built, 384, 7, 7, 832, 256, 3) == (0, 40402944)
    assert _plan(built, 384, 14, 14, 64, 64, 1) == (0, 28925952)
    # M = 1: g's planes are 384 bytes, rounded up to 512; M = 3 on 128 channels: 2304 bytes, a multiple of 256 already
    assert _plan(built, 1, 1, 1, 64, 64, 3) == (0, 9 * 64 * 64 * 6 + 512)
    assert _plan(built, 1, 1, 1, 64, 64, 1) == (0, 64 * 64 * 6 + 512)
    assert _plan(built, 3, 1, 1, 64, 128, 1) == (0, 128 * 64 * 6 + 2304)
    assert runtime.conv2d_backward_data_plan_split(6, 14, 14, 64, 64, 3) == _plan(built, 6, 14, 14, 64, 64, 3)[1]
    assert runtime.conv2d_backward_data_form_split(6, 14, 14, 64, 64, 3) == _form(built, 6, 14, 14, 64, 64, 3)[1:]
    assert runtime.DGRAD_ARITHS == ("fp32", "f32split") and runtime.BWD_ARITHS == ("fp32", "f32split")


# (ci per block, pixels per block) at n_img = 1, 6, 384 in cb.FUSION_SHAPES' order: 64 wide where Ci is 64; else 128 pixels where the
# 128 x 256 grid would have at most 128 blocks
FORMS_384 = [(64, 256), (64, 256), (64, 256), (128, 256), (128, 128), (128, 128), (128, 128), (128, 256), (128, 128), (128, 256), (128, 256),
             (128, 256), (128, 256)]


@pytest.mark.parametrize("shape,at384", list(zip(cb.FUSION_SHAPES, FORMS_384)), ids=SHAPE_IDS)
def test_the_block_form_is_pinned(built, shape, at384):
    H, ci, co, k = shape
    small = (64, 256) if ci == 64 else (128, 128)
    for n_img, want in ((1, small), (6, small), (384, at384)):
        got = _form(built, n_img, H, H, ci, co, k)
        assert got == (0,) + want, (shape, n_img, got)
        blocks256 = -(-n_img * H * H // 256) * -(-ci // 128)
        assert want == ((64, 256) if ci == 64 else (128, 128) if blocks256 <= 128 else (128, 256)), "the rule the header states"
        assert _form(built, n_img, H, H, ci, co, k) == got
    assert built.offk_conv2d_backward_data_form_split(6, H, H, ci, co, k, k, None, None) == 0, "the output pointers may be NULL"
    assert built.offk_conv2d_backward_data_form_split(6, H, H, ci, co, 5, 5, None, None) == -1
    assert FORM.encode() + b":" in built.offk_last_error(None)


def test_the_refusal_table_covers_the_fp32_entrys(built):
    assert len([1 for e, _m, _o in fp32_abi.REFUSALS.values() if e == "offk_conv2d_backward_data"]) == 14
    assert _plan(built, fp32_abi.N, fp32_abi.H, fp32_abi.H, fp32_abi.CI, fp32_abi.CO, 3) == (0, fp32_abi.DGRAD_SPLIT_SCRATCH)


@pytest.mark.parametrize("rule", sorted(fp32_abi.DGRAD_SPLIT_REFUSALS))
def test_refusals_name_the_split_entry(built, rule):
    over = fp32_abi.DGRAD_SPLIT_REFUSALS[rule]
    rc = getattr(built, DATA)(*fp32_abi.data_args(**over))
    assert rc == -1, (rule, rc, built.offk_last_error(None))
    assert DATA.encode() + b":" in built.offk_last_error(None), built.offk_last_error(None)


def test_the_scratch_message_and_both_stride_1_entries_on_k5_and_k7(built):
    rc = getattr(built, DATA)(*fp32_abi.data_args(scratch_bytes=0))
    assert rc == -1 and b"scratch too small (offk_conv2d_backward_data_plan_split)" in built.offk_last_error(None)
    rc = getattr(built, DATA)(*fp32_abi.data_args(scratch=ctypes.c_void_p(0x30000004)))
    assert rc == -1 and b"scratch must be 16-byte aligned" in built.offk_last_error(None)
    for k in (5, 7):
        for entry in (DATA, "offk_conv2d_backward_data"):
            rc = getattr(built, entry)(*fp32_abi.data_args(KH=k, KW=k, pad=(k - 1) // 2))
            assert rc == -1 and entry.encode() + b": the kernel must be 1x1 or 3x3" in built.offk_last_error(None), (k, entry)
    for bad in ((2, 14, 14, 64, 64, 5, 5), (2, 14, 14, 64, 64, 3, 1), (2, 14, 14, 96, 64, 3, 3), (2, 14, 14, 64, 96, 1, 1), (0, 14, 14, 64, 64, 3, 3)):
        assert built.offk_conv2d_backward_data_plan_split(*bad, None) == -1
        assert PLAN.encode() + b":" in built.offk_last_error(None)


def test_runtime_arith_keyword():
    from offk_amd import runtime
    assert inspect.signature(runtime.conv2d_backward_data).parameters["arith"].default == "fp32"
    assert list(inspect.signature(runtime.conv2d_backward_data).parameters)[-1] == "arith", "a new LAST keyword"
    for bad in ("bf16", "split", None, "FP32"):
        with pytest.raises(ValueError, match="arith must be one of"):
            runtime.conv2d_backward_data(None, None, 1, arith=bad)


def test_fusion_conv_bwd_arith_switch():
    from offk_amd.off_module import FusionConv2d
    forms = [((64, 64, 3), dict(padding=1)), ((128, 64, 1), dict()), ((64, 64, 7), dict(stride=2, padding=3)), ((96, 64, 5), dict(stride=2, padding=2))]
    assert inspect.signature(FusionConv2d.__init__).parameters["bwd_arith"].default == "fp32"
    for args, kw in forms:
        m = FusionConv2d(*args, **kw)
        assert m.bwd_arith == "fp32" and m.wgrad_arith == "fp32" and m.dgrad_arith == "fp32" and "arith" not in repr(m)
        assert repr(m) == repr(FusionConv2d(*args, bwd_arith="fp32", **kw))
        assert repr(m).endswith("relu=False, relu_in=False)"), "the default repr is unchanged"
        s = FusionConv2d(*args, relu=True, bwd_arith="f32split", **kw)
        assert s.bwd_arith == "f32split" and s.wgrad_arith == "fp32" and s.dgrad_arith == "fp32", "the two older attributes keep what was passed"
        assert repr(s).endswith("relu=True, relu_in=False, bwd_arith=f32split)")
        for bad in ("bf16", "split", None, "FP32"):
            with pytest.raises(ValueError, match="bwd_arith must be one of"):
                FusionConv2d(*args, bwd_arith=bad, **kw)
    # one way to say it
    with pytest.raises(ValueError, match="bwd_arith='f32split' already covers"):
        FusionConv2d(64, 64, 3, padding=1, bwd_arith="f32split", wgrad_arith="f32split")
    with pytest.raises(ValueError, match="bwd_arith='f32split' already covers"):
        FusionConv2d(64, 64, 7, stride=2, padding=3, bwd_arith="f32split", dgrad_arith="f32split")
    # the older keywords' refusals stand, in their words
    with pytest.raises(ValueError, match="no split entry"):
        FusionConv2d(64, 64, 3, padding=1, dgrad_arith="f32split")
    with pytest.raises(ValueError, match="no split entry"):
        FusionConv2d(64, 64, 3, padding=1, dgrad_arith="f32split", bwd_arith="f32split")
    with pytest.raises(ValueError, match="no split entry"):
        FusionConv2d(64, 64, 7, stride=2, padding=3, wgrad_arith="f32split")
    # and they still combine with the default bwd_arith
    assert "wgrad_arith=f32split" in repr(FusionConv2d(64, 64, 3, padding=1, wgrad_arith="f32split"))
    assert "dgrad_arith=f32split" in repr(FusionConv2d(64, 64, 7, stride=2, padding=3, dgrad_arith="f32split"))


def test_the_build_lists_the_file_with_the_split_flags_and_guards_every_form(built):
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("offk_build", os.path.join(os.path.dirname(_lib.LIB_PATH), "build.py"))
    b = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(b)
    src = "conv_dgrad_split.hip"
    assert src in b.SOURCES and "-fno-slp-vectorize" in b.EXTRA_FLAGS[src]
    assert "conv_dgrad_split_common.h" in b.HEADERS, "a change of the shared header rebuilds both split data gradients"
    cos = b._code_objects(os.path.join(b.OBJ, "conv_dgrad_split.o"))
    try:
        kernels = [k for co in cos for k in b.kernel_resources(co)]
    finally:
        for path in cos:
            os.remove(path)
    gemms = [k for k in kernels if "conv_dgrad_split_kernel<" in k["name"]]
    assert len(kernels) == 5 and len(gemms) == 3, "two pre-passes and one GEMM per block form"
    assert all(k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 for k in kernels), "no spills, no private segment"
    guard = [r for r in b.REGISTER_RESIDENT_KERNELS if r[0] == src]
    assert len(guard) == 3 and all(r[2] == 1 for r in guard), "a register-guard row per instantiation"
    for k in gemms:
        assert sum(1 for r in guard if re.search(r[1], k["name"])) == 1, k["name"]
    rows = b.check_register_resident(src, kernels)
    assert len(rows) == 3 and all(r["vgpr_count"] <= 256 for r in rows), "one block of eight waves per CU: two waves per SIMD"
    for victim in gemms:
        bad = [dict(k, vgpr_spill_count=3) if k["name"] == victim["name"] else dict(k) for k in kernels]
        with pytest.raises(RuntimeError, match="register guard failed"):
            b.check_register_resident(src, bad)


@pytest.mark.parametrize("c", cb.cases(), ids=cb.case_id)
def test_the_operands_summed_directly_equal_the_reference(built, c):
    """the helper's K order against the definition: fp64 sums over (tap, co) equal torch's fp64 dX"""
    from offk_amd import runtime
    if c.n is None:
        c = c._replace(n=cb.chunked_n(runtime.conv2d_backward_plan, c))
    inp, ref = cb.cached(c, "int", False)
    g, w = inp["g"].numpy(), inp["w"].numpy()
    assert np.array_equal(dg.direct(g, w), ref["dX"].numpy()), cb.case_id(c)
    Wm, Gm = dg.operands(g, w)
    assert Wm.shape == (c.ci, c.k * c.k * c.co) and Gm.shape == (c.n * c.H * c.W, c.k * c.k * c.co)
    # K index = tap * Co + co, tap = kh * k + kw
    kh, kw, co, ci = c.k - 1, 0, c.co - 3, 5
    assert Wm[ci, (kh * c.k + kw) * c.co + co] == w[co, ci, kh, kw]


WORST_IDS = ["k3_2x5x3_64to64", "k1_2x5x3_64to128"]


@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
@pytest.mark.parametrize("shape", cb.WORST, ids=WORST_IDS)
def test_the_gpu_inequality_discriminates_in_the_kernels_k_order(shape, pattern, signs):
    g, w = cb.worst_inputs(shape, pattern, signs)
    ref, dropped, mag = dg.terms(g, w)
    sb.assert_discriminates("k %d pattern 0x%06X %-11s" % (shape[0], pattern, signs), lambda skip: dg.emulate(g, w, skip=skip), ref, dropped, mag)
