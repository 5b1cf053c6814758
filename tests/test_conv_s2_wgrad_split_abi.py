"""CPU checks of the stride-2 fusion convs' split-fp32 weight gradient (offk_conv2d_s2_backward_weight_split /
offk_conv2d_s2_backward_weight_plan_split, csrc/conv_wgrad_s2_split.hip): both symbols exist and are bound under the unchanged ABI version;
the plan is a pure function with pinned bytes and chunks; every refusal of the fp32 entry is a refusal of the new one, under its own name
and before any HIP call (fake pointers, never dereferenced); the K layout of tests/conv_s2_wgrad_split.py against torch's dW / db;
FusionConv2d's keyword; build.py's register guard; and the inequality tests/test_gpu_conv_s2_wgrad_split.py asserts DISCRIMINATES in the
kernel's K layout: the CPU emulation satisfies it on worst-case mantissas, the same emulation with any one of the six issued plane
products left out does not."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from .conv_bwd import S2 as s2
from . import conv_s2_wgrad_split as ws
from . import split_bound as sb
from . import conv_bwd_s2_abi as fp32_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT, PLAN = "offk_conv2d_s2_backward_weight_split", "offk_conv2d_s2_backward_weight_plan_split"
FP32 = "offk_conv2d_s2_backward_weight"

# weight_chunks of the split plan at n_img = 1, 6, 384 for tests/conv_bwd.S2.REAL: the 7x7 has 35 tiles of one kernel row (7 chunks = 245
# blocks, one round of one block per CU), the 5x5 170 (3 chunks = 510 blocks, two rounds); a chunk is at least 256 positions long
PLAN_CHUNKS = {"motion_conv_trans_28": (1, 3, 7), "motion_conv_trans_14": (1, 1, 3)}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _plan(lib, n, H, W, ci, co, k):
    w, c = ctypes.c_size_t(0), ctypes.c_int(0)
    rc = lib.offk_conv2d_s2_backward_weight_plan_split(n, H, W, ci, co, k, k, ctypes.byref(w), ctypes.byref(c))
    return rc, w.value, c.value


def test_symbols_are_exported_bound_and_declared(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in (WEIGHT, PLAN):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert tuple(getattr(built, name).argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert built.offk_abi_version() == 10
    assert list(_lib.SIGNATURES[WEIGHT][1]) == list(_lib.SIGNATURES[FP32][1])
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)

    def args(name):
        return re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % name, src).group(1))
    assert args(WEIGHT) == args(FP32), "the argument list of the fp32 entry, word for word"
    doc = src[src.index("K4b, stride 2: the weight / bias gradient in split-fp32 arithmetic"):src.index("int %s(" % WEIGHT)]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)               # the comment as running text: a needle may straddle a line break
    for needle in ("|dw - exact| <= |dropped| + A * 2^-24 * sum |g x| + 2^-24 |exact|", "(2^-21 + 2^-30)", "A = max(1, 2 c_acc)",
                   "g_l x_h, g_h x_l, g_m x_m, g_m x_h, g_h x_m", "A1 + A2", "exactly one thread", "pure host code", "2^-109",
                   "OFFK_PRECISION_F32SPLIT", "real pixels only", "steps of 32", "chunk order", "No atomics", "no empty chunk", "NaN",
                   "problem too large", "tests/conv_s2_wgrad_split.py"):
        assert needle in doc, needle


@pytest.mark.parametrize("real", s2.REAL, ids=[r[0] for r in s2.REAL])
def test_plan_is_a_pure_function_with_pinned_bytes_and_chunks(built, real):
    key, ci, co, k, H = real
    for n_img, want in zip((1, 6, 384), PLAN_CHUNKS[key]):
        first = _plan(built, n_img, H, H, ci, co, k)
        assert first[0] == 0, built.offk_last_error(None)
        chunks = first[2]
        assert chunks == want, (key, n_img, chunks)
        assert chunks == -(-n_img // -(-n_img // chunks)), "whole images per chunk, no empty chunk"
        assert first[1] == chunks * (co * ci * k * k + co) * 4
        for _ in range(3):
            assert _plan(built, n_img, H, H, ci, co, k) == first
    assert built.offk_conv2d_s2_backward_weight_plan_split(6, H, H, ci, co, k, k, None, None) == 0, "output pointers may be NULL"


def test_plan_runs_from_the_python_wrapper_and_chunks_short(built):
    from offk_amd import runtime
    assert runtime.conv2d_s2_backward_weight_plan_split(6, 28, 28, 320, 64, 7) == _plan(built, 6, 28, 28, 320, 64, 7)[1:]
    for k in (7, 5):
        c = s2.resolve(lambda *a: (0,) + runtime.conv2d_s2_backward_weight_plan_split(*a), s2.Case(k, *s2.CHUNKED[k]))
        chunks = runtime.conv2d_s2_backward_weight_plan_split(c.n, c.H, c.W, c.ci, c.co, c.k)[1]
        assert chunks >= 3 and c.n % (-(-c.n // chunks)) != 0


def test_the_refusal_table_covers_the_fp32_entrys(built):
    assert len([1 for e, _m, _o in fp32_abi.REFUSALS.values() if e == FP32]) == 16
    assert _plan(built, fp32_abi.N, fp32_abi.H, fp32_abi.H, fp32_abi.CI, fp32_abi.CO, 5)[1:] == (fp32_abi.WGRAD_SPLIT_SCRATCH, 1)


@pytest.mark.parametrize("rule", sorted(fp32_abi.WGRAD_SPLIT_REFUSALS))
def test_refusals_name_the_split_entry(built, rule):
    over = fp32_abi.WGRAD_SPLIT_REFUSALS[rule]
    for entry in (WEIGHT, FP32):
        rc = getattr(built, entry)(*fp32_abi.weight_args(**over))
        assert rc == -1, (rule, entry, rc, built.offk_last_error(None))
        assert entry.encode() + b":" in built.offk_last_error(None), built.offk_last_error(None)


def test_db_may_be_null_short_scratch_names_the_plan_and_plan_refusals(built):
    # db = NULL is no refusal: the same call with a short scratch is refused for the scratch, not for the pointer
    rc = getattr(built, WEIGHT)(*fp32_abi.weight_args(db=None, scratch_bytes=fp32_abi.WGRAD_SPLIT_SCRATCH - 1))
    assert rc == -1 and (WEIGHT + ": scratch too small (" + PLAN + ")").encode() in built.offk_last_error(None)
    # the refusals of offk_conv2d_s2_backward_plan, under the new plan's name
    plan_rules = [over for _rule, (entry, _make, over) in fp32_abi.REFUSALS.items() if entry == "offk_conv2d_s2_backward_plan"]
    assert len(plan_rules) == 6
    for over in plan_rules:
        a = fp32_abi.plan_args(**over)[:9]
        assert built.offk_conv2d_s2_backward_weight_plan_split(*a) == -1, over
        assert PLAN.encode() + b":" in built.offk_last_error(None)
    assert built.offk_conv2d_s2_backward_weight_plan_split(0, 14, 14, 64, 64, 5, 5, None, None) == -1
    # positions above the fp32 entry's limit: "problem too large" from both plans
    for entry, tail in ((PLAN, [None, None]), ("offk_conv2d_s2_backward_plan", [None, None, None])):
        assert getattr(built, entry)(1 << 20, 128, 128, 64, 64, 5, 5, *tail) == -1
        assert entry.encode() + b": problem too large" in built.offk_last_error(None)


@pytest.mark.parametrize("c", s2.cases(), ids=s2.case_id)
def test_the_layout_pairs_every_tap_with_its_pixels(c):
    """the K layout against the definition: the helper's operands summed in fp64 over the position order equal torch's dW and db, at the
    ten cases of tests/conv_bwd.py (S2) (the plan-chosen n replaced by 5: the layout does not depend on the plan)"""
    c = c if c.n is not None else c._replace(n=5)
    for relu_in in (False, True):
        inp, ref = s2.cached(c, "int", relu_in)
        G, taps = ws.operands(inp["g"].numpy(), inp["x"].numpy(), c.k, relu_in=relu_in)
        OW, PP = ws.geometry(c.H, c.W)
        assert G.shape == (c.n * PP, c.co) and OW == c.W // 2 and len(taps) == c.k * c.k
        dw = np.stack([np.stack([G.astype(np.float64).T @ taps[(kh, kw)].astype(np.float64) for kw in range(c.k)], -1) for kh in range(c.k)], -2)
        assert np.array_equal(dw, ref["dW"].numpy()), (s2.case_id(c), relu_in)
        assert np.array_equal(G.astype(np.float64).sum(0), ref["db"].numpy())
    assert ws.chunk_bounds(5, c.H, c.W, 3) == [(0, 2 * PP), (2 * PP, 4 * PP), (4 * PP, 5 * PP)]


@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
@pytest.mark.parametrize("shape", [(7, 2, 6, 10, 32, 64), (5, 3, 6, 4, 32, 64)], ids=["k7_2x6x10", "k5_3x6x4"])
def test_the_gpu_inequality_discriminates_in_the_kernels_layout(shape, pattern, signs):
    k, n, H, W, ci, co = shape
    OH, OW = H // 2, W // 2
    g = synth.make_adversarial((n * OH * OW, co), pattern, "same", seed=11, relu=(pattern == 0x7FFFFF)).reshape(n, OH, OW, co)
    # the sign of x alternates along the map's columns, so that it alternates along the positions of every tap's stride-2 sample too
    x = synth.make_adversarial((n * H * (W // 2), ci), pattern, signs, seed=12, k_axis=0).reshape(n, H, W // 2, 1, ci)
    x = np.ascontiguousarray(np.broadcast_to(x, (n, H, W // 2, 2, ci))).reshape(n, H, W, ci) * np.float32(2.0 ** -4)
    G, taps = ws.operands(g, x, k)
    bounds = ws.chunk_bounds(n, H, W, n)                 # one image per chunk: the reduce's additions are part of the form
    ref, dropped, mag = ws.terms(G, taps, k)
    sb.assert_discriminates("k %d pattern 0x%06X %-11s" % (k, pattern, signs), lambda skip: ws.emulate_chunked(G, taps, bounds, k, skip=skip),
                            ref, dropped, mag)


def test_fusion_conv_keyword():
    from offk_amd import runtime
    from offk_amd.off_module import FusionConv2d
    forms = (dict(kernel_size=7, padding=3), dict(kernel_size=5, padding=2))
    for kw in forms:
        m = FusionConv2d(64, 64, stride=2, **kw)
        assert m.s2_wgrad_arith == "fp32" and "s2_wgrad_arith" not in repr(m)
        s = FusionConv2d(64, 64, stride=2, relu=True, s2_wgrad_arith="f32split", **kw)
        assert s.s2_wgrad_arith == "f32split" and repr(s).endswith(", s2_wgrad_arith=f32split)")
        assert repr(s).replace(", s2_wgrad_arith=f32split", "") == repr(FusionConv2d(64, 64, stride=2, relu=True, **kw))
        for bad in ("bf16", "split", None, "FP32"):
            with pytest.raises(ValueError, match="s2_wgrad_arith"):
                FusionConv2d(64, 64, stride=2, s2_wgrad_arith=bad, **kw)
        # the two pinned behaviours: wgrad_arith stays the stride-1 switch, bwd_arith leaves s2_wgrad_arith alone
        with pytest.raises(ValueError, match="stride"):
            FusionConv2d(64, 64, stride=2, wgrad_arith="f32split", **kw)
        b = FusionConv2d(64, 64, stride=2, bwd_arith="f32split", **kw)
        assert b.s2_wgrad_arith == "fp32" and b.wgrad_arith == "fp32" and "s2_wgrad_arith" not in repr(b)
        # it combines with dgrad_arith and with bwd_arith
        both = FusionConv2d(64, 64, stride=2, dgrad_arith="f32split", s2_wgrad_arith="f32split", **kw)
        assert (both.dgrad_arith, both.s2_wgrad_arith) == ("f32split", "f32split")
        assert ", dgrad_arith=f32split, s2_wgrad_arith=f32split" in repr(both)
        allb = FusionConv2d(64, 64, stride=2, bwd_arith="f32split", s2_wgrad_arith="f32split", **kw)
        assert (allb.bwd_arith, allb.s2_wgrad_arith) == ("f32split", "f32split") and ", bwd_arith=f32split, s2_wgrad_arith=f32split" in repr(allb)
    for k in (1, 3):
        assert FusionConv2d(64, 64, k, padding=(k - 1) // 2).s2_wgrad_arith == "fp32"
        assert FusionConv2d(64, 64, k, padding=(k - 1) // 2, s2_wgrad_arith="fp32").s2_wgrad_arith == "fp32"
        with pytest.raises(ValueError, match="wgrad_arith is the stride-1"):
            FusionConv2d(64, 64, k, padding=(k - 1) // 2, s2_wgrad_arith="f32split")
    assert inspect.signature(FusionConv2d.__init__).parameters["s2_wgrad_arith"].default == "fp32"
    assert inspect.signature(runtime.conv2d_s2_backward_weight).parameters["arith"].default == "fp32"
    with pytest.raises(ValueError, match="arith must be one of"):
        runtime.conv2d_s2_backward_weight(None, None, 7, 3, arith="bf16")
    doc = FusionConv2d.__doc__
    assert "no split entry yet" not in doc and "offk_conv2d_s2_backward_weight_split" in doc and "keyword of its own" in doc


def test_the_build_keeps_the_kernel_in_registers(built):
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("offk_build", os.path.join(os.path.dirname(_lib.LIB_PATH), "build.py"))
    b = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(b)
    name = "conv_wgrad_s2_split.hip"
    assert name in b.SOURCES and "-fno-slp-vectorize" in b.EXTRA_FLAGS[name]
    assert len([r for r in b.REGISTER_RESIDENT_KERNELS if r[0] == name]) == 2, "a register-guard row per kernel form"
    cos = b._code_objects(os.path.join(b.OBJ, "conv_wgrad_s2_split.o"))
    try:
        kernels = [k for co in cos for k in b.kernel_resources(co)]
        b.check_store_data_hazard("conv_wgrad_s2_split.o", cos)
    finally:
        for path in cos:
            os.remove(path)
    assert len(kernels) == 2, "the two forms and nothing else"
    rows = b.check_register_resident(name, kernels)
    assert len(rows) == 2
    assert all(k["vgpr_count"] <= 256 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0 for k in rows)
    bad = [dict(k) for k in kernels]
    for k in bad:
        if "conv_s2_wgrad_split_kernel<5>" in k["name"]:
            k["private_segment_fixed_size"] = 256
    with pytest.raises(RuntimeError, match="register guard failed"):
        b.check_register_resident(name, bad)
