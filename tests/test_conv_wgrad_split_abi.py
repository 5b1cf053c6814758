"""CPU checks of the fusion convs' split-fp32 weight gradient (offk_conv2d_backward_weight_split / offk_conv2d_backward_plan_split,
csrc/conv_wgrad_split.hip): both symbols exist and are bound under the unchanged ABI version; the plan is a pure function with pinned
chunks; every refusal of the fp32 entry is a refusal of the new one, under its own name and before any HIP call (fake pointers, never
dereferenced); FusionConv2d's switch; build.py's register guard; and the inequality tests/test_gpu_conv_wgrad_split.py asserts
DISCRIMINATES in the kernel's K layout: the CPU emulation (tests/conv_wgrad_split.py) satisfies it on worst-case mantissas, the same
emulation with any one of the six issued plane products left out does not."""
import ctypes
import os
import re

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

from .conv_bwd import S1 as cb
from . import conv_wgrad_split as cs
from . import split_bound as sb
from . import conv_bwd_abi as fp32_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT, PLAN = "offk_conv2d_backward_weight_split", "offk_conv2d_backward_plan_split"

# weight_chunks of the split plan at n_img = 1, 6, 384 for tests/conv_bwd.S1.FUSION_SHAPES, in that order
PLAN_CHUNKS = {(14, 64, 64, 1): (1, 3, 192), (14, 64, 64, 3): (1, 3, 192), (14, 64, 256, 1): (1, 3, 192), (14, 256, 64, 1): (1, 3, 192),
               (7, 128, 128, 1): (1, 1, 64), (7, 128, 128, 3): (1, 2, 64), (7, 128, 512, 1): (1, 1, 64), (7, 512, 128, 1): (1, 1, 64),
               (7, 128, 512, 3): (1, 2, 16), (7, 832, 256, 3): (1, 2, 4), (7, 256, 256, 1): (1, 1, 64), (7, 256, 256, 3): (1, 2, 16),
               (7, 256, 1024, 1): (1, 1, 16)}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _plan(lib, n, H, W, ci, co, k):
    w, c = ctypes.c_size_t(0), ctypes.c_int(0)
    rc = lib.offk_conv2d_backward_plan_split(n, H, W, ci, co, k, k, ctypes.byref(w), ctypes.byref(c))
    return rc, w.value, c.value


def test_symbols_are_exported_bound_and_declared(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in (WEIGHT, PLAN):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert tuple(getattr(built, name).argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert built.offk_abi_version() == 10
    assert list(_lib.SIGNATURES[WEIGHT][1]) == list(_lib.SIGNATURES["offk_conv2d_backward_weight"][1])
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    assert re.search(r"#define OFFK_ABI_VERSION 10\b", src)

    def args(name):
        return re.sub(r"\s+", " ", re.search(r"\bint %s\(([^;]*)\);" % name, src).group(1))
    assert args(WEIGHT) == args("offk_conv2d_backward_weight"), "the argument list of the fp32 entry, word for word"
    doc = src[src.index("K4b's weight / bias gradient in split-fp32 arithmetic"):src.index("int %s(" % WEIGHT)]
    for needle in ("(2^-21 + 2^-30)", "pitch = 8 * ceil((W + 1) / 8)", "PP = (H + 1) * pitch", "steps of 32", "chunk order", "No atomics", "NaN",
                   "OFFK_PRECISION_F32SPLIT", "g_l x_h, g_h x_l, g_m x_m, g_m x_h, g_h x_m", "pure host code", "no empty chunk", "2^-109"):
        assert needle in doc, needle


@pytest.mark.parametrize("shape", cb.FUSION_SHAPES, ids=["%dx%d_%dto%d_k%d" % (s[0], s[0], s[1], s[2], s[3]) for s in cb.FUSION_SHAPES])
def test_plan_is_a_pure_function_with_pinned_chunks(built, shape):
    H, ci, co, k = shape
    for n_img, want in zip((1, 6, 384), PLAN_CHUNKS[shape]):
        first = _plan(built, n_img, H, H, ci, co, k)
        assert first[0] == 0, built.offk_last_error(None)
        chunks = first[2]
        assert chunks == want, (shape, n_img, chunks)
        assert chunks == -(-n_img // -(-n_img // chunks)), "whole images per chunk, no empty chunk"
        assert first[1] == chunks * (co * ci * k * k + co) * 4
        for _ in range(3):
            assert _plan(built, n_img, H, H, ci, co, k) == first
    assert built.offk_conv2d_backward_plan_split(6, H, H, ci, co, k, k, None, None) == 0, "output pointers may be NULL"


def test_plan_runs_from_the_python_wrapper_and_chunks_short(built):
    from offk_amd import runtime
    assert runtime.conv2d_backward_plan_split(6, 14, 14, 64, 64, 3) == _plan(built, 6, 14, 14, 64, 64, 3)[1:]
    for k in (1, 3):
        c = cb.Case(k, *cb.CHUNKED[k])
        n = cb.chunked_n(lambda *a: (0,) + runtime.conv2d_backward_plan_split(*a), c)
        chunks = runtime.conv2d_backward_plan_split(n, c.H, c.W, c.ci, c.co, c.k)[1]
        assert chunks >= 3 and n % (-(-n // chunks)) != 0


def test_the_refusal_table_covers_the_fp32_entrys(built):
    assert len([1 for e, _m, _o in fp32_abi.REFUSALS.values() if e == "offk_conv2d_backward_weight"]) == 11
    assert _plan(built, fp32_abi.N, fp32_abi.H, fp32_abi.H, fp32_abi.CI, fp32_abi.CO, 3)[1:] == (fp32_abi.WGRAD_SPLIT_SCRATCH, 1)


@pytest.mark.parametrize("rule", sorted(fp32_abi.WGRAD_SPLIT_REFUSALS))
def test_refusals_name_the_split_entry(built, rule):
    over = fp32_abi.WGRAD_SPLIT_REFUSALS[rule]
    for entry in (WEIGHT, "offk_conv2d_backward_weight"):
        rc = getattr(built, entry)(*fp32_abi.weight_args(**over))
        assert rc == -1, (rule, entry, rc, built.offk_last_error(None))
        assert entry.encode() + b":" in built.offk_last_error(None), built.offk_last_error(None)


def test_db_may_be_null_and_plan_refusals(built):
    # db = NULL is no refusal: the same call with a short scratch is refused for the scratch, not for the pointer
    rc = getattr(built, WEIGHT)(*fp32_abi.weight_args(db=None, scratch_bytes=fp32_abi.WGRAD_SPLIT_SCRATCH - 1))
    assert rc == -1 and b"scratch too small" in built.offk_last_error(None)
    for a in ([2, 14, 14, 96, 64, 3, 3, None, None], [2, 14, 14, 64, 64, 5, 5, None, None], [0, 14, 14, 64, 64, 3, 3, None, None]):
        assert built.offk_conv2d_backward_plan_split(*a) == -1
        assert PLAN.encode() in built.offk_last_error(None)


def test_fusion_conv_switch():
    from offk_amd.off_module import FusionConv2d
    m = FusionConv2d(64, 64, 3, padding=1)
    assert m.wgrad_arith == "fp32" and "wgrad_arith" not in repr(m)
    s = FusionConv2d(64, 128, 3, padding=1, relu=True, wgrad_arith="f32split")
    assert s.wgrad_arith == "f32split" and "wgrad_arith=f32split" in repr(s)
    assert FusionConv2d(128, 64, 1, wgrad_arith="f32split").wgrad_arith == "f32split"
    for bad in ("bf16", "split", None, "FP32"):
        with pytest.raises(ValueError, match="wgrad_arith"):
            FusionConv2d(64, 64, 1, wgrad_arith=bad)
    for kw in (dict(kernel_size=7, padding=3), dict(kernel_size=5, padding=2)):
        assert FusionConv2d(64, 64, stride=2, **kw).wgrad_arith == "fp32"
        with pytest.raises(ValueError, match="stride"):
            FusionConv2d(64, 64, stride=2, wgrad_arith="f32split", **kw)
    import inspect
    from offk_amd import runtime
    assert inspect.signature(runtime.conv2d_backward_weight).parameters["arith"].default == "fp32"
    assert inspect.signature(FusionConv2d.__init__).parameters["wgrad_arith"].default == "fp32"
    with pytest.raises(ValueError, match="arith must be one of"):
        runtime.conv2d_backward_weight(None, None, 3, 1, arith="bf16")


def test_the_build_keeps_the_kernel_in_registers(built):
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("offk_build", os.path.join(os.path.dirname(_lib.LIB_PATH), "build.py"))
    b = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(b)
    assert "conv_wgrad_split.hip" in b.SOURCES and "-fno-slp-vectorize" in b.EXTRA_FLAGS["conv_wgrad_split.hip"]
    assert [r for r in b.REGISTER_RESIDENT_KERNELS if r[0] == "conv_wgrad_split.hip"], "the register-guard row"
    obj = os.path.join(b.OBJ, "conv_wgrad_split.o")
    cos = b._code_objects(obj)
    try:
        kernels = [k for co in cos for k in b.kernel_resources(co)]
    finally:
        for path in cos:
            os.remove(path)
    rows = b.check_register_resident("conv_wgrad_split.hip", kernels)
    assert len(rows) == 2 and all(k["vgpr_count"] <= 256 and k["private_segment_fixed_size"] == 0 for k in rows)
    bad = [dict(k) for k in kernels]
    bad[0]["private_segment_fixed_size"] = 256
    with pytest.raises(RuntimeError, match="register guard failed"):
        b.check_register_resident("conv_wgrad_split.hip", bad)


def test_the_layout_pairs_every_tap_with_its_pixels():
    """the K layout against the definition: exact fp64 sums over the position order equal the direct sums over (n, h, w), tap by tap, for
    maps on both sides of the pitch's boundaries and of the staged windows' (pitch 24 | 32 | 40)"""
    rng = np.random.default_rng(5)
    for k, H, W in ((3, 3, 7), (3, 3, 8), (3, 2, 15), (3, 2, 16), (3, 2, 23), (3, 2, 24), (3, 2, 31), (3, 2, 32), (3, 1, 1), (3, 2, 2), (1, 5, 3)):
        g = rng.integers(-8, 9, (2, H, W, 3)).astype(np.float32)
        x = rng.integers(-8, 9, (2, H, W, 2)).astype(np.float32)
        G, taps = cs.operands(g, x, k, relu_in=True)
        pitch, PP = cs.geometry(H, W, k)
        assert G.shape[0] == 2 * PP and (k == 1 or (pitch % 8 == 0 and pitch >= W + 1 and pitch - 8 < W + 1))
        xr = np.maximum(x, 0)
        pad = (k - 1) // 2
        xp = np.pad(xr, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
        for (kh, kw), X in taps.items():
            want = np.einsum("nhwo,nhwi->oi", g.astype(np.float64), xp[:, kh:kh + H, kw:kw + W].astype(np.float64))
            assert np.array_equal(G.astype(np.float64).T @ X.astype(np.float64), want), (k, H, W, kh, kw)


@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
@pytest.mark.parametrize("shape", [(3, 2, 5, 3, 64, 64), (1, 1, 7, 7, 64, 64)], ids=["k3_2x5x3", "k1_1x7x7"])
def test_the_gpu_inequality_discriminates_in_the_kernels_layout(shape, pattern, signs):
    k, n, H, W, ci, co = shape
    g = synth.make_adversarial((n, H, W, co), pattern, "same", seed=11, relu=(pattern == 0x7FFFFF))
    x = synth.make_adversarial((n * H * W, ci), pattern, signs, seed=12, k_axis=0).reshape(n, H, W, ci) * np.float32(2.0 ** -4)
    G, taps = cs.operands(g, x, k)
    bounds = cs.chunk_bounds(n, H, W, k, n)                # one image per chunk: the reduce's additions are part of the form
    ref, dropped, mag = cs.terms(G, taps, k)
    sb.assert_discriminates("k %d pattern 0x%06X %-11s" % (k, pattern, signs), lambda skip: cs.emulate_chunked(G, taps, bounds, k, skip=skip),
                            ref, dropped, mag)
