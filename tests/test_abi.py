"""CPU-side checks of the C-ABI boundary: liboffk.so builds, loads, and exports exactly
the symbols include/offk.h declares (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(ROOT, "include", "offk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(offk_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def test_header_and_binding_agree():
    syms = header_symbols()
    assert len(syms) >= 18
    assert sorted(_lib.SIGNATURES) == syms


def test_library_exports_every_declared_symbol(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in header_symbols():
        assert hasattr(raw, s), s
    assert built.offk_abi_version() == 10


def test_handleless_errors_are_reported(built):
    # argument validation happens before any HIP call, so this is safe without a GPU
    rc = built.offk_conv2d(None, None, 0, 0, 0, 0, 0, 0, None, None, 0, 0, 0, 0, 0, None, 0, 0, 0, None, 0, 0)
    assert rc == -1
    assert b"offk_conv2d" in built.offk_last_error(None)
    rc = built.offk_create(None, None)
    assert rc == -1


def test_create_without_gpu_fails_loudly(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = _lib.OffkConfig(1, 7, 0, 0, 0, 101, 0, 0, 0)
    h = ctypes.c_void_p()
    rc = built.offk_create(ctypes.byref(cfg), ctypes.byref(h))
    assert rc == -5 and not h.value
    from offk_amd import runtime
    with pytest.raises(_lib.OffkError):
        runtime.OffForward(1, 7)


# ---- offk_bottleneck_chain14_split refuses what it cannot run (views that do not hold their slice, in-place calls) ----

def _fake(addr):
    """A non-null device-pointer stand-in: validation precedes every HIP call, so it is never dereferenced."""
    return ctypes.cast(ctypes.c_void_p(addr), ctypes.POINTER(ctypes.c_float))


_N_IMG, _BASE = 2, 0x10000000
_SPAN = _N_IMG * 196 * 256 * 4                   # bytes of a [n_img * 196][256] fp32 view
_SCRATCH = 6 * (64 * 256 + 64 * 576 + 2 * 256 * 64)


def _chain_args(**over):
    """A call of the residual form (Cin = 256, res = x, dense 256-channel views, disjoint y) that passes validation; `over` replaces arguments."""
    a = dict(stream=None, x=_fake(_BASE), x_cstride=256, x_coff=0, n_img=_N_IMG, Cin=256, relu_in=0,
             w1=_fake(0x1000), b1=_fake(0x2000), w2=_fake(0x3000), b2=_fake(0x4000), w3=_fake(0x5000), b3=_fake(0x6000),
             branch_w=None, branch_b=None, res=_fake(_BASE), res_cstride=256, res_coff=0,
             y=_fake(_BASE + 4 * _SPAN), y_cstride=256, y_coff=0, scratch=ctypes.c_void_p(0x7000), scratch_bytes=_SCRATCH)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


_CHAIN_REFUSALS = {
    "x_stride_smaller_than_slice": dict(x_cstride=192),
    "x_offset_past_stride": dict(x_cstride=256, x_coff=64),
    "y_stride_smaller_than_slice": dict(y_cstride=128),
    "y_offset_past_stride": dict(y_cstride=320, y_coff=128),
    "res_stride_smaller_than_slice": dict(res_cstride=64),
    "res_offset_past_stride": dict(res_cstride=256, res_coff=32),
    "negative_x_offset": dict(x_coff=-64, x_cstride=512),
    "negative_y_offset": dict(y_coff=-4, y_cstride=512),
    "negative_res_offset": dict(res_coff=-4, res_cstride=512),
    "branch_with_residual": dict(Cin=64, branch_w=_fake(0x8000), branch_b=_fake(0x9000)),
    "in_place_y_is_x": dict(y=_fake(_BASE), res=None),
    "y_overlaps_x_tail": dict(y=_fake(_BASE + _SPAN - 1024), res=None),
    "y_overlaps_x_from_below": dict(y=_fake(_BASE - _SPAN + 1024), res=None),
    "y_overlaps_res": dict(res=_fake(_BASE + 8 * _SPAN), y=_fake(_BASE + 8 * _SPAN + 4096)),
    "y_into_slice_of_x_buffer": dict(x_cstride=512, y=_fake(_BASE), y_cstride=512, y_coff=256, res=None),
}


@pytest.mark.parametrize("rule", sorted(_CHAIN_REFUSALS))
def test_chain14_split_refuses_bad_views_and_aliasing(built, rule):
    """One refused call per rule of include/offk.h (K4cs): OFFK_ERR_INVALID with the entry's name, before anything is enqueued -- a stride
    smaller than the slice would store outside the caller's buffer, an in-place call races with the other half-image block's halo reads."""
    rc = built.offk_bottleneck_chain14_split(*_chain_args(**_CHAIN_REFUSALS[rule]))
    assert rc == -1, (rule, rc, built.offk_last_error(None))
    assert b"offk_bottleneck_chain14_split" in built.offk_last_error(None)
