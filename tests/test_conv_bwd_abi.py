"""CPU-side checks of the fusion convs' backward entries (include/offk.h, K4b): the four symbols exist and are bound, the plan is a pure
function of its integers, and every refusal comes back OFFK_ERR_INVALID with the entry's name before any HIP call (the pointers are
fakes that are never dereferenced, as in tests/test_abi.py)."""
import ctypes

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

from .conv_bwd import S1 as cb

ENTRIES = ("offk_relu_backward", "offk_conv2d_backward_data", "offk_conv2d_backward_weight", "offk_conv2d_backward_plan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _fake(addr):
    return ctypes.c_void_p(addr)


def _plan(lib, n, H, W, ci, co, k):
    d, w, c = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(0)
    rc = lib.offk_conv2d_backward_plan(n, H, W, ci, co, k, k, ctypes.byref(d), ctypes.byref(w), ctypes.byref(c))
    return rc, d.value, w.value, c.value


def test_symbols_are_exported_and_bound(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert tuple(getattr(built, name).argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert built.offk_abi_version() == 10


@pytest.mark.parametrize("n_img", [1, 6, 384])
@pytest.mark.parametrize("shape", cb.FUSION_SHAPES, ids=["%dx%d_%dto%d_k%d" % (s[0], s[0], s[1], s[2], s[3]) for s in cb.FUSION_SHAPES])
def test_plan_is_a_pure_function(built, shape, n_img):
    H, ci, co, k = shape
    first = _plan(built, n_img, H, H, ci, co, k)
    assert first[0] == 0, built.offk_last_error(None)
    assert first[1] > 0 and first[2] > 0 and first[3] >= 1
    assert first[1] >= 4 * co * ci * k * k                       # the rotated weight at least
    assert first[2] >= 4 * first[3] * (co * ci * k * k + co)      # the slabs [chunk][Co][Ci k k] and [chunk][Co]
    assert first[3] <= n_img                                      # chunks are whole images
    for _ in range(3):
        assert _plan(built, n_img, H, H, ci, co, k) == first


def test_plan_runs_from_python_wrapper(built):
    from offk_amd import runtime
    assert runtime.conv2d_backward_plan(6, 14, 14, 64, 64, 3) == _plan(built, 6, 14, 14, 64, 64, 3)[1:]
    c = cb.Case(3, *cb.CHUNKED[3])
    n = cb.chunked_n(runtime.conv2d_backward_plan, c)
    chunks = runtime.conv2d_backward_plan(n, c.H, c.W, c.ci, c.co, c.k)[2]
    assert chunks >= 3 and n % (-(-n // chunks)) != 0


_N, _H, _CI, _CO = 2, 14, 64, 128
_ROWS = _N * _H * _H
_BIG = 1 << 30                     # bytes: no plan of these shapes comes near


def _data_args(**over):
    a = dict(stream=None, g=_fake(0x10000000), g_cstride=_CO, g_coff=0, n_img=_N, H=_H, W=_H, Co=_CO, w=_fake(0x1000), Ci=_CI, KH=3, KW=3,
             pad=1, dx=_fake(0x20000000), dx_cstride=_CI, dx_coff=0, accumulate=0, scratch=_fake(0x30000000), scratch_bytes=_BIG)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def _weight_args(**over):
    a = dict(stream=None, x=_fake(0x20000000), x_cstride=_CI, x_coff=0, g=_fake(0x10000000), g_cstride=_CO, g_coff=0, n_img=_N, H=_H, W=_H,
             Ci=_CI, Co=_CO, KH=3, KW=3, pad=1, relu_in=0, dw=_fake(0x1000), db=_fake(0x2000), accumulate=0, scratch=_fake(0x30000000),
             scratch_bytes=_BIG)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def _relu_args(**over):
    a = dict(stream=None, dy=_fake(0x10000000), dy_cstride=_CO, dy_coff=0, y=_fake(0x20000000), y_cstride=_CO, y_coff=0, rows=_ROWS, C=_CO,
             g=_fake(0x30000000), g_cstride=_CO, g_coff=0, accumulate=0)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


_G_BYTES = _ROWS * _CO * 4
_REFUSALS = {
    "data_null_g": ("offk_conv2d_backward_data", _data_args, dict(g=None)),
    "data_null_w": ("offk_conv2d_backward_data", _data_args, dict(w=None)),
    "data_null_dx": ("offk_conv2d_backward_data", _data_args, dict(dx=None)),
    "data_null_scratch": ("offk_conv2d_backward_data", _data_args, dict(scratch=None)),
    "data_ci_96": ("offk_conv2d_backward_data", _data_args, dict(Ci=96, dx_cstride=96)),
    "data_kh_5": ("offk_conv2d_backward_data", _data_args, dict(KH=5, KW=5, pad=2)),
    "data_pad_not_half": ("offk_conv2d_backward_data", _data_args, dict(pad=0)),
    "data_g_stride_short": ("offk_conv2d_backward_data", _data_args, dict(g_cstride=_CO, g_coff=64)),
    "data_dx_stride_short": ("offk_conv2d_backward_data", _data_args, dict(dx_cstride=32)),
    "data_negative_offset": ("offk_conv2d_backward_data", _data_args, dict(dx_coff=-4, dx_cstride=256)),
    "data_short_scratch": ("offk_conv2d_backward_data", _data_args, dict(scratch_bytes=4 * _CO * _CI * 9 - 4)),
    "data_dx_is_g": ("offk_conv2d_backward_data", _data_args, dict(dx=_fake(0x10000000))),
    "data_dx_overlaps_g_tail": ("offk_conv2d_backward_data", _data_args, dict(dx=_fake(0x10000000 + _G_BYTES - 1024))),
    "data_dx_slice_of_g_buffer": ("offk_conv2d_backward_data", _data_args, dict(g_cstride=256, dx=_fake(0x10000000), dx_cstride=256, dx_coff=128)),
    "weight_null_x": ("offk_conv2d_backward_weight", _weight_args, dict(x=None)),
    "weight_null_g": ("offk_conv2d_backward_weight", _weight_args, dict(g=None)),
    "weight_null_dw": ("offk_conv2d_backward_weight", _weight_args, dict(dw=None)),
    "weight_null_scratch": ("offk_conv2d_backward_weight", _weight_args, dict(scratch=None)),
    "weight_ci_96": ("offk_conv2d_backward_weight", _weight_args, dict(Ci=96, x_cstride=96)),
    "weight_kh_5": ("offk_conv2d_backward_weight", _weight_args, dict(KH=5, KW=5, pad=2)),
    "weight_pad_not_half": ("offk_conv2d_backward_weight", _weight_args, dict(pad=2)),
    "weight_x_stride_short": ("offk_conv2d_backward_weight", _weight_args, dict(x_cstride=128, x_coff=96)),
    "weight_g_stride_short": ("offk_conv2d_backward_weight", _weight_args, dict(g_cstride=64)),
    "weight_odd_offset": ("offk_conv2d_backward_weight", _weight_args, dict(x_cstride=130, x_coff=2)),
    "weight_short_scratch": ("offk_conv2d_backward_weight", _weight_args, dict(scratch_bytes=4 * (_CO * _CI * 9 + _CO) - 4)),
    "relu_null_dy": ("offk_relu_backward", _relu_args, dict(dy=None)),
    "relu_null_y": ("offk_relu_backward", _relu_args, dict(y=None)),
    "relu_null_g": ("offk_relu_backward", _relu_args, dict(g=None)),
    "relu_stride_short": ("offk_relu_backward", _relu_args, dict(g_cstride=_CO, g_coff=4)),
    "relu_partial_overlap": ("offk_relu_backward", _relu_args, dict(g=_fake(0x10000000 + 4096))),
    "relu_same_pointer_other_offset": ("offk_relu_backward", _relu_args, dict(dy_cstride=256, g=_fake(0x10000000), g_cstride=256, g_coff=128)),
    "relu_g_overlaps_y": ("offk_relu_backward", _relu_args, dict(g=_fake(0x20000000 + 256))),
    "plan_ci_96": ("offk_conv2d_backward_plan", lambda **o: [2, 14, 14, 96, 64, 3, 3, None, None, None], {}),
    "plan_kh_5": ("offk_conv2d_backward_plan", lambda **o: [2, 14, 14, 64, 64, 5, 5, None, None, None], {}),
}


@pytest.mark.parametrize("rule", sorted(_REFUSALS))
def test_refusals_name_the_entry(built, rule):
    entry, make, over = _REFUSALS[rule]
    rc = getattr(built, entry)(*make(**over))
    assert rc == -1, (rule, rc, built.offk_last_error(None))
    assert entry.encode() in built.offk_last_error(None), built.offk_last_error(None)


def test_in_place_relu_backward_passes_validation_order(built):
    """g = dy (same pointer, stride, offset) is the one allowed overlap: the same call with a short stride is still refused for the stride,
    and the in-place form itself is not refused for overlap (its refusal here would be the overlap message)."""
    rc = built.offk_relu_backward(*_relu_args(g=_fake(0x10000000), g_cstride=_CO, g_coff=0, C=_CO + 4))
    assert rc == -1 and b"cstride < coff + C" in built.offk_last_error(None)


def test_module_refuses_what_the_entries_do_not_cover(built):
    from offk_amd.off_module import FusionConv2d
    with pytest.raises(ValueError):
        FusionConv2d(64, 64, 3, stride=2)
    for kw in (dict(kernel_size=5, padding=2), dict(kernel_size=3, padding=0), dict(kernel_size=3, padding=1, groups=2),
               dict(kernel_size=3, padding=1, dilation=2)):
        with pytest.raises(ValueError):
            FusionConv2d(64, 64, **kw)
    with pytest.raises(ValueError):
        FusionConv2d(96, 64, 1)
    m = FusionConv2d(64, 128, 3, padding=1, relu=True)
    assert sorted(m.state_dict()) == ["bias", "weight"] and m.weight.shape == (128, 64, 3, 3)
