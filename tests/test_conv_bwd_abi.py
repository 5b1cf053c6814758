"""CPU-side checks of the fusion convs' backward entries (include/offk.h, K4b): the four symbols exist and are bound, the plan is a pure
function of its integers, and every refusal comes back OFFK_ERR_INVALID with the entry's name before any HIP call (the pointers are
fakes that are never dereferenced, as in tests/test_abi.py)."""
import ctypes

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

from . import conv_bwd_abi as abi
from .conv_bwd import S1 as cb

ENTRIES = ("offk_relu_backward", "offk_conv2d_backward_data", "offk_conv2d_backward_weight", "offk_conv2d_backward_plan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


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


@pytest.mark.parametrize("rule", sorted(abi.REFUSALS))
def test_refusals_name_the_entry(built, rule):
    entry, make, over = abi.REFUSALS[rule]
    rc = getattr(built, entry)(*make(**over))
    assert rc == -1, (rule, rc, built.offk_last_error(None))
    assert entry.encode() in built.offk_last_error(None), built.offk_last_error(None)


def test_in_place_relu_backward_passes_validation_order(built):
    """g = dy (same pointer, stride, offset) is the one allowed overlap: the same call with a short stride is still refused for the stride,
    and the in-place form itself is not refused for overlap (its refusal here would be the overlap message)."""
    rc = built.offk_relu_backward(*abi.relu_args(g=abi.fake(0x10000000), g_cstride=abi.CO, g_coff=0, C=abi.CO + 4))
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
