"""CPU-side checks of the stride-2 fusion convs' backward entries (include/offk.h, K4b stride 2): the three symbols exist and are bound, the
plan is a pure function of its integers, every refusal comes back OFFK_ERR_INVALID with the entry's name before any HIP call (the
pointers are fakes that are never dereferenced, as in tests/test_conv_bwd_abi.py), and FusionConv2d accepts exactly the two forms."""
import ctypes
import importlib.util
import os

import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib

from . import conv_bwd_s2_abi as abi
from .conv_bwd import S2 as cs

ENTRIES = ("offk_conv2d_s2_backward_data", "offk_conv2d_s2_backward_weight", "offk_conv2d_s2_backward_plan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _plan(lib, n, H, W, ci, co, k):
    d, w, c = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(0)
    rc = lib.offk_conv2d_s2_backward_plan(n, H, W, ci, co, k, k, ctypes.byref(d), ctypes.byref(w), ctypes.byref(c))
    return rc, d.value, w.value, c.value


def test_symbols_are_exported_and_bound(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert tuple(getattr(built, name).argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert built.offk_abi_version() == 10


@pytest.mark.parametrize("n_img", [1, 6, 384])
@pytest.mark.parametrize("real", cs.REAL, ids=[r[0] for r in cs.REAL])
def test_plan_is_a_pure_function(built, real, n_img):
    _, ci, co, k, H = real
    first = _plan(built, n_img, H, H, ci, co, k)
    assert first[0] == 0, built.offk_last_error(None)
    assert first[1] >= 4 * co * ci * k * k                       # the phase-major weight at least
    assert first[2] >= 4 * first[3] * (co * ci * k * k + co)      # the slabs [chunk][Co][Ci k k] and [chunk][Co]
    assert 1 <= first[3] <= n_img                                 # chunks are whole images
    for _ in range(3):
        assert _plan(built, n_img, H, H, ci, co, k) == first


def test_plan_runs_from_python_wrapper(built):
    from offk_amd import runtime
    assert runtime.conv2d_s2_backward_plan(6, 28, 28, 320, 64, 7) == _plan(built, 6, 28, 28, 320, 64, 7)[1:]
    for c in cs.cases():
        if c.n is None:
            c = cs.resolve(runtime.conv2d_s2_backward_plan, c)
            chunks = runtime.conv2d_s2_backward_plan(c.n, c.H, c.W, c.ci, c.co, c.k)[2]
            assert chunks >= 3 and c.n % (-(-c.n // chunks)) != 0


@pytest.mark.parametrize("rule", sorted(abi.REFUSALS))
def test_refusals_name_the_entry(built, rule):
    entry, make, over = abi.REFUSALS[rule]
    rc = getattr(built, entry)(*make(**over))
    assert rc == -1, (rule, rc, built.offk_last_error(None))
    assert entry.encode() in built.offk_last_error(None), built.offk_last_error(None)


def test_the_unmodified_arguments_are_not_refused_for_their_shape(built):
    """the refusal table's base arguments are valid: the same call with only a short scratch is refused for the scratch, nothing else"""
    rc = built.offk_conv2d_s2_backward_data(*abi.data_args(scratch_bytes=0))
    assert rc == -1 and b"scratch too small" in built.offk_last_error(None)
    rc = built.offk_conv2d_s2_backward_weight(*abi.weight_args(scratch_bytes=0, db=None))
    assert rc == -1 and b"scratch too small" in built.offk_last_error(None)
    for k, pad in cs.FORMS.items():
        assert built.offk_conv2d_s2_backward_plan(*abi.plan_args(kh=k, kw=k)) == 0


def test_stride1_entries_keep_refusing_the_large_kernels(built):
    for k in (5, 7):
        assert built.offk_conv2d_backward_plan(2, 14, 14, 64, 64, k, k, None, None, None) == -1
        assert b"offk_conv2d_backward_plan" in built.offk_last_error(None)


def test_the_build_keeps_the_weight_gradient_in_registers(built):
    """conv_bwd_s2.hip is built with conv_bwd.hip's flags, and build.py's register guard covers both forms of the weight-gradient
    kernel at the occupancy the plan assumes (two waves per SIMD: at most 256 registers, no spill, no private segment)."""
    spec_ = importlib.util.spec_from_file_location("offk_build", os.path.join(os.path.dirname(_lib.LIB_PATH), "build.py"))
    b = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(b)
    assert "conv_bwd_s2.hip" in b.SOURCES and b.EXTRA_FLAGS["conv_bwd_s2.hip"] == b.EXTRA_FLAGS["conv_bwd.hip"]
    cos = b._code_objects(os.path.join(b.OBJ, "conv_bwd_s2.o"))
    try:
        kernels = [k for co in cos for k in b.kernel_resources(co)]
    finally:
        for path in cos:
            os.remove(path)
    rows = b.check_register_resident("conv_bwd_s2.hip", kernels)
    assert len(rows) == 2 and all(k["vgpr_count"] <= 256 and k["private_segment_fixed_size"] == 0 for k in rows)
    bad = [dict(k) for k in kernels]
    for k in bad:
        if "conv_s2_wgrad_kernel<7>" in k["name"]:
            k["vgpr_spill_count"] = 3
    with pytest.raises(RuntimeError, match="register guard failed"):
        b.check_register_resident("conv_bwd_s2.hip", bad)


def test_module_accepts_exactly_the_two_forms(built):
    from offk_amd.off_module import FusionConv2d
    for (key, ci, co, k, _H_) in cs.REAL:
        m = FusionConv2d(ci, co, k, stride=2, padding=cs.FORMS[k])
        assert sorted(m.state_dict()) == ["bias", "weight"], key
        assert m.weight.shape == (co, ci, k, k) and m.bias.shape == (co,)
    for args, kw in (((320, 64, 7), dict(stride=2, padding=2)), ((320, 64, 5), dict(stride=2, padding=3)), ((48, 64, 7), dict(stride=2, padding=3)),
                     ((48, 64, 5), dict(stride=2, padding=2)), ((64, 64, 7), dict(stride=1, padding=3)), ((64, 64, 3), dict(stride=2, padding=1)),
                     ((64, 96, 5), dict(stride=2, padding=2)), ((64, 64, 1), dict(stride=2))):
        with pytest.raises(ValueError):
            FusionConv2d(*args, **kw)
