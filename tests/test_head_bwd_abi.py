"""CPU-side checks of the heads' training entries (include/offk.h, K5t / K5b): the three symbols exist and are bound, the plan is a pure
function of its three integers, every refusal comes back OFFK_ERR_INVALID with the entry's name before any HIP call (the pointers are
fakes that are never dereferenced, as in tests/test_conv_bwd_abi.py), MotionHead refuses what it cannot run, and
synth.head_dropout_keep is the documented integer function."""
import ctypes

import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import _lib, synth

ENTRIES = ("offk_head_train", "offk_head_backward", "offk_head_backward_plan")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


def _fake(addr):
    return ctypes.c_void_p(addr)


def _plan(lib, n, c, ncls):
    s, ch = ctypes.c_size_t(0), ctypes.c_int(0)
    rc = lib.offk_head_backward_plan(n, c, ncls, ctypes.byref(s), ctypes.byref(ch))
    return rc, s.value, ch.value


def test_symbols_are_exported_and_bound(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        assert tuple(getattr(built, name).argtypes) == tuple(_lib.SIGNATURES[name][1])
    assert built.offk_abi_version() == 10


@pytest.mark.parametrize("n_img", [1, 6, 384])
@pytest.mark.parametrize("C", [256, 512, 1024])
def test_plan_is_a_pure_function(built, C, n_img):
    first = _plan(built, n_img, C, 101)
    assert first[0] == 0, built.offk_last_error(None)
    chunks = first[2]
    assert 1 <= chunks <= n_img                                   # chunks are whole images
    assert first[1] >= 4 * chunks * (101 * C + 101)               # the slabs [chunk][classes][C] and [chunk][classes]
    ipc = -(-n_img // chunks)
    assert (chunks - 1) * ipc < n_img                             # no empty chunk
    for _ in range(3):
        assert _plan(built, n_img, C, 101) == first
    # a function of the three integers: other classes and channels change the bytes, not the chunks
    assert _plan(built, n_img, C, 7)[2] == chunks


def test_plan_runs_from_python_wrapper_and_has_a_short_last_chunk(built):
    from offk_amd import runtime
    assert runtime.head_backward_plan(6, 512, 101) == _plan(built, 6, 512, 101)[1:]
    # the smallest n_img whose plan has >= 3 chunks with a shorter last one is 34 (tests/test_gpu_head_bwd_exact.py runs it)
    found = None
    for n in range(1, 200):
        chunks = runtime.head_backward_plan(n, 64, 7)[1]
        if chunks >= 3 and n % (-(-n // chunks)) != 0:
            found = n
            break
    assert found == 34, found


_N, _H, _C, _CLS = 2, 7, 512, 101
_X, _DX, _G, _Z = 0x10000000, 0x20000000, 0x30000000, 0x40000000
_X_BYTES = _N * _H * _H * _C * 4
_BIG = 1 << 30


def _train_args(**over):
    a = dict(stream=None, x=_fake(_X), x_cstride=_C, x_coff=0, n_img=_N, H=_H, W=_H, C=_C, maxpool=0, fc_w=_fake(0x1000), fc_b=_fake(0x2000),
             num_classes=_CLS, head_index=1, drop_seed=7, drop_p=0.8, z=_fake(_Z), out=_fake(0x50000000))
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def _bwd_args(**over):
    a = dict(stream=None, g=_fake(_G), x=_fake(_X), x_cstride=_C, x_coff=0, n_img=_N, H=_H, W=_H, C=_C, maxpool=0, fc_w=_fake(0x1000),
             num_classes=_CLS, z=_fake(_Z), head_index=1, drop_seed=7, drop_p=0.8, dx=_fake(_DX), dx_cstride=_C, dx_coff=0, accumulate_dx=0,
             dw=_fake(0x3000), db=_fake(0x4000), accumulate_w=0, scratch=_fake(0x60000000), scratch_bytes=_BIG)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def _plan_args(n=2, c=512, ncls=101):
    return [n, c, ncls, None, None]


_T, _B, _P = ENTRIES
_REFUSALS = {
    "train_null_x": (_T, _train_args, dict(x=None)),
    "train_null_w": (_T, _train_args, dict(fc_w=None)),
    "train_null_b": (_T, _train_args, dict(fc_b=None)),
    "train_null_z": (_T, _train_args, dict(z=None)),
    "train_null_out": (_T, _train_args, dict(out=None)),
    "train_c_mod_4": (_T, _train_args, dict(C=510)),
    "train_c_too_large": (_T, _train_args, dict(C=1028, x_cstride=1028)),
    "train_c_too_small": (_T, _train_args, dict(C=0)),
    "train_odd_stride": (_T, _train_args, dict(x_cstride=_C + 2)),
    "train_odd_offset": (_T, _train_args, dict(x_cstride=_C + 6, x_coff=2)),
    "train_negative_offset": (_T, _train_args, dict(x_coff=-4, x_cstride=1024)),
    "train_stride_short": (_T, _train_args, dict(x_cstride=_C, x_coff=64)),
    "train_maxpool_h2": (_T, _train_args, dict(maxpool=1, H=2)),
    "train_maxpool_w2": (_T, _train_args, dict(maxpool=1, W=2)),
    "train_drop_p_1": (_T, _train_args, dict(drop_p=1.0)),
    "train_drop_p_negative": (_T, _train_args, dict(drop_p=-0.1)),
    "train_drop_p_nan": (_T, _train_args, dict(drop_p=float("nan"))),
    "train_no_images": (_T, _train_args, dict(n_img=0)),
    "train_no_classes": (_T, _train_args, dict(num_classes=0)),
    "train_head_index": (_T, _train_args, dict(head_index=-1)),
    "bwd_null_g": (_B, _bwd_args, dict(g=None)),
    "bwd_null_x": (_B, _bwd_args, dict(x=None)),
    "bwd_null_w": (_B, _bwd_args, dict(fc_w=None)),
    "bwd_null_z": (_B, _bwd_args, dict(z=None)),
    "bwd_null_scratch": (_B, _bwd_args, dict(scratch=None)),
    "bwd_null_scratch_db_only": (_B, _bwd_args, dict(scratch=None, dx=None, dw=None)),
    "bwd_c_mod_4": (_B, _bwd_args, dict(C=510)),
    "bwd_c_too_large": (_B, _bwd_args, dict(C=1028, x_cstride=1028, dx_cstride=1028)),
    "bwd_odd_x_stride": (_B, _bwd_args, dict(x_cstride=_C + 2)),
    "bwd_odd_dx_offset": (_B, _bwd_args, dict(dx_cstride=_C + 6, dx_coff=2)),
    "bwd_negative_dx_offset": (_B, _bwd_args, dict(dx_coff=-4, dx_cstride=1024)),
    "bwd_x_stride_short": (_B, _bwd_args, dict(x_cstride=_C, x_coff=64)),
    "bwd_dx_stride_short": (_B, _bwd_args, dict(dx_cstride=256)),
    "bwd_maxpool_h2": (_B, _bwd_args, dict(maxpool=1, H=2)),
    "bwd_drop_p_1": (_B, _bwd_args, dict(drop_p=1.0)),
    "bwd_short_scratch": (_B, _bwd_args, dict(scratch_bytes=4 * (_CLS * _C + _CLS) - 4)),
    "bwd_short_scratch_db_only": (_B, _bwd_args, dict(scratch_bytes=0, dx=None, dw=None)),
    "bwd_dx_is_x": (_B, _bwd_args, dict(dx=_fake(_X))),
    "bwd_dx_overlaps_x_tail": (_B, _bwd_args, dict(dx=_fake(_X + _X_BYTES - 1024))),
    "bwd_dx_other_slice_of_x_buffer": (_B, _bwd_args, dict(x_cstride=1024, dx=_fake(_X), dx_cstride=1024, dx_coff=512)),
    "bwd_dx_overlaps_g": (_B, _bwd_args, dict(g=_fake(_DX + 4096))),
    "bwd_g_tail_inside_dx": (_B, _bwd_args, dict(g=_fake(_DX - 16))),
    "plan_c_mod_4": (_P, _plan_args, dict(c=510)),
    "plan_c_too_large": (_P, _plan_args, dict(c=1028)),
    "plan_no_images": (_P, _plan_args, dict(n=0)),
    "plan_no_classes": (_P, _plan_args, dict(ncls=0)),
}


@pytest.mark.parametrize("rule", sorted(_REFUSALS))
def test_refusals_name_the_entry(built, rule):
    entry, make, over = _REFUSALS[rule]
    rc = getattr(built, entry)(*make(**over))
    assert rc == -1, (rule, rc, built.offk_last_error(None))
    assert entry.encode() in built.offk_last_error(None), built.offk_last_error(None)


def test_the_unmodified_arguments_are_not_refused_for_their_shape(built):
    """the refusal table's base arguments are valid: the same backward call with only a short scratch is refused for the scratch, nothing
    else, with max-pool and a middle slice too (the train entry has no refusal that comes last: its base call would launch)"""
    for over in (dict(), dict(maxpool=1), dict(x_cstride=1024, x_coff=256, dx_cstride=768, dx_coff=128), dict(drop_p=0.0), dict(head_index=2)):
        rc = built.offk_head_backward(*_bwd_args(scratch_bytes=0, **over))
        assert rc == -1 and b"scratch too small" in built.offk_last_error(None), (over, built.offk_last_error(None))
    assert built.offk_head_backward_plan(*_plan_args()) == 0


def test_motion_head_construction_errors(built):
    import torch
    from offk_amd.off_module import MotionHead
    m = MotionHead(256, maxpool=True, head_index=0)
    assert sorted(m.state_dict()) == ["bias", "weight"] and m.weight.shape == (101, 256) and m.bias.shape == (101,)
    assert isinstance(m, torch.nn.Linear) and m.drop_p == 0.8
    for args, kw in (((0,), {}), ((510,), {}), ((1028,), {}), ((2,), {}), ((256,), dict(drop_p=1.0)), ((256,), dict(drop_p=-0.5)),
                     ((256,), dict(dtype=torch.float64)), ((256,), dict(dtype=torch.bfloat16)), ((256,), dict(head_index=-1)),
                     ((256,), dict(bias=False))):
        with pytest.raises(ValueError):
            MotionHead(*args, **kw)


# ---- the mask ---------------------------------------------------------------------------------------------------------------------
_MASK64 = (1 << 64) - 1


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def _keep_literal(seed, head_index, n, c, C, p):
    """splitmix64 in Python integers: stream (seed, 16 + head_index), draw n * (C / 4) + c / 4, field c % 4"""
    gold = 0x9E3779B97F4A7C15
    stream = ((seed & 0xFFFFFFFFFFFF) << 8) | (16 + head_index)
    base = _mix((stream * gold + gold) & _MASK64)
    q = n * (C // 4) + c // 4
    u = _mix((base + (q + 1) * gold) & _MASK64)
    return ((u >> (16 * (c % 4))) & 0xFFFF) >= int(round(p * 65536))


def test_head_dropout_keep_is_the_documented_integer_function():
    for seed, hi, N, C, p in ((1, 0, 3, 256, 0.8), (0xDEADBEEF1234, 2, 5, 1024, 0.5), (77, 1, 2, 64, 0.75)):
        keep = synth.head_dropout_keep(seed, hi, N, C, p)
        assert keep.shape == (N, C) and keep.dtype == bool
        for n, c in ((0, 0), (0, 1), (0, 3), (0, 4), (N - 1, C - 1), (N - 1, C // 2 + 2), (1, 7)):
            assert bool(keep[n, c]) == _keep_literal(seed, hi, n, c, C, p), (seed, hi, n, c)
    # the heads' streams differ from one another and from the units' stream of the same seed
    a, b = synth.head_dropout_keep(5, 0, 4, 256, 0.5), synth.head_dropout_keep(5, 1, 4, 256, 0.5)
    assert (a != b).any()
    assert synth.head_dropout_keep(5, 0, 4, 256, 0.0).all()


def test_head_dropout_keep_rate():
    """p = 0.8 over 10^5 draws (100 images x 1000 channels): the keep rate lies within four binomial standard deviations of 1 - p, which the
    16-bit threshold realises as 1 - 52429 / 65536 (0.19999695: 3e-6 from 0.2, against a standard deviation of 1.26e-3)"""
    keep = synth.head_dropout_keep(2024, 2, 100, 1000, 0.8)
    n = keep.size
    assert n == 100000
    sd = (0.2 * 0.8 / n) ** 0.5
    assert abs(keep.mean() - 0.2) <= 4 * sd, (keep.mean(), sd)
    per_image = keep.mean(axis=1)                                 # 1000 draws each: sd 1.26e-2; no image is all kept or all dropped
    assert np.all(np.abs(per_image - 0.2) <= 5 * (0.2 * 0.8 / 1000) ** 0.5), per_image
