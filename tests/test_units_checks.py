"""CPU checks of what the GPU tests of the units' training side rest on (tests/units_grad.py, tests/featmaps.py): the bit predicates tell
what they are meant to tell, the row views are the permute + reshape they stand for, exact.down_rows is the row mapping written out, every
entry a row of the dX forms table or of the kinds table names is in the library, the forms' trace names are the library's, and the split dX
inequality rejects a result that lost one product.  Nothing here touches a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, runtime, spec, synth

from . import arena
from . import featmaps as fm
from . import split_bound as sb
from . import units_grad as ug

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    return _lib.load()


INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
NAN_BITS = {torch.float32: 0x7FC00123, torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}


@pytest.mark.parametrize("dtype", list(INT), ids=["fp32", "bf16", "fp16"])
def test_bit_predicates(dtype):
    same = [ug.same_bits_any] + ([arena.same_bits] if dtype == torch.float32 else [ug.same_bits16])
    x = torch.tensor([[1.5, -2.25, 0.0], [3.0, 0.0, -0.5]]).to(dtype)
    for eq in same:
        assert eq(x, x.clone())
        neg = x.clone()
        neg[0, 2] = -0.0
        assert torch.equal(neg, x) and not eq(neg, x)                   # +0 against -0: equal values, other bits
        low = x.clone().view(INT[dtype])
        low[1, 0] ^= 1
        assert not eq(low.view(dtype), x)                               # one flipped low mantissa bit
        nan = x.clone().view(INT[dtype])
        nan[0, 0] = NAN_BITS[dtype]
        nan = nan.view(dtype)
        assert bool(torch.isnan(nan[0, 0])) and not torch.equal(nan, nan.clone()) and eq(nan, nan.clone())      # equal NaN payloads: equal bits
        other = nan.clone().view(INT[dtype])
        other[0, 0] ^= 2
        assert bool(torch.isnan(other.view(dtype)[0, 0])) and not eq(other.view(dtype), nan)
        assert not eq(x, x.reshape(3, 2))
    assert not ug.same_bits_any(x, x.to(torch.float16 if dtype != torch.float16 else torch.bfloat16))
    if dtype != torch.float32:
        assert not ug.same_bits16(x, x.to(torch.float16 if dtype != torch.float16 else torch.bfloat16))


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_row_views(layout):
    t = torch.arange(24, dtype=torch.float32).reshape(2, 3, 2, 2)
    if layout == "cl":
        t = ug.to_cl(t)
        assert not t.is_contiguous() and t.stride() == (12, 1, 6, 3)
    want = t.permute(0, 2, 3, 1).reshape(2, 4, 3)                      # [N, HW, C]
    assert want[1, 2].tolist() == [14.0, 18.0, 22.0]                   # frame 1, pixel (1, 0): channels 0, 1, 2
    assert torch.equal(ug.as_rows(t, layout), want)
    assert torch.equal(ug.rows_of(t), want.reshape(8, 3))
    h = t.to(torch.bfloat16)
    assert torch.equal(ug.rows16(h, layout), want.reshape(8, 3).to(torch.bfloat16))
    wrong = "nchw" if layout == "cl" else "cl"
    with pytest.raises(AssertionError):
        ug.as_rows(t, wrong)
    with pytest.raises(AssertionError):
        ug.rows16(h, wrong)
    assert [ug.to_cl(x).stride() for x in ug.to_cl([t.contiguous()])] == [(12, 1, 6, 3)]


def rows_written_out(B, L, slice_mode):
    """Quirk Q1 spelled out frame by frame: flat slicing takes the FIRST P = B (L - 1) frames of the batch as they lie, whichever clip
    they belong to; per-clip slicing takes the first L - 1 frames of every clip, numbered in the order they come."""
    out, taken = [], 0
    for b in range(B):
        for t in range(L):
            inside = b * L + t < B * (L - 1) if slice_mode == spec.SLICE_FLAT else t < L - 1
            out.append(taken if inside else -1)
            taken += inside
    return out


def test_down_rows_is_the_row_mapping_written_out():
    """tests/exact.py's down_rows is the one definition (tests/test_gpu_feat_grad.py's copy agreed with it on all of these before it was
    deleted): every B <= 5, L <= 9 in both modes, which holds every case of the family's shape tables but (8, 7) per-clip, and that case
    and the full-size one."""
    cases = {(B, L, sm) for B, L, _v, sm in ug.SHAPES} | {(64, 7, spec.SLICE_FLAT)}
    cases |= {(B, L, sm) for B in range(1, 6) for L in range(2, 10) for sm in (spec.SLICE_FLAT, spec.SLICE_PER_CLIP)}
    assert len(cases) == 82
    for B, L, sm in sorted(cases):
        got = ug.down_rows(B, L, sm)
        assert got == rows_written_out(B, L, sm), (B, L, sm)
        assert sorted(r for r in got if r >= 0) == list(range(B * (L - 1)))
    assert ug.down_rows(2, 3, spec.SLICE_FLAT) == [0, 1, 2, 3, -1, -1] and ug.down_rows(2, 3, spec.SLICE_PER_CLIP) == [0, 1, -1, 2, 3, -1]


def test_every_entry_of_the_tables_is_in_the_library(built):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert [f.name for f in ug.DX_FORMS] == ["fp32", "typed", "split"]
    for form in ug.DX_FORMS:
        for name in (form.entry, form.f32_entry):
            assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[form.entry][1]) == (7 if form.takes_dtype else 6)        # the grad_dtype argument, or none
        assert form.named_in(_lib.FEAT_BF16) == form.entry
    assert sorted(fm.KINDS) == ["cl", "typed"]
    for kind in fm.KINDS.values():
        for stem in fm.STEMS + ("offk_forward", "offk_forward_parts", "offk_off_units_fused"):
            assert hasattr(raw, stem + kind.suffix) and kind.entry(built, stem) is getattr(built, stem + kind.suffix), stem + kind.suffix
        assert callable(getattr(runtime, kind.check))
    assert ug.FEAT == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2} and fm.FDT == {"f32": 0, "bf16": 1, "f16": 2}


def test_trace_names_are_the_librarys():
    split = ug.DX_SPLIT.traces
    # the three strings tests/test_gpu_feat_grad_split.py::test_trace_names holds the library to
    assert split[torch.float32, "nchw"] == "units:feature-map gradient (dX, NCHW, split)"
    assert split[torch.bfloat16, "cl"] == "units:feature-map gradient (dX, NHWC, split, bf16)"
    assert split[torch.float16, "nchw"] == "units:feature-map gradient (dX, NCHW, split, fp16)"
    assert ug.DX_FP32.traces[torch.float32, "cl"] == "units:feature-map gradient (dX, NHWC)"
    assert ug.DX_TYPED.traces[torch.float16, "nchw"] == "units:feature-map gradient (dX, NCHW, fp16)"
    api = open(os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "csrc", "offk_api.hip")).read()
    for form in ug.DX_FORMS:
        assert len(form.traces) == 6
        assert all('"%s"' % name in api for name in form.traces.values())


@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
def test_the_split_dx_inequality_rejects_a_lost_product(pattern, signs):
    """The operands of tests/test_feat_grad_split_abi.py (K = 160, worst-case mantissas): split_bound.assert_discriminates on them, and
    units_grad.dx_check_inequality -- the helper the GPU tests call -- passes the emulation and raises on each of the six lost products."""
    rows, C, K = 96, 64, 160
    a = synth.make_adversarial((rows, K), pattern, "same", seed=3, relu=(pattern == 0x7FFFFF))
    w = synth.make_adversarial((C, K), pattern, signs, seed=4) * np.float32(2.0 ** -4)
    ref, dropped, mag = synth.split_terms(w, a)
    emulate = lambda skip: synth.emulate_split_dot(w, a, form="units", skip=skip)  # noqa: E731
    sb.assert_discriminates("split dX 0x%06X %s" % (pattern, signs), emulate, ref, dropped, mag)
    c_emu, c_same = ug.dx_check_inequality("emulation", emulate(None), a, w)
    assert c_emu == c_same
    for skip in range(len(synth.SPLIT_PRODUCTS)):
        with pytest.raises(AssertionError, match="misses the limit"):
            ug.dx_check_inequality("lost product %d" % skip, emulate(skip), a, w)
