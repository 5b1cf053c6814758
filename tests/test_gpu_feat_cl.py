"""torch.channels_last feature maps on split-fp32 handles (offk_forward_cl, offk_forward_parts_cl, offk_off_units_fused_cl;
csrc/pw_tdiff_cl.hip).  The contract is equality, not a tolerance: for finite maps everything the channels-last path computes is
torch.equal to what the same handle computes from the contiguous (NCHW) copy of the same logical tensor (include/offk.h)."""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from . import featmaps as fm
from .featmaps import (  # noqa: F401
    bit_maps, bit_maps32, heavy_maps, relu_maps, rt, to_cl, make_handle)

pytestmark = pytest.mark.gpu

KIND = fm.KINDS["cl"]
DTYPES = KIND.dtypes
RTOL = 2e-4                                            # tests/test_gpu_parity.py's, of the tensor's max magnitude


def to_nchw(x):
    return x.contiguous()


def units_equal(h, x):
    fm.units_equal(h, KIND, x)


def split_parts(x, i):
    return fm.split_parts(KIND, x, i)


# ---- 1. the units stage ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("slice_mode", [spec.SLICE_FLAT, spec.SLICE_PER_CLIP])
@pytest.mark.parametrize("B,L", [(1, 2), (3, 3), (2, 9), (3, 7)])
def test_units_stage_equals_nchw_maps(rt, name, slice_mode, B, L):
    """fusion_* unit channels and D_<site> after off_units_fused(to_cl(x)) == after off_units_fused(to_nchw(x)): one pair; odd
    batches (the 32-pixel stream crosses clip boundaries at every site and ends in a partial block: 3 * 49, 3 * 196 and 3 * 784 are
    not all multiples of 32); two temporal groups (L = 9); flat slicing at (3, 7) puts quirk Q1's down rows across clips."""
    h = make_handle(rt, B, L, slice_mode=slice_mode)
    units_equal(h, relu_maps(B, L, DTYPES[name], 11 * B + L))


# ---- 2. input kinds ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("kind", ["full_mantissa", "random_bits", "heavy_tail"])
def test_units_stage_input_kinds(rt, name, kind):
    """Every mantissa bit set, random bit patterns (negative values, subnormals, exponents over 60 (fp32) / 37 (bf16) / 25 (fp16)
    octaves; fp32: a share of values below 2^-109), a heavy tail."""
    B, L = 3, 4
    dt = DTYPES[name]
    if kind == "heavy_tail":
        x = heavy_maps(B, L, dt, 3)
    elif dt == torch.float32:
        x = bit_maps32(B, L, 4, full_mantissa=kind == "full_mantissa")
    else:
        x = bit_maps(B, L, dt, 4, full_mantissa=kind == "full_mantissa")
    assert all(torch.isfinite(t).all() for t in x)
    h = make_handle(rt, B, L)
    units_equal(h, x)


# ---- 3. the whole forward ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("variant,consensus,parts", [(spec.VARIANT_RGB, False, False), (spec.VARIANT_RGB, True, True),
                                                     (spec.VARIANT_FLOW, False, True), (spec.VARIANT_FLOW, True, False)])
def test_forward_equals_nchw_maps(rt, name, variant, consensus, parts):
    """The three heads of forward(channels_last maps) == forward(their contiguous copies); parts: every map as its channel groups,
    each group a channels_last tensor of its own (offk_forward_parts_cl)."""
    B, L = 2, 3
    h = make_handle(rt, B, L, variant, consensus=consensus)
    x = relu_maps(B, L, DTYPES[name], 7)
    ref = h.forward([to_nchw(t) for t in x])
    got = h.forward([split_parts(t, i) for i, t in enumerate(x)] if parts else [to_cl(t) for t in x])
    torch.cuda.synchronize()
    assert len(got) == 3 and len(ref) == 3
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and torch.isfinite(a).all()
        assert torch.equal(a, b)


def test_forward_cl_against_oracle(rt):
    """An anchor that does not go through the NCHW kernels: channels_last fp16 maps against the CPU oracle on the same values."""
    from oracle import off_oracle as orc
    B, L = 2, 3
    w = synth.make_weights(spec.VARIANT_RGB)
    x16 = [to_cl(torch.from_numpy(f).cuda().half()) for f in synth.make_features(B, L, 9)]
    h = rt.OffForward(B, L, spec.VARIANT_RGB, precision="f32split")
    h.load_state_dict(w)
    assert h.takes_channels_last(x16)
    out = h.forward(x16)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = orc.off_forward([t.float().cpu().contiguous() for t in x16], orc.to_torch_weights(w), B, L, spec.VARIANT_RGB)
    for o, r in zip(out, ref):
        err = (o.cpu().double() - r.double()).abs().max().item() / r.double().abs().max().item()
        assert err < RTOL, err


# ---- 4. the mirror class ----

def test_off_subnetwork_takes_channels_last_maps(rt):
    from offk_amd.off_module import OFFSubNetwork
    B, L = 2, 3
    m = OFFSubNetwork(spec.NUM_CLASSES, B, L, "rgb", precision="f32split").cuda()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(spec.VARIANT_RGB).items()})
    x = relu_maps(B, L, torch.float16, 13)
    ref = m([to_nchw(t) for t in x])
    xc = [to_cl(t) for t in x]
    seen = []
    real = m._rt._forward_cl
    m._rt._forward_cl = lambda feats, want28: (seen.append([f.data_ptr() for f in feats]), real(feats, want28))[1]
    got = m(xc)
    torch.cuda.synchronize()
    assert seen == [[t.data_ptr() for t in xc]]                      # handed over as they are: no copy, no cast
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and torch.isfinite(a).all()
        assert torch.equal(a, b)


# ---- 5. capture and determinism ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_forward_cl_capture_and_determinism(rt, name):
    fm.forward_capture_and_determinism(rt, KIND, name)


# ---- 6. what is refused, before any launch ----

def _assert_refused(h, rt, fdt, xs, needle):
    fm.assert_forward_refused(h, rt, KIND, fdt, xs, needle)


def test_refusals(rt, monkeypatch):
    B, L = 2, 3
    x = relu_maps(B, L, torch.float32, 1)
    xc = [to_cl(t) for t in x]
    # unknown dtype
    _assert_refused(make_handle(rt, B, L), rt, 7, xc, "unknown feat_dtype")
    # fp32-pipe handle: in C, and in Python with a message naming precision="f32split"
    h32 = make_handle(rt, B, L, precision="fp32")
    _assert_refused(h32, rt, _lib.FEAT_F32, xc, "OFFK_PRECISION_F32SPLIT")
    with pytest.raises(ValueError, match="f32split"):
        h32.forward(xc)
    with pytest.raises(ValueError, match="f32split"):
        h32.off_units_fused(xc)
    # OFFK_FUSED_UNITS=0
    monkeypatch.setenv("OFFK_FUSED_UNITS", "0")
    hu = make_handle(rt, B, L)
    monkeypatch.delenv("OFFK_FUSED_UNITS")
    _assert_refused(hu, rt, _lib.FEAT_F32, xc, "OFFK_FUSED_UNITS")
    # a bound gen weight
    hb = make_handle(rt, B, L)
    wg = torch.from_numpy(synth.make_weights(spec.VARIANT_RGB)["motion_conv_gen_3a.weight"]).cuda().contiguous()
    hb.bind_weight("motion_conv_gen_3a.weight", wg)
    _assert_refused(hb, rt, _lib.FEAT_F32, xc, "offk_bind_weight")
    # a pointer 4 bytes off 16-byte alignment
    h = make_handle(rt, B, L)
    bad = list(xc)
    s = xc[4]
    buf = torch.empty(s.numel() + 1, dtype=s.dtype, device="cuda")
    bad[4] = buf[1:].view(s.shape[0], s.shape[2], s.shape[3], s.shape[1]).permute(0, 3, 1, 2)
    bad[4].copy_(s)
    assert bad[4].is_contiguous(memory_format=torch.channels_last) and bad[4].data_ptr() % 16 == 4
    _assert_refused(h, rt, _lib.FEAT_F32, bad, "16-byte aligned")
    # in Python: mixed layouts
    with pytest.raises(ValueError, match="one layout"):
        h.forward(xc[:8] + [x[8]])
    with pytest.raises(ValueError, match="one layout"):
        h.off_units_fused([x[0]] + xc[1:])


# ---- 7. non-finite maps ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_nonfinite_maps(rt, name):
    """Inf / NaN in a channels_last map: every D row it touches is non-finite in all 32 channels; every other unit output stays finite."""
    fm.nonfinite_maps(rt, KIND, name)
