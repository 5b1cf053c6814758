"""16-bit feature maps on split-fp32 handles (offk_forward_typed, offk_forward_parts_typed, offk_off_units_fused_typed;
csrc/pw_tdiff_f16.hip).  The contract is equality, not a tolerance: for finite maps everything the 16-bit path computes is
torch.equal to what the same handle computes from the maps upcast to fp32 (include/offk.h)."""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from . import featmaps as fm
from .featmaps import (  # noqa: F401
    bit_maps, heavy_maps, relu_maps, rt, make_handle)

pytestmark = pytest.mark.gpu

KIND = fm.KINDS["typed"]
DTYPES = KIND.dtypes


def units_equal(h, x16):
    fm.units_equal(h, KIND, x16)


def split_parts(x, i):
    return fm.split_parts(KIND, x, i)


# ---- 1. the units stage ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("slice_mode", [spec.SLICE_FLAT, spec.SLICE_PER_CLIP])
@pytest.mark.parametrize("B,L", [(1, 2), (3, 3), (2, 9), (5, 7), (3, 7)])
def test_units_stage_equals_fp32_maps(rt, name, slice_mode, B, L):
    """fusion_* unit channels and D_<site> after off_units_fused(x16) == after off_units_fused(x16.float()): short clips, two temporal
    groups (L = 9), odd batches (pixel pairs and the 7x7 stream across clip boundaries); flat slicing at (3, 7) puts quirk Q1's
    down rows across clips."""
    h = make_handle(rt, B, L, slice_mode=slice_mode)
    units_equal(h, relu_maps(B, L, DTYPES[name], 11 * B + L))


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("kind", ["full_mantissa", "random_bits", "heavy_tail"])
def test_units_stage_input_kinds(rt, name, kind):
    """Every mantissa bit set, random bit patterns (negative values, subnormals of the 16-bit type, exponents over 37 octaves), a heavy tail."""
    B, L = 3, 4
    dt = DTYPES[name]
    x = heavy_maps(B, L, dt, 3) if kind == "heavy_tail" else bit_maps(B, L, dt, 4, full_mantissa=kind == "full_mantissa")
    h = make_handle(rt, B, L)
    units_equal(h, x)


@pytest.mark.parametrize("name", list(DTYPES))
def test_units_stage_subnormal_maps(rt, name):
    """Maps of subnormals only (bf16: 2^-133 .. 2^-126; fp16: 2^-24 .. 2^-14): the accumulators themselves end up fp32 subnormals,
    so the MFMAs the 16-bit kernel drops (all products +-0) are shown to leave such an accumulator as it is."""
    B, L = 2, 3
    dt = DTYPES[name]
    g = torch.Generator(device="cuda").manual_seed(9)
    x = []
    for _, C, H in spec.SITES:
        n = B * L * C * H * H
        r = torch.randint(0, 1 << 20, (n,), device="cuda", generator=g, dtype=torch.int64)
        bits = ((r & 1) << 15) | ((r >> 1) & (0x3ff if dt == torch.float16 else 0x7f))
        bits = torch.where(bits >= 1 << 15, bits - (1 << 16), bits)
        x.append(bits.to(torch.int16).view(dt).view(B * L, C, H, H).contiguous())
    h = make_handle(rt, B, L)
    units_equal(h, x)


# ---- 2. the whole forward ----

@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("B,L,variant,consensus,parts", [(64, 7, spec.VARIANT_RGB, False, False), (64, 7, spec.VARIANT_FLOW, True, True),
                                                         (10, 25, spec.VARIANT_RGB, True, True), (10, 25, spec.VARIANT_FLOW, False, False)])
def test_forward_equals_fp32_maps(rt, name, B, L, variant, consensus, parts):
    h = make_handle(rt, B, L, variant, consensus=consensus)
    x16 = relu_maps(B, L, DTYPES[name], 7)
    ref = h.forward([x.float() for x in x16])
    got = h.forward([split_parts(x, i) for i, x in enumerate(x16)] if parts else x16)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and torch.isfinite(a).all()
        assert torch.equal(a, b)


# ---- 4. the oracle anchor ----

def test_forward_f16_against_oracle(rt):
    from oracle import off_oracle as orc
    B, L = 2, 3
    w = synth.make_weights(spec.VARIANT_RGB)
    x16 = [torch.from_numpy(f).cuda().half().contiguous() for f in synth.make_features(B, L, 9)]
    h = rt.OffForward(B, L, spec.VARIANT_RGB, precision="f32split")
    h.load_state_dict(w)
    out = h.forward(x16)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = orc.off_forward([x.float().cpu() for x in x16], orc.to_torch_weights(w), B, L, spec.VARIANT_RGB)
    for o, r in zip(out, ref):
        err = (o.cpu().double() - r.double()).abs().max().item() / r.double().abs().max().item()
        assert err < 1e-3, err


# ---- 5. capture and determinism ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_forward_typed_capture_and_determinism(rt, name):
    fm.forward_capture_and_determinism(rt, KIND, name)


# ---- 6. what is refused, before any launch ----

def _assert_refused(h, rt, fdt, x16, needle):
    fm.assert_forward_refused(h, rt, KIND, fdt, x16, needle)


def test_refusals(rt, monkeypatch):
    B, L = 2, 3
    x16 = relu_maps(B, L, torch.bfloat16, 1)
    # unknown dtype
    _assert_refused(make_handle(rt, B, L), rt, 7, x16, "unknown feat_dtype")
    # fp32-pipe handle: in C, and in Python with a message naming precision="f32split"
    h32 = make_handle(rt, B, L, precision="fp32")
    _assert_refused(h32, rt, _lib.FEAT_BF16, x16, "OFFK_PRECISION_F32SPLIT")
    with pytest.raises(ValueError, match="f32split"):
        h32.forward(x16)
    # NHWC handle
    _assert_refused(make_handle(rt, B, L, feat_layout=1), rt, _lib.FEAT_BF16, x16, "NCHW")
    # OFFK_FUSED_UNITS=0
    monkeypatch.setenv("OFFK_FUSED_UNITS", "0")
    hu = make_handle(rt, B, L)
    monkeypatch.delenv("OFFK_FUSED_UNITS")
    _assert_refused(hu, rt, _lib.FEAT_F16, [x.half() for x in x16], "OFFK_FUSED_UNITS")
    # a bound gen weight
    hb = make_handle(rt, B, L)
    wg = torch.from_numpy(synth.make_weights(spec.VARIANT_RGB)["motion_conv_gen_3a.weight"]).cuda().contiguous()
    hb.bind_weight("motion_conv_gen_3a.weight", wg)
    _assert_refused(hb, rt, _lib.FEAT_BF16, x16, "offk_bind_weight")
    # a pointer one element off alignment
    h = make_handle(rt, B, L)
    bad = list(x16)
    s = x16[4]
    buf = torch.empty(s.numel() + 1, dtype=s.dtype, device="cuda")
    bad[4] = buf[1:].view(s.shape)
    bad[4].copy_(s)
    _assert_refused(h, rt, _lib.FEAT_BF16, bad, "4-byte aligned")
    # mixed dtypes, and the module at its fp32 default
    with pytest.raises(ValueError, match="one dtype"):
        h.forward(x16[:8] + [x16[8].half()])
    from offk_amd.off_module import OFFSubNetwork
    m = OFFSubNetwork(spec.NUM_CLASSES, B, L, "rgb").cuda()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(spec.VARIANT_RGB).items()})
    with pytest.raises(ValueError, match="f32split"):
        m(x16)


# ---- 7. non-finite maps ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_nonfinite_maps(rt, name):
    """Inf / NaN in a 16-bit map: every D row it touches is non-finite in all 32 channels; every other unit output stays finite."""
    fm.nonfinite_maps(rt, KIND, name)


# ---- 8. the modules under torch.autocast ----

@pytest.mark.parametrize("name", list(DTYPES))
def test_bninception_off_under_autocast(rt, name):
    from offk_amd.off_module import BNInception_OFF
    B, L = 2, 3
    torch.manual_seed(0)
    bb = fm.ToyBackbone(score=True).cuda()
    model = BNInception_OFF(num_classes=spec.NUM_CLASSES, batch=B, length=L, variant="rgb", backbone=bb, precision="f32split").cuda()
    model.off.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(spec.VARIANT_RGB).items()})
    x = torch.randn(B * L, 3, 28, 28, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=DTYPES[name]):
        feats, _ = bb(x)
        assert all(f.dtype == DTYPES[name] for f in feats)
        fc7, _fgs, fc14 = model(x)
    with torch.no_grad():
        r7, r14, _ = model.off([f.float() for f in feats], want28=False)
    torch.cuda.synchronize()
    assert fc7.dtype == torch.float32
    assert torch.equal(fc7, model._squeeze(r7)) and torch.equal(fc14, model._squeeze(r14))
