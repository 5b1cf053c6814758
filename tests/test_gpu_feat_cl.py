"""torch.channels_last feature maps on split-fp32 handles (offk_forward_cl, offk_forward_parts_cl, offk_off_units_fused_cl;
csrc/pw_tdiff_cl.hip).  The contract is equality, not a tolerance: for finite maps everything the channels-last path computes is
torch.equal to what the same handle computes from the contiguous (NCHW) copy of the same logical tensor (include/offk.h)."""
import ctypes

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from .featmaps import (  # noqa: F401
    bit_maps, bit_maps32, heavy_maps, relu_maps, rt, unit_regions, make_handle)

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FDT = {"f32": _lib.FEAT_F32, "bf16": _lib.FEAT_BF16, "f16": _lib.FEAT_F16}
RTOL = 2e-4                                            # tests/test_gpu_parity.py's, of the tensor's max magnitude


def to_cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def to_nchw(x):
    return x.contiguous()


def units_equal(h, x):
    """off_units_fused on the channels_last copies == off_units_fused on the contiguous copies, every region finite."""
    xn, xc = [to_nchw(t) for t in x], [to_cl(t) for t in x]
    assert all(t.is_contiguous() for t in xn)
    assert all(c.shape == t.shape and not c.is_contiguous() and c.is_contiguous(memory_format=torch.channels_last) for c, t in zip(xc, xn))
    assert h.takes_channels_last(xc) and not h.takes_channels_last(xn)
    h.workspace.fill_(0xff)                            # (NaN in every float: what the units leave unwritten shows)
    h.off_units_fused(xn)
    ref = unit_regions(h)
    h.workspace.fill_(0xff)
    h.off_units_fused(xc)
    got = unit_regions(h)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(a, b)


def split_parts(x, i):
    """Channel groups of map i in concat order (multiples of 32; 1 .. 4 groups by site), each channels_last on its own."""
    C = x.shape[1]
    cuts = [[C], [C // 2 // 32 * 32, C], [64, 128, C], [32, 96, 224, C]][i % 4]
    parts, a = [], 0
    for b in cuts:
        parts.append(to_cl(x[:, a:b]))
        a = b
    return parts


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
    B, L = 3, 7
    h = make_handle(rt, B, L)
    xc = [to_cl(t) for t in relu_maps(B, L, DTYPES[name], 21)]
    arr = h._feat_array(xc, rt._check_dev_cl)
    out = [torch.empty(h.out_rows(), spec.NUM_CLASSES, device="cuda") for _ in range(3)]

    def launch():
        _lib.check(h.lib.offk_forward_cl(h._h, rt._stream(h.device), FDT[name], arr, *[ctypes.c_void_p(o.data_ptr()) for o in out],
                                         ctypes.c_void_p(h.workspace.data_ptr())), h._h)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [o.clone() for o in out]
    assert all(torch.isfinite(o).all() for o in eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, out))
    again = h.forward(xc)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))


# ---- 6. what is refused, before any launch ----

def _raw_call(h, rt, fdt, xs):
    """offk_forward_cl straight through ctypes (no Python-side checks); returns (rc, message)."""
    arr = (ctypes.c_void_p * spec.NUM_SITES)(*[x.data_ptr() for x in xs])
    out = [torch.empty(h.out_rows(), spec.NUM_CLASSES, device="cuda") for _ in range(3)]
    rc = h.lib.offk_forward_cl(h._h, rt._stream(h.device), fdt, arr, *[ctypes.c_void_p(o.data_ptr()) for o in out],
                               ctypes.c_void_p(h.workspace.data_ptr()))
    return rc, h.lib.offk_last_error(h._h).decode()


def _assert_refused(h, rt, fdt, xs, needle):
    h.workspace.fill_(0x5a)
    torch.cuda.synchronize()
    rc, msg = _raw_call(h, rt, fdt, xs)
    torch.cuda.synchronize()
    assert rc == -1 and needle in msg, (rc, msg)
    assert bool((h.workspace == 0x5a).all())              # nothing was enqueued


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
    B, L = 2, 3
    x = relu_maps(B, L, DTYPES[name], 5)
    x[0][1, 7, 3, 4] = float("inf")                    # site 3a, frame 1 (clip 0), pixel (3, 4)
    x[8][2, 100, 5, 6] = float("nan")                  # site 5b, frame 2 (clip 0), pixel (5, 6)
    h = make_handle(rt, B, L)
    h.off_units_fused([to_cl(t) for t in x])
    torch.cuda.synchronize()
    P = h.P
    D3a = h.region("D_3a", 32).view(P, 28, 28, 32)
    D5b = h.region("D_5b", 32).view(P, 7, 7, 32)
    assert not torch.isfinite(D3a[1, 3, 4]).any() and not torch.isfinite(D5b[2, 5, 6]).any()
    m3 = torch.ones(P, 28, 28, dtype=torch.bool, device="cuda")
    m3[1, 3, 4] = False
    m5 = torch.ones(P, 7, 7, dtype=torch.bool, device="cuda")
    m5[2, 5, 6] = False
    assert torch.isfinite(D3a[m3]).all() and torch.isfinite(D5b[m5]).all()
