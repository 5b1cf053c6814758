"""Helpers the GPU tests of the feature-map kinds share (tests/test_gpu_feat16.py, test_gpu_feat_cl.py, test_gpu_feat16_train.py,
test_gpu_feat_cl_train.py, test_gpu_bounds.py): the `rt` fixture, handles, the map generators, what the units' calls write, and the
backward's inputs.  A helper module like tests/arena.py: no tests of its own.  The generators draw on the device from a seeded
generator; a test's inputs are a function of (generator, B, L, dtype, seed) alone."""
import functools

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPES16 = {"bf16": torch.bfloat16, "f16": torch.float16}
DROP_SEED, DROP_P = 7, 0.8


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def make_handle(rt, B, L, variant=spec.VARIANT_RGB, slice_mode=spec.SLICE_FLAT, consensus=None, precision="f32split", **kw):
    h = rt.OffForward(B, L, variant, slice_mode, consensus, precision=precision, **kw)
    assert h.load_state_dict(synth.make_weights(variant)) == []
    return h


def make_train_handle(rt, B, L, variant=spec.VARIANT_RGB, slice_mode=spec.SLICE_FLAT, precision="fp32", **kw):
    h = rt.OffForward(B, L, variant, slice_mode, precision=precision, training=True, **kw)
    assert h.load_state_dict(synth.make_weights(variant)) == []
    return h


# ---- inputs ----

def relu_maps(B, L, dtype, seed):
    """ReLU-like synthetic maps, made on the device and rounded to `dtype`."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.relu(torch.randn(B * L, C, H, H, device="cuda", generator=g)).to(dtype).contiguous() for _, C, H in spec.SITES]


def bit_maps(B, L, dtype, seed, full_mantissa=False):
    """Random finite bit patterns: both signs, every mantissa bit in play (or all set), exponents from the subnormals
    (exponent field 0) up to 2^10.  fp32: bf16's sign / exponent / upper mantissa with sixteen more mantissa bits below."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for _, C, H in spec.SITES:
        n = B * L * C * H * H
        r = torch.randint(0, 1 << 30, (n,), device="cuda", generator=g, dtype=torch.int64)
        sign = (r & 1) << 15
        if dtype == torch.float16:
            mant = torch.full_like(r, 0x3ff) if full_mantissa else (r >> 1) & 0x3ff
            e = (r >> 11) % 26                                        # 0 (subnormal) .. 25 (2^10)
            bits = sign | (e << 10) | mant
        else:
            mant = torch.full_like(r, 0x7f) if full_mantissa else (r >> 1) & 0x7f
            e = (r >> 11) % 38
            e = torch.where(e == 0, e, e + 100)                       # 0 (subnormal) or 101 .. 137
            bits = sign | (e << 7) | mant
        if dtype == torch.float32:
            low = torch.full_like(r, 0xffff) if full_mantissa else (r >> 14) & 0xffff
            bits = (bits << 16) | low
            bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits)
            out.append(bits.to(torch.int32).view(torch.float32).view(B * L, C, H, H).contiguous())
            continue
        bits = torch.where(bits >= 1 << 15, bits - (1 << 16), bits)
        out.append(bits.to(torch.int16).view(dtype).view(B * L, C, H, H).contiguous())
    return out


def bit_maps32(B, L, seed, full_mantissa=False):
    """Random finite fp32 patterns: both signs, all 23 mantissa bits in play (or all set), exponents over +-30 octaves around 1, and
    one value in eight below 2^-109 (exponent fields 0 .. 17, the subnormals among them): there the lower planes of the cut run
    into the subnormals."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for _, C, H in spec.SITES:
        n = B * L * C * H * H
        r = torch.randint(0, 1 << 62, (n,), device="cuda", generator=g, dtype=torch.int64)
        sign = (r & 1) << 31
        mant = torch.full_like(r, 0x7fffff) if full_mantissa else (r >> 1) & 0x7fffff
        e = 97 + (r >> 24) % 61                                       # 2^-30 .. 2^30
        e = torch.where((r >> 32) % 8 == 0, (r >> 36) % 18, e)        # 0 (subnormal) .. 17 (2^-110)
        bits = sign | (e << 23) | mant
        bits = torch.where(bits >= 1 << 31, bits - (1 << 32), bits)
        out.append(bits.to(torch.int32).view(torch.float32).view(B * L, C, H, H).contiguous())
    return out


def heavy_maps(B, L, dtype, seed):
    """Heavy-tailed maps within fp16's range (expm1 of a scaled normal, up to ~1e4)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.expm1(1.5 * torch.randn(B * L, C, H, H, device="cuda", generator=g)).clamp(max=3e4).to(dtype).contiguous()
            for _, C, H in spec.SITES]


def maps_of_kind(kind, B, L, dtype, seed):
    if kind == "relu":
        return relu_maps(B, L, dtype, seed)
    if kind == "heavy_tail":
        return heavy_maps(B, L, dtype, seed)
    x = bit_maps(B, L, dtype, seed, full_mantissa=kind == "full_mantissa")
    if kind == "random_bits":                                   # the generator does reach the type's subnormals
        tiny = 2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126
        assert any(bool(((t.float().abs() < tiny) & (t.float() != 0)).any()) for t in x)
    return x


# ---- what the calls write ----

def unit_regions(h):
    """Copies of what the units write: the 160 unit channels of every site in its fusion buffer, and D_<site>."""
    P = h.P
    out = []
    for fkey, fd in spec.FUSION.items():
        width = 160 * len(fd["sites"]) + fd["carry"]
        buf = h.region("fusion_" + fkey, width).view(P, fd["H"], fd["H"], width)
        for i, sname in enumerate(fd["sites"]):
            out.append(buf[..., 160 * i:160 * i + 160].clone())
            out.append(h.region("D_" + sname, 32).clone())
    return out


def written(h):
    """Copies of everything K1 + K2 write: G_<site> and D_<site> of every site, and its 160 unit channels in the fusion buffer."""
    P = h.P
    out = []
    for fkey, fd in spec.FUSION.items():
        width = 160 * len(fd["sites"]) + fd["carry"]
        buf = h.region("fusion_" + fkey, width).view(P, fd["H"], fd["H"], width)
        for i, sname in enumerate(fd["sites"]):
            out.append(("unit_" + sname, buf[..., 160 * i:160 * i + 160].clone()))
            out.append(("G_" + sname, h.region("G_" + sname, 128).clone()))
            out.append(("D_" + sname, h.region("D_" + sname, 32).clone()))
    return out


def run_units(h, x, train):
    h.workspace.fill_(0xff)                            # (NaN in every float: what the units leave unwritten shows)
    if train:
        h.off_units_train(x, DROP_SEED, DROP_P)
    else:
        h.off_units(x)
    return written(h)


# ---- the backward's inputs, and the anchors against the oracle ----

def cotangents(P):
    return [torch.from_numpy(synth.uniform_values(0xC07 + i, P * spec.NUM_CLASSES, 1.0).reshape(P, spec.NUM_CLASSES))
            for i in range(3)]


def unit_drop(seed, P, p=DROP_P):
    return [torch.from_numpy(synth.dropout_keep(seed, si, P, H, p)).float() / (1.0 - p)
            for si, (_n, _c, H) in enumerate(spec.SITES)]


def grad_views(dm):
    """nine [P,160,H,H] -> the three fusion-buffer gradients, channels-last, + per-site (tensor, coff)."""
    groups = ((0, 1), (2, 3, 4, 5, 6), (7, 8))
    views = [None] * spec.NUM_SITES
    for grp in groups:
        buf = torch.cat([dm[i] for i in grp], dim=1).permute(0, 2, 3, 1).contiguous().cuda()
        for k, i in enumerate(grp):
            views[i] = (buf, 160 * k)
    return views


@functools.lru_cache(maxsize=None)
def oracle_dm(variant, B, L, slice_mode):
    """dM as tests/test_gpu_backward.py makes it: the head cotangents of cotangents(P) taken back through the oracle's fusion
    stages (on the synthetic fp32 maps; the equality below holds for any dM, so it need not belong to the maps under test).
    Computed once per configuration and shared by every test that needs it."""
    w = orc.to_torch_weights(synth.make_weights(variant))
    tf = [torch.from_numpy(f) for f in synth.make_features(B, L, 9)]
    P = B * (L - 1)
    _g, dm = orc.unit_backward(tf, w, B, L, variant, slice_mode, cotangents(P), unit_drop(DROP_SEED, P), None)
    return [d.detach() for d in dm]


def rel_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def device_relu_masks(h, feats_cpu, w, B, L, slack=1e-5):
    """The ReLU decisions the device took (saved G > 0), after checking that they differ from the oracle's own only for
    pre-activations within rounding distance of zero (as tests/test_gpu_backward.py)."""
    masks = []
    for (site, _c, H), x in zip(spec.SITES, feats_cpu):
        G = h.region("G_" + site, 128).view(B * L, H * H, 128).permute(0, 2, 1).reshape(B * L, 128, H, H).cpu()
        with torch.no_grad():
            pre = torch.nn.functional.conv2d(x, w["motion_conv_gen_%s.weight" % site], w["motion_conv_gen_%s.bias" % site])
        mask = (G > 0)
        flip = mask != (pre > 0)
        assert int(flip.sum()) <= 5 + slack * flip.numel(), site
        if flip.any():
            assert float(pre[flip].abs().max()) < slack * max(1.0, float(pre.abs().max())), site
        masks.append(mask.float())
    return masks


def _units_node(out):
    """The autograd node of OFFUnits behind one of its outputs (the object the forward stored its ctx attributes on)."""
    node = out.grad_fn
    while node is not None and not hasattr(node, "feats"):
        node = node.next_functions[0][0]
    assert node is not None
    return node
