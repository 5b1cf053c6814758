"""Helpers the GPU tests of the feature-map kinds share (tests/test_gpu_feat16.py, test_gpu_feat_cl.py, test_gpu_feat16_train.py,
test_gpu_feat_cl_train.py, test_gpu_bounds.py, and through tests/units_grad.py every GPU test file of the units' training side): the one
`rt` fixture, handles, the map generators, what the units' calls write, the backward's inputs and the anchors against the oracle; then the
kinds table (KINDS: "typed" and "cl", the two kinds runtime._KINDS and offk_api.hip's kKind16 / kKindCl have) and the bodies the two
kinds' test files share, written once against a row of it -- equality with the plain call, the raw calls of the refusal tests, capture
and replay, non-finite maps, the toy backbone.  A helper module like tests/arena.py: no tests of its own.  The generators draw on the
device from a seeded generator; a test's inputs are a function of (generator, B, L, dtype, seed) alone."""
import ctypes
import functools

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth
from oracle import off_oracle as orc

from . import forward

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPES16 = {"bf16": torch.bfloat16, "f16": torch.float16}
DROP_SEED, DROP_P = 7, 0.8


@pytest.fixture(scope="module")
def rt():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime
    return runtime


def make_handle(rt, B, L, variant=spec.VARIANT_RGB, slice_mode=spec.SLICE_FLAT, consensus=None, precision="f32split", **kw):
    return forward.make_handle(rt, B, L, variant, slice_mode, consensus, precision=precision, **kw)[0]


def make_train_handle(rt, B, L, variant=spec.VARIANT_RGB, slice_mode=spec.SLICE_FLAT, precision="fp32", **kw):
    return forward.make_handle(rt, B, L, variant, slice_mode, precision=precision, training=True, **kw)[0]


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
    pre-activations within rounding distance of zero."""
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


# ---- the two kinds of feature maps, and what their test files share ----

FDT = {"f32": _lib.FEAT_F32, "bf16": _lib.FEAT_BF16, "f16": _lib.FEAT_F16}
STEMS = ("offk_pw_reduce", "offk_off_units", "offk_off_units_train", "offk_off_units_backward")      # + the kind's suffix


def to_cl(x):
    """The channels_last copy of a map (or of each of a list of maps): the same logical tensor, physically [N, H, H, C]."""
    if isinstance(x, (list, tuple)):
        out = [to_cl(t) for t in x]
        assert all(not c.is_contiguous() and c.is_contiguous(memory_format=torch.channels_last) and torch.equal(c, t) for c, t in zip(out, x))
        return out
    return x.contiguous(memory_format=torch.channels_last)


def as_it_is(x):
    """A contiguous map (or each of a list of them) as it stands."""
    return [as_it_is(t) for t in x] if isinstance(x, (list, tuple)) else x.contiguous()


class Kind:
    """One feature-map kind.  suffix: of its C entries; dtypes: the map dtypes it takes; put: a test map, or a list of them, into the kind's
    form (typed: as it is, cl: the channels_last copy, checked to hold the same values); plain: the same map the plain way, whose results
    the kind's must equal (typed: x.float(), cl: the contiguous copy); check: the name of the runtime's per-map check of the kind."""

    def __init__(self, name, suffix, dtypes, put, plain, check):
        self.name, self.suffix, self.dtypes, self.put, self.plain, self.check = name, suffix, dtypes, put, plain, check

    def __repr__(self):
        return "Kind(%s)" % self.name

    def pair(self, x):
        """(the maps the plain way, the maps in the kind's form): the same logical tensors"""
        plain = [self.plain(t) for t in x]
        assert all(t.is_contiguous() for t in plain)
        return plain, self.put(x)

    def entry(self, lib, stem):
        return getattr(lib, stem + self.suffix)


KINDS = {"typed": Kind("typed", "_typed", DTYPES16, as_it_is, lambda t: t.float(), "_check_dev16"),
         "cl": Kind("cl", "_cl", DTYPES, to_cl, lambda t: t.contiguous(), "_check_dev_cl")}


def units_equal(h, kind, x):
    """off_units_fused on the maps in the kind's form == off_units_fused on the same maps the plain way, every region finite."""
    plain, maps = kind.pair(x)
    if kind.name == "cl":
        assert h.takes_channels_last(maps) and not h.takes_channels_last(plain)
    h.workspace.fill_(0xff)                            # (NaN in every float: what the units leave unwritten shows)
    h.off_units_fused(plain)
    ref = unit_regions(h)
    h.workspace.fill_(0xff)
    h.off_units_fused(maps)
    got = unit_regions(h)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(a, b)


def split_parts(kind, x, i):
    """Channel groups of map i in concat order (multiples of 32; 1 .. 4 groups by site), each in the kind's form on its own."""
    C = x.shape[1]
    cuts = [[C], [C // 2 // 32 * 32, C], [64, 128, C], [32, 96, 224, C]][i % 4]
    parts, a = [], 0
    for b in cuts:
        parts.append(kind.put(x[:, a:b]))
        a = b
    return parts


def assert_forward_equal(h, kind, x):
    """off_units and off_units_train on the maps in the kind's form write what they write on the same maps the plain way."""
    plain, maps = kind.pair(x)
    for train in (False, True):
        ref = run_units(h, plain, train)
        got = run_units(h, maps, train)
        torch.cuda.synchronize()
        assert len(got) == 27
        for (name, a), (_n, b) in zip(got, ref):
            assert a.dtype == torch.float32 and torch.isfinite(a).all(), (name, train)
            assert torch.equal(a, b), (name, train)


def assert_backward_equal(h, kind, x, views):
    """The flat gradient buffer of the backward on the maps in the kind's form equals the plain one's: overwritten, and accumulated onto a
    pre-filled buffer.  Each backward follows the forward on the same maps (G / D are bit-equal either way)."""
    plain, maps = kind.pair(x)
    n = h.new_unit_grads().numel()
    g = torch.Generator(device="cuda").manual_seed(n)
    fill = torch.randn(n, device="cuda", generator=g)
    res = {}
    for tag, xs in (("plain", plain), ("kind", maps)):
        h.off_units_train(xs, DROP_SEED, DROP_P)
        over = torch.full((n,), float("nan"), device="cuda")
        h.off_units_backward(xs, views, DROP_SEED, DROP_P, grads=over, accumulate=False)
        acc = fill.clone()
        h.off_units_backward(xs, views, DROP_SEED, DROP_P, grads=acc, accumulate=True)
        res[tag] = (over, acc)
    torch.cuda.synchronize()
    for a, b in zip(res["kind"], res["plain"]):
        assert a.dtype == torch.float32 and torch.isfinite(a).all()
        assert torch.equal(a, b)
    assert not torch.equal(res["kind"][1], fill) and float(res["kind"][0].abs().max()) > 0


def captured(launch):
    """`launch` warmed up on a side stream, then captured into a torch.cuda.CUDAGraph: the graph, not yet replayed."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    return g


def train_and_backward_capture(rt, kind, name):
    """off_units_train followed by off_units_backward on maps of the kind, captured in a torch.cuda.graph on one stream and replayed
    twice: bit-identical to the eager run."""
    B, L = 3, 4
    h = make_train_handle(rt, B, L)
    x = kind.put(relu_maps(B, L, kind.dtypes[name], 21))
    views = grad_views(oracle_dm(spec.VARIANT_RGB, B, L, spec.SLICE_FLAT))
    grads = h.new_unit_grads()

    def launch():
        h.off_units_train(x, DROP_SEED, DROP_P)
        h.off_units_backward(x, views, DROP_SEED, DROP_P, grads=grads, accumulate=False)

    launch()
    torch.cuda.synchronize()
    eager_g, eager_w = grads.clone(), written(h)
    g = captured(launch)                               # (with its warm-up on the capture stream)
    for _ in range(2):
        grads.fill_(float("nan"))
        h.workspace.fill_(0xff)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(grads, eager_g)
        for (n, a), (_n, b) in zip(written(h), eager_w):
            assert torch.equal(a, b), n


def forward_capture_and_determinism(rt, kind, name):
    """offk_forward<suffix> straight through ctypes on a side stream, then captured and replayed onto zeroed outputs, and h.forward on the
    same maps before and after: all the same finite values."""
    B, L = 3, 7
    h = make_handle(rt, B, L)
    x = kind.put(relu_maps(B, L, kind.dtypes[name], 21))
    arr = h._feat_array(x, getattr(rt, kind.check))
    out = [torch.empty(h.out_rows(), spec.NUM_CLASSES, device="cuda") for _ in range(3)]

    def launch():
        _lib.check(kind.entry(h.lib, "offk_forward")(h._h, rt._stream(h.device), FDT[name], arr, *[ctypes.c_void_p(o.data_ptr()) for o in out],
                                                     ctypes.c_void_p(h.workspace.data_ptr())), h._h)

    g = captured(launch)
    eager = [o.clone() for o in out]                   # the warm-up run's values: the capture itself ran nothing
    assert all(torch.isfinite(o).all() for o in eager)
    again = h.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, out))
    again = h.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))


def nonfinite_maps(rt, kind, name):
    """Inf / NaN in a map of the kind: every D row it touches is non-finite in all 32 channels; every other unit output stays finite."""
    B, L = 2, 3
    x = relu_maps(B, L, kind.dtypes[name], 5)
    x[0][1, 7, 3, 4] = float("inf")                    # site 3a, frame 1 (clip 0), pixel (3, 4)
    x[8][2, 100, 5, 6] = float("nan")                  # site 5b, frame 2 (clip 0), pixel (5, 6)
    h = make_handle(rt, B, L)
    h.off_units_fused([kind.put(t) for t in x])        # (map by map: the list form of `put` compares values, and NaN != NaN)
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


# what is refused, before any launch: the kinds' entries straight through ctypes (no Python-side checks)

def raw_forward(h, rt, kind, fdt, ptrs):
    """offk_forward<suffix>; returns (rc, message)."""
    arr = (ctypes.c_void_p * spec.NUM_SITES)(*ptrs)
    out = [torch.empty(h.out_rows(), spec.NUM_CLASSES, device="cuda") for _ in range(3)]
    rc = kind.entry(h.lib, "offk_forward")(h._h, rt._stream(h.device), fdt, arr, *[ctypes.c_void_p(o.data_ptr()) for o in out],
                                           ctypes.c_void_p(h.workspace.data_ptr()))
    return rc, h.lib.offk_last_error(h._h).decode()


def assert_forward_refused(h, rt, kind, fdt, xs, needle):
    h.workspace.fill_(0x5a)
    torch.cuda.synchronize()
    rc, msg = raw_forward(h, rt, kind, fdt, [x.data_ptr() for x in xs])
    torch.cuda.synchronize()
    assert rc == -1 and needle in msg, (rc, msg)
    assert bool((h.workspace == 0x5a).all())              # nothing was enqueued


def raw_calls(h, rt, kind, fdt, ptrs, views, grads, stems):
    """The training-side entries named in `stems` (+ the kind's suffix); [(entry, rc, message)]."""
    arr = (ctypes.c_void_p * spec.NUM_SITES)(*ptrs)
    gv = (_lib.OffkGradView * spec.NUM_SITES)()
    for i, (t, coff) in enumerate(views):
        gv[i].data, gv[i].cstride, gv[i].coff = t.data_ptr(), t.shape[-1], int(coff)
    ws, st = ctypes.c_void_p(h.workspace.data_ptr()), rt._stream(h.device)
    G = torch.zeros(h.N * 28 * 28, 128, device="cuda")
    D = torch.zeros(h.P * 28 * 28, 32, device="cuda")
    fn = lambda stem: kind.entry(h.lib, stem)  # noqa: E731
    out = []
    for stem, call in (
            ("offk_pw_reduce", lambda: fn("offk_pw_reduce")(h._h, st, fdt, 0, ctypes.c_void_p(ptrs[0]),
                                                            ctypes.c_void_p(G.data_ptr()), ctypes.c_void_p(D.data_ptr()))),
            ("offk_off_units", lambda: fn("offk_off_units")(h._h, st, fdt, arr, ws)),
            ("offk_off_units_train", lambda: fn("offk_off_units_train")(h._h, st, fdt, arr, ws, DROP_SEED, DROP_P)),
            ("offk_off_units_backward", lambda: fn("offk_off_units_backward")(h._h, st, fdt, arr, gv, ws, DROP_SEED, DROP_P,
                                                                              ctypes.c_void_p(grads.data_ptr()), 0))):
        if stem not in stems:
            continue
        rc = call()
        out.append((stem + kind.suffix, rc, h.lib.offk_last_error(h._h).decode()))
    torch.cuda.synchronize()
    assert not G.any() and not D.any()
    return out


def assert_refused(h, rt, kind, fdt, ptrs, views, needle, stems=STEMS):
    """Every entry named refuses with the needle and its own name in the text, and nothing was enqueued."""
    h.workspace.fill_(0x5a)
    grads = torch.full((h.new_unit_grads().numel(),), 3.25, device="cuda")
    torch.cuda.synchronize()
    seen = 0
    for entry, rc, msg in raw_calls(h, rt, kind, fdt, ptrs, views, grads, stems):
        assert rc == -1 and needle in msg and entry in msg, (entry, rc, msg)
        seen += 1
    assert seen == len(stems)
    torch.cuda.synchronize()
    assert bool((h.workspace == 0x5a).all()) and bool((grads == 3.25).all())      # nothing was enqueued


class ToyBackbone(torch.nn.Module):
    """Nine maps of the inception shapes out of a 3-channel 28 x 28 input (1x1 convs after average pooling), handed over in
    `memory_format`; score=True: (maps, a score from a linear layer) as a whole backbone returns them."""

    def __init__(self, memory_format=torch.contiguous_format, score=False):
        super().__init__()
        self.memory_format = memory_format
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(3, C, 1) for _, C, _ in spec.SITES)
        self.fc = torch.nn.Linear(3, spec.NUM_CLASSES) if score else None

    def forward(self, x):
        feats = [torch.relu(conv(torch.nn.functional.avg_pool2d(x, 28 // H))).contiguous(memory_format=self.memory_format)
                 for (_, _C, H), conv in zip(spec.SITES, self.convs)]
        return (feats, self.fc(x.mean(dim=(2, 3)))) if self.fc is not None else feats
