"""Guard-band and stale-memory tests: every entry point of include/offk.h that writes device memory, run with every buffer it
touches carved out of one sentinel-filled arena (tests/arena.py) at exactly the documented size.

Each case runs the same call twice on the same inputs and weights.  Run A uses ordinary allocations.  Run B carves inputs,
bound weights, outputs, scratch and the workspace from one arena; outputs, scratch and workspace are LEFT full of the sentinel
(a NaN in fp32, bf16 and fp16).  Then

* arena.check(): no word outside a carve changed (an out-of-bounds write of up to a whole 128-row tile lands in a guard band);
* every output and every region the path documents as filled is finite (a read of memory the call did not write meets a NaN);
* every such output and region is bit-equal to run A's (the result does not depend on what the buffers held before);
* regions a path documents as NOT written still hold the sentinel, word for word (interior guards of the one workspace carve).

No tolerance anywhere: same handle, same kernels, fixed summation orders.  Values are held to torch / the oracle elsewhere.

Entry points that write device memory, and the case that guards each:

    offk_forward                      test_forward_paths (every path switch, both variants, both precisions), test_forward_consensus_avg,
                                      test_forward_without_out28, test_forward_training_superset_stays_untouched,
                                      test_forward_bound_weights, test_two_handles_on_two_streams
    offk_forward_parts                test_forward_entry_forms[f32-parts]
    offk_forward_typed                test_forward_entry_forms[bf16 / f16], test_minimal_alignment[forward_typed-4]
    offk_forward_parts_typed          test_forward_entry_forms[bf16-parts / f16-parts]
    offk_forward_cl                   test_forward_entry_forms[f32cl / bf16cl / f16cl], test_minimal_alignment[forward_cl-16]
    offk_forward_parts_cl             test_forward_entry_forms[f32cl-parts / f16cl-parts]
    offk_pw_reduce / _typed / _cl     test_pw_reduce_writes_all_of_g_and_d
    offk_sobel_tdiff                  test_sobel_tdiff
    offk_sobel_tdiff_all              test_sobel_tdiff_all_after_units
    offk_off_units / _typed / _cl     test_off_units[units-*]
    offk_off_units_fused / _typed / _cl   test_off_units[fused-*]
    offk_off_units_train / _typed / _cl, offk_off_units_backward / _typed / _cl
                                      test_units_train_and_backward (both accumulate modes, wide gradient views),
                                      test_minimal_alignment[train_typed-8], test_minimal_alignment[train_cl-16]
    offk_conv2d / offk_conv2d_ex      test_conv2d_tile_plans (offk_conv2d is offk_conv2d_ex with the automatic plan: tile_cfg -1),
                                      test_conv2d_patch_kernel
    offk_pack_conv_weight             test_pack_conv_weight
    offk_bottleneck_chain14           test_bottleneck_chain14
    offk_bottleneck_chain14_split     test_bottleneck_chain14_split
    offk_winograd_conv3x3             test_winograd_conv3x3
    offk_winograd_conv5x5s2           test_winograd_conv5x5s2
    offk_winograd_conv7x7s2           test_winograd_conv7x7s2
    offk_winograd_between / _ex       test_winograd_between
    offk_batched_gemm_nt              test_batched_gemm_nt
    offk_head                         test_head
    offk_segment_consensus / _backward    test_segment_consensus_and_backward
    offk_nchw_to_nhwc / offk_nhwc_to_nchw   test_layout_helpers
    offk_score_fusion                 test_score_fusion

(offk_set_weight writes the library's own copies, not caller memory.)
"""
import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from .arena import same_bits
from .featmaps import DTYPES, rt  # noqa: F401
from .forward import BOUNDS_PATHS as PATHS
from .forward import HANDLE_PRECISIONS, chain_inputs, make_handle
from .guarded import FUSION, Guarded, forward_body, g_regions_stay, np_feats, put_feats, two_runs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (3, 3)]      # one pair, 49-row 7x7 sites; P = 6: 294 rows at 7x7 -- partial against 16-, 32-, 96- and 128-row tiles
VARIANTS = [spec.VARIANT_RGB, spec.VARIANT_FLOW]
_HANDLES = {}


def handle(rt, B, L, variant=spec.VARIANT_RGB, prec="fp32", path="default", consensus=False):
    """One handle per configuration for the module (the switches are read once, at offk_create)."""
    key = (B, L, variant, prec, path, consensus)
    if key not in _HANDLES:
        _HANDLES[key] = make_handle(rt, B, L, variant, consensus=consensus, precision=prec, env=PATHS[path])[0]
    h = _HANDLES[key]
    h.training = False
    return h


def test_arena_checker_on_the_device():
    """tests/test_arena.py on the CPU is the proof of the checker; here the same three facts on the device the kernels write to."""
    g = Guarded([4096, 4096])
    x = g.out("x", (1024,))
    g.out("y", (1024,))
    assert bool(torch.isnan(x).all())
    g.arena.check()
    _name, start, nbytes = g.arena.carves[0]
    g.arena.words[(start + nbytes) // 4 + 2] = 0
    g.arena.words[start // 4 - 1] = 0
    assert g.arena.breaches() == [("x", "before", -4, -4, 1), ("x", "after", 8, 8, 1)]


# ---- the whole forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_paths(rt, B, L, variant, prec, path):
    """offk_forward through every path switch: about 32 launches over about 40 workspace regions, split-K slabs, pool partials and
    Winograd V / M, on a workspace, logits buffers and maps that sit between guard bands and start out as NaN."""
    h = handle(rt, B, L, variant, prec, path)
    two_runs(forward_body(h, np_feats(B, L), fused=path != "unfused_units"))


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
def test_forward_consensus_avg(rt, prec):
    """Consensus AVG at (3, 3): the caller's logits buffers hold B = 3 rows while the heads compute P = 6 -- a head that writes its
    per-pair rows into the caller's buffer breaches the guard behind it."""
    h = handle(rt, 3, 3, spec.VARIANT_FLOW, prec, consensus=True)
    assert h.out_rows() == 3 and h.P == 6
    two_runs(forward_body(h, np_feats(3, 3)))


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
def test_forward_without_out28(rt, prec):
    h = handle(rt, 3, 3, spec.VARIANT_RGB, prec)
    a, _b = two_runs(forward_body(h, np_feats(3, 3), want28=False))
    assert "out28" not in a


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_training_superset_stays_untouched(rt, B, L, prec):
    """A training handle's workspace is the superset offk_train_workspace_bytes; a forward may write only the forward layout."""
    h = handle(rt, B, L, spec.VARIANT_RGB, prec)
    h.training = True
    two_runs(forward_body(h, np_feats(B, L), superset=True))


FORMS = [("f32", True), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True), ("f32cl", False), ("f32cl", True),
         ("bf16cl", False), ("f16cl", False), ("f16cl", True)]


@pytest.mark.parametrize("form,parts", FORMS, ids=["%s%s" % (f, "-parts" if p else "") for f, p in FORMS])
@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_entry_forms(rt, B, L, form, parts):
    """Split-fp32 handles: the forward from channel groups (two to four per site), from bf16 / fp16 maps and from channels_last maps
    of all three dtypes.  Beside the two runs: equal to the same handle on x.float() / the contiguous copy, as the entries' own
    modules hold them."""
    h = handle(rt, B, L, spec.VARIANT_RGB, "f32split")
    feats = [f.to(DTYPES[form.replace("cl", "")]) for f in np_feats(B, L)]
    a, _b = two_runs(forward_body(h, feats, form, parts))
    h._ws = None
    want = h.forward([f.float().cuda() for f in feats])
    torch.cuda.synchronize()
    for k, w in zip(("out7", "out14", "out28"), want):
        assert torch.equal(a[k], w), k
    for name, ch, units in FUSION:
        assert torch.equal(a[name], h.region(name, ch)), name


def test_forward_bound_weights(rt):
    """offk_bind_weight: the units' parameters read in place from carves of the arena (a read past a parameter's end meets a NaN)."""
    B, L = 3, 3
    feats = np_feats(B, L)
    wnp = synth.make_weights(spec.VARIANT_RGB)
    keys = [k for k in spec.weight_shapes(spec.VARIANT_RGB) if k.startswith(spec.UNIT_PARAM_PREFIXES)]
    alive = []                                           # handles and bound tensors outlive the comparison

    def body(r):
        h = rt.OffForward(B, L, spec.VARIANT_RGB)
        assert h.load_state_dict(wnp) == []
        bound = [(k, r.put(k, torch.from_numpy(wnp[k]))) for k in keys]
        for k, t in bound:
            h.bind_weight(k, t)
        alive.append((h, bound))
        return forward_body(h, feats, fused=None)(r)      # (bound weights: the register-staged kernel; nothing is promised about G_<site>)
    two_runs(body)


# ---- the units and their training side -----------------------------------------------------------------------------------------------
def units_regions(h, with_g):
    out = {}
    for name, _c, _h in spec.SITES:
        out["D_" + name] = h.region("D_" + name, 32)
        if with_g:
            out["G_" + name] = h.region("G_" + name, 128)
    for name, ch, units in FUSION:
        out[name + "[units]"] = h.region(name, ch)[:, :units]
    return out


def fusion_tails_stay(r, h):
    for name, ch, units in FUSION:
        if units < ch:
            r.must_stay(h.region(name, ch)[:, units:], "%s channels %d.. (the units write their own 160 channels per site)" % (name, units))


# (the 16-bit / channels-last fused entries exist on split-fp32 handles only)
UNIT_CASES = [(p, e, f) for p in HANDLE_PRECISIONS for e, f in (("units", "f32"), ("units", "bf16"), ("units", "f16cl"), ("units", "f32cl"),
                                                                 ("fused", "f32"), ("fused", "f16"), ("fused", "bf16cl"))
              if e == "units" or f == "f32" or p == "f32split"]


@pytest.mark.parametrize("prec,entry,form", UNIT_CASES, ids=["%s-%s-%s" % c for c in UNIT_CASES])
@pytest.mark.parametrize("B,L", SHAPES)
def test_off_units(rt, B, L, prec, entry, form):
    """offk_off_units (K1 + K2: G, D and the unit channels) and offk_off_units_fused (D and the unit channels; G_<site> untouched), their
    16-bit and channels-last forms included; neither may write another channel of the fusion buffers."""
    h = handle(rt, B, L, spec.VARIANT_RGB, prec)
    h.training = True
    feats = [f.to(DTYPES[form.replace("cl", "")]) for f in np_feats(B, L)]

    def body(r):
        fs = put_feats(r, feats, form)
        r.workspace(h)
        (h.off_units if entry == "units" else h.off_units_fused)(fs)
        fusion_tails_stay(r, h)
        if entry == "fused":
            g_regions_stay(r, h)
        return units_regions(h, entry == "units")
    two_runs(body)


def wide_grad_views(r, P, seed):
    """The cotangents of the nine units as offk_grad_view: one channels-last buffer per fusion stage, WIDER than the units' channels
    (32 in front, 32 behind) and every view at a non-zero coff."""
    groups = ((0, 1), (2, 3, 4, 5, 6), (7, 8))
    views = [None] * spec.NUM_SITES
    for gi, grp in enumerate(groups):
        H = spec.SITES[grp[0]][2]
        cs = 160 * len(grp) + 64
        buf = torch.from_numpy(synth.uniform_values(seed + gi, P * H * H * cs, 1.0).reshape(P * H * H, cs))
        buf = r.put("grad_view_%d" % H, buf)
        for k, i in enumerate(grp):
            views[i] = (buf, 32 + 160 * k)
    return views


def train_body(h, feats, form, drop_p, accumulate, offset=0):
    def body(r):
        fs = put_feats(r, feats, form, offset)
        ws = r.workspace(h)
        views = wide_grad_views(r, h.P, 0xD00)
        n = int(h.lib.offk_unit_grad_floats(h._h))
        grads = r.out("unit_grads", (n,))                 # exactly offk_unit_grad_floats
        if accumulate:
            grads.fill_(0.25)
        h.off_units_train(fs, drop_seed=11, drop_p=drop_p)
        fusion_tails_stay(r, h)
        res = units_regions(h, True)
        res = dict((k, v.clone()) for k, v in res.items())
        flat, _views = h.off_units_backward(fs, views, drop_seed=11, drop_p=drop_p, grads=grads, accumulate=accumulate)
        assert flat.data_ptr() == grads.data_ptr()
        res["unit_grads"] = flat
        assert ws.numel() == int(h.lib.offk_train_workspace_bytes(h._h)) > int(h.lib.offk_workspace_bytes(h._h))
        return res
    return body


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("drop_p", [0.0, 0.8])
@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_units_train_and_backward(rt, B, L, prec, drop_p, accumulate):
    """offk_off_units_train then offk_off_units_backward: accumulate = 0 into a sentinel-filled gradient carve of exactly
    offk_unit_grad_floats (every slot must be overwritten), accumulate = 1 onto a finite fill; gradient views with a wider cstride
    and a non-zero coff; the workspace is the training superset, between guards."""
    h = handle(rt, B, L, spec.VARIANT_RGB, prec)
    h.training = True
    two_runs(train_body(h, np_feats(B, L), "f32", drop_p, accumulate))


PW_FORMS = ["f32", "bf16", "f16cl", "f32cl"]


@pytest.mark.parametrize("form", PW_FORMS)
@pytest.mark.parametrize("site", [0, 3, 8], ids=["3a", "4a", "5b"])
@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("B,L", SHAPES)
def test_pw_reduce_writes_all_of_g_and_d(rt, B, L, prec, site, form):
    """offk_pw_reduce alone with G and D both full of the sentinel: K1 writes every row of both (runtime.pw_reduce allocates D
    with torch.empty on the strength of this test)."""
    h = handle(rt, B, L, spec.VARIANT_RGB, prec)
    _name, C, H = spec.SITES[site]
    x = np_feats(B, L)[site].to(DTYPES[form.replace("cl", "")])

    def body(r):
        f = r.put("feat", x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2) if form.endswith("cl") else r.put("feat", x)
        G, D = h.pw_reduce(site, f, G=r.out("G", (h.N * H * H, 128)), D=r.out("D", (h.P * H * H, 32)))
        return {"G": G, "D": D}
    two_runs(body)
    G, D = h.pw_reduce(site, x.cuda().contiguous() if not form.endswith("cl") else x.cuda().contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(D).all()) and bool(torch.isfinite(G).all())


@pytest.mark.parametrize("algo", [0, 1, 4])
@pytest.mark.parametrize("site", [0, 3, 8], ids=["3a", "4a", "5b"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_sobel_tdiff(rt, variant, site, algo):
    """offk_sobel_tdiff into a 160-channel slice of a 352-channel carve: channels AND rows guarded."""
    B, L = 3, 3
    h = handle(rt, B, L, variant)
    H = spec.SITES[site][2]
    g = torch.Generator().manual_seed(site + 10 * variant)
    Gin = torch.relu(torch.randn(h.N * H * H, 128, generator=g))
    Din = torch.randn(h.P * H * H, 32, generator=g)

    def body(r):
        G, D = r.put("G", Gin), r.put("D", Din)
        M = r.out("M", (h.P * H * H, 352))
        h.sobel_tdiff(site, G, D, M, 160, algo)
        r.must_stay(M[:, :160], "M channels 0..159")
        r.must_stay(M[:, 320:], "M channels 320..351")
        return {"M[160:320]": M[:, 160:320]}
    two_runs(body)


@pytest.mark.parametrize("algo", [0, 1, 4])
@pytest.mark.parametrize("B,L", SHAPES)
def test_sobel_tdiff_all_after_units(rt, B, L, algo):
    """offk_sobel_tdiff_all reads the G / D regions of the matching offk_off_units: that one runs in the arena first."""
    h = handle(rt, B, L, spec.VARIANT_FLOW)
    feats = np_feats(B, L)

    def body(r):
        fs = put_feats(r, feats)
        r.workspace(h)
        h.off_units(fs)
        before = dict((k, v.clone()) for k, v in units_regions(h, True).items())
        h.sobel_tdiff_all(algo)
        fusion_tails_stay(r, h)
        res = units_regions(h, True)
        torch.cuda.synchronize()
        for k in before:
            if k.startswith(("G_", "D_")):
                assert torch.equal(before[k], res[k]), "%s changed under K2" % k
        return res
    two_runs(body)


# ---- minimal legal alignment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,offset", [("forward_typed", 4), ("train_typed", 8), ("forward_cl", 16), ("train_cl", 16)],
                         ids=["forward_typed-4", "train_typed-8", "forward_cl-16", "train_cl-16"])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_minimal_alignment(rt, entry, offset, dt):
    """All nine maps at the least alignment the header accepts (4 bytes: offk_forward_typed; 8: the _typed training entries; 16: the
    _cl entries) and no more: bit-equal to the run on 256-byte-aligned maps, guards clean."""
    B, L = 3, 3
    h = handle(rt, B, L, spec.VARIANT_RGB, "f32split")
    feats = [f.to(DTYPES[dt]) for f in np_feats(B, L)]
    form = dt + ("cl" if entry.endswith("_cl") else "")
    if entry.startswith("forward"):
        body = forward_body(h, feats, form, offset=offset)
    else:
        h.training = True
        body = train_body(h, feats, form, 0.8, False, offset=offset)
    probe = Guarded([f.numel() * 2 for f in feats])
    for f in put_feats(probe, feats, form, offset):
        assert f.data_ptr() % 256 == offset and f.data_ptr() % (2 * offset) != 0
    two_runs(body)               # run A: the same maps in ordinary (256-byte-aligned) allocations


# ---- distinct handles are independent -------------------------------------------------------------------------------------------------
def test_two_handles_on_two_streams(rt):
    """offk.h: "distinct handles are independent".  Two handles on one device, each with its own carves, their forwards enqueued
    alternately, three times, on two streams with no synchronisation in between: each one's logits equal its own serial run."""
    cfgs = [(1, 2, spec.VARIANT_RGB, "fp32"), (3, 3, spec.VARIANT_FLOW, "f32split")]
    hs = [handle(rt, *c) for c in cfgs]
    feats = [np_feats(c[0], c[1], 6 + i) for i, c in enumerate(cfgs)]
    serial = []
    for h, f in zip(hs, feats):
        h._ws = None
        out = h.forward([t.cuda() for t in f])
        torch.cuda.synchronize()
        serial.append([o.clone() for o in out])
    sizes = [h.workspace_bytes for h in hs] + [t.numel() * 4 for f in feats for t in f] + [h.out_rows() * h.num_classes * 4 for h in hs] * 3
    g = Guarded(sizes)
    fs, outs = [], []
    for i, (h, f) in enumerate(zip(hs, feats)):
        fs.append([g.arena.put("h%d_feat_%s" % (i, spec.SITES[s][0]), t) for s, t in enumerate(f)])
        h.set_workspace(g.arena.carve("h%d_workspace" % i, h.workspace_bytes))
        outs.append(tuple(g.arena.empty("h%d_out%d" % (i, s), (h.out_rows(), h.num_classes)) for s in (7, 14, 28)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    for _rep in range(3):
        for h, s, f, o in zip(hs, streams, fs, outs):
            with torch.cuda.stream(s):
                h.forward(f, out=o)
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    g.arena.check()
    for i in range(2):
        for got, want in zip(outs[i], serial[i]):
            assert bool(torch.isfinite(got).all()) and same_bits(got, want), "handle %d" % i


# ---- stage entry points ---------------------------------------------------------------------------------------------------------
NS = [1, 5]       # 49 and 245 rows at 7x7: odd against every tile


def randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("cfg,splitk", [(c, k) for c in range(6) for k in (1, 3)] + [(-1, 0)])
@pytest.mark.parametrize("n", NS)
def test_conv2d_tile_plans(rt, n, cfg, splitk):
    """offk_conv2d_ex on every block tile (and the automatic plan, which is offk_conv2d) with split-K 1 and 3: y, and the partial
    slabs carved at exactly splitk * M * Co floats."""
    g = torch.Generator().manual_seed(77)
    H, Ci, Co = 7, 128, 256
    x, w, b, res = randn(g, n, H, H, Ci), randn(g, Co, Ci, 3, 3, scale=1 / 34.0), randn(g, Co), randn(g, n, H, H, Co)

    def body(r):
        wp = rt.pack_conv_weight(r.put("w", w), out=r.out("w_packed", (Co, 3, 3, Ci)))
        part = r.out("partial", (splitk * n * H * H * Co,)) if splitk > 1 else None
        y = rt.conv2d_nhwc(r.put("x", x), w, r.put("bias", b), 1, 1, res=r.put("res", res), flags=_lib.CONV_RELU_PRE | _lib.CONV_RELU_POST,
                           y=r.out("y", (n, H, H, Co)), tile_cfg=cfg, splitk=splitk, w_packed=wp, partial=part)
        return {"y": y}
    two_runs(body)


PATCH = [(7, 2, 28, 64, 128, 6, 2), (5, 2, 14, 1056, 128, 6, 3), (3, 1, 14, 64, 64, 7, 2), (3, 1, 7, 832, 256, 6, 4)]


@pytest.mark.parametrize("k,stride,H,Ci,Co,cfg,splitk", PATCH, ids=["7x7s2@28", "5x5s2@14", "3x3@14", "3x3@7"])
@pytest.mark.parametrize("n", NS)
def test_conv2d_patch_kernel(rt, n, k, stride, H, Ci, Co, cfg, splitk):
    """The LDS-patch kernel (tile_cfg 6 / 7) on its four shapes, channel-sliced input and output views, partial last groups."""
    g = torch.Generator().manual_seed(k * 1000 + Ci + Co + n)
    pad, Ho = k // 2, (H + 2 * (k // 2) - k) // stride + 1
    x, w, b = randn(g, n, H, H, Ci + 32), randn(g, Co, Ci, k, k, scale=(Ci * k * k) ** -0.5), randn(g, Co)
    res = randn(g, n, Ho, Ho, Co)
    flags = _lib.CONV_RELU_IN | _lib.CONV_RELU_PRE | _lib.CONV_RELU_POST

    def body(r):
        wp = rt.pack_conv_weight(r.put("w", w), out=r.out("w_packed", (Co, k, k, Ci)))
        ybuf = r.out("y", (n, Ho, Ho, Co + 64))
        rt.conv2d_nhwc(r.put("x", x), w, r.put("bias", b), stride, pad, res=r.put("res", res), flags=flags, x_coff=32, ci=Ci, y=ybuf, y_coff=32,
                       tile_cfg=cfg, splitk=splitk, w_packed=wp, partial=r.out("partial", (splitk * n * Ho * Ho * Co,)))
        r.must_stay(ybuf[..., :32], "y channels 0..31")
        r.must_stay(ybuf[..., 32 + Co:], "y channels behind the slice")
        return {"y[slice]": ybuf[..., 32:32 + Co]}
    two_runs(body)


def test_pack_conv_weight(rt):
    g = torch.Generator().manual_seed(3)
    w = randn(g, 64, 96, 5, 5)
    two_runs(lambda r: {"w_packed": rt.pack_conv_weight(r.put("w", w), out=r.out("w_packed", (64, 5, 5, 96)))})


CHAIN_CASES = ["28a", "28b_residual", "28c_into_slice"]


@pytest.mark.parametrize("case", CHAIN_CASES)
@pytest.mark.parametrize("n", NS)
def test_bottleneck_chain14(rt, case, n):
    """offk_bottleneck_chain14 (half-image blocks of 98 rows): the merged 28a form, the residual form, output into a channel slice."""
    merged = case == "28a"
    x, w1, b1, w2, b2, w3, b3, wb, bb = chain_inputs("28a_branch" if merged else case, n, "normal", 100 + n)
    if merged:
        w3, b3 = torch.cat([w3, wb], 1).contiguous(), b3 + bb          # c3 over [t2 | x0], K3 = 128

    def body(r):
        xd = r.put("x", x)
        args = [r.put(k, v) for k, v in (("w1", w1), ("b1", b1))]
        w2p = rt.pack_conv_weight(r.put("w2", w2), out=r.out("w2_packed", (64, 3, 3, 64)))
        args += [w2, r.put("b2", b2), r.put("w3", w3), r.put("b3", b3)]
        kw = dict(res=None if merged else xd, relu_in=merged, x_coff=64 if merged else 0, w2_packed=w2p)
        if case == "28c_into_slice":
            ybuf = r.out("y", (n, 14, 14, 352))
            rt.bottleneck_chain14(xd, *args, y=ybuf, y_coff=64, **kw)
            r.must_stay(ybuf[..., :64], "y channels 0..63")
            r.must_stay(ybuf[..., 320:], "y channels 320..351")
            return {"y[64:320]": ybuf[..., 64:320]}
        return {"y": rt.bottleneck_chain14(xd, *args, y=r.out("y", (n, 14, 14, 256)), **kw)}
    two_runs(body)


@pytest.mark.parametrize("case", CHAIN_CASES)
@pytest.mark.parametrize("n", NS)
def test_bottleneck_chain14_split(rt, case, n):
    """offk_bottleneck_chain14_split (stores y and loads res through raw pointers): the branch form of 28a, the residual form, output
    into a channel slice; scratch at exactly the header's 6 * (64 * Cin + 64 * 576 + 2 * 256 * 64) bytes."""
    branch = case == "28a"
    x, w1, b1, w2, b2, w3, b3, wb, bb = chain_inputs("28a_branch" if branch else case, n, "normal", 300 + n)
    Cin = 64 if branch else 256

    def body(r):
        xd = r.put("x", x)
        args = [r.put(k, v) for k, v in (("w1", w1), ("b1", b1))]
        w2p = rt.pack_conv_weight(r.put("w2", w2), out=r.out("w2_packed", (64, 3, 3, 64)))
        args += [w2, r.put("b2", b2), r.put("w3", w3), r.put("b3", b3)]
        kw = dict(res=None if branch else xd, branch=(r.put("branch_w", wb), r.put("branch_b", bb)) if branch else None, relu_in=branch,
                  x_coff=64 if branch else 0, w2_packed=w2p,
                  scratch=r.out("scratch", (6 * (64 * Cin + 64 * 576 + 2 * 256 * 64),), torch.uint8))
        if case == "28c_into_slice":
            ybuf = r.out("y", (n, 14, 14, 352))
            rt.bottleneck_chain14_split(xd, *args, y=ybuf, y_coff=64, **kw)
            r.must_stay(ybuf[..., :64], "y channels 0..63")
            r.must_stay(ybuf[..., 320:], "y channels 320..351")
            return {"y[64:320]": ybuf[..., 64:320]}
        return {"y": rt.bottleneck_chain14_split(xd, *args, y=r.out("y", (n, 14, 14, 256)), **kw)}
    two_runs(body)


@pytest.mark.parametrize("ci,co", [(128, 128), (832, 256)])
@pytest.mark.parametrize("n", NS)
def test_winograd_conv3x3(rt, ci, co, n):
    """offk_winograd_conv3x3 with the 14b epilogue and the per-tile sums: scratch at exactly 121 * (Co Ci + n (Ci + Co)) floats, the
    pool carve at [4 n][Co]."""
    g = torch.Generator().manual_seed(7 * ci + co + n)
    x = randn(g, n, 7, 7, ci + 32).clamp_min(0)
    w, b = randn(g, co, ci, 3, 3, scale=(9 * ci) ** -0.5), randn(g, co, scale=(9 * ci) ** -0.5)
    res = randn(g, n, 7, 7, co, scale=0.3).clamp_min(0)

    def body(r):
        wp = rt.pack_conv_weight(r.put("w", w), out=r.out("w_packed", (co, 3, 3, ci)))
        y, pool = rt.winograd_conv3x3(r.put("x", x), w, r.put("bias", b), res=r.put("res", res), flags=2 | 4, x_coff=32, y=r.out("y", (n, 7, 7, co)),
                                      want_pool=True, w_packed=wp, scratch=r.out("scratch", (121 * (co * ci + n * (ci + co)),)),
                                      pool=r.out("pool", (4 * n, co)))
        return {"y": y, "pool": pool}
    two_runs(body)


@pytest.mark.parametrize("n", NS)
def test_winograd_conv5x5s2(rt, n):
    ci, co = 64, 64
    g = torch.Generator().manual_seed(11 * ci + co)
    x = randn(g, n, 14, 14, ci + 32).clamp_min(0)
    w, b = randn(g, co, ci, 5, 5, scale=(25 * ci) ** -0.5), randn(g, co, scale=(25 * ci) ** -0.5)

    def body(r):
        wp = rt.pack_conv_weight(r.put("w", w), out=r.out("w_packed", (co, 5, 5, ci)))
        ybuf = r.out("y", (n, 7, 7, co + 96))
        rt.winograd_conv5x5s2(r.put("x", x), w, r.put("bias", b), flags=2, x_coff=32, y=ybuf, y_coff=96, w_packed=wp,
                              scratch=r.out("scratch", (400 * ci * (co + n) + 121 * n * co,)))
        r.must_stay(ybuf[..., :96], "y channels 0..95")
        return {"y[96:]": ybuf[..., 96:]}
    two_runs(body)


@pytest.mark.parametrize("n", NS)
def test_winograd_conv7x7s2(rt, n):
    ci, co = 32, 64
    g = torch.Generator().manual_seed(7 * ci + co)
    x = randn(g, n, 28, 28, ci + 32).clamp_min(0)
    w, b = randn(g, co, ci, 7, 7, scale=(49 * ci) ** -0.5), randn(g, co, scale=(49 * ci) ** -0.5)

    def body(r):
        wp = rt.pack_conv_weight(r.put("w", w), out=r.out("w_packed", (co, 7, 7, ci)))
        ybuf = r.out("y", (n, 14, 14, co + 64))
        rt.winograd_conv7x7s2(r.put("x", x), w, r.put("bias", b), x_coff=32, y=ybuf, y_coff=64, w_packed=wp,
                              scratch=r.out("scratch", (225 * ci * (co + 9 * n) + 64 * 9 * n * co,)))
        r.must_stay(ybuf[..., :64], "y channels 0..63")
        return {"y[64:]": ybuf[..., 64:]}
    two_runs(body)


BETWEEN = [(128, 4, True, "fp32"), (256, 1, True, "fp32"), (128, 1, False, "fp32"), (128, 4, True, "f32split"), (256, 1, True, "f32split")]


@pytest.mark.parametrize("cin,phases,gemm,prec", BETWEEN)
@pytest.mark.parametrize("n", NS)
def test_winograd_between(rt, cin, phases, gemm, prec, n):
    """offk_winograd_between / _ex: V, the activation stored into a channel slice of a wider carve, and (split-fp32) scratch at
    exactly Cmid * Cin * 6 bytes."""
    g = np.random.default_rng(1000 * cin + 10 * phases + n)
    M = torch.from_numpy(g.standard_normal((121, n, cin)).astype(np.float32))
    bias = torch.from_numpy((g.standard_normal(cin) * 0.5).astype(np.float32))
    w1 = torch.from_numpy((g.standard_normal((cin, cin)) / cin ** 0.5).astype(np.float32)) if gemm else None
    b1 = torch.from_numpy((g.standard_normal(cin) * 0.1).astype(np.float32)) if gemm else None

    def body(r):
        xbuf = r.out("x", (n, 7, 7, cin + 64))
        kw = dict(scratch=r.out("scratch", (cin * cin * 6,), torch.uint8)) if prec == "f32split" else {}
        V = rt.winograd_between(r.put("M", M), r.put("bias_in", bias), phases, r.put("w1", w1) if gemm else None, r.put("b1", b1) if gemm else None,
                                x=xbuf, x_coff=32, precision=prec, V=r.out("V", (121, n, cin)), **kw)
        r.must_stay(xbuf[..., :32], "x channels 0..31")
        r.must_stay(xbuf[..., 32 + cin:], "x channels behind the slice")
        return {"V": V, "x[slice]": xbuf[..., 32:32 + cin]}
    two_runs(body)


@pytest.mark.parametrize("prec", ["fp32", "f32split"])
@pytest.mark.parametrize("batch,M,K,Co", [(3, 100, 128, 128), (7, 64, 64, 512), (4, 245, 256, 64), (2, 245, 832, 256)])
def test_batched_gemm_nt(rt, batch, M, K, Co, prec):
    """offk_batched_gemm_nt (96- / 128-row items over M rows): y at [batch][M][Co], scratch at exactly batch * Co * K * 6 bytes."""
    g = torch.Generator().manual_seed(batch * 1000 + M + K + Co)
    x, w = randn(g, batch, M, K).clamp_min(0), randn(g, batch, Co, K, scale=K ** -0.5)

    def body(r):
        kw = dict(scratch=r.out("scratch", (batch * Co * K * 6,), torch.uint8)) if prec == "f32split" else {}
        return {"y": rt.batched_gemm_nt(r.put("x", x), r.put("w", w), prec, y=r.out("y", (batch, M, Co)), **kw)}
    two_runs(body)


@pytest.mark.parametrize("C,H,maxpool", [(256, 14, True), (512, 7, False), (1024, 7, False)])
@pytest.mark.parametrize("n", NS)
def test_head(rt, n, C, H, maxpool):
    g = torch.Generator().manual_seed(9)
    x, w, b = randn(g, n, H, H, C + 64), randn(g, 101, C, scale=C ** -0.5), randn(g, 101)
    two_runs(lambda r: {"out": rt.head(r.put("x", x), r.put("fc_w", w), r.put("fc_b", b), maxpool, x_coff=32, c=C, out=r.out("out", (n, 101)))})


def test_segment_consensus_and_backward(rt):
    g = torch.Generator().manual_seed(10)
    x, go = randn(g, 5 * 3, 101), randn(g, 5, 101)
    two_runs(lambda r: {"out": rt.segment_consensus(r.put("x", x), 5, out=r.out("out", (5, 101))),
                        "grad_in": rt.segment_consensus_backward(r.put("grad_out", go), 3, out=r.out("grad_in", (15, 101)))})


@pytest.mark.parametrize("n", NS)
def test_layout_helpers(rt, n):
    """C = 37, HW = 35: no multiple of anything."""
    g = torch.Generator().manual_seed(0)
    x = randn(g, n, 37, 7, 5)

    def body(r):
        y = rt.nchw_to_nhwc(r.put("x", x), out=r.out("nhwc", (n, 7, 5, 37)))
        z = rt.nhwc_to_nchw(y, coff=5, c=20, out=r.out("nchw", (n, 20, 7, 5)))
        return {"nhwc": y, "nchw": z}
    a, _b = two_runs(body)
    assert torch.equal(a["nhwc"].cpu(), x.permute(0, 2, 3, 1).contiguous()) and torch.equal(a["nchw"].cpu(), x[:, 5:25].contiguous())


def test_score_fusion(rt):
    g = torch.Generator().manual_seed(12)
    sets = [randn(g, 5, 10, 101) for _ in range(3)]

    def body(r):
        fused, pred = rt.score_fusion([r.put("scores_%d" % i, s) for i, s in enumerate(sets)], [1.0, 1.5, 1.6],
                                      out=(r.out("fused", (5, 101)), r.out("pred", (5,), torch.int32)))
        return {"fused": fused, "pred": pred}
    two_runs(body)
