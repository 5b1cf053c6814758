"""The OFF units and the whole forward at a batch whose largest feature map is past 2 GiB: B = 306 clips of L = 7 frames (N = 2142 frames, P = 1836 pairs),
RGB, per-clip slicing, an fp32 and a split-fp32 handle.  Site 3b is 2142 x 320 x 28 x 28 x 4 B = 2.15 GB, past the 0x7fffff00 mark
at which the units' kernels leave their buffer-descriptor loaders; every other map is below it.  None of the kernels that then run
had run in the suite before:

  launch                       below the mark                                         at N = 2142 (read in csrc/ before the first run)
  ---------------------------  -----------------------------------------------------  -----------------------------------------------------------
  K1  offk_pw_reduce,          pw_reduce_kernel<0, 1>: buffer descriptors per part     pw_reduce_kernel<0, 0> (pw_reduce.hip:423-430, :465-478):
      offk_off_units           (pw_reduce.hip:198-201)                                 pointer loads, (size_t)frame * cpart ... (:206-227); G and D
                                                                                       stores (size_t)m * 128, (size_t)dr * HW (:409-415)
  K1T offk_off_units_fused,    fp32 handle: pw_tdiff16_kernel; split handle:           BOTH handles: pw_tdiff_kernel<0, 0> in the 32-pixel block
      offk_forward             pw_tdiff_split_kernel (pw_tdiff.hip:676, :732)          layout (pw_tdiff.hip:663-676, :730): `lean` is one flag per
                                                                                       launch, so all nine sites take it; pointer loads (size_t)
                                                                                       (b L + t) * cpart (:149-152), stores (size_t) (:281-303).
                                                                                       A split-fp32 handle therefore computes its units in fp32
                                                                                       arithmetic as soon as one map part has 2 GiB or more.
  K2  sobel_tdiff              one kernel on either side; every index is size_t (sobel_tdiff.hip:148-200, :221-293)

In per-clip mode a clip's unit outputs depend on its own frames only, so the reference is the fp64-accurate oracle
(oracle/off_oracle.py) run on single clips: clip 0, the middle clip, clip B - 2 (the last one wholly below byte 2^31 of the 3b map) and the last clip -- whose
frames 2139 .. 2141 are the ones that hold and follow byte 2^31 (2^31 / 1 003 520 B = 2139.9), so "the straddling clip" and "the last
clip" are the same one at this N.

Which K1T kernel ran cannot be read from the per-launch trace: "units:pw_tdiff (K1T)" is marked once, before pw_tdiff_launch picks among
pw_tdiff16_kernel, pw_tdiff_split_kernel and pw_tdiff_kernel<0, 0> (offk_api.hip:583, pw_tdiff.hip:727-735); the trace shows K1T against
K1 + K2 only.  The bits show the rest: with the whole 3b map both handle kinds must write the SAME bits into fusion_28 (one fp32 kernel),
with the maps as parts the split handle's bits must differ from the fp32 handle's (its own split-fp32 kernel ran).  Tolerance: RTOL of tests/forward.py, max-normalised as test_pw_reduce_vs_oracle and the stage-tensor tests have it.

The 3b map and the workspace each sit behind a 2 GiB margin of arena.SENTINEL inside their own allocation (tests/big.py has the
reasoning: a byte offset wrapped as int32 lands there, changes a sentinel or reads a NaN, and faults nothing); both margins must be
intact after every call.  Device memory of the module, asserted to fit with 10 % to spare before anything is allocated and printed:
the nine maps 9.7 GB + the guarded copy of 3b 4.3 GB (2.15 GB of it the margin) + workspace and margin + the generator's temporaries.

offk_forward at the same N is the first run of the fusion stage with Winograd arrays past 4 GiB (V of the 7x7 / 2 conv is
225 x 9 P x 320 x 4 B = 4.76 GB at P = 1836).  Read before it ran: the transforms index V / M / x / y with size_t (winograd.hip:44-69,
:116-142, winograd7.hip:91-102, :170, wino_mid.hip:66-144); the fp32 batched GEMM builds one buffer descriptor PER PROBLEM from a 64-bit
problem offset, its per-problem extents checked below 0x7fffff00 (wino_gemm.hip:90-96, :155, :208-215); the split GEMM takes whole-array
descriptors only while every array is below 0x7fffff00 bytes and otherwise hands over to the fp32 one (wino_gemm_split.hip:378-387);
the direct convs, chains and heads are the kernels of tests/test_gpu_big_slabs.py (fusion_14 at P = 1836 is 1.52 GB, below the chains'
refusal).  Logits and stage tensors of the checked clips against the oracle's single-clip forward.

offk_forward_parts with spec.SITE_PARTS at the same N: every part is below the mark (the widest, 96 channels of 3b, is 0.64 GB), so the
buffer-descriptor kernels run -- pw_tdiff16_kernel on the fp32 handle and pw_tdiff_split_kernel on the split one, one descriptor per
part, extents below 0x7fffff00 by the same check, stores (size_t) (pw_tdiff.hip:407-410, :557-587; pw_tdiff_split.hip:112-115, :343-374).

The training side of the units on the same fp32 maps (offk_off_units_train, offk_off_units_backward, offk_off_units_backward_feats):
test_units_training_side_at_n_2142, whose docstring has the index widths of units_bwd.hip and units_dx.hip.  16-bit maps of 2 GiB:
tests/test_gpu_big_batch16.py.
"""
import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

from . import arena, big, featmaps
from .big import guarded, margin_intact
from .forward import RTOL, RTOL_NORTH_STAR, STAGES, check_whole_forward, rel_err, signal_err

pytestmark = pytest.mark.gpu
B, L = 306, 7
N, P = B * L, B * (L - 1)
MARGIN = big.FRONT_MARGIN
SITE_3B = 1
PRECS = ["fp32", "f32split"]


class World:
    pass


@pytest.fixture(scope="module")
def world():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from offk_amd import runtime as rt
    wd = World()
    weights = synth.make_weights(spec.VARIANT_RGB)
    wd.w = orc.to_torch_weights(weights)
    wd.h = {}
    for prec in PRECS:
        h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, False, precision=prec)
        assert h.load_state_dict(weights) == []
        wd.h[prec] = h
    ws_bytes = max(h.workspace_bytes for h in wd.h.values())
    map_bytes = [N * C * H * H * 4 for _n, C, H in spec.SITES]
    assert map_bytes[SITE_3B] >= 0x7fffff00 and max(b for i, b in enumerate(map_bytes) if i != SITE_3B) < 0x7fffff00
    # the maps, the guarded copy of 3b, the workspace behind its margin, G and D of 3b for the stage entry, and the generator's
    # temporaries (randn + relu of the largest map), the maps once more as their inception branches
    # (test_forward_parts_at_n_2142) or as the map gradients of the training case
    need = 3 * sum(map_bytes) + MARGIN + map_bytes[SITE_3B] + MARGIN + ws_bytes + N * 784 * 160 * 4 + 2 * map_bytes[SITE_3B]
    free = torch.cuda.mem_get_info()[0]
    print("big batch B = %d L = %d: workspace %.2f GB, maps %.2f GB, in all %.2f GB of %.2f GB free"
          % (B, L, ws_bytes / 1e9, sum(map_bytes) / 1e9, need / 1e9, free / 1e9))
    assert need * 1.1 < free, "B = %d needs %.1f GB of device memory with its margins, %.1f GB are free" % (B, need / 1e9, free / 1e9)
    wd.need = need
    wd.x = featmaps.relu_maps(B, L, torch.float32, 0xB16)
    wd.x3b_words, payload = guarded(map_bytes[SITE_3B])
    guarded_3b = payload.view(torch.float32).view(N, 320, 28, 28)
    guarded_3b.copy_(wd.x[SITE_3B])
    wd.x[SITE_3B] = guarded_3b
    wd.ws_words, wd.ws = guarded(ws_bytes)
    for h in wd.h.values():
        h.set_workspace(wd.ws)
    torch.cuda.empty_cache()
    # the frame that holds byte 2^31 of the 3b map lies in the last clip at this N
    frame = 2 ** 31 // (320 * 784 * 4)
    assert frame // L == B - 1 and frame < N
    wd.clips = (0, B // 2, B - 2, B - 1)                             # B - 2: the last clip wholly below byte 2^31 of the 3b map
    wd.units = {}                                                     # (clip, site) -> the oracle's [L - 1, 160, H, H]
    wd.fwd = {}                                                       # clip -> the oracle's ((fc7, fc14, fc28), stages) of that clip alone
    yield wd
    del wd.x, wd.ws, wd.ws_words, wd.x3b_words, wd.h, guarded_3b, payload
    torch.cuda.empty_cache()


def clip_frames(wd, site, c):
    return wd.x[site][c * L:(c + 1) * L].cpu()


def oracle_unit(wd, site, c):
    if (c, site) not in wd.units:
        with torch.no_grad():
            wd.units[(c, site)] = orc.off_unit(clip_frames(wd, site, c), wd.w, spec.SITES[site][0], 1, L, spec.VARIANT_RGB, orc.SLICE_PER_CLIP,
                                               None, None)
    return wd.units[(c, site)]


def check_margins(wd):
    assert margin_intact(wd.x3b_words), "the 2 GiB in front of the 3b map changed"
    assert margin_intact(wd.ws_words), "the 2 GiB in front of the workspace changed"


@pytest.mark.parametrize("prec", PRECS)
def test_pw_reduce_site_3b_past_2_gib(world, prec):
    """offk_pw_reduce on the one map past the mark: the pointer-loader form of K1.  G (ReLU of the 128-channel reduce of every frame) and D
    (the 32-channel reduce of each clip's first L - 1 frames) of the checked clips against fp64; every row of G and D is written."""
    wd, h = world, world.h[prec]
    name = spec.SITES[SITE_3B][0]
    G = torch.full((N * 784, 128), float("nan"), device="cuda")
    D = torch.full((P * 784, 32), float("nan"), device="cuda")
    h.pw_reduce(SITE_3B, wd.x[SITE_3B], G, D)
    torch.cuda.synchronize()
    assert not bool(G.isnan().any()) and not bool(D.isnan().any())
    Gv, Dv = G.view(N, 28, 28, 128), D.view(P, 28, 28, 32)
    for c in wd.clips:
        x = clip_frames(wd, SITE_3B, c).double()
        g_ref = torch.relu(F.conv2d(x, wd.w["motion_conv_gen_%s.weight" % name].double(), wd.w["motion_conv_gen_%s.bias" % name].double()))
        d_ref = F.conv2d(orc.spatial_frames(x, 1, L, orc.SLICE_PER_CLIP), wd.w["motion_spatial_down_%s.weight" % name].double(),
                         wd.w["motion_spatial_down_%s.bias" % name].double())
        eg = rel_err(Gv[c * L:(c + 1) * L].permute(0, 3, 1, 2), g_ref)
        ed = rel_err(Dv[c * (L - 1):(c + 1) * (L - 1)].permute(0, 3, 1, 2), d_ref)
        print("pw_reduce 3b %s clip %d: G %.2e D %.2e" % (prec, c, eg, ed))
        assert eg < RTOL and ed < RTOL, (c, eg, ed)
    check_margins(wd)
    del G, D
    torch.cuda.empty_cache()


def clip_rows_28(wd, h):
    rows = torch.cat([torch.arange(c * (L - 1), (c + 1) * (L - 1)) for c in wd.clips]).cuda()
    return h.region("fusion_28", 320).view(P, 28, 28, 320)[rows].clone()


def run_units(wd, h, fused):
    wd.ws_words[MARGIN // 4:].fill_(arena.SENTINEL)                    # NaN in every float: what the units leave unwritten shows
    h.set_profiling(2)
    (h.off_units_fused if fused else h.off_units)(wd.x)
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    return names


@pytest.mark.parametrize("fused", [False, True], ids=["off_units", "off_units_fused"])
@pytest.mark.parametrize("prec", PRECS)
def test_units_at_all_nine_sites(world, prec, fused):
    """offk_off_units (K1 + K2) and offk_off_units_fused (K1T + the S-blocks of K2): the 160 unit channels of every site in
    fusion_28 / 14 / 7, for the checked clips, against the oracle -- the pointer-loader kernels at all nine site shapes."""
    wd, h = world, world.h[prec]
    names = run_units(wd, h, fused)
    if fused:
        assert "units:pw_tdiff (K1T)" in names and not any("pw_reduce" in n for n in names), names
    else:
        assert "units:pw_reduce (K1)" in names and "units:sobel_tdiff (K2)" in names and not any("K1T" in n for n in names), names
    worst = {}
    for fkey, fd in spec.FUSION.items():
        width = 160 * len(fd["sites"]) + fd["carry"]
        buf = h.region("fusion_" + fkey, width).view(P, fd["H"], fd["H"], width)
        for i, sname in enumerate(fd["sites"]):
            site = spec.SITE_NAMES.index(sname)
            for c in wd.clips:
                got = buf[c * (L - 1):(c + 1) * (L - 1), :, :, 160 * i:160 * i + 160].permute(0, 3, 1, 2)
                assert not bool(got.isnan().any()), (sname, c)
                worst[(sname, c)] = rel_err(got, oracle_unit(wd, site, c))
    print("units %s %s: largest error %.2e at %s" % (prec, "fused" if fused else "K1 + K2", max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) < RTOL, worst
    check_margins(wd)


def oracle_forward(wd, c):
    if c not in wd.fwd:
        with torch.no_grad():
            wd.fwd[c] = orc.off_forward([clip_frames(wd, s, c) for s in range(spec.NUM_SITES)], wd.w, 1, L, spec.VARIANT_RGB, orc.SLICE_PER_CLIP,
                                        consensus=False, return_stages=True)
    return wd.fwd[c]


@pytest.mark.parametrize("prec", PRECS)
def test_forward_at_n_2142(world, prec):
    """offk_forward with the 3b map past 2 GiB and the Winograd arrays past 4 GiB: the three logit sets and the stage tensors
    (offk_stage_tensors fills sum_7) of the checked clips against the oracle, with the bounds of the B = 64 tests; every logit row is
    written."""
    wd, h = world, world.h[prec]
    wd.ws_words[MARGIN // 4:].fill_(arena.SENTINEL)
    outs = h.forward(wd.x, out=tuple(torch.full((P, spec.NUM_CLASSES), float("nan"), device="cuda") for _ in range(3)))
    torch.cuda.synchronize()
    for o in outs:
        assert tuple(o.shape) == (P, spec.NUM_CLASSES) and not bool(o.isnan().any())
    rows = torch.cat([torch.arange(c * (L - 1), (c + 1) * (L - 1)) for c in wd.clips]).cuda()
    refs = [oracle_forward(wd, c) for c in wd.clips]
    want = [torch.cat([r[0][k] for r in refs]) for k in range(3)]
    stages = dict((name, torch.cat([r[1][name] for r in refs])) for name, _ch, _H in STAGES)
    check_whole_forward(h, [o[rows] for o in outs], None, wd.w, "forward %s at N = %d" % (prec, N), rows=rows, oracle_run=(want, stages))
    check_margins(wd)


def make_parts(wd):
    """the nine maps as contiguous copies of their inception branches (spec.SITE_PARTS), every part below the mark"""
    parts = []
    for f, widths in zip(wd.x, spec.SITE_PARTS):
        assert sum(widths) == f.shape[1]
        off, grp = 0, []
        for wdt in widths:
            grp.append(f[:, off:off + wdt].contiguous())
            assert grp[-1].numel() * 4 < 0x7fffff00
            off += wdt
        parts.append(grp)
    return parts


def test_which_units_kernel_ran_is_told_by_the_bits(world):
    """The trace has one name for the three K1T kernels, so the bits say which ran.  Whole maps (3b past the mark): both handle kinds
    take pw_tdiff_kernel<0, 0>, an fp32 kernel -- fusion_28 of the checked clips is bit-equal between them.  Parts (all below the mark):
    the split handle takes pw_tdiff_split_kernel, whose sums are rounded differently -- its bits differ from the fp32 handle's."""
    wd = world
    got = {}
    for feats_kind, feats in (("whole", wd.x), ("parts", make_parts(wd))):
        for prec in PRECS:
            wd.ws_words[MARGIN // 4:].fill_(arena.SENTINEL)
            wd.h[prec].forward(feats)
            torch.cuda.synchronize()
            got[(feats_kind, prec)] = clip_rows_28(wd, wd.h[prec])
            assert not bool(got[(feats_kind, prec)].isnan().any())
        del feats
    torch.cuda.empty_cache()
    assert torch.equal(got[("whole", "fp32")], got[("whole", "f32split")]), "whole 2 GiB map: the split handle did not run the fp32 fallback kernel"
    assert not torch.equal(got[("parts", "fp32")], got[("parts", "f32split")]), "parts below the mark: the split handle did not run its own kernel"
    print("fp32 handle, fusion_28 from parts bit-equal to fusion_28 from whole maps: %s" % torch.equal(got[("parts", "fp32")], got[("whole", "fp32")]))
    check_margins(wd)


@pytest.mark.parametrize("prec", PRECS)
def test_forward_parts_at_n_2142(world, prec):
    """The maps handed over as their inception branches: no part reaches the mark, so the units run in the handle's own kernels at
    N = 2142 (the split-fp32 kernel on the split handle).  The three clips against the oracle within RTOL, and against the
    concatenated call's logits within twice that."""
    wd, h = world, world.h[prec]
    parts = make_parts(wd)
    wd.ws_words[MARGIN // 4:].fill_(arena.SENTINEL)
    whole = [o.clone() for o in h.forward(wd.x)]
    wd.ws_words[MARGIN // 4:].fill_(arena.SENTINEL)
    h.set_profiling(2)
    outs = h.forward(parts)
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    assert "units:pw_tdiff (K1T)" in names, names
    rows = torch.cat([torch.arange(c * (L - 1), (c + 1) * (L - 1)) for c in wd.clips]).cuda()
    refs = [oracle_forward(wd, c) for c in wd.clips]
    for k, name in enumerate(("fc7", "fc14", "fc28")):
        assert not bool(outs[k].isnan().any())
        want = torch.cat([r[0][k] for r in refs])
        e, sg, ew = rel_err(outs[k][rows], want), signal_err(outs[k][rows], want), rel_err(outs[k][rows], whole[k][rows])
        print("forward_parts %s %s at N = %d: error %.2e, signal error %.2e, against the concatenated call %.2e" % (prec, name, N, e, sg, ew))
        assert e < RTOL and sg < RTOL_NORTH_STAR and ew < 2 * RTOL, (name, e, sg, ew)
    check_margins(wd)
    del parts, whole, outs
    torch.cuda.empty_cache()


# ---- the training side of the units on fp32 maps at N = 2142 ----------------------------------------------------------------------
DROP_SEED, DROP_P = 7, 0.8


def keep_rows(seed, site_index, first_pair, npairs, H, p):
    """synth.dropout_keep for pairs first_pair .. first_pair + npairs - 1 only: the draws are indexed by (pair, pixel, quad), so a
    clip's part of the mask is a window of the stream (the whole mask at P = 1836 would be 150 M draws)"""
    import numpy as np
    hw = H * H
    x = synth.raw_u64(synth.dropout_stream(seed, site_index), first_pair * hw * 8, npairs * hw * 8).reshape(npairs, hw, 8)
    thr = np.uint64(synth.dropout_threshold(p))
    keep = np.empty((npairs, hw, 8, 4), dtype=bool)
    for c in range(4):
        keep[..., c] = ((x >> np.uint64(16 * c)) & np.uint64(0xFFFF)) >= thr
    return torch.from_numpy(np.ascontiguousarray(keep.reshape(npairs, H, H, 32).transpose(0, 3, 1, 2)))


def test_keep_rows_is_a_window_of_the_whole_mask():
    for si, H in ((1, 28), (8, 7)):
        whole = torch.from_numpy(synth.dropout_keep(DROP_SEED, si, 12, H, DROP_P))
        assert torch.equal(keep_rows(DROP_SEED, si, 6, 6, H, DROP_P), whole[6:])


def test_units_training_side_at_n_2142(world):
    """offk_off_units_train + offk_off_units_backward + offk_off_units_backward_feats on the fp32 maps with 3b past 2 GiB.  Read first:
    K1 / K2 as above with the dropout draw index (unsigned long long)pair * HW (sobel_tdiff.hip:286); units_bwd.hip's K2b and K1b index
    with (size_t)frame * HW, (size_t)frame * xfs (:99-104, :141-203, :369-431); units_dx.hip with (size_t)row * C, ((size_t)ef * C + c) *
    HW (:112-240); no buffer descriptor in either.
    The output gradients are non-zero in the checked clips only, so the reference is the oracle on those clips as a batch of their
    own (per-clip slicing; their windows of the dropout mask; the device's own ReLU decisions, checked against the oracle's as
    tests/test_gpu_backward.py does): every unit-parameter gradient within that file's RTOL, the feature-map gradient of the checked
    clips within it too, and the feature-map gradient of EVERY other clip exactly zero."""
    from offk_amd import runtime as rt
    from .units_grad import RTOL as RTOL_GRAD
    wd = world
    h = rt.OffForward(B, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, False, precision="fp32", training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    free = torch.cuda.mem_get_info()[0]
    more = h.workspace_bytes + N * 4 * (784 * 576 + 196 * 2944 + 49 * 2048) + P * 4 * (784 * 320 + 196 * 800 + 49 * 320)
    print("training side at N = %d: train workspace %.2f GB, %.2f GB more of %.2f GB free" % (N, h.workspace_bytes / 1e9, more / 1e9, free / 1e9))
    assert more * 1.1 < free, "the training case needs %.1f GB more, %.1f GB are free" % (more / 1e9, free / 1e9)
    ws_words, ws = guarded(h.workspace_bytes)
    h.set_workspace(ws)
    clips = wd.clips
    nc, Ps = len(clips), len(clips) * (L - 1)
    frames = torch.cat([torch.arange(c * L, (c + 1) * L) for c in clips])
    pairs = torch.cat([torch.arange(c * (L - 1), (c + 1) * (L - 1)) for c in clips])
    h.off_units_train(wd.x, DROP_SEED, DROP_P)
    torch.cuda.synchronize()
    tf, drops, masks, dm = [], [], [], []
    gen = torch.Generator().manual_seed(0xD16)
    for si, (site, C, H) in enumerate(spec.SITES):
        x = wd.x[si][frames.cuda()].cpu()
        tf.append(x)
        drops.append(torch.cat([keep_rows(DROP_SEED, si, c * (L - 1), L - 1, H, DROP_P) for c in clips]).float() / (1.0 - DROP_P))
        G = h.region("G_" + site, 128).view(N, H * H, 128)[frames.cuda()].permute(0, 2, 1).reshape(nc * L, 128, H, H).cpu()
        assert not bool(G.isnan().any())
        with torch.no_grad():
            pre = F.conv2d(x, wd.w["motion_conv_gen_%s.weight" % site], wd.w["motion_conv_gen_%s.bias" % site])
        flip = (G > 0) != (pre > 0)
        assert int(flip.sum()) <= 5 + 1e-5 * flip.numel(), site
        if flip.any():
            assert float(pre[flip].abs().max()) < 1e-5 * max(1.0, float(pre.abs().max())), site
        masks.append((G > 0).float())
        dm.append(torch.randn(Ps, 160, H, H, generator=gen))
    # the training forward itself: [dropout(S) | T] of the checked clips
    with torch.no_grad():
        m28 = orc.off_unit(tf[1], wd.w, "3b", nc, L, spec.VARIANT_RGB, orc.SLICE_PER_CLIP, drops[1])
    f28 = h.region("fusion_28", 320).view(P, 28, 28, 320)[pairs.cuda()].permute(0, 3, 1, 2)
    assert rel_err(f28[:, 160:], m28) < RTOL
    # gradient buffers: zero everywhere but in the checked clips
    bufs = [torch.zeros(P, H, H, width, device="cuda") for H, width in ((28, 320), (14, 800), (7, 320))]
    views = [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]
    for si in range(spec.NUM_SITES):
        buf, coff = views[si]
        buf[pairs.cuda(), :, :, coff:coff + 160] = dm[si].permute(0, 2, 3, 1).cuda()
    _flat, got = h.off_units_backward(wd.x, views, DROP_SEED, DROP_P)
    torch.cuda.synchronize()
    ref = orc.unit_param_grads_from_dm(tf, wd.w, nc, L, spec.VARIANT_RGB, orc.SLICE_PER_CLIP, dm, drops, masks)
    assert set(got) == set(ref)
    errs = dict((k, rel_err(got[k], ref[k])) for k in ref)
    print("units backward at N = %d: largest weight-gradient error %.2e (%s)" % (N, max(errs.values()), max(errs, key=errs.get)))
    bad = dict((k, "%.2e" % e) for k, e in errs.items() if not e < RTOL_GRAD or got[k].shape != ref[k].shape)
    assert not bad, bad
    # the feature-map gradient
    dx = h.off_units_backward_feats()
    torch.cuda.synchronize()
    other = torch.ones(N, dtype=torch.bool)
    other[frames] = False
    other = other.cuda()
    worst = 0.0
    for si, (site, C, H) in enumerate(spec.SITES):
        assert tuple(dx[si].shape) == (N, C, H, H)
        nz = int((dx[si][other] != 0).sum())
        assert nz == 0, "%s: %d non-zero feature-map gradients in clips that had no output gradient" % (site, nz)
        xr = tf[si].clone().requires_grad_(True)
        m = orc.off_unit(xr, wd.w, site, nc, L, spec.VARIANT_RGB, orc.SLICE_PER_CLIP, drops[si], masks[si])
        (m * dm[si]).sum().backward()
        worst = max(worst, rel_err(dx[si][frames.cuda()], xr.grad))
    print("units backward at N = %d: largest feature-map gradient error %.2e" % (N, worst))
    assert worst < RTOL_GRAD
    assert margin_intact(ws_words), "the 2 GiB in front of the training workspace changed"
    check_margins(wd)
    del ws, ws_words, bufs, views, dx, h, f28
    torch.cuda.empty_cache()
