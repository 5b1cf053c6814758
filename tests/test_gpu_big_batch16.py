"""16-bit feature maps of 2 GiB: B = 612 clips of L = 7 frames, where site 3b as bf16 / fp16 is 4284 x 320 x 28 x 28 x 2 B = 2.15 GB.

  the training side (offk_pw_reduce_typed, offk_off_units_typed, offk_off_units_train_typed, offk_off_units_backward_typed) refuses such
      a map before it enqueues anything and writes nothing: check_feat_train (offk_api.hip:725-740), "16-bit feature maps of 2 GiB or
      more are not supported (site 3b)".  The check is a function of the handle's N and the site's shape; the maps, the workspace and
      the gradient views are nevertheless real and of the full size, so that a library that did NOT refuse would stay inside them.
  the inference side (offk_forward_typed on a split-fp32 handle) RUNS: the 16-bit units kernel is a pointer loader,
      ((size_t)frame * cpart + kl + 8 g) * HW + px (pw_tdiff_f16.hip:39-56), its stores (size_t)(pair0 + j) * HW ... * m_cs
      (pw_tdiff_staged.h:231-256), no buffer descriptor anywhere in pw_tdiff_f16.hip, pw_tdiff_cl.hip (size_t it_row * cpart, :47-57) or
      pw_tdiff_staged.h.  At P = 3672 fusion_28 (3.7 GB) and fusion_14 (3.0 GB) are past 2 GiB as well: their readers and writers are the
      kernels of tests/test_gpu_big_slabs.py (pointer loaders and stores, the fp32 chain for 28c), the Winograd V array is 9.5 GB
      (winograd7.hip:127 and :150 index it with size_t, one GEMM descriptor per problem).

A module of its own so that the buffers of tests/test_gpu_big_batch.py are gone when these are made: about 70 GB at the peak, asserted
to fit with 10 % to spare and printed.
"""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import arena, featmaps
from .arena import sentinel_floats, untouched

pytestmark = pytest.mark.gpu
L = 7
SITE_3B = 1


# ---- the training side ----
B16 = 612                                                                 # N = 4284 frames: 3b as a 16-bit map is 2.15 GB
REFUSAL_16 = r"error -1: offk_\w+: 16-bit feature maps of 2 GiB or more are not supported \(site 3b\)"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_training_entries_refuse_16_bit_maps_of_2_gib(dtype):
    """offk_pw_reduce_typed, offk_off_units_typed, offk_off_units_train_typed and offk_off_units_backward_typed at B = 612: the documented
    OFFK_ERR_INVALID, and not a word of the workspace, of G / D or of the gradient buffer is written.  The maps, the workspace and the
    gradient views are real and of the full size: a library that did NOT refuse would stay inside them."""
    from offk_amd import _lib, runtime as rt
    Nb, Pb = B16 * L, B16 * (L - 1)
    assert Nb * 320 * 784 * 2 >= 0x7fffff00 > Nb * 256 * 784 * 2, "3b is the only 16-bit map past the mark"
    h = rt.OffForward(B16, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, False, precision="fp32", training=True)
    assert h.load_state_dict(synth.make_weights(spec.VARIANT_RGB)) == []
    map_bytes = sum(Nb * C * H * H * 2 for _n, C, H in spec.SITES)
    gm_bytes = Pb * 4 * (784 * 320 + 196 * 800 + 49 * 320)
    gd_bytes = (Nb * 128 + Pb * 32) * 784 * 4
    need = h.workspace_bytes + map_bytes + 3 * Nb * 320 * 784 * 4 + gm_bytes + gd_bytes
    free = torch.cuda.mem_get_info()[0]
    print("16-bit maps at B = %d: train workspace %.2f GB, in all %.2f GB of %.2f GB free" % (B16, h.workspace_bytes / 1e9, need / 1e9, free / 1e9))
    assert need * 1.1 < free, "B = %d needs %.1f GB of device memory, %.1f GB are free" % (B16, need / 1e9, free / 1e9)
    x = featmaps.relu_maps(B16, L, featmaps.DTYPES16[dtype], 0xB17)
    torch.cuda.empty_cache()
    ws = torch.full(((h.workspace_bytes + 3) // 4,), arena.SENTINEL, dtype=torch.int32, device="cuda")
    h.set_workspace(ws.view(torch.uint8))
    G, D = sentinel_floats(Nb * 784, 128), sentinel_floats(Pb * 784, 32)
    bufs = [torch.zeros(Pb, H, H, width, device="cuda") for H, width in ((28, 320), (14, 800), (7, 320))]
    views = [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]
    grads = sentinel_floats(int(h.lib.offk_unit_grad_floats(h._h)))
    calls = {
        "pw_reduce": lambda: h.pw_reduce(SITE_3B, x[SITE_3B], G, D),
        "off_units": lambda: h.off_units(x),
        "off_units_train": lambda: h.off_units_train(x, 7, 0.8),
        "off_units_backward": lambda: h.off_units_backward(x, views, 7, 0.8, grads=grads),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.OffkError, match=REFUSAL_16):
            call()
        torch.cuda.synchronize()
        assert untouched(ws) and untouched(G) and untouched(D) and untouched(grads), "%s wrote something before it refused" % name
    del x, ws, G, D, bufs, views, grads, h, calls
    torch.cuda.empty_cache()


# ---- the inference side ----
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_forward_typed_on_16_bit_maps_of_2_gib(dtype):
    """offk_forward_typed on a split-fp32 handle at B = 612 (N = 4284, P = 3672): 3b as a 16-bit map is 2.15 GB, fusion_28 3.7 GB,
    fusion_14 3.0 GB (past the split chain's limit: chain 28c runs the fp32 chain), the Winograd V array 9.5 GB.  Clip 0, the middle
    clip, the last clip wholly below byte 2^31 of the 3b map and the last clip (which holds that byte) against the oracle on the
    upcast maps, with the bounds of the B = 64 tests; the 3b map and the workspace behind 2 GiB sentinel margins."""
    from offk_amd import runtime as rt
    from oracle import off_oracle as orc
    from .big import FRONT_MARGIN as MARGIN, guarded, margin_intact
    from .forward import RTOL, RTOL_NORTH_STAR, rel_err, signal_err
    Nb, Pb = B16 * L, B16 * (L - 1)
    weights = synth.make_weights(spec.VARIANT_RGB)
    h = rt.OffForward(B16, L, spec.VARIANT_RGB, spec.SLICE_PER_CLIP, False, precision="f32split")
    assert h.load_state_dict(weights) == []
    w = orc.to_torch_weights(weights)
    map_bytes = [Nb * C * H * H * 2 for _n, C, H in spec.SITES]
    assert map_bytes[SITE_3B] >= 0x7fffff00 > max(b for i, b in enumerate(map_bytes) if i != SITE_3B)
    need = sum(map_bytes) + 2 * MARGIN + map_bytes[SITE_3B] + h.workspace_bytes + 3 * Nb * 320 * 784 * 4
    free = torch.cuda.mem_get_info()[0]
    print("forward_typed at B = %d: workspace %.2f GB, in all %.2f GB of %.2f GB free" % (B16, h.workspace_bytes / 1e9, need / 1e9, free / 1e9))
    assert need * 1.1 < free, "B = %d needs %.1f GB of device memory, %.1f GB are free" % (B16, need / 1e9, free / 1e9)
    x = featmaps.relu_maps(B16, L, featmaps.DTYPES16[dtype], 0xB17)
    x3b_words, payload = guarded(map_bytes[SITE_3B])
    g3b = payload.view(featmaps.DTYPES16[dtype]).view(Nb, 320, 28, 28)
    g3b.copy_(x[SITE_3B])
    x[SITE_3B] = g3b
    torch.cuda.empty_cache()
    ws_words, ws = guarded(h.workspace_bytes)
    h.set_workspace(ws)
    h.set_profiling(2)
    outs = h.forward(x, out=tuple(torch.full((Pb, spec.NUM_CLASSES), float("nan"), device="cuda") for _ in range(3)))
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    assert any(n.startswith("units:pw_tdiff (K1T, %s maps)" % ("bf16" if dtype == "bf16" else "fp16")) for n in names), names
    frame = 2 ** 31 // (320 * 784 * 2)
    assert frame // L == B16 - 1
    clips = (0, B16 // 2, B16 - 2, B16 - 1)
    rows = torch.cat([torch.arange(c * (L - 1), (c + 1) * (L - 1)) for c in clips]).cuda()
    refs = []
    for c in clips:
        with torch.no_grad():
            refs.append(orc.off_forward([t[c * L:(c + 1) * L].float().cpu() for t in x], w, 1, L, spec.VARIANT_RGB, orc.SLICE_PER_CLIP, consensus=False,
                                        return_stages=True))
    for k, name in enumerate(("fc7", "fc14", "fc28")):
        assert not bool(outs[k].isnan().any())
        want = torch.cat([r[0][k] for r in refs])
        e, sg = rel_err(outs[k][rows], want), signal_err(outs[k][rows], want)
        print("forward_typed %s %s at N = %d: error %.2e, row-to-row signal error %.2e" % (dtype, name, Nb, e, sg))
        assert e < RTOL and sg < RTOL_NORTH_STAR, (name, e, sg)
    for name, ch, H in (("fusion_28", 320, 28), ("fusion_14", 1056, 14), ("fusion_7", 832, 7), ("sum_7", 1024, 7)):
        got = h.region(name, ch).view(Pb, H, H, ch)[rows].permute(0, 3, 1, 2)
        e = rel_err(got, torch.cat([r[1][name] for r in refs]))
        print("forward_typed %s %s at N = %d: error %.2e" % (dtype, name, Nb, e))
        assert e < RTOL, (name, e)
    assert margin_intact(x3b_words) and margin_intact(ws_words), "a 2 GiB margin changed"
    del x, g3b, payload, x3b_words, ws, ws_words, outs, h
    torch.cuda.empty_cache()
