"""The classifier heads the forward really runs, isolated from everything upstream of them.

`test_head_and_consensus` exercises `head_kernel` (the stage entry offk_head), which the forward never launches.  The forward's heads are
`maxpool_rows_kernel` + `fc_pooled_multi_kernel` in tiles mode (28-head; 14-head behind a Winograd conv), the pooling epilogues of
`conv_igemm` / `wino_gemm_split` / the Winograd output transform + `fc_pooled_multi_kernel` (slab mode: 7-head; 14-head with
OFFK_WINOGRAD=0), and `pool_kernel` + `fc_kernel` (OFFK_FOLD_POOL=0).  Until this module they were checked only through whole-forward
logits, which are bias-dominated (test_gpu_parity.signal_err): RTOL of max |logit| admits ~1 % of the signal, room enough for a head that
drops one of 49 pooled cells or mis-weights an image that straddles two 32-row slabs.

Here a forward runs, the handle's own stage tensors are read back (fusion_14[..., 800:1056], fusion_7[..., 320:832], sum_7 -- no workspace
region aliases another) and each head is recomputed in fp64 FROM THE DEVICE'S OWN INPUT, so no upstream conv error masks or excuses a head
error.  The FC weights are N(0, 1) / sqrt(C) with N(0, 0.1) biases: logits that are not bias-dominated.  Every logit obeys

    |got - ref| <= c 2^-24 (sum_c |w_c| mean|x_c| + |b|)          (28-head: mean |window max|)

A-priori ceiling: c <= C + 64 (an fp32 sum of C products, the 49 pooled cells, the slab / wave combines).  c is pinned per head at 4 x the
worst ratio measured on an MI355X over every case of this module (paths x shapes x arithmetic modes x class counts):

    head    C     ceiling   measured worst ratio   pinned c
    7      1024    1088      0.67                   2.68
    14      512     576      1.12                   4.48
    28      256     320      1.42                   5.68

(per path, worst over shapes / modes / class counts -- default: 0.64 / 1.00 / 1.29, OFFK_WINOGRAD=0: 0.67 / 1.12 / 1.42, OFFK_FOLD_POOL=0:
0.35 / 0.62 / 0.74.)  A head that ignores which of a slab's two partial sums belongs to a straddling image (fc_pooled_body: slot = 0) shows
ratios of 1.1e6 (7-head) and 2.0e6 (14-head, OFFK_WINOGRAD=0) and fails every slab-mode case with more than one image.

The pooled partial sums (`poolpart_28`; `pooled_7 / 14 / 28` under OFFK_FOLD_POOL=0) are held to 16 2^-24 sum |v| of their own cells (the
max of the 28-head is exact); measured: poolpart_28 <= 2.6, pooled_* <= 4.1.
"""
import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from .featmaps import rt  # noqa: F401
from .forward import HEAD_CH, HEAD_KEY, HANDLE_PRECISIONS, check_trace, dev, head_handle, rel_err, traced_forward
from .forward import HEAD_PATHS as PATHS

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
CEILING = dict((k, c + 64) for k, c in HEAD_CH.items())
MEASURED = {"7": 0.67, "14": 1.12, "28": 1.42}       # worst |err| / (2^-24 mag) seen on an MI355X, all cases of this module
HEAD_C = dict((k, 4.0 * v) for k, v in MEASURED.items())
PART_C = 16.0

# P = 1: one image, one 16-image block, two slabs; P = 18: two blocks, a last partial slab; P = 33: a third block holding ONE image, 1617 rows = 50.5 slabs
SHAPES = {"p1": (1, 2), "p18": (3, 7), "p33": (3, 12)}


def head_inputs(h, P):
    """The three heads' inputs as the device holds them, fp64 NCHW on the host; the 28-head's after its (exact) max pool."""
    f14 = h.region("fusion_14", 1056).view(P, 14, 14, 1056)[..., 800:1056]
    f7 = h.region("fusion_7", 832).view(P, 7, 7, 832)[..., 320:832]
    s7 = h.region("sum_7", 1024).view(P, 7, 7, 1024)
    x28, x14, x7 = (t.double().cpu().permute(0, 3, 1, 2).contiguous() for t in (f14, f7, s7))
    return {"28": F.max_pool2d(x28, 3, 2, ceil_mode=True), "14": x14, "7": x7}


def head_ratio(got, x, w, k):
    """max |got - ref| / (2^-24 (sum_c |w_c| mean|x_c| + |b|)) of head k on its [P, C, 7, 7] input."""
    W = torch.from_numpy(w[HEAD_KEY[k] + ".weight"]).double()
    b = torch.from_numpy(w[HEAD_KEY[k] + ".bias"]).double()
    assert x.shape[1:] == (HEAD_CH[k], 7, 7)
    ref = x.mean((2, 3)) @ W.t() + b
    mag = x.abs().mean((2, 3)) @ W.abs().t() + b.abs()
    got = got.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs() / (EPS * mag)).max().item()


def check_heads(logits, xs, w, what):
    ratios = dict((k, head_ratio(logits[k], xs[k], w, k)) for k in logits)
    print("%s: max |err| / (2^-24 (sum |w| mean|x| + |b|)) %s" % (what, " ".join("head_%s %.2f" % kv for kv in ratios.items())))
    for k, r in ratios.items():
        assert HEAD_C[k] < CEILING[k] / 16         # far below the a-priori worst case
        assert r < HEAD_C[k], (k, r)
    return ratios


def check_partial(got, ref, mag, name):
    err = (got.double().cpu() - ref).abs()
    ratio = (err / (EPS * mag).clamp_min(1e-300)).max().item()
    print("  %s: max |err| / (2^-24 sum |v|) = %.2f" % (name, ratio))
    assert (err <= PART_C * EPS * mag).all(), (name, ratio)


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("path", list(PATHS))
def test_forward_heads_vs_fp64_from_device_input(rt, path, shape, prec):
    env, must, must_not = PATHS[path]
    B, L = SHAPES[shape]
    P = B * (L - 1)
    h, w = head_handle(rt, env, B, L, prec)
    names, (o7, o14, o28) = traced_forward(h, [dev(f) for f in synth.make_features(B, L, 5)])
    check_trace(names, must, must_not)
    xs = head_inputs(h, P)
    check_heads({"7": o7, "14": o14, "28": o28}, xs, w, "heads %s %s %s" % (path, shape, prec))
    if path != "fold_pool0":
        # poolpart_28 [4 P][256]: block (img, j) sums pool rows [2 j, 2 j + 2) of the 7 x 7 max-pooled map, the last block has one row
        mp = xs["28"]
        ref = torch.stack([mp[:, :, 2 * j:2 * j + 2].sum((2, 3)) for j in range(4)], 1)
        mag = torch.stack([mp[:, :, 2 * j:2 * j + 2].abs().sum((2, 3)) for j in range(4)], 1)
        check_partial(h.region("poolpart_28", 256).view(P, 4, 256), ref, mag, "poolpart_28")
    else:
        for k in ("7", "14", "28"):        # pool_kernel: the mean of the 49 cells
            check_partial(h.region("pooled_" + k, HEAD_CH[k]), xs[k].mean((2, 3)), xs[k].abs().sum((2, 3)) / 49.0, "pooled_" + k)


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("path", list(PATHS))
def test_heads_without_the_28_head(rt, path, prec):
    """forward(want28=False): the 7- and 14-heads alone (two jobs in the one FC launch)."""
    B, L = 3, 7
    h, w = head_handle(rt, PATHS[path][0], B, L, prec)
    feats = [dev(f) for f in synth.make_features(B, L, 5)]
    o7, o14, o28 = h.forward(feats, want28=False)
    torch.cuda.synchronize()
    assert o28 is None
    check_heads({"7": o7, "14": o14}, head_inputs(h, B * (L - 1)), w, "heads %s %s, no 28-head" % (path, prec))


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("path", list(PATHS))
def test_heads_under_consensus(rt, path, prec):
    """Consensus on: the per-pair logits sit in the logit_* regions and obey the same bound; the outputs are their mean over T."""
    B, L = 3, 7
    P, T = B * (L - 1), L - 1
    h, w = head_handle(rt, PATHS[path][0], B, L, prec, consensus=True)
    outs = h.forward([dev(f) for f in synth.make_features(B, L, 5)])
    torch.cuda.synchronize()
    logits = dict((k, h.region("logit_" + k, spec.NUM_CLASSES)) for k in ("7", "14", "28"))
    check_heads(logits, head_inputs(h, P), w, "heads %s %s, consensus" % (path, prec))
    for out, k in zip(outs, ("7", "14", "28")):
        assert out.shape == (B, spec.NUM_CLASSES)
        assert rel_err(out, logits[k].double().view(B, T, -1).mean(1)) < 1e-6, k


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("shape", ["p18", "p33"])
@pytest.mark.parametrize("path", list(PATHS))
def test_heads_with_51_classes(rt, path, shape, prec):
    """51 classes: no multiple of 4, 8 or 32 -- the class tails of fc_pooled_body (a second class block with 19 live rows, a lane's
    last class quad cut at 3) and of fc_kernel (a last block of 3), and the min(cls, ncls - 1) clamps of their weight-row loads."""
    B, L = SHAPES[shape]
    ncls = 51
    h, w = head_handle(rt, PATHS[path][0], B, L, prec, ncls=ncls)
    o7, o14, o28 = h.forward([dev(f) for f in synth.make_features(B, L, 5)])
    torch.cuda.synchronize()
    assert o7.shape == (B * (L - 1), ncls)
    check_heads({"7": o7, "14": o14, "28": o28}, head_inputs(h, B * (L - 1)), w, "heads %s %s %s, 51 classes" % (path, shape, prec))
