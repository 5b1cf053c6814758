"""Split-fp32 arithmetic (OFFK_PRECISION_F32SPLIT, round 5): fp32 operands as three bf16 planes on the bf16 matrix pipe.

The claim these tests pin: the split kernels are fp32 arithmetic in the sense that matters for parity -- against an fp64
contraction of the same fp32 inputs their error is NO LARGER than the error of the library's own fp32-pipe kernels
(v_mfma_f32_16x16x4_f32 / 32x32x2_f32: a chain of fp32 FMAs) -- on every input distribution the parity suite uses: the
synthetic maps, 24-bit mantissas, a heavy tail, and the cancellation case.  Reference arithmetic: RGB_OFF.py:597-610 (fp32
nn.Conv2d); the tolerance north_star states is 1e-3 relative, both modes sit four orders inside it.

Reported per mode (print, -s shows it; bench.py carries the same numbers in `f32split_mode.error_vs_fp64`):
    max |err| / max |ref|, rms err / max |ref|, and c of |err| <= c 2^-24 sum_k |w_k x_k| (max and rms over elements).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import forward
from .featmaps import rt  # noqa: F401
from .forward import chain_inputs, dev, rel_err
from .wino_ref import between_reference

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KINDS = ["synth", "full_mantissa", "heavy_tail"]


def make_handle(rt, B, L, precision, weights=None, variant=spec.VARIANT_RGB, env=None):
    """-> (handle, its weights as numpy arrays)"""
    w = synth.make_weights(variant) if weights is None else weights
    return forward.make_handle(rt, B, L, variant, weights=w, precision=precision, env=env)[0], w


def units_reference_fp64(feats, w, B, L):
    """Per site: (T, magT, D, magD) in fp64.  T[b (L-1) + t] = relu(G)[b L + t + 1] - relu(G)[b L + t]  (RGB_OFF.py:597-604),
    D = down(X[:P]) (quirk Q1, :609-610); mag = sum_k |w_k x_k| (+ |bias|), for T the two frames' magnitudes added."""
    out = []
    P = B * (L - 1)
    for (name, C, H), x in zip(spec.SITES, feats):
        xd = torch.from_numpy(x).double()
        wg = torch.from_numpy(w["motion_conv_gen_%s.weight" % name]).double()
        bg = torch.from_numpy(w["motion_conv_gen_%s.bias" % name]).double()
        wd = torch.from_numpy(w["motion_spatial_down_%s.weight" % name]).double()
        bd = torch.from_numpy(w["motion_spatial_down_%s.bias" % name]).double()
        G = torch.relu(F.conv2d(xd, wg, bg)).view(B, L, 128, H, H)
        mG = (F.conv2d(xd.abs(), wg.abs()) + bg.abs().view(1, -1, 1, 1)).view(B, L, 128, H, H)
        T = (G[:, 1:] - G[:, :-1]).reshape(P, 128, H, H)
        mT = (mG[:, 1:] + mG[:, :-1]).reshape(P, 128, H, H)
        D = F.conv2d(xd[:P], wd, bd)
        mD = F.conv2d(xd[:P].abs(), wd.abs()) + bd.abs().view(1, -1, 1, 1)
        out.append((T, mT, D, mD))
    return out


def units_outputs(h, B, L):
    """(T, D) per site as the fused units left them: T in the fusion buffers (channels coff + 32 .. coff + 160), D in D_<site>."""
    P = B * (L - 1)
    res = []
    for fkey, fd in spec.FUSION.items():
        width = 160 * len(fd["sites"]) + fd["carry"]
        buf = h.region("fusion_" + fkey, width).view(P, fd["H"], fd["H"], width)
        for i, sname in enumerate(fd["sites"]):
            T = buf[..., 160 * i + 32:160 * i + 160].permute(0, 3, 1, 2).double().cpu()
            D = h.region("D_" + sname, 32).view(P, fd["H"], fd["H"], 32).permute(0, 3, 1, 2).double().cpu()
            res.append((T, D))
    return res


def error_stats(pairs):
    """pairs: [(got, ref, mag)] -> dict of the four numbers, over all elements of all tensors (each tensor normalised by its own max)."""
    mx, cmx, se, sc, n = 0.0, 0.0, 0.0, 0.0, 0
    for got, ref, mag in pairs:
        e = (got - ref).abs()
        s = ref.abs().max().clamp_min(1e-30)
        c = e / (mag.clamp_min(1e-30) * EPS)
        mx = max(mx, (e.max() / s).item())
        cmx = max(cmx, c.max().item())
        se += ((e / s) ** 2).sum().item()
        sc += (c ** 2).sum().item()
        n += e.numel()
    return {"max_over_max": mx, "rms_over_max": (se / n) ** 0.5, "c_max": cmx, "c_rms": (sc / n) ** 0.5}


def run_units(rt, B, L, precision, feats_np, weights=None):
    h, w = make_handle(rt, B, L, precision, weights)
    h.off_units_fused([dev(f) for f in feats_np])
    torch.cuda.synchronize()
    return units_outputs(h, B, L), w


@pytest.mark.parametrize("kind", KINDS)
def test_units_split_error_is_no_larger_than_the_fp32_pipes(rt, kind):
    B, L = 2, 7
    feats_np = synth.make_features_kind(B, L, 4, kind)
    stats = {}
    ref = None
    for prec in ("fp32", "f32split"):
        outs, w = run_units(rt, B, L, prec, feats_np)
        if ref is None:
            ref = units_reference_fp64(feats_np, w, B, L)
        pairs = []
        for (T, D), (Tr, mT, Dr, mD) in zip(outs, ref):
            pairs += [(T, Tr, mT), (D, Dr, mD)]
        stats[prec] = error_stats(pairs)
        print("units %-8s on %-13s maps vs fp64: max %.3e  rms %.3e  c_max %.3f  c_rms %.4f"
              % (prec, kind, stats[prec]["max_over_max"], stats[prec]["rms_over_max"], stats[prec]["c_max"], stats[prec]["c_rms"]))
    for key in ("max_over_max", "rms_over_max", "c_max", "c_rms"):
        assert stats["f32split"][key] <= stats["fp32"][key], (kind, key, stats)
    assert stats["f32split"]["max_over_max"] < 2e-6 and stats["f32split"]["c_max"] < 16.0


def test_units_split_cancellation_case(rt):
    """tests/test_gpu_parity.py::test_pw_reduce_cancellation_case on the fused kernels: every channel of a pixel carries the
    same value and every weight row sums to zero -- the exact G is relu(bias), the exact T is 0, the exact D is the bias."""
    B, L = 2, 7
    wnp = synth.make_weights(spec.VARIANT_RGB)
    for name, _C, _H in spec.SITES:
        for key in ("motion_conv_gen_%s.weight" % name, "motion_spatial_down_%s.weight" % name):
            wk = wnp[key].astype(np.float64)
            wnp[key] = (wk - wk.mean(axis=1, keepdims=True)).astype(np.float32)
    base = synth.make_features_kind(B, L, 4, "heavy_tail")
    feats_np = [np.ascontiguousarray(np.broadcast_to(f[:, :1] + np.float32(0.5), f.shape)) for f in base]
    stats, ref = {}, None
    for prec in ("fp32", "f32split"):
        outs, w = run_units(rt, B, L, prec, feats_np, wnp)
        if ref is None:
            ref = units_reference_fp64(feats_np, w, B, L)
        pairs = [(D, Dr, mD) for (_T, D), (_Tr, _mT, Dr, mD) in zip(outs, ref)]
        stats[prec] = error_stats(pairs)
        print("units %-8s cancellation case (D rows) vs fp64: max err / max|out| %.3e  c_max %.3f  c_rms %.4f"
              % (prec, stats[prec]["max_over_max"], stats[prec]["c_max"], stats[prec]["c_rms"]))
    for key in ("max_over_max", "rms_over_max", "c_max", "c_rms"):
        assert stats["f32split"][key] <= stats["fp32"][key], (key, stats)
    assert stats["f32split"]["c_max"] < 4.0


@pytest.mark.parametrize("B,L", [(1, 2), (3, 3), (2, 9), (5, 7)])
def test_units_split_shapes(rt, B, L):
    """Short clips (frames past the group read zeros), two temporal groups (L = 9), odd batches (packed 14x14 leftovers, the 7x7
    quad stream crossing clip boundaries): every T and D element against fp64."""
    feats_np = synth.make_features(B, L, 5)
    outs, w = run_units(rt, B, L, "f32split", feats_np)
    ref = units_reference_fp64(feats_np, w, B, L)
    for (name, _C, _H), (T, D), (Tr, _mT, Dr, _mD) in zip(spec.SITES, outs, ref):
        assert ((T - Tr).abs().max() / Tr.abs().max()).item() < 2e-6, name
        assert ((D - Dr).abs().max() / Dr.abs().max()).item() < 2e-6, name


# ---- the batched GEMMs of the Winograd convs in split-fp32 arithmetic (wino_gemm_split.hip) ----

def gemm_inputs(batch, M, K, Co, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, M, K, generator=g)
    w = torch.randn(batch, Co, K, generator=g) * (1.0 / K ** 0.5)
    if kind == "relu":                # what V looks like behind a ReLU and B^T . B: mostly small, some zeros
        x = torch.relu(x)
    elif kind == "heavy_tail":
        x = x * torch.exp(2.0 * torch.randn(batch, M, 1, generator=g))
    elif kind == "cancellation":      # every row of w sums to zero, x constant along k (+ noise of 2^-12): the result is the noise's
        w = w - w.mean(dim=2, keepdim=True)
        x = 3.0 + torch.randn(batch, M, 1, generator=g) + torch.randn(batch, M, K, generator=g) * 2.0 ** -12
    return x.float().contiguous(), w.float().contiguous()


@pytest.mark.parametrize("batch,M,K,Co", [(5, 384, 832, 256), (121, 384, 256, 256), (3, 100, 128, 128), (7, 64, 64, 512),
                                          (2, 777, 1056, 128), (9, 200, 320, 64), (3, 130, 1280, 192), (70, 3456, 64, 64)])
def test_batched_gemm_split_shapes(rt, batch, M, K, Co):
    """Item streams longer than the persistent grid (121 x 6 x 2 items; 70 x 54 of the 64-channel form), row tails (M % 64 != 0), the
    shortest K the kernel takes (two K-tiles: the three cursors cross item boundaries on consecutive steps), Co = 64 / 192 (the
    64-channel form), every element against fp64."""
    x, w = gemm_inputs(batch, M, K, Co, "relu", 11)
    ref = torch.einsum("bmk,bnk->bmn", x.double(), w.double())
    y = rt.batched_gemm_nt(dev(x), dev(w), "f32split").double().cpu()
    assert ((y - ref).abs().max() / ref.abs().max()).item() < 1e-6
    y32 = rt.batched_gemm_nt(dev(x), dev(w), "fp32").double().cpu()
    assert ((y32 - ref).abs().max() / ref.abs().max()).item() < 3e-6


@pytest.mark.parametrize("kind", ["relu", "normal", "heavy_tail", "cancellation"])
def test_batched_gemm_split_error_is_no_larger_than_the_fp32_pipes(rt, kind):
    batch, M, K, Co = 6, 384, 832, 256
    x, w = gemm_inputs(batch, M, K, Co, kind, 5)
    ref = torch.einsum("bmk,bnk->bmn", x.double(), w.double())
    mag = torch.einsum("bmk,bnk->bmn", x.double().abs(), w.double().abs())
    stats = {}
    for prec in ("fp32", "f32split"):
        y = rt.batched_gemm_nt(dev(x), dev(w), prec).double().cpu()
        stats[prec] = error_stats([(y, ref, mag)])
        print("batched GEMM %-8s on %-12s inputs vs fp64: max %.3e  rms %.3e  c_max %.3f  c_rms %.4f"
              % (prec, kind, stats[prec]["max_over_max"], stats[prec]["rms_over_max"], stats[prec]["c_max"], stats[prec]["c_rms"]))
    for key in ("max_over_max", "rms_over_max", "c_max", "c_rms"):
        assert stats["f32split"][key] <= stats["fp32"][key], (kind, key, stats)


@pytest.mark.parametrize("B", [2, 12])
def test_forward_split_gemms_against_fp32_pipe_gemms(rt, B):
    """A split-fp32 handle with its GEMMs / 1x1 convs on the bf16 pipe (default) against the same handle with OFFK_SPLIT_GEMM=0 (only the
    units kernel split): same logits and stage tensors to summation-order noise (the convs' own Winograd error is 1e-5 of max |ref|), and
    the 7-head's folded pool of the split kernel's epilogue gives the same logits."""
    L = 7
    feats = [dev(f) for f in synth.make_features(B, L, 3)]
    h1, _ = make_handle(rt, B, L, "f32split")
    h0, _ = make_handle(rt, B, L, "f32split", env={"OFFK_SPLIT_GEMM": "0"})
    a, b = h1.forward(feats), h0.forward(feats)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert ((x - y).abs().max() / y.abs().max()).item() < 2e-5
        sig = (y - y.mean(dim=0, keepdim=True)).abs().max().item()        # the logits are bias-dominated: compare on the row-to-row signal
        assert (x - y).abs().max().item() < 1e-3 * sig
    for name, ch in (("sum_7", 1024), ("fusion_7", 832)):
        x, y = h1.region(name, ch), h0.region(name, ch)
        assert ((x - y).abs().max() / y.abs().max()).item() < 5e-5, name


# ---- the whole forward of both modes against an fp64 evaluation of the oracle ----

@pytest.mark.parametrize("case", ["rgb_golden_inputs", "flow_golden_inputs", "rgb_heavy_tail"])
def test_whole_forward_error_vs_fp64_oracle(rt, case):
    """oracle/off_oracle.py evaluated in fp64 (torch CPU, the same op sequence on double tensors: RGB_OFF.py:596-847) on the inputs of the
    B = 3 x 7 goldens (synth.make_features(3, 7, cfg) -- what gen_golden.py fed the reference) and on heavy-tailed maps: the error of
    `sum_7` and of the three logit tensors of BOTH arithmetic modes.  The split mode may not be further from fp64 than the fp32 pipe is
    (10 % slack: what both share -- the fp32 Winograd transforms -- dominates the whole-forward error and is the same code)."""
    from oracle import off_oracle as orc
    B, L = 3, 7
    variant = spec.VARIANT_FLOW if case.startswith("flow") else spec.VARIANT_RGB
    cfg = 2 if variant == spec.VARIANT_RGB else 3
    feats_np = synth.make_features_kind(B, L, cfg, "heavy_tail" if case.endswith("heavy_tail") else "synth")
    wnp = synth.make_weights(variant)
    w64 = dict((k, v.double()) for k, v in orc.to_torch_weights(wnp).items())
    with torch.no_grad():
        ref, st = orc.off_forward([torch.from_numpy(f).double() for f in feats_np], w64, B, L, variant, orc.SLICE_FLAT, consensus=False,
                                  return_stages=True)
    P = B * (L - 1)
    errs = {}
    for prec in ("fp32", "f32split"):
        h = rt.OffForward(B, L, variant, spec.SLICE_FLAT, False, precision=prec)
        assert h.load_state_dict(wnp) == []
        out = h.forward([dev(f) for f in feats_np])
        torch.cuda.synchronize()
        s7 = h.region("sum_7", 1024).view(P, 7, 7, 1024).permute(0, 3, 1, 2).double().cpu()
        e7 = (s7 - st["sum_7"]).abs()
        el = [(o.double().cpu() - r).abs() for o, r in zip(out, ref)]
        sig = [(r - r.mean(0, keepdim=True)).abs().max() for r in ref]      # the logits are bias-dominated: normalise by the row-to-row signal
        errs[prec] = {"sum_7_max": (e7.max() / st["sum_7"].abs().max()).item(), "sum_7_rms": ((e7 ** 2).mean().sqrt() / st["sum_7"].abs().max()).item(),
                      "logit_signal_max": max((e.max() / s).item() for e, s in zip(el, sig))}
        print("whole forward %-8s %-18s vs fp64 oracle: sum_7 max %.2e rms %.2e, logits / row-to-row signal %.2e"
              % (prec, case, errs[prec]["sum_7_max"], errs[prec]["sum_7_rms"], errs[prec]["logit_signal_max"]))
        assert errs[prec]["sum_7_max"] < 2e-4 and errs[prec]["logit_signal_max"] < 1e-3
    for key in ("sum_7_max", "sum_7_rms", "logit_signal_max"):
        assert errs["f32split"][key] <= 1.1 * errs["fp32"][key], (key, errs)


def test_split_nonfinite_and_tiny_inputs(rt):
    """what include/offk.h states next to OFFK_PRECISION_F32SPLIT.  +-Inf in an operand: NaN in every output it touches (the
    fp32 pipe: +-Inf or NaN) and nowhere else; operands down to 2^-100 (all three planes still bf16 normals or subnormals): the same result
    as the fp32 pipe to the usual error."""
    batch, M, K, Co = 2, 64, 128, 64
    x, w = gemm_inputs(batch, M, K, Co, "normal", 3)
    x[0, 5, 17] = float("inf")
    x[1, 9, 3] = float("-inf")
    y = rt.batched_gemm_nt(dev(x), dev(w), "f32split").cpu()
    y32 = rt.batched_gemm_nt(dev(x), dev(w), "fp32").cpu()
    bad = torch.zeros(batch, M, dtype=torch.bool)
    bad[0, 5] = bad[1, 9] = True
    assert torch.isnan(y[bad]).all() and not torch.isfinite(y32[bad]).any()
    assert torch.isfinite(y[~bad]).all() and torch.isfinite(y32[~bad]).all()
    ref = torch.einsum("bmk,bnk->bmn", x.double(), w.double())
    assert ((y[~bad].double() - ref[~bad]).abs().max() / ref[~bad].abs().max()).item() < 1e-6
    # tiny operands: x scaled by 2^-100 (planes down to 2^-116: bf16 normals), w by 2^-20 -- products ~2^-120, sums fp32 normals
    xs, ws = gemm_inputs(batch, M, K, Co, "normal", 4)
    xs, ws = xs * 2.0 ** -100, ws * 2.0 ** -20
    yt = rt.batched_gemm_nt(dev(xs), dev(ws), "f32split").double().cpu()
    reft = torch.einsum("bmk,bnk->bmn", xs.double(), ws.double())
    assert ((yt - reft).abs().max() / reft.abs().max()).item() < 1e-6


# ---- the bottleneck chains of fusion@28 in split-fp32 arithmetic (chain_split.hip) through their C-ABI entry point (ABI v10) ----

@pytest.mark.parametrize("kind", ["normal", "heavy_tail"])
@pytest.mark.parametrize("case", ["28a_branch", "28b_residual", "28c_into_slice"])
@pytest.mark.parametrize("n", [1, 5, 11])
def test_bottleneck_chain14_split_vs_fp64(rt, case, n, kind):
    """offk_bottleneck_chain14_split (RGB_OFF.py:658-667 / :670-685) against an fp64 chain: the branch form of block 28a (c1 on relu(x0), the
    branch conv on the pre-ReLU x0, inside the kernel), the residual form, output into a channel slice; odd image counts exercise the grid
    rounding.  Beside it the fp32-pipe kernel (offk_bottleneck_chain14, direct 3x3): the split chain may not be further from fp64."""
    branch = case == "28a_branch"
    x, w1, b1, w2, b2, w3, b3, wb, bb = chain_inputs(case, n, kind, 300 + n)
    Cin, x_coff = (64, 64) if branch else (256, 0)
    xin = x[..., x_coff:x_coff + Cin].permute(0, 3, 1, 2).double()
    t1 = F.relu(F.conv2d(F.relu(xin) if branch else xin, w1.double()[:, :, None, None], b1.double()))
    t2 = F.relu(F.conv2d(t1, w2.double(), b2.double(), padding=1))
    want = F.conv2d(t2, w3.double()[:, :, None, None], b3.double())
    want = want + (F.conv2d(xin, wb.double()[:, :, None, None], bb.double()) if branch else xin)
    want = F.relu(want).permute(0, 2, 3, 1)
    res = None if branch else dev(x)
    kw = dict(res=res, branch=(dev(wb), dev(bb)) if branch else None, relu_in=branch, x_coff=x_coff)
    if case == "28c_into_slice":
        ybuf = torch.full((n, 14, 14, 352), -3.0, device="cuda")
        rt.bottleneck_chain14_split(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(w3), dev(b3), y=ybuf, y_coff=64, **kw)
        got = ybuf[..., 64:320]
        assert torch.all(ybuf[..., :64] == -3.0) and torch.all(ybuf[..., 320:] == -3.0)
    else:
        got = rt.bottleneck_chain14_split(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(w3), dev(b3), **kw)
    # the fp32-pipe kernel on the same chain (28a: its merged form, c3 over [t2 | x0] with K3 = 128)
    if branch:
        w3m = torch.cat([w3, wb], 1).contiguous()
        got32 = rt.bottleneck_chain14(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(w3m), dev(b3 + bb), relu_in=True, x_coff=x_coff)
    else:
        got32 = rt.bottleneck_chain14(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(w3), dev(b3), res=res)
    torch.cuda.synchronize()
    s = want.abs().max()
    e = ((got.double().cpu() - want).abs().max() / s).item()
    e32 = ((got32.double().cpu() - want).abs().max() / s).item()
    rms = (((got.double().cpu() - want) ** 2).mean().sqrt() / s).item()
    rms32 = (((got32.double().cpu() - want) ** 2).mean().sqrt() / s).item()
    print("chain %-15s n = %2d %-10s vs fp64: split max %.2e rms %.2e | fp32 pipe max %.2e rms %.2e" % (case, n, kind, e, rms, e32, rms32))
    assert e < 2e-6 and e <= 1.05 * e32 and rms <= 1.05 * rms32


# ---- worst-case mantissas: the true dropped-term bound and the accumulation error, separated (tests/test_split_contract.py is the CPU side) ----
#
# Operands from synth.make_adversarial: +-2^e (1 + mant / 2^23), e in -3 .. 3, mant one of the patterns whose truncating cut leaves the
# largest lower planes (0x00FFFF: dropped products 7.83 x 2^-24 |w x|, against the bound 8.015625).  Per output element
#     |gpu - ref64| <= |ref64 - kept64| + A 2^-24 sum_k |w_k x_k|  (+ 2^-24 |value| per fp32 operation of the epilogue behind the accumulators)
# where kept64 = the six kept plane products in fp64 (synth.split_terms: the EXACT dropped part, up to 7.83) and A = max(1, 2 c_acc) with
# c_acc the maximum over elements of the CPU emulation's own accumulation error (synth.emulate_split_dot, two-accumulator form, against
# kept64) ON THE SAME INPUTS: A is computed in the test from the emulation, never from the kernel's output.  The factor 2: the order and
# rounding of the products inside one MFMA is recorded only as far as tools/probe_split_mfma.hip part 2 goes.
# tests/test_split_contract.py::test_losing_any_kept_product_breaks_the_gpu_inequality shows that this inequality fails when any one of the
# six products is lost (the smallest are 2^-16 of the leading one: c ~ 256).  On these inputs "split <= fp32 pipe" is NOT a property of the
# arithmetic (the dropped part alone is up to 7.8 where a K = 64 fp32 chain stays near 1): the fp32 pipe is printed beside, not asserted.
ADV_PATTERNS = [0x00FFFF, 0x7FFFFF, 0x7F7F7F]
ADV_SIGNS = ["same", "alternating"]
SECOND_ORDER = 2.0 ** -40          # x sum |w x|: an epilogue rounding is 2^-24 of the COMPUTED value, which is within ~2^-16 sum |w x| of the fp64 one


def _pow2_scale(C):
    """1 / sqrt(C) rounded to a power of two: scaling by it keeps the adversarial mantissas."""
    return np.float32(2.0 ** -round(np.log2(C) / 2))


def adversarial_units_inputs(B, L, pattern, signs, relu):
    """Nine adversarial maps and the synthetic weights with every motion_conv_gen_* / motion_spatial_down_* weight adversarial too
    (sign mode along C, scaled by ~1 / sqrt(C)); biases as synth makes them."""
    feats = [synth.make_adversarial((B * L, C, H, H), pattern, "same", seed=10 + si, relu=relu, k_axis=1) for si, (_n, C, H) in enumerate(spec.SITES)]
    w = synth.make_weights(spec.VARIANT_RGB)
    for si, (name, C, _H) in enumerate(spec.SITES):
        for j, key in enumerate(("motion_conv_gen_%s.weight" % name, "motion_spatial_down_%s.weight" % name)):
            w[key] = synth.make_adversarial(w[key].shape, pattern, signs, seed=100 + 2 * si + j, k_axis=1) * _pow2_scale(C)
    return feats, w


def adversarial_units_model(feats, w, B, L):
    """CPU side of the units test.  Per site the limits of T and D (see above) and the pieces the report prints; and the emulation's
    c_acc maximum over every pre-epilogue sum the outputs use.  Epilogue (pw_tdiff_split.hip): G = relu((A1 + A2) + b) -- A1 + A2 belongs to
    the emulation, the bias add is one fp32 operation --, T = G[t + 1] - G[t] one more; D = (A1 + A2) + b."""
    P = B * (L - 1)
    sites, c_acc = [], 0.0
    for (name, C, H), x in zip(spec.SITES, feats):
        HW = H * H
        X = np.ascontiguousarray(x.transpose(0, 2, 3, 1)).reshape(B * L * HW, C)
        W = np.concatenate([w["motion_conv_gen_%s.weight" % name].reshape(128, C), w["motion_spatial_down_%s.weight" % name].reshape(32, C)])
        ref, dropped, mag = synth.split_terms(W, X)
        c = synth.split_c_acc(synth.emulate_split_dot(W, X, "units"), ref, dropped, mag)
        c_acc = max(c_acc, c[:, :128].max(), c[:P * HW, 128:].max())
        bg = w["motion_conv_gen_%s.bias" % name].astype(np.float64)
        bd = w["motion_spatial_down_%s.bias" % name].astype(np.float64)
        nchw = lambda a, n, ch: torch.from_numpy(np.ascontiguousarray(a.reshape(n, H, H, ch).transpose(0, 3, 1, 2)))
        pairs = lambda a: (a.reshape(B, L, HW, 128)[:, 1:], a.reshape(B, L, HW, 128)[:, :-1])
        s, dr, mg = ref[:, :128], dropped[:, :128], mag[:, :128]
        g1, g0 = pairs(np.maximum(s + bg, 0.0))
        k1, k0 = pairs(np.maximum(s - dr + bg, 0.0))
        m1, m0 = pairs(mg)
        v1, v0 = pairs(np.abs(s + bg))
        sd, dd, md = ref[:P * HW, 128:], dropped[:P * HW, 128:], mag[:P * HW, 128:]
        sites.append({"T_kept": nchw((k1 - k0), P, 128), "T_mag": nchw(m1 + m0, P, 128),
                      "T_epi": nchw(EPS * (v1 + v0 + np.abs(g1 - g0)) + SECOND_ORDER * (m1 + m0), P, 128),
                      "D_kept": nchw(sd - dd + bd, P, 32), "D_mag": nchw(md, P, 32),
                      "D_epi": nchw(EPS * np.abs(sd + bd) + SECOND_ORDER * md, P, 32)})
    return sites, float(c_acc)


def split_report(what, got, ref, kept, mag, epi, A):
    """Prints the measured c = error / (2^-24 sum |w x|) split into its dropped and accumulation parts, returns the worst excess over the limit."""
    e_drop, e_acc, e_tot = (ref - kept).abs(), (got - kept).abs(), (got - ref).abs()
    unit = (EPS * mag).clamp_min(1e-300)
    limit = e_drop + A * EPS * mag + epi
    over = (e_tot - limit).max().item()
    i = int((e_tot - limit).argmax())
    print("%s: c_total max %.3f | dropped (exact, CPU) max %.3f | accumulation + epilogue (gpu - kept64) max %.3f, allowed A = %.3f | worst element %d: err %.3e limit %.3e"
          % (what, (e_tot / unit).max().item(), (e_drop / unit).max().item(), (e_acc / unit).max().item(), A, i,
             e_tot.reshape(-1)[i].item(), limit.reshape(-1)[i].item()))
    return over


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pattern", ADV_PATTERNS)
@pytest.mark.parametrize("signs", ADV_SIGNS)
def test_units_split_worst_case_mantissas(rt, signs, pattern, relu):
    """h.off_units_fused, all nine sites, B = 2 x L = 7, every T and D element against units_reference_fp64 under the inequality above.
    Emulated c_acc (CPU, maximum over the nine sites' sums) and A = max(1, 2 c_acc) per case; GPU columns: measured accumulation part
    (gpu - kept64) / (2^-24 sum |w x|), the epilogue's bias add included, T and D maxima (first MI355X run; also DESIGN.md 5.1):

        signs        pattern   relu   c_acc (emulation)   A       gpu accumulation max (T / D)
        same         0x00FFFF  no     1.337               2.675   1.496 / 2.035
        same         0x00FFFF  yes    1.295               2.590   1.773 / 2.013
        same         0x7FFFFF  no     14.331              28.661  9.979 / 12.268
        same         0x7FFFFF  yes    14.690              29.381  8.969 / 14.097
        same         0x7F7F7F  no     13.773              27.547  9.570 / 13.173
        same         0x7F7F7F  yes    15.586              31.173  9.349 / 13.388
        alternating  0x00FFFF  no     0.459               1.000   0.511 / 0.767
        alternating  0x00FFFF  yes    0.651               1.301   0.727 / 1.007
        alternating  0x7FFFFF  no     2.668               5.337   1.341 / 2.507
        alternating  0x7FFFFF  yes    4.221               8.443   2.443 / 4.076
        alternating  0x7F7F7F  no     2.826               5.652   1.582 / 2.874
        alternating  0x7F7F7F  yes    4.426               8.853   2.337 / 3.850
    """
    B, L = 2, 7
    feats_np, w = adversarial_units_inputs(B, L, pattern, signs, relu)
    model, c_acc = adversarial_units_model(feats_np, w, B, L)
    A = max(1.0, 2.0 * c_acc)
    print("units worst case %s 0x%06X relu %d: emulated c_acc %.3f -> A %.3f" % (signs, pattern, relu, c_acc, A))
    ref = units_reference_fp64(feats_np, w, B, L)
    outs, _ = run_units(rt, B, L, "f32split", feats_np, w)
    outs32, _ = run_units(rt, B, L, "fp32", feats_np, w)
    worst = []
    for (name, _C, _H), (T, D), (T32, D32), (Tr, _mT, Dr, _mD), m in zip(spec.SITES, outs, outs32, ref, model):
        tag = "units worst case %-11s 0x%06X relu %d site %s" % (signs, pattern, relu, name)
        worst.append((split_report(tag + " T", T, Tr, m["T_kept"], m["T_mag"], m["T_epi"], A), name, "T"))
        worst.append((split_report(tag + " D", D, Dr, m["D_kept"], m["D_mag"], m["D_epi"], A), name, "D"))
        print("%s: fp32 pipe beside it (not a limit): c_total T %.3f D %.3f" % (tag, ((T32 - Tr).abs() / (EPS * m["T_mag"]).clamp_min(1e-300)).max().item(),
                                                                               ((D32 - Dr).abs() / (EPS * m["D_mag"]).clamp_min(1e-300)).max().item()))
    assert max(worst)[0] <= 0.0, max(worst)


ADV_GEMM_SHAPES = [(3, 100, 64, 64), (5, 384, 832, 256), (3, 130, 1280, 192)]


def adversarial_gemm_inputs(batch, M, K, Co, pattern, signs):
    x = synth.make_adversarial((batch, M, K), pattern, "same", seed=500 + K)
    w = synth.make_adversarial((batch, Co, K), pattern, signs, seed=501 + K) * _pow2_scale(K)
    return x, w


def adversarial_gemm_model(x, w):
    """(ref, kept, mag) in fp64 and the emulation's c_acc maximum.  wino_gemm_split.hip runs the two-accumulator form (`acc += acs` once per
    item: form "units" of the emulation); nothing follows the accumulators."""
    terms = [synth.split_terms(w[b], x[b]) for b in range(x.shape[0])]
    c_acc = max(synth.split_c_acc(synth.emulate_split_dot(w[b], x[b], "units"), *terms[b]).max() for b in range(x.shape[0]))
    ref, dropped, mag = (torch.from_numpy(np.stack([t[i] for t in terms])) for i in range(3))
    return ref, ref - dropped, mag, float(c_acc)


@pytest.mark.parametrize("pattern", ADV_PATTERNS)
@pytest.mark.parametrize("signs", ADV_SIGNS)
@pytest.mark.parametrize("batch,M,K,Co", ADV_GEMM_SHAPES)
def test_batched_gemm_split_worst_case_mantissas(rt, batch, M, K, Co, signs, pattern):
    """batched_gemm_nt(..., "f32split") at the shortest K, a production shape, and the longest K with a row tail and the 64-channel form.
    Emulated c_acc / A = max(1, 2 c_acc) / measured GPU accumulation part max (first MI355X run), per (shape, signs), patterns 0x00FFFF |
    0x7FFFFF | 0x7F7F7F:

        (batch, M, K, Co)     signs        c_acc (emulation)         A                         gpu accumulation max
        (3, 100, 64, 64)      same         1.027 | 3.304 | 3.304     2.054 | 6.608 | 6.609     1.027 | 3.304 | 3.304
        (3, 100, 64, 64)      alternating  0.608 | 1.875 | 1.640     1.215 | 3.750 | 3.280     0.608 | 1.875 | 2.130
        (5, 384, 832, 256)    same         1.344 | 12.245 | 12.348   2.688 | 24.490 | 24.696   1.344 | 12.422 | 12.348
        (5, 384, 832, 256)    alternating  0.327 | 2.442 | 2.712     1.000 | 4.884 | 5.424     0.327 | 2.442 | 2.712
        (3, 130, 1280, 192)   same         1.305 | 15.148 | 15.579   2.610 | 30.297 | 31.158   1.305 | 15.148 | 15.579
        (3, 130, 1280, 192)   alternating  0.192 | 1.838 | 1.879     1.000 | 3.677 | 3.757     0.222 | 1.838 | 1.879
    """
    x, w = adversarial_gemm_inputs(batch, M, K, Co, pattern, signs)
    ref, kept, mag, c_acc = adversarial_gemm_model(x, w)
    A = max(1.0, 2.0 * c_acc)
    tag = "batched GEMM worst case (%d, %d, %d, %d) %-11s 0x%06X" % (batch, M, K, Co, signs, pattern)
    print("%s: emulated c_acc %.3f -> A %.3f" % (tag, c_acc, A))
    y = rt.batched_gemm_nt(dev(x), dev(w), "f32split").double().cpu()
    y32 = rt.batched_gemm_nt(dev(x), dev(w), "fp32").double().cpu()
    over = split_report(tag, y, ref, kept, mag, torch.zeros_like(mag), A)
    print("%s: fp32 pipe beside it (not a limit): c_total %.3f" % (tag, ((y32 - ref).abs() / (EPS * mag)).max().item()))
    assert over <= 0.0


@pytest.mark.parametrize("pattern", ADV_PATTERNS)
@pytest.mark.parametrize("signs", ADV_SIGNS)
@pytest.mark.parametrize("case", ["28a_branch", "28b_residual"])
def test_bottleneck_chain14_split_worst_case_mantissas(rt, case, signs, pattern):
    """The chains with the FIRST contraction's operands (the chain input and c1's weight) adversarial; t1's bound is asserted indirectly,
    through the whole chain against fp64 exactly as test_bottleneck_chain14_split_vs_fp64 measures it (max error / max |want| < 2e-6).  The
    fp32-pipe kernel is printed beside it and is not a limit here."""
    n, branch = 5, case == "28a_branch"
    _x, _w1, b1, w2, b2, w3, b3, wb, bb = chain_inputs(case, n, "normal", 900)
    Cin, x_coff = (64, 64) if branch else (256, 0)
    x = torch.from_numpy(synth.make_adversarial((n, 14, 14, Cin + x_coff), pattern, "same", seed=40))
    w1 = torch.from_numpy(synth.make_adversarial((64, Cin), pattern, signs, seed=41) * _pow2_scale(Cin))
    xin = x[..., x_coff:x_coff + Cin].permute(0, 3, 1, 2).double()
    t1 = F.relu(F.conv2d(F.relu(xin) if branch else xin, w1.double()[:, :, None, None], b1.double()))
    t2 = F.relu(F.conv2d(t1, w2.double(), b2.double(), padding=1))
    want = F.conv2d(t2, w3.double()[:, :, None, None], b3.double())
    want = want + (F.conv2d(xin, wb.double()[:, :, None, None], bb.double()) if branch else xin)
    want = F.relu(want).permute(0, 2, 3, 1)
    res = None if branch else dev(x)
    got = rt.bottleneck_chain14_split(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(w3), dev(b3), res=res,
                                      branch=(dev(wb), dev(bb)) if branch else None, relu_in=branch, x_coff=x_coff)
    if branch:
        got32 = rt.bottleneck_chain14(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(torch.cat([w3, wb], 1).contiguous()), dev(b3 + bb),
                                      relu_in=True, x_coff=x_coff)
    else:
        got32 = rt.bottleneck_chain14(dev(x), dev(w1), dev(b1), dev(w2), dev(b2), dev(w3), dev(b3), res=res)
    torch.cuda.synchronize()
    s = want.abs().max()
    e = ((got.double().cpu() - want).abs().max() / s).item()
    e32 = ((got32.double().cpu() - want).abs().max() / s).item()
    rms = (((got.double().cpu() - want) ** 2).mean().sqrt() / s).item()
    print("chain worst case %-13s %-11s 0x%06X vs fp64: split max %.2e rms %.2e | fp32 pipe beside it (not a limit) max %.2e" % (case, signs, pattern, e, rms, e32))
    assert e < 2e-6


@pytest.mark.parametrize("pattern", ADV_PATTERNS)
@pytest.mark.parametrize("signs", ADV_SIGNS)
def test_winograd_between_split_worst_case_mantissas(rt, signs, pattern):
    """winograd_between with its 1x1 conv in split arithmetic (Cin = Cmid = 128, n = 5): w1 adversarial, the Winograd-domain input too (the
    activations the 1x1 contracts are its output transform); limits and normalisation of tests/test_gpu_paths.py::
    test_winograd_between_vs_fp64, the fp32-pipe kernel printed beside it."""
    n, cin = 5, 128
    M = synth.make_adversarial((121, n, cin), pattern, "same", seed=60) * np.float32(0.125)
    bias = synth.uniform_values(61, cin, 0.5)
    w1 = synth.make_adversarial((cin, cin), pattern, signs, seed=62) * _pow2_scale(cin)
    b1 = synth.uniform_values(63, cin, 0.1)
    x_ref, v_ref = between_reference(M.astype(np.float64), bias.astype(np.float64), 1, w1.astype(np.float64), b1.astype(np.float64))
    errs = {}
    for prec in ("f32split", "fp32"):
        xbuf = torch.full((n, 7, 7, cin + 64), -3.0, device="cuda")
        V = rt.winograd_between(dev(M), dev(bias), 1, dev(w1), dev(b1), x=xbuf, x_coff=32, precision=prec)
        torch.cuda.synchronize()
        errs[prec] = (rel_err(xbuf[..., 32:32 + cin], x_ref), rel_err(V, v_ref))
    print("winograd between worst case %-11s 0x%06X: split x %.2e V %.2e | fp32 pipe beside it (not a limit) x %.2e V %.2e"
          % ((signs, pattern) + errs["f32split"] + errs["fp32"]))
    assert errs["f32split"][0] < 1e-5 and errs["f32split"][1] < 2e-5
