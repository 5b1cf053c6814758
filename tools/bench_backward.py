"""Training side of the OFF units on MI355X: train-mode forward (K1 + K2 with dropout) and the units'
backward (K2b + K1b + reductions) at BASELINE config 2 size, with algorithmic bytes / FLOPs.
    python tools/bench_backward.py [--batch 64] [--length 7] [--iters 20] [--feat-dtype fp32|bf16|fp16] [--feat-layout nchw|cl|copy] [--feat-grad]
                                     [--feat-grad-dtype map|fp32] [--feat-grad-arith fp32|f32split] [--wgrad-arith fp32|f32split] [--fwd-arith fp32|f32split]
--feat-dtype bf16 / fp16: the maps go in as 16-bit tensors (offk_off_units_train_typed / offk_off_units_backward_typed), and the nine
.float() casts that path makes unnecessary are timed beside it.
--feat-layout cl: the maps are torch.channels_last tensors and go in as they are (offk_off_units_train_cl / offk_off_units_backward_cl);
copy: the same channels_last maps made contiguous inside the timed region of the forward (nine .contiguous() calls, what a caller
without the _cl entries does; the backward then reads the copies); nchw (default): contiguous maps.  units_step_ms is forward + backward.
--feat-grad: the gradient w.r.t. the nine maps (offk_off_units_backward_feats, in the maps' layout) joins the timed backward, so
units_backward_ms / units_step_ms are those of a step that trains through the maps; the call alone and the same gradient composed
from torch ops (torch.nn.grad.conv2d_input for the two 1x1 convs, the add into the frames of the slice) are timed beside it.
--feat-grad-dtype map (default): dX comes in the maps' dtype -- with --feat-dtype bf16 / fp16 from offk_off_units_backward_feats_typed,
rounded in the kernel; fp32: the route without that entry -- the fp32 launch plus nine .to(dtype) casts of its result (what
OFFUnits(feat_grad=True) did on 16-bit maps before), for the A/B.  feat_grad_ms is the whole route, feat_grad_launch_ms the launch
alone, feat_grad_casts_ms the nine casts alone.
--feat-grad-arith f32split: dX from offk_off_units_backward_feats_split (split-fp32 on the bf16 matrix pipe; feat_grad_launch_ms then
covers its two launches, the weight pre-pass included); fp32 (default): the fp32 matrix pipe's entries.
--wgrad-arith f32split: the parameter backward from offk_off_units_backward_split (K1b's GEMM in split-fp32 arithmetic on the bf16
matrix pipe, for every --feat-dtype / --feat-layout; with copy the backward reads the contiguous copies); fp32 (default): the
fp32 matrix pipe's entries.  The matrix floors printed beside it count the plane products that form issues: 6 (fp32 maps), 5
(fp16), 3 (bf16) bf16 MFMA passes over K1b's FLOPs at 2.5 PFLOP/s.
--fwd-arith f32split: the train forward from offk_off_units_train_split (K1 in split-fp32 arithmetic on the bf16 matrix pipe, for every
--feat-dtype / --feat-layout; units_train_forward_ms then covers its three launches, the weight pre-pass included); fp32 (default):
the fp32 matrix pipe's entries.  The train-forward time is reported separately either way.
Under rocprofv3 --kernel-trace --stats the per-kernel split is in the stats CSV."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import offk_amd  # noqa: E402,F401
from offk_amd import runtime, spec, synth  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--length", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--variant", type=int, default=spec.VARIANT_RGB)
    ap.add_argument("--feat-dtype", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--feat-layout", default="nchw", choices=["nchw", "cl", "copy"])
    ap.add_argument("--feat-grad", action="store_true")
    ap.add_argument("--feat-grad-dtype", default="map", choices=["map", "fp32"])
    ap.add_argument("--feat-grad-arith", default="fp32", choices=list(runtime.FEAT_GRAD_ARITHS))
    ap.add_argument("--wgrad-arith", default="fp32", choices=list(runtime.WGRAD_ARITHS))
    ap.add_argument("--fwd-arith", default="fp32", choices=list(runtime.FWD_ARITHS))
    a = ap.parse_args()
    B, L = a.batch, a.length
    N, P = B * L, B * (L - 1)
    h = runtime.OffForward(B, L, a.variant, precision=a.precision, training=True)
    h.load_state_dict(synth.make_weights(a.variant))
    fdt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[a.feat_dtype]
    feats = [torch.from_numpy(f).cuda().to(fdt).contiguous() for f in synth.make_features(B, L, 2)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    bufs = [torch.randn(P, H, H, C, device="cuda", generator=gen) for H, C in ((28, 320), (14, 1056), (7, 832))]
    views = [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]
    grads = h.new_unit_grads()
    fwd_kw = {} if a.fwd_arith == "fp32" else {"arith": a.fwd_arith}      # (the default makes today's call)
    dx_layout = "nchw" if a.feat_layout == "nchw" else "cl"      # (copy: the maps the model holds are the channels_last ones)
    dx = None
    dx_dt = fdt if a.feat_grad_dtype == "map" else torch.float32
    if a.feat_grad:
        h.off_units_train(feats, 21, 0.8, **fwd_kw)
        h.off_units_backward(feats, views, 21, 0.8, grads=grads, arith=a.wgrad_arith)
        dx = h.off_units_backward_feats(layout=dx_layout, dtype=dx_dt, arith=a.feat_grad_arith)

    def dx_casts():
        return [g.to(fdt) for g in dx] if dx_dt != fdt else dx

    def dx_route():
        h.off_units_backward_feats(layout=dx_layout, out=dx, dtype=dx_dt, arith=a.feat_grad_arith)
        return dx_casts()

    def bwd(x):
        h.off_units_backward(x, views, 21, 0.8, grads=grads, arith=a.wgrad_arith)
        if a.feat_grad:
            dx_route()
    if a.feat_layout != "nchw":
        feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    if a.feat_layout == "copy":
        held = [None]

        def fwd():
            held[0] = [f.contiguous() for f in feats]        # the copies live until the backward has run, as in an autograd node
            h.off_units_train(held[0], 21, 0.8, **fwd_kw)
        t_fwd = timed(fwd, a.iters)
        t_copy = timed(lambda: [f.contiguous() for f in feats], a.iters)
        t_bwd = timed(lambda: bwd(held[0]), a.iters)
    else:
        t_fwd = timed(lambda: h.off_units_train(feats, 21, 0.8, **fwd_kw), a.iters)
        t_copy = 0.0
        t_bwd = timed(lambda: bwd(feats), a.iters)
    t_cast = timed(lambda: [f.float() for f in feats], a.iters) if fdt != torch.float32 else 0.0
    extra = {}
    if a.feat_grad:
        w = {k: torch.from_numpy(v).cuda() for k, v in synth.make_weights(a.variant).items()}

        def composed():
            out = []
            for site, C, H in spec.SITES:
                dG = h.region("dG_" + site, 128).view(N, H, H, 128).permute(0, 3, 1, 2)
                dD = h.region("dD_" + site, 32).view(P, H, H, 32).permute(0, 3, 1, 2)
                g = torch.nn.grad.conv2d_input((N, C, H, H), w["motion_conv_gen_%s.weight" % site], dG)
                g[:P].add_(torch.nn.grad.conv2d_input((P, C, H, H), w["motion_spatial_down_%s.weight" % site], dD))   # flat slice
                out.append(g)
            return out
        t_dx = timed(dx_route, a.iters)
        t_launch = timed(lambda: h.off_units_backward_feats(layout=dx_layout, out=dx, dtype=dx_dt, arith=a.feat_grad_arith), a.iters)
        t_casts = timed(dx_casts, a.iters) if dx_dt != fdt else 0.0
        t_torch = timed(composed, a.iters)
        ref = composed()
        err = max(float((a_.float() - b_).abs().max() / b_.abs().max()) for a_, b_ in zip(dx_route(), ref))
        dx_write = sum(N * C * H * H * dx[0].element_size() for _n, C, H in spec.SITES)
        dx_read = sum((N * 128 + P * 32) * H * H * 4 for _n, _c, H in spec.SITES)
        dx_flops = sum(2 * N * H * H * C * 160 for _n, C, H in spec.SITES)
        extra = {"feat_grad_arith": a.feat_grad_arith, "feat_grad_layout": dx_layout, "feat_grad_dtype": str(dx_dt).replace("torch.", ""), "feat_grad_ms": round(t_dx, 4),
                 "feat_grad_launch_ms": round(t_launch, 4), "feat_grad_casts_ms": round(t_casts, 4), "feat_grad_torch_composed_ms": round(t_torch, 4),
                 "feat_grad_vs_torch_max_rel": float("%.3g" % err), "feat_grad_bytes_read": dx_read, "feat_grad_bytes_written": dx_write,
                 "feat_grad_flops": dx_flops, "feat_grad_floor_ms_hbm_6TBs": round((dx_read + dx_write) / 6e12 * 1e3, 4),
                 "feat_grad_floor_ms_fp32_mfma_157TF": round(dx_flops / 157e12 * 1e3, 4)}
    esz = 4 if fdt == torch.float32 else 2
    hw = sum(H * H for _n, _c, H in spec.SITES)
    # K2b: read dM (160 ch, P rows) + G (128, N) + D (32, P), write dG (128, N) + dD (32, P)
    k2b = B * hw * 4 * ((160 + 32 + 32) * (L - 1) + 256 * L)
    # K1b: read X once + dG + dD (ideal); FLOPs as the forward's K1
    x_bytes = sum(N * C * H * H * esz for _n, C, H in spec.SITES)
    k1b = x_bytes + B * hw * 4 * (128 * L + 32 * (L - 1))
    flops = sum(2 * N * H * H * C * 128 + 2 * P * H * H * C * 32 for _n, C, H in spec.SITES)
    products = {"fp32": 6, "fp16": 5, "bf16": 3}[a.feat_dtype]
    extra["wgrad_arith"] = a.wgrad_arith
    extra["fwd_arith"] = a.fwd_arith
    if a.fwd_arith == "f32split":
        extra["k1_split_products"] = products
        extra["k1_floor_ms_bf16_mfma_2500TF"] = round(products * flops / 2.5e15 * 1e3, 4)
        extra["k1_floor_ms_hbm_8TBs"] = round((x_bytes + B * hw * 4 * (128 * L + 32 * (L - 1))) / 8e12 * 1e3, 4)
    if a.wgrad_arith == "f32split":
        extra["k1b_split_products"] = products
        extra["k1b_floor_ms_bf16_mfma_2500TF"] = round(products * flops / 2.5e15 * 1e3, 4)
    print(json.dumps({**extra, "feat_grad": bool(a.feat_grad), "batch": B, "length": L, "precision_fwd": a.precision, "feat_dtype": a.feat_dtype,
                      "feat_layout": a.feat_layout, "nine_contiguous_copies_ms": round(t_copy, 4),
                      "nine_float_casts_ms": round(t_cast, 4),
                      "units_train_forward_ms": round(t_fwd, 4), "units_backward_ms": round(t_bwd, 4),
                      "units_step_ms": round(t_fwd + t_bwd, 4),
                      "clips_per_s_fwd_bwd_units": round(B / (t_fwd + t_bwd) * 1e3, 1),
                      "k2b_algorithmic_bytes": k2b, "k1b_algorithmic_bytes": k1b, "k1b_flops": flops,
                      "backward_floor_ms_hbm_8TBs": round((k2b + k1b) / 8e12 * 1e3, 4),
                      "k1b_floor_ms_fp32_mfma_157TF": round(flops / 157e12 * 1e3, 4)}))


if __name__ == "__main__":
    main()
