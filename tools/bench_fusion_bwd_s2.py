"""Times the backward of the two stride-2 fusion convs (offk_relu_backward, offk_conv2d_s2_backward_data, offk_conv2d_s2_backward_weight)
against torch's own backward of F.conv2d(stride=2) on the same channels-last fp32 tensors, in one process and one session.

    python tools/bench_fusion_bwd_s2.py [--n-img 384] [--iters 30] [--warmup 5] [--out FILE]
    python tools/bench_fusion_bwd_s2.py --dgrad-arith f32split      # the split-fp32 data gradient beside the fp32 entry and torch
    python tools/bench_fusion_bwd_s2.py --wgrad-arith f32split      # the split-fp32 weight gradient beside the fp32 entry and torch

tools/bench_fusion_bwd.py calls table() and prints it behind its stride-1 table.  Device-event times; TF/s counts
2 n OH OW Ci Co k^2 per gradient against the fp32-matrix peak.  --dgrad-arith f32split prints another table instead: per shape the
fp32 entry's data gradient (offk_conv2d_s2_backward_data) and the split entry's (offk_conv2d_s2_backward_data_split, all three launches in
one event pair), INTERLEAVED iteration by iteration with torch's backward beside them, --repeats times (min / mean / max and the spread
over the repeats); then the split entry's launches one by one from torch.profiler's device times (the two pre-passes, the GEMM, their
sum).  --wgrad-arith f32split does the same for the weight gradient: offk_conv2d_s2_backward_weight and
offk_conv2d_s2_backward_weight_split (the GEMM and the reduce in one event pair), interleaved with torch's backward, then both entries'
launches one by one.  Nothing here gates anything: the numbers are reported.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import offk_amd  # noqa: E402,F401
from offk_amd import runtime, spec  # noqa: E402

PEAK_TF = 157.3


def shapes():
    """[(key, H of the input map, ci, co, k, pad)] of the stride-2 fusion convs in spec order"""
    return [(key, 28 if "28" in key else 14, ci, co, k, pad) for key, co, ci, k, stride, pad in spec.FUSION_CONVS if stride == 2]


def timed(fn, iters, warmup, setup=None):
    """mean ms of fn() by device events, one pair per iteration (setup() runs outside the timed region)"""
    for _ in range(warmup):
        arg = setup() if setup else None
        fn(arg) if setup else fn()
    total = 0.0
    for _ in range(iters):
        arg = setup() if setup else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(arg) if setup else fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
    return total / iters


def table(n, iters, warmup):
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    for key, H, ci, co, k, pad in shapes():
        OH = H // 2
        x = torch.randn(n, H, H, ci, device="cuda", generator=gen)
        g = torch.randn(n, OH, OH, co, device="cuda", generator=gen)
        y = torch.randn(n, OH, OH, co, device="cuda", generator=gen)
        w = torch.randn(co, ci, k, k, device="cuda", generator=gen) * 0.05
        dbytes, wbytes, chunks = runtime.conv2d_s2_backward_plan(n, H, H, ci, co, k)
        sd, sw = torch.empty(dbytes, dtype=torch.uint8, device="cuda"), torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        gm, dx = torch.empty_like(g), torch.empty_like(x)
        dw, db = torch.empty_like(w), torch.empty(co, device="cuda")
        t_relu = timed(lambda: runtime.relu_backward(g, y, out=gm), iters, warmup)
        t_data = timed(lambda: runtime.conv2d_s2_backward_data(g, w, pad, dx=dx, scratch=sd), iters, warmup)
        t_wgt = timed(lambda: runtime.conv2d_s2_backward_weight(x, g, k, pad, dw=dw, db=db, scratch=sw), iters, warmup)
        # torch: the same tensors as logical NCHW views of the channels-last memory
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)
        wt = w.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bt = torch.zeros(co, device="cuda", requires_grad=True)
        gt = g.permute(0, 3, 1, 2)
        t_torch = timed(lambda yy: torch.autograd.grad(yy, (xt, wt, bt), gt), iters, warmup,
                        setup=lambda: F.conv2d(xt, wt, bt, stride=2, padding=pad))
        flop = 2.0 * n * OH * OH * ci * co * k * k
        rows.append((key, H, ci, co, k, chunks, t_relu, t_data, t_wgt, t_torch, flop / t_data / 1e9, flop / t_wgt / 1e9))
        del x, g, y, w, sd, sw, gm, dx, dw, db, xt, wt, bt, gt
    lines = ["Backward of the two stride-2 fusion convs at n_img = %d (%s), %d iterations after %d warm-ups, device events, one process." % (
                 n, torch.cuda.get_device_name(0), iters, warmup), "",
             "| conv | input map | Ci -> Co, k / 2 | K chunks | relu_backward ms | data grad ms | TF/s (%% of %.0f) | weight grad ms | TF/s (%% of %.0f) | "
             "liboffk data + weight ms | torch backward ms |" % (PEAK_TF, PEAK_TF),
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for key, H, ci, co, k, chunks, tr, td, tw, tt, fd, fw in rows:
        lines.append("| %s | %dx%d | %d -> %d, %dx%d | %d | %.3f | %.3f | %.1f (%.0f %%) | %.3f | %.1f (%.0f %%) | %.3f | %.3f |" % (
            key, H, H, ci, co, k, k, chunks, tr, td, fd, 100 * fd / PEAK_TF, tw, fw, 100 * fw / PEAK_TF, td + tw, tt))
    slower = ["%s (%.3f vs %.3f ms)" % (r[0], r[7] + r[8], r[9]) for r in rows if r[7] + r[8] > r[9]]
    lines += ["", "Slower than torch: %s." % ("; ".join(slower) if slower else "none")]
    return "\n".join(lines) + "\n"


def once(fn, arg=None):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(arg) if arg is not None else fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launch_times(fn, iters):
    """{kernel name: mean device ms per call of fn} from torch.profiler, over `iters` calls"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if t and "offk" in ev.key:
            out[ev.key] = t / 1000.0 / iters
    return out


def split_table(n, iters, warmup, repeats):
    """the data gradient in both arithmetics, interleaved, beside torch's backward; then the split entry's launches one by one"""
    lines = ["Data gradient of the two stride-2 fusion convs in both arithmetics at n_img = %d (%s): per repeat %d iterations after %d warm-ups, "
             "the fp32 entry, the split entry (three launches in one event pair) and torch's backward interleaved iteration by iteration, "
             "device events, one process, %d repeats." % (n, torch.cuda.get_device_name(0), iters, warmup, repeats), "",
             "| conv | Ci -> Co, k / 2 | fp32 entry ms: repeats (min / max) | f32split entry ms: repeats (min / max) | split / fp32 (means) | "
             "fp32 - split, mean ms | larger min-max spread ms | faster by more than the spread | torch backward ms (mean) |",
             "|---|---|---|---|---|---|---|---|---|"]
    parts = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    for key, H, ci, co, k, pad in shapes():
        OH = H // 2
        x = torch.randn(n, H, H, ci, device="cuda", generator=gen)
        g = torch.randn(n, OH, OH, co, device="cuda", generator=gen)
        w = torch.randn(co, ci, k, k, device="cuda", generator=gen) * 0.05
        sd = torch.empty(runtime.conv2d_s2_backward_plan(n, H, H, ci, co, k)[0], dtype=torch.uint8, device="cuda")
        ss = torch.empty(runtime.conv2d_s2_backward_plan_split(n, H, H, ci, co, k), dtype=torch.uint8, device="cuda")
        dx, dxs = torch.empty_like(x), torch.empty_like(x)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)
        wt = w.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bt = torch.zeros(co, device="cuda", requires_grad=True)
        gt = g.permute(0, 3, 1, 2)

        def f32():
            runtime.conv2d_s2_backward_data(g, w, pad, dx=dx, scratch=sd)

        def spl():
            runtime.conv2d_s2_backward_data(g, w, pad, dx=dxs, scratch=ss, arith="f32split")

        def tor(yy):
            torch.autograd.grad(yy, (xt, wt, bt), gt)

        reps = {"f32": [], "split": [], "torch": []}
        for _ in range(repeats):
            tot = {"f32": 0.0, "split": 0.0, "torch": 0.0}
            for it in range(warmup + iters):
                yy = F.conv2d(xt, wt, bt, stride=2, padding=pad)
                t = {"f32": once(f32), "split": once(spl), "torch": once(tor, yy)}
                if it >= warmup:
                    for name in tot:
                        tot[name] += t[name]
            for name in tot:
                reps[name].append(tot[name] / iters)
        mean = dict((name, sum(v) / len(v)) for name, v in reps.items())
        spread = max(max(reps[name]) - min(reps[name]) for name in ("f32", "split"))
        gain = mean["f32"] - mean["split"]
        lines.append("| %s | %d -> %d, %dx%d | %s (%.3f / %.3f) | %s (%.3f / %.3f) | %.2f | %.3f | %.3f | %s | %.3f |" % (
            key, ci, co, k, k, ", ".join("%.3f" % v for v in reps["f32"]), min(reps["f32"]), max(reps["f32"]),
            ", ".join("%.3f" % v for v in reps["split"]), min(reps["split"]), max(reps["split"]), mean["split"] / mean["f32"], gain, spread,
            "yes" if gain > spread else "NO", mean["torch"]))
        kt = launch_times(spl, iters)
        parts.append((key, kt, mean["split"]))
        del x, g, w, sd, ss, dx, dxs, xt, wt, bt, gt
    lines += ["", "The split entry's launches one by one (torch.profiler device time per call, mean of %d calls; the entry's event time beside "
              "their sum):" % iters, "", "| conv | weight pre-pass ms | g pre-pass ms | GEMM ms | sum ms | entry by events ms |", "|---|---|---|---|---|---|"]
    for key, kt, ev in parts:
        def pick(sub):
            v = [t for name, t in kt.items() if sub in name]
            return sum(v) if v else float("nan")
        a, b, c = pick("conv_s2_wpack_split_kernel"), pick("conv_s2_gcut_split_kernel"), pick("conv_s2_dgrad_split_kernel")
        lines.append("| %s | %.4f | %.4f | %.4f | %.4f | %.3f |" % (key, a, b, c, a + b + c, ev))
    return "\n".join(lines) + "\n"


def wgrad_split_table(n, iters, warmup, repeats):
    """the weight gradient in both arithmetics, interleaved, beside torch's backward; then both entries' launches one by one"""
    lines = ["Weight gradient of the two stride-2 fusion convs in both arithmetics at n_img = %d (%s): per repeat %d iterations after %d warm-ups, "
             "the fp32 entry, the split entry (the GEMM and the reduce in one event pair each) and torch's backward interleaved iteration by "
             "iteration, device events, one process, %d repeats." % (n, torch.cuda.get_device_name(0), iters, warmup, repeats), "",
             "| conv | Ci -> Co, k / 2 | K chunks fp32 / split | fp32 entry ms: repeats (min / max) | f32split entry ms: repeats (min / max) | "
             "split / fp32 (means) | fp32 - split, mean ms | larger min-max spread ms | faster by more than the spread | torch backward ms (mean) |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    parts = []
    gen = torch.Generator(device="cuda").manual_seed(2)
    for key, H, ci, co, k, pad in shapes():
        OH = H // 2
        x = torch.randn(n, H, H, ci, device="cuda", generator=gen)
        g = torch.randn(n, OH, OH, co, device="cuda", generator=gen)
        w = torch.randn(co, ci, k, k, device="cuda", generator=gen) * 0.05
        _d, fbytes, fchunks = runtime.conv2d_s2_backward_plan(n, H, H, ci, co, k)
        sbytes, schunks = runtime.conv2d_s2_backward_weight_plan_split(n, H, H, ci, co, k)
        sf, ss = torch.empty(fbytes, dtype=torch.uint8, device="cuda"), torch.empty(sbytes, dtype=torch.uint8, device="cuda")
        dw, dws = torch.empty_like(w), torch.empty_like(w)
        db, dbs = torch.empty(co, device="cuda"), torch.empty(co, device="cuda")
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)
        wt = w.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bt = torch.zeros(co, device="cuda", requires_grad=True)
        gt = g.permute(0, 3, 1, 2)

        def f32():
            runtime.conv2d_s2_backward_weight(x, g, k, pad, dw=dw, db=db, scratch=sf)

        def spl():
            runtime.conv2d_s2_backward_weight(x, g, k, pad, dw=dws, db=dbs, scratch=ss, arith="f32split")

        def tor(yy):
            torch.autograd.grad(yy, (xt, wt, bt), gt)

        reps = {"f32": [], "split": [], "torch": []}
        for _ in range(repeats):
            tot = {"f32": 0.0, "split": 0.0, "torch": 0.0}
            for it in range(warmup + iters):
                yy = F.conv2d(xt, wt, bt, stride=2, padding=pad)
                t = {"f32": once(f32), "split": once(spl), "torch": once(tor, yy)}
                if it >= warmup:
                    for name in tot:
                        tot[name] += t[name]
            for name in tot:
                reps[name].append(tot[name] / iters)
        mean = dict((name, sum(v) / len(v)) for name, v in reps.items())
        spread = max(max(reps[name]) - min(reps[name]) for name in ("f32", "split"))
        gain = mean["f32"] - mean["split"]
        lines.append("| %s | %d -> %d, %dx%d | %d / %d | %s (%.3f / %.3f) | %s (%.3f / %.3f) | %.2f | %.3f | %.3f | %s | %.3f |" % (
            key, ci, co, k, k, fchunks, schunks, ", ".join("%.3f" % v for v in reps["f32"]), min(reps["f32"]), max(reps["f32"]),
            ", ".join("%.3f" % v for v in reps["split"]), min(reps["split"]), max(reps["split"]), mean["split"] / mean["f32"], gain, spread,
            "yes" if gain > spread else "NO", mean["torch"]))
        parts.append((key, launch_times(f32, iters), mean["f32"], launch_times(spl, iters), mean["split"]))
        del x, g, w, sf, ss, dw, dws, db, dbs, xt, wt, bt, gt
    lines += ["", "Both entries' launches one by one (torch.profiler device time per call, mean of %d calls; the entry's event time beside their "
              "sum):" % iters, "", "| conv | entry | GEMM ms | reduce ms | sum ms | entry by events ms |", "|---|---|---|---|---|---|"]
    for key, kf, ef, ks, es in parts:
        for name, kt, ev, sub in (("fp32", kf, ef, "conv_s2_wgrad_kernel"), ("f32split", ks, es, "conv_s2_wgrad_split_kernel")):
            def pick(sub_):
                v = [t for kname, t in kt.items() if sub_ in kname]
                return sum(v) if v else float("nan")
            a, b = pick(sub), pick("conv_wgrad_reduce_kernel")
            lines.append("| %s | %s | %.4f | %.4f | %.4f | %.3f |" % (key, name, a, b, a + b, ev))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-img", type=int, default=384)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dgrad-arith", choices=runtime.DGRAD_ARITHS, default="fp32")
    ap.add_argument("--wgrad-arith", choices=runtime.WGRAD_ARITHS, default="fp32")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.wgrad_arith == "f32split":
        text = wgrad_split_table(a.n_img, a.iters, a.warmup, a.repeats)
    elif a.dgrad_arith == "f32split":
        text = split_table(a.n_img, a.iters, a.warmup, a.repeats)
    else:
        text = table(a.n_img, a.iters, a.warmup)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
