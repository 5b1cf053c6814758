"""Times the backward of the stride-1 fusion convs (offk_relu_backward, offk_conv2d_backward_data, offk_conv2d_backward_weight) against
torch's own backward of F.conv2d on the same channels-last fp32 tensors, in one process and one session.

    python tools/bench_fusion_bwd.py [--n-img 384] [--iters 30] [--warmup 5] [--out profiles/fusion_bwd/README.md]
    python tools/bench_fusion_bwd.py --wgrad-arith f32split      # the split-fp32 weight gradient beside the fp32 entry and torch
    python tools/bench_fusion_bwd.py --dgrad-arith f32split      # the split-fp32 data gradient beside the fp32 entry and torch

For each of the 13 distinct shapes of the 22 stride-1 fusion convs (spec.FUSION_CONVS): device-event time over --iters iterations after
--warmup warm-ups of the three entries separately, torch.autograd.grad of F.conv2d (input, weight and bias gradients in one call; its
forward runs outside the timed region), and the achieved TFLOP/s against the 157 TF fp32-matrix peak.  Prints a markdown table and the
sums over the 22 convs, then the table of the two stride-2 convs (tools/bench_fusion_bwd_s2.py); --out
writes the same text to a file.  --wgrad-arith f32split prints another table instead: per shape the fp32 entry's weight gradient, the
split entry's (offk_conv2d_backward_weight_split, with its own plan's chunks), the unchanged data gradient and torch's backward, same
method, same session.  --dgrad-arith f32split prints a third one in tools/bench_fusion_bwd_s2.py's method: per shape the fp32 entry's data
gradient (offk_conv2d_backward_data) and the split entry's (offk_conv2d_backward_data_split, all three launches in one event pair),
INTERLEAVED iteration by iteration with torch's backward beside them, --repeats times; the block form the plan chose; the sums over the 22
convs and over the eight 3x3 convs with their spread over the repeats; the shapes whose split entry is slower; and the split entry's
launches one by one from torch.profiler's device times.  Nothing here gates anything: the numbers are reported.
"""
import argparse
import collections
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import offk_amd  # noqa: E402,F401
from offk_amd import runtime, spec  # noqa: E402
import bench_fusion_bwd_s2  # noqa: E402  (the sibling tool: the two stride-2 convs)

PEAK_TF = 157.3


def shapes():
    """[(H, ci, co, k, how many of the 22 convs have this shape, their names)] in spec order"""
    seen = collections.OrderedDict()
    for key, co, ci, k, stride, _pad in spec.FUSION_CONVS:
        if stride != 1:
            continue
        H = 14 if "28" in key else 7
        seen.setdefault((H, ci, co, k), []).append(key)
    return [(H, ci, co, k, len(v), v) for (H, ci, co, k), v in seen.items()]


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


def split_table(n, iters, warmup):
    """the weight gradient in both arithmetics beside the data gradient and torch's backward, one session"""
    rows, tot = [], collections.Counter()
    gen = torch.Generator(device="cuda").manual_seed(1)
    for H, ci, co, k, mult, _names in shapes():
        pad = (k - 1) // 2
        x = torch.randn(n, H, H, ci, device="cuda", generator=gen)
        g = torch.randn(n, H, H, co, device="cuda", generator=gen)
        w = torch.randn(co, ci, k, k, device="cuda", generator=gen) * 0.05
        dbytes, wbytes, chunks = runtime.conv2d_backward_plan(n, H, H, ci, co, k)
        sbytes, schunks = runtime.conv2d_backward_plan_split(n, H, H, ci, co, k)
        sd, sw, ss = (torch.empty(b, dtype=torch.uint8, device="cuda") for b in (dbytes, wbytes, sbytes))
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty(co, device="cuda")
        t_data = timed(lambda: runtime.conv2d_backward_data(g, w, pad, dx=dx, scratch=sd), iters, warmup)
        t_f32 = timed(lambda: runtime.conv2d_backward_weight(x, g, k, pad, dw=dw, db=db, scratch=sw), iters, warmup)
        t_spl = timed(lambda: runtime.conv2d_backward_weight(x, g, k, pad, dw=dw, db=db, scratch=ss, arith="f32split"), iters, warmup)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)
        wt = w.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bt = torch.zeros(co, device="cuda", requires_grad=True)
        gt = g.permute(0, 3, 1, 2)
        t_torch = timed(lambda yy: torch.autograd.grad(yy, (xt, wt, bt), gt), iters, warmup, setup=lambda: F.conv2d(xt, wt, bt, padding=pad))
        rows.append((H, ci, co, k, mult, chunks, schunks, t_f32, t_spl, t_data, t_torch))
        for key, t in (("f32", t_f32), ("split", t_spl), ("data", t_data), ("torch", t_torch)):
            tot[key] += mult * t
        del x, g, w, sd, sw, ss, dx, dw, db, xt, wt, bt, gt
    lines = ["Weight gradient of the 22 stride-1 fusion convs in both arithmetics at n_img = %d (%s), %d iterations after %d warm-ups, device "
             "events, one process." % (n, torch.cuda.get_device_name(0), iters, warmup), "",
             "| map | Ci -> Co, k | convs | chunks fp32 / split | weight grad fp32 ms | weight grad f32split ms | split / fp32 | data grad ms | "
             "data + split weight ms | torch backward ms |", "|---|---|---|---|---|---|---|---|---|---|"]
    for H, ci, co, k, mult, chunks, schunks, tf, ts, td, tt in rows:
        lines.append("| %dx%d | %d -> %d, %dx%d | %d | %d / %d | %.3f | %.3f | %.2f | %.3f | %.3f | %.3f |" % (
            H, H, ci, co, k, k, mult, chunks, schunks, tf, ts, ts / tf, td, td + ts, tt))
    lines += ["", "Sum over the 22 convs: weight gradient fp32 %.3f ms, f32split %.3f ms; data gradient %.3f ms; backward with the fp32 weight "
              "gradient %.3f ms, with the split one %.3f ms; torch's backward of the same convs %.3f ms." % (
                  tot["f32"], tot["split"], tot["data"], tot["data"] + tot["f32"], tot["data"] + tot["split"], tot["torch"])]
    slower = ["%dx%d %d -> %d %dx%d (%.3f vs %.3f ms)" % (r[0], r[0], r[1], r[2], r[3], r[3], r[8], r[7]) for r in rows if r[8] > r[7]]
    lines.append("Shapes whose split weight gradient is slower than the fp32 entry's: %s." % ("; ".join(slower) if slower else "none"))
    return "\n".join(lines) + "\n"


def dgrad_split_table(n, iters, warmup, repeats):
    """the data gradient in both arithmetics, interleaved, beside torch's backward; then the split entry's launches one by one"""
    once, launch_times = bench_fusion_bwd_s2.once, bench_fusion_bwd_s2.launch_times
    lines = ["Data gradient of the 22 stride-1 fusion convs in both arithmetics at n_img = %d (%s): per repeat %d iterations after %d warm-ups, "
             "the fp32 entry, the split entry (three launches in one event pair) and torch's backward interleaved iteration by iteration, "
             "device events, one process, %d repeats." % (n, torch.cuda.get_device_name(0), iters, warmup, repeats), "",
             "| map | Ci -> Co, k | convs | block ci x pixels (blocks) | fp32 entry ms: repeats | f32split entry ms: repeats | split / fp32 (means) | "
             "fp32 - split, mean ms | larger min-max spread ms | faster by more than the spread | torch backward ms (mean) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    rows, parts = [], []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for H, ci, co, k, mult, _names in shapes():
        pad = (k - 1) // 2
        x = torch.randn(n, H, H, ci, device="cuda", generator=gen)
        g = torch.randn(n, H, H, co, device="cuda", generator=gen)
        w = torch.randn(co, ci, k, k, device="cuda", generator=gen) * 0.05
        sd = torch.empty(runtime.conv2d_backward_plan(n, H, H, ci, co, k)[0], dtype=torch.uint8, device="cuda")
        ss = torch.empty(runtime.conv2d_backward_data_plan_split(n, H, H, ci, co, k), dtype=torch.uint8, device="cuda")
        cb, pb = runtime.conv2d_backward_data_form_split(n, H, H, ci, co, k)
        blocks = -(-n * H * H // pb) * -(-ci // cb)
        dx, dxs = torch.empty_like(x), torch.empty_like(x)
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)
        wt = w.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bt = torch.zeros(co, device="cuda", requires_grad=True)
        gt = g.permute(0, 3, 1, 2)

        def f32():
            runtime.conv2d_backward_data(g, w, pad, dx=dx, scratch=sd)

        def spl():
            runtime.conv2d_backward_data(g, w, pad, dx=dxs, scratch=ss, arith="f32split")

        def tor(yy):
            torch.autograd.grad(yy, (xt, wt, bt), gt)

        reps = {"f32": [], "split": [], "torch": []}
        for _ in range(repeats):
            tot = {"f32": 0.0, "split": 0.0, "torch": 0.0}
            for it in range(warmup + iters):
                yy = F.conv2d(xt, wt, bt, padding=pad)
                t = {"f32": once(f32), "split": once(spl), "torch": once(tor, yy)}
                if it >= warmup:
                    for name in tot:
                        tot[name] += t[name]
            for name in tot:
                reps[name].append(tot[name] / iters)
        mean = dict((name, sum(v) / len(v)) for name, v in reps.items())
        spread = max(max(reps[name]) - min(reps[name]) for name in ("f32", "split"))
        gain = mean["f32"] - mean["split"]
        lines.append("| %dx%d | %d -> %d, %dx%d | %d | %d x %d (%d) | %s | %s | %.2f | %.3f | %.3f | %s | %.3f |" % (
            H, H, ci, co, k, k, mult, cb, pb, blocks, ", ".join("%.3f" % v for v in reps["f32"]), ", ".join("%.3f" % v for v in reps["split"]),
            mean["split"] / mean["f32"], gain, spread, "yes" if gain > spread else "NO", mean["torch"]))
        rows.append((H, ci, co, k, mult, reps, mean))
        parts.append((H, ci, co, k, launch_times(spl, 10), mean["split"]))
        del x, g, w, sd, ss, dx, dxs, xt, wt, bt, gt

    def sums(pick):
        """per repeat, the sum over the convs `pick` keeps (each shape times its count): {name: [repeats]}"""
        return dict((name, [sum(r[4] * r[5][name][i] for r in rows if pick(r)) for i in range(repeats)]) for name in ("f32", "split", "torch"))

    lines.append("")
    for what, pick in (("the 22 convs", lambda r: True), ("the eight 3x3 convs", lambda r: r[3] == 3)):
        sm = sums(pick)
        mean = dict((name, sum(v) / len(v)) for name, v in sm.items())
        spread = max(max(sm[name]) - min(sm[name]) for name in ("f32", "split"))
        gain = mean["f32"] - mean["split"]
        lines.append("Sum over %s (%d): data gradient fp32 %s ms (mean %.3f), f32split %s ms (mean %.3f); fp32 - split %.3f ms, larger min-max "
                     "spread %.3f ms: %s; torch's whole backward of the same convs %.3f ms." % (
                         what, sum(r[4] for r in rows if pick(r)), " / ".join("%.3f" % v for v in sm["f32"]), mean["f32"],
                         " / ".join("%.3f" % v for v in sm["split"]), mean["split"], gain, spread,
                         "faster by more than the spread" if gain > spread else "NOT faster by more than the spread", mean["torch"]))
    slower = ["%dx%d %d -> %d %dx%d (%.3f vs %.3f ms)" % (r[0], r[0], r[1], r[2], r[3], r[3], r[6]["split"], r[6]["f32"]) for r in rows
              if r[6]["split"] >= r[6]["f32"]]
    lines.append("Shapes whose split data gradient is not faster than the fp32 entry's: %s." % ("; ".join(slower) if slower else "none"))
    lines += ["", "The split entry's launches one by one (torch.profiler device time per call, mean of 10 calls; the entry's event time beside "
              "their sum):", "", "| map | Ci -> Co, k | weight pre-pass ms | g pre-pass ms | GEMM ms | sum ms | entry by events ms |", "|---|---|---|---|---|---|---|"]
    for H, ci, co, k, kt, ev in parts:
        def pick(sub):
            v = [t for name, t in kt.items() if sub in name]
            return sum(v) if v else float("nan")
        a, b, c = pick("conv_wpack_split_kernel"), pick("conv_s2_gcut_split_kernel"), pick("conv_dgrad_split_kernel")
        lines.append("| %dx%d | %d -> %d, %dx%d | %.4f | %.4f | %.4f | %.4f | %.3f |" % (H, H, ci, co, k, k, a, b, c, a + b + c, ev))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-img", type=int, default=384)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--wgrad-arith", choices=runtime.WGRAD_ARITHS, default="fp32")
    ap.add_argument("--dgrad-arith", choices=runtime.DGRAD_ARITHS, default="fp32")
    ap.add_argument("--repeats", type=int, default=3, help="--dgrad-arith f32split: repeats of the interleaved measurement")
    a = ap.parse_args()
    n = a.n_img
    if a.wgrad_arith == "f32split" or a.dgrad_arith == "f32split":
        text = dgrad_split_table(n, a.iters, a.warmup, a.repeats) if a.dgrad_arith == "f32split" else split_table(n, a.iters, a.warmup)
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        return
    rows, tot = [], collections.Counter()
    gen = torch.Generator(device="cuda").manual_seed(1)
    for H, ci, co, k, mult, names in shapes():
        pad = (k - 1) // 2
        x = torch.randn(n, H, H, ci, device="cuda", generator=gen)
        g = torch.randn(n, H, H, co, device="cuda", generator=gen)
        y = torch.randn(n, H, H, co, device="cuda", generator=gen)
        w = torch.randn(co, ci, k, k, device="cuda", generator=gen) * 0.05
        dbytes, wbytes, chunks = runtime.conv2d_backward_plan(n, H, H, ci, co, k)
        sd, sw = torch.empty(dbytes, dtype=torch.uint8, device="cuda"), torch.empty(wbytes, dtype=torch.uint8, device="cuda")
        gm, dx = torch.empty_like(g), torch.empty_like(x)
        dw, db = torch.empty_like(w), torch.empty(co, device="cuda")
        t_relu = timed(lambda: runtime.relu_backward(g, y, out=gm), a.iters, a.warmup)
        t_data = timed(lambda: runtime.conv2d_backward_data(g, w, pad, dx=dx, scratch=sd), a.iters, a.warmup)
        t_wgt = timed(lambda: runtime.conv2d_backward_weight(x, g, k, pad, dw=dw, db=db, scratch=sw), a.iters, a.warmup)
        # torch: the same tensors as logical NCHW views of the channels-last memory
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)
        wt = w.contiguous(memory_format=torch.channels_last).requires_grad_(True)
        bt = torch.zeros(co, device="cuda", requires_grad=True)
        gt = g.permute(0, 3, 1, 2)
        t_torch = timed(lambda yy: torch.autograd.grad(yy, (xt, wt, bt), gt), a.iters, a.warmup, setup=lambda: F.conv2d(xt, wt, bt, padding=pad))
        flop = 2.0 * n * H * H * ci * co * k * k
        rows.append((H, ci, co, k, mult, chunks, t_relu, t_data, t_wgt, t_torch, flop / t_data / 1e9, flop / t_wgt / 1e9))
        tot["relu"] += mult * t_relu
        tot["data"] += mult * t_data
        tot["weight"] += mult * t_wgt
        tot["torch"] += mult * t_torch
        del x, g, y, w, sd, sw, gm, dx, dw, db, xt, wt, bt, gt
    lines = ["Backward of the 22 stride-1 fusion convs at n_img = %d (%s), %d iterations after %d warm-ups, device events, one process." % (
                 n, torch.cuda.get_device_name(0), a.iters, a.warmup), "",
             "| map | Ci -> Co, k | convs | K chunks | relu_backward ms | data grad ms | TF/s (%% of %.0f) | weight grad ms | TF/s (%% of %.0f) | "
             "liboffk data + weight ms | torch backward ms |" % (PEAK_TF, PEAK_TF),
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for H, ci, co, k, mult, chunks, tr, td, tw, tt, fd, fw in rows:
        lines.append("| %dx%d | %d -> %d, %dx%d | %d | %d | %.3f | %.3f | %.1f (%.0f %%) | %.3f | %.1f (%.0f %%) | %.3f | %.3f |" % (
            H, H, ci, co, k, k, mult, chunks, tr, td, fd, 100 * fd / PEAK_TF, tw, fw, 100 * fw / PEAK_TF, td + tw, tt))
    lines += ["", "Sum over the 22 convs: data gradient %.3f ms, weight gradient %.3f ms, together %.3f ms (+ %.3f ms if every conv had a ReLU "
              "to undo); torch's backward of the same convs %.3f ms." % (tot["data"], tot["weight"], tot["data"] + tot["weight"], tot["relu"],
                                                                          tot["torch"])]
    slower = ["%dx%d %d -> %d %dx%d (%.3f vs %.3f ms)" % (r[0], r[0], r[1], r[2], r[3], r[3], r[7] + r[8], r[9]) for r in rows if r[7] + r[8] > r[9]]
    lines.append("Shapes slower than torch: %s." % ("; ".join(slower) if slower else "none"))
    text = "\n".join(lines) + "\n"
    text += "\n" + bench_fusion_bwd_s2.table(n, a.iters, a.warmup)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
