"""Times the training side of the three classifier heads (offk_head_train, offk_head_backward) against the same head composed from torch
ops (max_pool2d / mean / mask multiply / linear, with their autograd) on the same channels-last fp32 tensors, in one process and one session.

    python tools/bench_head_bwd.py [--n-img 384] [--iters 30] [--warmup 5] [--out FILE]

Device-event times.  The floor beside each launch is its algorithmic bytes (what it must read and write once: the map, the gradient map,
x again for the max-pool's argmax, fc_w, g, z, dw, db) over the 8 TB/s of the data sheet.  Nothing here gates anything: the numbers are
reported, whichever way they fall.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import offk_amd  # noqa: E402,F401
from offk_amd import runtime, synth  # noqa: E402

from bench_fusion_bwd_s2 import timed  # noqa: E402

PEAK_BPS = 8.0e12
CLASSES, DROP_P, SEED = 101, 0.8, 5
# (state_dict key, map size, channels, maxpool, head_index): RGB_OFF.py:782-787, 789-793, 843-847
HEADS = (("fc_action_motion_28", 14, 256, True, 0), ("fc_action_motion_14", 7, 512, False, 1), ("fc_action_motion", 7, 1024, False, 2))


def table(n, iters, warmup):
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(3)
    drop = (SEED, DROP_P)
    for key, H, C, maxpool, hi in HEADS:
        x = torch.randn(n, H, H, C, device="cuda", generator=gen).clamp_(min=0.0)
        w = (torch.rand(CLASSES, C, device="cuda", generator=gen) * 2 - 1) / C ** 0.5
        b = (torch.rand(CLASSES, device="cuda", generator=gen) * 2 - 1) / C ** 0.5
        g = torch.randn(n, CLASSES, device="cuda", generator=gen)
        nbytes, chunks = runtime.head_backward_plan(n, C, CLASSES)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        z, out = torch.empty(n, C, device="cuda"), torch.empty(n, CLASSES, device="cuda")
        dx, dw, db = torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
        t_fwd = timed(lambda: runtime.head_train(x, w, b, maxpool, hi, drop, z=z, out=out), iters, warmup)
        t_all = timed(lambda: runtime.head_backward(g, x, w, z, maxpool, hi, drop, dx=dx, dw=dw, db=db, scratch=scratch), iters, warmup)
        t_dx = timed(lambda: runtime.head_backward(g, x, w, z, maxpool, hi, drop, dx=dx, want_dw=False, want_db=False), iters, warmup)
        # torch: the same tensors as logical NCHW views of the channels-last memory, the same mask as a multiplier
        xt = x.permute(0, 3, 1, 2).requires_grad_(True)
        wt, bt = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        mask = torch.from_numpy(synth.head_dropout_keep(SEED, hi, n, C, DROP_P)).cuda().float() * (1.0 / (1.0 - DROP_P))

        def fwd():
            p = F.max_pool2d(xt, 3, 2, ceil_mode=True) if maxpool else xt
            return F.linear(p.mean(dim=(2, 3)) * mask, wt, bt)

        tt_fwd = timed(fwd, iters, warmup)
        tt_all = timed(lambda o: torch.autograd.grad(o, (xt, wt, bt), g), iters, warmup, setup=fwd)
        tt_dx = timed(lambda o: torch.autograd.grad(o, (xt,), g), iters, warmup, setup=fwd)
        fmap, small = 4.0 * n * H * H * C, 4.0 * (n * C + CLASSES * C + n * CLASSES)
        by_fwd = fmap + small + 4.0 * n * C
        by_dx = fmap * (2 if maxpool else 1) + 4.0 * (CLASSES * C + n * CLASSES)
        by_all = by_dx + 4.0 * (n * C + n * CLASSES + CLASSES * C + CLASSES)
        rows.append((key, H, C, maxpool, chunks, (t_fwd, tt_fwd, by_fwd), (t_all, tt_all, by_all), (t_dx, tt_dx, by_dx)))
        del x, w, b, g, scratch, z, out, dx, dw, db, xt, wt, bt, mask
    lines = ["Training side of the three heads at n_img = %d (%s), p = %.1f, %d classes, %d iterations after %d warm-ups, device events, one "
             "process.  Each cell: liboffk ms / torch composition ms / floor ms (algorithmic bytes over 8 TB/s)." % (
                 n, torch.cuda.get_device_name(0), DROP_P, CLASSES, iters, warmup), "",
             "| head | map | maxpool | chunks | train forward | backward dx + dw + db | backward dx only | forward + backward: liboffk / torch |",
             "|---|---|---|---|---|---|---|---|"]
    for key, H, C, maxpool, chunks, f, a, d in rows:
        cell = lambda t: "%.3f / %.3f / %.3f" % (t[0], t[1], 1e3 * t[2] / PEAK_BPS)      # noqa: E731
        lines.append("| %s | %dx%dx%d | %s | %d | %s | %s | %s | %.3f / %.3f |" % (key, H, H, C, "yes" if maxpool else "no", chunks, cell(f), cell(a),
                                                                                  cell(d), f[0] + a[0], f[1] + a[1]))
    slower = ["%s (%.3f vs %.3f ms)" % (r[0], r[5][0] + r[6][0], r[5][1] + r[6][1]) for r in rows if r[5][0] + r[6][0] > r[5][1] + r[6][1]]
    lines += ["", "Forward + backward slower than the torch composition: %s." % ("; ".join(slower) if slower else "none")]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-img", type=int, default=384)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    text = table(a.n_img, a.iters, a.warmup)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
