"""One process, one library (OFFK_LIB selects an A/B build): wall-clock ms per forward and the per-launch trace.
    python tools/time_forward.py [batch] [length] [steps] [substring of the launches to list, default: all]
OFFK_FEAT_DTYPE=bf16|f16 (with OFFK_PRECISION=f32split): the maps in that dtype through offk_forward_typed (the cast is not timed).
OFFK_FEAT_LAYOUT=cl (with OFFK_PRECISION=f32split): torch.channels_last maps of that dtype through offk_forward_cl; =copy: the same
channels_last maps made contiguous inside the timed region, then the NCHW forward; =nhwc: an OFFK_FEAT_NHWC handle on offk_forward."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import offk_amd  # noqa: E402,F401
from offk_amd import _lib, runtime, spec, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
L = int(sys.argv[2]) if len(sys.argv) > 2 else 7
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
pat = sys.argv[4] if len(sys.argv) > 4 else ""
variant = spec.VARIANT_RGB
layout = os.environ.get("OFFK_FEAT_LAYOUT", "") or "nchw"
assert layout in ("nchw", "cl", "copy", "nhwc"), layout
h = runtime.OffForward(B, L, variant, precision=os.environ.get("OFFK_PRECISION", "fp32"), feat_layout=1 if layout == "nhwc" else 0)
h.load_state_dict(synth.make_weights(variant))
feats = [torch.from_numpy(f).cuda() for f in synth.make_features(B, L, 2)]
out = [torch.empty(h.out_rows(), 101, device="cuda") for _ in range(3)]
fdt = {"": None, "f32": None, "bf16": torch.bfloat16, "f16": torch.float16}[os.environ.get("OFFK_FEAT_DTYPE", "")]
if fdt is not None:
    feats = [f.to(fdt) for f in feats]
code = {None: _lib.FEAT_F32, torch.bfloat16: _lib.FEAT_BF16, torch.float16: _lib.FEAT_F16}[fdt]


def _outs(o7, o14, o28):
    return [ctypes.c_void_p(o.data_ptr()) for o in (o7, o14, o28)] + [ctypes.c_void_p(h.workspace.data_ptr())]


def _typed(arr, o7, o14, o28):
    _lib.check(h.lib.offk_forward_typed(h._h, runtime._stream(h.device), code, arr, *_outs(o7, o14, o28)), h._h)


if layout == "cl":          # the maps as a channels_last backbone hands them over, through offk_forward_cl
    feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    arr = h._feat_array(feats, runtime._check_dev_cl)

    def _cl(arr, o7, o14, o28):
        _lib.check(h.lib.offk_forward_cl(h._h, runtime._stream(h.device), code, arr, *_outs(o7, o14, o28)), h._h)
    h.forward_into = _cl
elif layout == "copy":      # the same maps made contiguous first, the nine copies inside the timed region, then the NCHW forward
    feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    arr = None

    def _copy(arr, o7, o14, o28):
        xs = [f.contiguous() for f in feats]
        a = h._feat_array(xs, runtime._check_dev if fdt is None else runtime._check_dev16)
        _typed(a, o7, o14, o28)
    h.forward_into = _copy
elif layout == "nhwc":      # an OFFK_FEAT_NHWC handle on offk_forward (fp32 maps only; the unfused units on the fp32 pipe)
    assert fdt is None, "an NHWC handle takes fp32 maps only"
    feats = [f.permute(0, 2, 3, 1).contiguous() for f in feats]
    arr = h._feat_array(feats)
elif fdt is None:
    arr = h._feat_array(feats)
else:
    arr = h._feat_array(feats, runtime._check_dev16)
    h.forward_into = _typed
for _ in range(10):
    h.forward_into(arr, *out)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    h.forward_into(arr, *out)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / steps * 1e3
print("lib=%s maps=%s layout=%s B=%d L=%d: %.4f ms / forward (%.0f clips/s), checksum %.6f" % (
    os.path.basename(os.environ.get("OFFK_LIB", "liboffk.so")), os.environ.get("OFFK_FEAT_DTYPE", "f32") or "f32", layout, B, L, ms, B / ms * 1e3, float(out[0].double().sum())))
h.set_profiling(2)
h.launch_times(reset=True)
for _ in range(20):
    h.forward_into(arr, *out)
torch.cuda.synchronize()
tot = 0.0
for name, (t, calls) in h.launch_times().items():
    tot += t / max(calls, 1)
    if pat in name:
        print("   %-86s %8.1f us" % (name[:86], t / max(calls, 1) * 1e3))
print("   sum of launch groups %.1f us" % (tot * 1e3))
