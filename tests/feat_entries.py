"""The case lists of tests/test_gpu_feat_entries.py and the World that runs them (tools/record_feat_entries.py writes
tests/golden/feat_entry_refusals.json from the same lists): what every feature-map entry of include/offk.h refuses and the launch names
of its good calls.  A helper module: no tests of its own."""
import ctypes

import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from .forward import make_handle

B, L = 1, 2
GOLDEN_FILE = "feat_entry_refusals.json"
FAMILIES = ("forward", "forward_parts", "off_units_fused", "off_units", "off_units_train", "off_units_backward", "pw_reduce")
INFER = FAMILIES[:3]
SUFFIX = {"plain": "", "typed": "_typed", "cl": "_cl"}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FDT = {"f32": _lib.FEAT_F32, "bf16": _lib.FEAT_BF16, "f16": _lib.FEAT_F16}
KIND_DTYPES = {"plain": ("f32",), "typed": ("bf16", "f16"), "cl": ("f32", "bf16", "f16")}
REFUSAL_DTYPES = {"plain": ("f32",), "typed": ("bf16",), "cl": ("f32", "f16")}     # (no check tells bf16 from fp16)
SITE = 4                       # the map a defect sits in; the site of every pw_reduce call
SENTINEL = 0x5a


def case_id(handle, family, kind, dt, defects=()):
    return "%s|offk_%s%s|%s|%s" % (handle, family, SUFFIX[kind], dt, "+".join(defects) or "-")


def refusal_cases():
    """(handle, family, kind, dtype of the maps, defects): every one is refused before anything is enqueued.  Handles: "split" / "fp32" by
    precision, "nhwc" (feat_layout 1, split-fp32), "unfused" (OFFK_FUSED_UNITS=0, split-fp32), "bound" (a gen weight bound in place)."""
    out = []
    for family in FAMILIES:
        nine = family != "pw_reduce"
        drops = family in ("off_units_train", "off_units_backward")
        for kind, dts in REFUSAL_DTYPES.items():
            for dt in dts:
                def add(handle, *defects):
                    out.append((handle, family, kind, dt, defects))
                add("split", "null_feats")
                add("split", "null_ws")
                if nine:
                    add("split", "null_map")
                else:
                    add("split", "bad_site")
                if kind != "plain":
                    add("split", "unknown_dtype")
                    add("fp32", "unknown_dtype")
                    add("split", "misaligned")
                    if nine:
                        add("split", "unknown_dtype", "null_map")
                if kind == "typed":
                    add("nhwc")
                    add("nhwc", "misaligned")
                    if nine:
                        add("nhwc", "null_map")
                if family in INFER and kind != "plain":
                    add("fp32")
                    add("bound")
                    add("unfused")
                if drops:
                    add("split", "bad_drop_p")
                    add("split", "bad_drop_p", "null_map")
                    add("split", "bad_drop_p", "null_feats")
                    if kind != "plain":
                        add("split", "bad_drop_p", "unknown_dtype")
                        add("split", "bad_drop_p", "misaligned")
                if family == "off_units_backward":
                    add("split", "bad_grad_view")
                    add("split", "null_grad")
                    add("split", "null_grads")
                    add("split", "bad_drop_p", "bad_grad_view")
        if family == "off_units_backward":
            out.append(("nhwc", family, "plain", "f32", ()))
    return out


def trace_cases():
    """(handle, family, kind, dtype): one good call each.  _typed with fp32 maps forwards to the plain entry; 16-bit and channels-last
    maps reach the inference entries on the split-fp32 handle only, the training-side entries on either."""
    out = []
    for handle in ("fp32", "split"):
        for family in FAMILIES:
            for kind in SUFFIX:
                for dt in (("f32",) + KIND_DTYPES["typed"] if kind == "typed" else KIND_DTYPES[kind]):
                    if handle == "fp32" and family in INFER and (kind == "cl" or dt != "f32"):
                        continue
                    out.append((handle, family, kind, dt))
    return out


class World:
    """The handles, maps and buffers every case shares.  Nothing here is written by a refused call."""

    def __init__(self, rt):
        self.rt = rt
        self.keep = []
        self.handles = {"split": self._handle("f32split"), "fp32": self._handle("fp32"), "nhwc": self._handle("f32split", feat_layout=1)}
        self.handles["unfused"] = self._handle("f32split", env={"OFFK_FUSED_UNITS": "0"})
        self.handles["bound"] = self._handle("f32split")
        wg = torch.from_numpy(synth.make_weights(spec.VARIANT_RGB)["motion_conv_gen_3a.weight"]).cuda().contiguous()
        self.handles["bound"].bind_weight("motion_conv_gen_3a.weight", wg)
        self.keep.append(wg)
        N, P = B * L, B * (L - 1)
        g = torch.Generator(device="cuda").manual_seed(5)
        base = [torch.relu(torch.randn(N, C, H, H, device="cuda", generator=g)) for _, C, H in spec.SITES]
        self.maps, self.offset = {}, {}
        for name, dtype in DTYPES.items():
            for cl in (False, True):
                fmt = torch.channels_last if cl else torch.contiguous_format
                self.maps[(cl, name)] = [t.to(dtype).contiguous(memory_format=fmt) for t in base]
                # the map of SITE one element off its allocation: 2 or 4 bytes past a 256-byte boundary, inside a buffer one element longer
                buf = torch.zeros(base[SITE].numel() + 1, dtype=dtype, device="cuda")
                self.offset[(cl, name)] = buf[1:]
                assert buf[1:].data_ptr() % 8 in (2, 4)
        _n, _C, H = spec.SITES[SITE]
        self.buffers = {"out7": torch.empty(P, spec.NUM_CLASSES, device="cuda"), "out14": torch.empty(P, spec.NUM_CLASSES, device="cuda"),
                        "out28": torch.empty(P, spec.NUM_CLASSES, device="cuda"),
                        "G": torch.empty(N * H * H, spec.GEN_CH, device="cuda"), "D": torch.empty(P * H * H, spec.DOWN_CH, device="cuda"),
                        "grads": self.handles["split"].new_unit_grads()}
        self.dm = [torch.zeros(P * Hs * Hs, 160, device="cuda") for _, _C, Hs in spec.SITES]      # gradient views: 160 channels, coff 0

    def _handle(self, precision, **kw):
        return make_handle(self.rt, B, L, spec.VARIANT_RGB, consensus=False, precision=precision, training=True, **kw)[0]

    def guarded(self, h):
        return [h.workspace.view(torch.uint8)] + [t.view(torch.uint8) for t in self.buffers.values()]

    def fill(self, h):
        for t in self.guarded(h):
            t.fill_(SENTINEL)
        torch.cuda.synchronize()

    def untouched(self, h):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.guarded(h))

    def call(self, handle, family, kind, dt, defects=()):
        """One call of offk_<family><suffix>; returns (return code, offk_last_error of the handle)."""
        h = self.handles[handle]
        p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
        cl = kind == "cl"
        ptrs = [t.data_ptr() for t in self.maps[(cl, dt)]]
        if "misaligned" in defects:
            assert kind != "plain" and not (kind == "typed" and dt == "f32")       # the plain entries have no alignment check
            ptrs[SITE] = self.offset[(cl, dt)].data_ptr()
        if "null_map" in defects:
            ptrs[SITE] = 0
        head = [h._h, self.rt._stream(h.device)] + ([7 if "unknown_dtype" in defects else FDT[dt]] if kind != "plain" else [])
        ws = None if "null_ws" in defects else p(h.workspace)
        b = self.buffers
        if family == "pw_reduce":
            feat = None if "null_feats" in defects else ctypes.c_void_p(ptrs[SITE])
            args = [9 if "bad_site" in defects else SITE, feat, None if "null_ws" in defects else p(b["G"]), p(b["D"])]
        else:
            if family == "forward_parts":
                arr = (_lib.OffkFeatParts * spec.NUM_SITES)()
                for i, (_n, C, _H) in enumerate(spec.SITES):
                    arr[i].n_parts, arr[i].channels[0], arr[i].data[0] = 1, C, ptrs[i]
            else:
                arr = (ctypes.c_void_p * spec.NUM_SITES)(*ptrs)
            feats = None if "null_feats" in defects else arr
            drop_p = 1.0 if "bad_drop_p" in defects else 0.5
            if family in ("forward", "forward_parts"):
                args = [feats, p(b["out7"]), p(b["out14"]), p(b["out28"]), ws]
            elif family in ("off_units", "off_units_fused"):
                args = [feats, ws]
            elif family == "off_units_train":
                args = [feats, ws, 7, drop_p]
            else:
                gv = (_lib.OffkGradView * spec.NUM_SITES)()
                for i, t in enumerate(self.dm):
                    gv[i].data, gv[i].cstride, gv[i].coff = t.data_ptr(), 160, 0
                if "bad_grad_view" in defects:
                    gv[3].coff = 2
                if "null_grad" in defects:
                    gv[3].data = None
                args = [feats, gv, ws, 7, drop_p, None if "null_grads" in defects else p(b["grads"]), 0]
        rc = getattr(h.lib, "offk_%s%s" % (family, SUFFIX[kind]))(*(head + args))
        msg = h.lib.offk_last_error(h._h)
        return rc, msg.decode() if msg else ""

    def refused(self, case):
        """[return code, message] of a call that must be refused; the sentinel check is the caller's."""
        rc, msg = self.call(*case)
        return [rc, msg]

    def traced(self, handle, family, kind, dt):
        """The launch names of one good call, in launch order."""
        h = self.handles[handle]
        if family == "off_units_backward":     # the G / D state the backward reads: the matching forward call, outside the trace
            rc, msg = self.call(handle, "off_units_train", kind, dt)
            assert rc == 0, (rc, msg)
        h.set_profiling(2)
        try:
            h.launch_times()                   # (reset)
            rc, msg = self.call(handle, family, kind, dt)
            torch.cuda.synchronize()
            assert rc == 0, (rc, msg)
            return list(h.launch_times().keys())
        finally:
            h.set_profiling(0)
