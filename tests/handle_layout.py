"""The handle list of tests/test_gpu_handle_layout.py and what it records of every handle (tools/record_handle_layout.py writes
tests/golden/handle_layout.json from the same lists): workspace sizes, regions and unit-gradient slots by name, and on the smallest handles
what the unit entries answer while a weight is missing and what binding a parameter returns.  A helper module: no tests of its own."""
import ctypes

import numpy as np
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth

from .forward import switches

GOLDEN_FILE = "handle_layout.json"
# (batch, length, OFFK_POOL_FIRST_7): P = 96 is the default gate of the pool-first 7-head, P = 240 the size with a tuned plan table
HANDLES = ((1, 2, None), (2, 3, None), (16, 7, None), (16, 7, "0"), (10, 25, None), (64, 7, None))
VARIANTS = {"rgb": spec.VARIANT_RGB, "flow": spec.VARIANT_FLOW}
PRECISIONS = ("fp32", "f32split")
SITE_FAMILIES = ("G_", "D_", "dG_", "dD_", "dwp_", "wgs_", "wgb_")
FIXED_REGIONS = ("fusion_28", "fusion_14", "fusion_7", "xt_28", "t1_28", "sa_28", "sb_28", "xu_14", "u1_14", "sa_14", "xv_7", "v1_7", "sum_7",
                 "logit_7", "logit_14", "logit_28", "pooled_7", "pooled_14", "pooled_28", "poolpart_28", "poolpart_7", "poolpart_14",
                 "wino_v", "wino_m", "poolpart_14t", "poolpart_7t", "splitk")
NEVER_REGIONS = ("G_", "wgb_5c")             # a family's bare prefix, a family with a site there is none of
UNIT_SUFFIXES = (".weight", ".bias")
# the trail: one key of each of the six unit kinds at each of two sites, and the Sobel key where the variant has it
TRAIL_SITES = ("3b", "5a")
TRAIL_HANDLE = (1, 2, None)
BIND_KEY = "motion_conv_gen_3b.weight"
UNBINDABLE = ("motion_conv1_trans_28a.weight", "fc_action_motion.bias", spec.SOBEL_KEY)


def handle_id(batch, length, pool_first, variant, precision):
    return "b%d_l%d%s|%s|%s" % (batch, length, "" if pool_first is None else "_poolfirst" + pool_first, variant, precision)


HANDLE_IDS = [handle_id(b, l, pf, v, p) for b, l, pf in HANDLES for v in VARIANTS for p in PRECISIONS]
TRAIL_IDS = [handle_id(*TRAIL_HANDLE, v, p) for v in VARIANTS for p in PRECISIONS]


def region_names():
    return [f + name for name in spec.SITE_NAMES for f in SITE_FAMILIES] + list(FIXED_REGIONS) + list(NEVER_REGIONS)


def unit_keys():
    """every unit-parameter key of either variant (the Flow variant has no motion_spatial_grad_*), and the Sobel key, which has no gradient"""
    keys = [p + name + sfx for name in spec.SITE_NAMES for p in spec.UNIT_PARAM_PREFIXES for sfx in UNIT_SUFFIXES] + [spec.SOBEL_KEY]
    return keys + ["module." + k for k in keys]


def left_out_keys(variant):
    have = spec.weight_shapes(VARIANTS[variant])
    keys = [p + name + sfx for name in TRAIL_SITES for p in spec.UNIT_PARAM_PREFIXES for sfx in UNIT_SUFFIXES] + [spec.SOBEL_KEY]
    return [k for k in keys if k in have]


class Handle:
    """offk_create / offk_destroy around a `with` block; `h` is the raw handle"""

    def __init__(self, lib, batch, length, pool_first, variant, precision):
        self.lib = lib
        cfg = _lib.OffkConfig(batch=batch, length=length, variant=VARIANTS[variant], slice_mode=spec.SLICE_FLAT,
                              consensus=1 if variant == "flow" else 0, num_classes=spec.NUM_CLASSES, feat_layout=_lib.FEAT_NCHW, device=0,
                              precision=_lib.PRECISIONS[precision])
        self.h = ctypes.c_void_p()
        with switches({} if pool_first is None else {"OFFK_POOL_FIRST_7": pool_first}):      # (read once, at offk_create)
            _lib.check(lib.offk_create(ctypes.byref(cfg), ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.offk_destroy(self.h)
        self.h = None

    def answer(self, rc, *values):
        """[0, values...] of a call that succeeded, [code, the handle's whole error text] of one that did not"""
        return [0] + [int(v) for v in values] if rc == 0 else [rc, self.lib.offk_last_error(self.h).decode()]

    def missing(self):
        buf = ctypes.create_string_buffer(256)
        n = self.lib.offk_missing_weights(self.h, buf, len(buf))
        return [n, buf.value.decode()]

    def set_weight(self, key, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        return self.lib.offk_set_weight(self.h, key.encode(), ctypes.c_void_p(a.ctypes.data), (ctypes.c_int64 * a.ndim)(*a.shape), a.ndim)

    def bind_weight(self, key, tensor):
        return self.lib.offk_bind_weight(self.h, key.encode(), ctypes.c_void_p(tensor.data_ptr()), (ctypes.c_int64 * tensor.dim())(*tensor.shape),
                                         tensor.dim())


def record_layout(lib, batch, length, pool_first, variant, precision):
    with Handle(lib, batch, length, pool_first, variant, precision) as hd:
        out = {"workspace_bytes": int(lib.offk_workspace_bytes(hd.h)), "train_workspace_bytes": int(lib.offk_train_workspace_bytes(hd.h)),
               "unit_grad_floats": int(lib.offk_unit_grad_floats(hd.h)), "missing": hd.missing(), "regions": {}, "grad_slots": {}}
        a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
        for name in region_names():
            rc = lib.offk_workspace_region(hd.h, name.encode(), ctypes.byref(a), ctypes.byref(b))
            out["regions"][name] = hd.answer(rc, a.value, b.value)
        for key in unit_keys():
            rc = lib.offk_unit_grad_slot(hd.h, key.encode(), ctypes.byref(a), ctypes.byref(b))
            out["grad_slots"][key] = hd.answer(rc, a.value, b.value)
    return out


class TrailBuffers:
    """Real device buffers for the four entries of the trail on a TRAIL_HANDLE handle: an entry that does not refuse computes on them."""

    def __init__(self, lib, hd):
        batch, length, _pf = TRAIL_HANDLE
        N, P = batch * length, batch * (length - 1)
        self.feats = [torch.from_numpy(f).cuda() for f in synth.make_features(batch, length, 3)]
        self.ws = torch.zeros(int(lib.offk_train_workspace_bytes(hd.h)), dtype=torch.uint8, device="cuda")
        self.G = [torch.zeros(N * H * H, spec.GEN_CH, device="cuda") for _n, _C, H in spec.SITES]
        self.D = [torch.zeros(P * H * H, spec.DOWN_CH, device="cuda") for _n, _C, H in spec.SITES]
        self.dm = [torch.zeros(P * H * H, spec.UNIT_CH, device="cuda") for _n, _C, H in spec.SITES]
        self.grads = torch.zeros(int(lib.offk_unit_grad_floats(hd.h)), device="cuda")
        self.feat_ptrs = (ctypes.c_void_p * spec.NUM_SITES)(*[t.data_ptr() for t in self.feats])
        self.views = (_lib.OffkGradView * spec.NUM_SITES)(*[_lib.OffkGradView(t.data_ptr(), spec.UNIT_CH, 0) for t in self.dm])


def record_trail(lib, variant, precision):
    weights = synth.make_weights(VARIANTS[variant])
    out = {}
    for left in left_out_keys(variant):
        with Handle(lib, *TRAIL_HANDLE, variant, precision) as hd:
            for key, value in weights.items():
                if key != left:
                    assert hd.set_weight(key, value) == 0, key
            buf = TrailBuffers(lib, hd)
            name = left.split(".")[0].rsplit("_", 1)[1]
            site = spec.SITE_NAMES.index(name) if name in spec.SITE_NAMES else spec.SITE_NAMES.index(TRAIL_SITES[0])
            ws = ctypes.c_void_p(buf.ws.data_ptr())
            row = {"missing": hd.missing()}
            row["offk_off_units"] = hd.answer(lib.offk_off_units(hd.h, None, buf.feat_ptrs, ws))
            row["offk_pw_reduce"] = hd.answer(lib.offk_pw_reduce(hd.h, None, site, buf.feats[site].data_ptr(), buf.G[site].data_ptr(),
                                                                 buf.D[site].data_ptr()))
            row["offk_sobel_tdiff_all"] = hd.answer(lib.offk_sobel_tdiff_all(hd.h, None, ws, 0))
            row["offk_off_units_backward"] = hd.answer(lib.offk_off_units_backward(hd.h, None, buf.feat_ptrs, buf.views, ws, 0, 0.0,
                                                                                   buf.grads.data_ptr(), 0))
            torch.cuda.synchronize()
            out["without " + left] = row
    with Handle(lib, *TRAIL_HANDLE, variant, precision) as hd:
        bound = torch.from_numpy(weights[BIND_KEY]).cuda().contiguous()
        row = {"bind": hd.answer(hd.bind_weight(BIND_KEY, bound)), "missing after bind": hd.missing(),
               "set the bound key": hd.answer(hd.set_weight(BIND_KEY, weights[BIND_KEY])),
               "bind with module.": hd.answer(hd.bind_weight("module." + BIND_KEY, bound))}
        for key in UNBINDABLE:
            shape = spec.weight_shapes(spec.VARIANT_FLOW if key == spec.SOBEL_KEY else spec.VARIANT_RGB)[key]
            row["bind " + key] = hd.answer(hd.bind_weight(key, torch.zeros(shape, device="cuda")))
        torch.cuda.synchronize()
        out["bind"] = row
    return out


def record(lib):
    """what the golden file holds, from `lib`"""
    return {"layout": {handle_id(b, l, pf, v, p): record_layout(lib, b, l, pf, v, p) for b, l, pf in HANDLES for v in VARIANTS for p in PRECISIONS},
            "trail": {handle_id(*TRAIL_HANDLE, v, p): record_trail(lib, v, p) for v in VARIANTS for p in PRECISIONS}}
