"""Thin PyTorch-ROCm host wrapper around the liboffk handle.

PyTorch is plumbing here (device memory, the current HIP stream); all arithmetic runs
in liboffk's HIP kernels.  Nothing in this file computes on the CPU and nothing falls
back to torch ops.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, spec


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device=None):
    """HIP stream the call is enqueued on: torch's current stream OF THE DEVICE THE DATA LIVES ON (a handle on cuda:1
    must not launch on cuda:0's stream just because cuda:0 is torch's current device)."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_dev(t, name, device):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError("%s must be a contiguous fp32 CUDA/HIP tensor" % name)
    if t.device != device:
        raise ValueError("%s lives on %s, handle on %s" % (name, t.device, device))


def _given(t, shape, name, device, dtype=torch.float32):
    """A buffer the caller supplies instead of the one the wrapper would allocate (tests that guard the memory around it):
    contiguous, on `device`, of `dtype` and of EXACTLY the documented element count; None: allocate as ever."""
    n = int(np.prod(shape))
    if t is None:
        return torch.empty(n, dtype=dtype, device=device).view(*shape)
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError("%s must be a contiguous %s CUDA/HIP tensor" % (name, dtype))
    if t.device != torch.device(device):
        raise ValueError("%s lives on %s, the call runs on %s" % (name, t.device, device))
    if t.numel() != n:
        raise ValueError("%s holds %d elements, the documented size is %d %s" % (name, t.numel(), n, tuple(shape)))
    return t.view(*shape)


# 16-bit feature maps (offk_forward_typed): what an autocast backbone hands over
_FEAT_DTYPES = {torch.bfloat16: _lib.FEAT_BF16, torch.float16: _lib.FEAT_F16}


def _check_dev16(t, name, device):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in _FEAT_DTYPES and t.is_contiguous()):
        raise ValueError("%s must be a contiguous bf16 or fp16 CUDA/HIP tensor" % name)
    if t.device != device:
        raise ValueError("%s lives on %s, handle on %s" % (name, t.device, device))


def feat_dtype(feats):
    """The one dtype of nine feature maps (tensors or lists of channel groups); ValueError when they mix dtypes."""
    dts = set()
    for f in feats:
        for t in ([f] if torch.is_tensor(f) else list(f)):
            dts.add(t.dtype if torch.is_tensor(t) else type(t))
    if len(dts) != 1:
        raise ValueError("feature maps must all have one dtype, got %s" % sorted(str(d) for d in dts))
    return dts.pop()


# channels_last feature maps (offk_forward_cl): what a backbone run in torch.channels_last hands over, in any of the three dtypes
_CL_DTYPES = {torch.float32: _lib.FEAT_F32, torch.bfloat16: _lib.FEAT_BF16, torch.float16: _lib.FEAT_F16}


def feat_layout(feats, batch, length):
    """The one physical layout of nine feature maps (tensors or lists of channel groups); works on CPU tensors.
    "nchw": every tensor is_contiguous() (what every entry took so far; shapes are the entry's business).
    "cl":   every tensor has the reference's logical shape [B*L, C, H, H] (a channel group: its own C) and is
            contiguous in torch.channels_last, i.e. physically [B*L, H, H, C].
    ValueError when the maps do not have one layout, or when a tensor is neither."""
    if len(feats) != spec.NUM_SITES:
        raise ValueError("need nine feature maps")
    shapes = spec.feature_shapes(batch, length)
    kinds = set()
    for i, (f, s) in enumerate(zip(feats, shapes)):
        for q, t in enumerate([f] if torch.is_tensor(f) else list(f)):
            name = "feats[%d]" % i if torch.is_tensor(f) else "feats[%d][%d]" % (i, q)
            if not torch.is_tensor(t):
                raise ValueError("%s is not a tensor" % name)
            if t.is_contiguous():
                kinds.add("nchw")
            elif t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
                want = (s[0], t.shape[1], s[2], s[3])
                if tuple(t.shape) != want:
                    raise ValueError("%s is channels_last with logical shape %s, expected %s" % (name, tuple(t.shape), want))
                kinds.add("cl")
            else:
                raise ValueError("%s is neither contiguous nor torch.channels_last" % name)
    if len(kinds) != 1:
        raise ValueError("feature maps must all have one layout (all contiguous or all torch.channels_last), got a mix")
    return kinds.pop()


def _check_dev_cl(t, name, device):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in _CL_DTYPES and t.dim() == 4
            and t.is_contiguous(memory_format=torch.channels_last)):
        raise ValueError("%s must be a channels_last fp32, bf16 or fp16 CUDA/HIP tensor" % name)
    if t.device != device:
        raise ValueError("%s lives on %s, handle on %s" % (name, t.device, device))


# ---- where nine maps go: ONE rule for every entry that takes them ("Feature-map kinds") ----
Route = collections.namedtuple("Route", "route fdt parts")   # "cl" / "typed" / "plain"; enum offk_feat_dtype; any map in channel groups
# route -> (suffix of the C entry, the check every map pointer passes before the call)
_KINDS = {"plain": ("", _check_dev), "typed": ("_typed", _check_dev16), "cl": ("_cl", _check_dev_cl)}
# operation -> the side of the rule it follows; a side is the ladder below with ("infer") or without ("train") conditions on the handle
_SIDES = {"forward": "infer", "forward_parts": "infer", "off_units_fused": "infer",
          "off_units": "train", "off_units_train": "train", "off_units_backward": "train", "pw_reduce": "train"}
# {operation: {route: (entry name, pointer check)}}
_ENTRIES = {op: {route: ("offk_" + op + sfx, check) for route, (sfx, check) in _KINDS.items()} for op in _SIDES}


def _is_channels_last(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)


def _all_channels_last(feats, batch, length, side, split):
    """The first rung: every map a torch.channels_last tensor of the reference's logical shape.  Mixed layouts raise (feat_layout);
    whatever else is not this case is False and meets the checks it always met.  The inference side looks into channel groups and
    needs a split-fp32 handle; the training side has no parts form (a list is not this case) and no condition on the handle."""
    ts = list(feats) if side == "train" else [t for f in feats for t in ([f] if torch.is_tensor(f) else list(f))]
    if any(not torch.is_tensor(t) for t in ts) or all(t.is_contiguous() for t in ts) or not any(_is_channels_last(t) for t in ts):
        return False                                   # no channels_last map among them: the contiguity checks name the offender
    if feat_layout(feats, batch, length) != "cl":
        return False
    if side == "infer" and not split:
        raise ValueError("feature maps must be contiguous fp32 CUDA/HIP tensors on this handle (the fp32 pipe): channels_last "
                         "maps need a split-fp32 handle (precision=\"f32split\")")
    return True


def feat_route(feats, batch, length, handle_layout, handle_precision, side):
    """Route(route, fdt, parts) of nine feature maps (tensors or lists of channel groups); a pure function of dtypes, shapes and
    strides, so it works on CPU tensors.  side "infer" (forward, off_units_fused) or "train" (off_units, off_units_train,
    off_units_backward).  The ladder:
      "cl"     all nine torch.channels_last: the _cl entries, maps as they are.  Inference: on a feat_layout 0 handle only, and a
               ValueError unless it is split-fp32; training: any handle.
      "typed"  bf16 / fp16 maps of one dtype: the _typed entries.  Inference: a ValueError unless the handle is split-fp32.
      "plain"  everything else: the untyped entries and the checks they always made (parts: some map came as channel groups)."""
    if len(feats) != spec.NUM_SITES:
        raise ValueError("need nine feature maps")
    split = handle_precision in (_lib.PRECISION_F32SPLIT, "f32split")      # (the code or its name in _lib.PRECISIONS)
    parts = any(not torch.is_tensor(f) for f in feats)
    if (side == "train" or handle_layout == 0) and _all_channels_last(feats, batch, length, side, split):
        dt = feat_dtype(feats)
        if dt not in _CL_DTYPES:
            raise ValueError("channels_last feature maps must be fp32, bf16 or fp16, got %s" % dt)
        return Route("cl", _CL_DTYPES[dt], parts)
    if side == "infer" or not parts:                   # (training side, a non-tensor among the nine: _feat_array names the offender)
        dt = feat_dtype(feats)
        if dt in _FEAT_DTYPES:
            if side == "infer" and not split:
                raise ValueError("bf16 / fp16 feature maps need a split-fp32 handle (precision=\"f32split\"); this one runs the fp32 pipe")
            return Route("typed", _FEAT_DTYPES[dt], parts)
    return Route("plain", _lib.FEAT_F32, parts)


def train_feat_layout(feats, batch, length):
    """"cl" where feat_route(side="train") sends nine maps to the offk_*_cl training entries, else "nchw"; the dtype plays no part
    here.  Works on CPU tensors.  A mix of layouts raises, as feat_layout does."""
    if len(feats) != spec.NUM_SITES:
        raise ValueError("need nine feature maps")
    return "cl" if _all_channels_last(feats, batch, length, "train", True) else "nchw"


# the arithmetic of the feature-map gradient: "fp32" = offk_off_units_backward_feats[_typed], "f32split" = offk_off_units_backward_feats_split
FEAT_GRAD_ARITHS = ("fp32", "f32split")
# the arithmetic of the weight-gradient GEMM of the units' backward: "fp32" = offk_off_units_backward[_typed / _cl], "f32split" =
# offk_off_units_backward_split
WGRAD_ARITHS = ("fp32", "f32split")
# the arithmetic of the units' forward (off_units, off_units_train): "fp32" = K1 on the fp32 matrix pipe, "f32split" = offk_off_units_train_split
FWD_ARITHS = ("fp32", "f32split")
# the arithmetic of the fusion convs' data gradient: "fp32" = offk_conv2d[_s2]_backward_data, "f32split" = offk_conv2d[_s2]_backward_data_split
DGRAD_ARITHS = ("fp32", "f32split")
# FusionConv2d's one switch for all its gradient GEMMs: "f32split" = every one of them that has a split entry runs on it
BWD_ARITHS = ("fp32", "f32split")


def feat_grad_sites(needs_input_grad, first=0):
    """The sites whose map wants a gradient, from an autograd node's ``ctx.needs_input_grad``: the nine maps are its inputs
    ``first .. first + 8``.  A pure function of the flags (CPU)."""
    flags = tuple(needs_input_grad)[first:first + spec.NUM_SITES]
    if len(flags) != spec.NUM_SITES:
        raise ValueError("need the flags of nine feature maps, got %d" % len(flags))
    return [i for i, f in enumerate(flags) if f]


def feat_grad_sites_mask(sites):
    """sites (None: all nine, else site indices 0..8, each once) -> nine booleans."""
    if sites is None:
        return [True] * spec.NUM_SITES
    sites = [int(i) for i in sites]
    if any(not 0 <= i < spec.NUM_SITES for i in sites) or len(set(sites)) != len(sites):
        raise ValueError("sites must be distinct indices in 0..8, got %s" % (sites,))
    return [i in sites for i in range(spec.NUM_SITES)]


def _check_fwd_arith(arith):
    if arith not in FWD_ARITHS:
        raise ValueError("arith must be one of %s, got %r" % (", ".join(repr(a) for a in FWD_ARITHS), arith))


class OffForward:
    """One liboffk handle for a fixed (batch, length, variant).

    Stands for the OFF part of BNInception_OFF (reference RGB_OFF.py:265-358 declarations,
    :596-860 forward; Flow_OFF.py:606-887).
    """

    def __init__(self, batch, length, variant=spec.VARIANT_RGB, slice_mode=spec.SLICE_FLAT,
                 consensus=None, num_classes=spec.NUM_CLASSES, feat_layout=0, device=None, precision=0,
                 training=False):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.OffkError("no HIP device visible: the OFF forward has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if consensus is None:  # reference default: only the Flow / v2 files apply it
            consensus = variant == spec.VARIANT_FLOW
        self.batch, self.length, self.variant = int(batch), int(length), int(variant)
        self.slice_mode, self.consensus, self.num_classes = int(slice_mode), bool(consensus), int(num_classes)
        self.feat_layout = int(feat_layout)
        self.precision = _lib.PRECISIONS[precision] if isinstance(precision, str) else int(precision)
        self.N = self.batch * self.length
        self.P = self.batch * (self.length - 1)
        cfg = _lib.OffkConfig(self.batch, self.length, self.variant, self.slice_mode, int(self.consensus),
                              self.num_classes, self.feat_layout, self.device.index or 0, self.precision)
        h = ctypes.c_void_p()
        _lib.check(self.lib.offk_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self._ws = None
        self.training = bool(training)   # allocate the workspace superset the units' backward needs

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.offk_destroy(h)
            self._h = None

    # ---- weights ----------------------------------------------------------------
    def set_weight(self, key, value):
        if torch.is_tensor(value):
            t = value.detach().to(dtype=torch.float32).contiguous()
            shape = tuple(t.shape)
            ptr, keep = ctypes.c_void_p(t.data_ptr()), t
        else:
            a = np.ascontiguousarray(value, dtype=np.float32)
            shape = a.shape
            ptr, keep = ctypes.c_void_p(a.ctypes.data), a
        arr = (ctypes.c_int64 * len(shape))(*shape)
        _lib.check(self.lib.offk_set_weight(self._h, key.encode(), ptr, arr, len(shape)), self._h)
        del keep

    def bind_weight(self, key, tensor):
        """offk_bind_weight: the library reads ``tensor`` (a contiguous fp32 parameter on this device, reference layout)
        in place from now on -- no copy now, none after an optimizer step.  The caller keeps it alive."""
        _check_dev(tensor, key, self.device)
        kk = key[7:] if key.startswith("module.") else key
        want = spec.weight_shapes(self.variant).get(kk)
        if want is not None and tuple(tensor.shape) != tuple(want):
            raise ValueError("%s has shape %s, the reference's is %s" % (key, tuple(tensor.shape), tuple(want)))
        shape = (ctypes.c_int64 * tensor.dim())(*tensor.shape)
        _lib.check(self.lib.offk_bind_weight(self._h, key.encode(), ctypes.c_void_p(tensor.data_ptr()), shape, tensor.dim()), self._h)

    def load_state_dict(self, state_dict, strict=True):
        """Accepts a reference-format state_dict (extra backbone keys are ignored;
        a 'module.' prefix is accepted, test_flow_off.py:52-58)."""
        want = spec.weight_shapes(self.variant)
        seen = set()
        for k, v in state_dict.items():
            kk = k[7:] if k.startswith("module.") else k
            if kk in want:
                self.set_weight(kk, v)
                seen.add(kk)
        missing = [k for k in want if k not in seen]
        if strict and missing:
            raise KeyError("missing OFF weights: %s" % ", ".join(missing[:5]))
        return missing

    def missing_weights(self):
        buf = ctypes.create_string_buffer(256)
        n = self.lib.offk_missing_weights(self._h, buf, 256)
        return n, buf.value.decode()

    # ---- workspace ----------------------------------------------------------------
    @property
    def workspace_bytes(self):
        if self.training:
            return int(self.lib.offk_train_workspace_bytes(self._h))
        return int(self.lib.offk_workspace_bytes(self._h))

    @property
    def workspace(self):
        if self._ws is None:
            self._ws = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def set_workspace(self, t):
        """Use the caller's buffer (uint8, on the handle's device, at least workspace_bytes) instead of the cached allocation."""
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise ValueError("the workspace must be a contiguous uint8 CUDA/HIP tensor")
        if t.device != self.device:
            raise ValueError("the workspace lives on %s, handle on %s" % (t.device, self.device))
        if t.numel() < self.workspace_bytes:
            raise ValueError("the workspace holds %d bytes, the handle needs %d" % (t.numel(), self.workspace_bytes))
        self._ws = t

    def region(self, name, channels):
        """View of a named workspace region as [rows, channels] fp32 (channels-last).  sum_7: filled first where the last forward left
        it out (offk_stage_tensors; handles that take the 7-head pool-first)."""
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        if name == "sum_7":
            _lib.check(self.lib.offk_stage_tensors(self._h, _stream(self.device), _ptr(self.workspace)), self._h)
        _lib.check(self.lib.offk_workspace_region(self._h, name.encode(), ctypes.byref(off), ctypes.byref(nb)), self._h)
        flat = self.workspace[off.value:off.value + nb.value].view(torch.float32)
        return flat.view(-1, channels)

    # ---- forward --------------------------------------------------------------------
    def out_rows(self):
        return self.batch if self.consensus else self.P

    def _route(self, feats, side):
        return feat_route(feats, self.batch, self.length, self.feat_layout, self.precision, side)

    def takes_channels_last(self, feats):
        """True when these nine maps go to the channels-last entries as they are (offk_forward_cl: no copy, no cast): the "cl" rung
        of feat_route's inference side, whatever their dtype."""
        return (self.feat_layout == 0 and len(feats) == spec.NUM_SITES
                and _all_channels_last(feats, self.batch, self.length, "infer", self.precision == _lib.PRECISION_F32SPLIT))

    def train_takes_channels_last(self, feats):
        """True when these nine maps go to the channels-last training entries as they are (offk_off_units_cl and its siblings: no
        copy, no cast, any handle); see train_feat_layout."""
        return train_feat_layout(feats, self.batch, self.length) == "cl"

    def _call(self, op, r, *args):
        """offk_<op>, offk_<op>_typed or offk_<op>_cl by the route; args: what follows (h, stream[, feat_dtype])."""
        head = (self._h, _stream(self.device)) + (() if r.route == "plain" else (r.fdt,))
        _lib.check(getattr(self.lib, _ENTRIES[op][r.route][0])(*(head + args)), self._h)

    def _units_call(self, op, feats, *tail):
        """resolve, build the array, call: the entries that take nine whole maps and the workspace"""
        r = self._route(feats, _SIDES[op])
        self._call(op, r, self._feat_array(feats, _ENTRIES[op][r.route][1]), _ptr(self.workspace), *tail)

    def _feat_array(self, feats, check=_check_dev):
        if len(feats) != spec.NUM_SITES:
            raise ValueError("need nine feature maps")
        shapes = spec.feature_shapes(self.batch, self.length)
        for i, (f, s) in enumerate(zip(feats, shapes)):
            check(f, "feats[%d]" % i, self.device)
            want = s if self.feat_layout == 0 or check is _check_dev_cl else (s[0], s[2], s[3], s[1])   # channels_last: the logical shape
            if tuple(f.shape) != tuple(want):
                raise ValueError("feats[%d] has shape %s, expected %s" % (i, tuple(f.shape), tuple(want)))
        return (ctypes.c_void_p * spec.NUM_SITES)(*[f.data_ptr() for f in feats])

    def _parts_array(self, feats, check=_check_dev):
        """feats[i] is a tensor or a sequence of 1..4 tensors (channel groups in concat order)."""
        shapes = spec.feature_shapes(self.batch, self.length)
        arr = (_lib.OffkFeatParts * spec.NUM_SITES)()
        for i, (f, s) in enumerate(zip(feats, shapes)):
            parts = [f] if torch.is_tensor(f) else list(f)
            if not 1 <= len(parts) <= 4:
                raise ValueError("feats[%d]: 1..4 channel groups" % i)
            arr[i].n_parts = len(parts)
            for q, t in enumerate(parts):
                check(t, "feats[%d][%d]" % (i, q), self.device)
                c = t.shape[1] if self.feat_layout == 0 else t.shape[3]
                want = (s[0], c, s[2], s[3]) if self.feat_layout == 0 else (s[0], s[2], s[3], c)
                if tuple(t.shape) != want:
                    raise ValueError("feats[%d][%d] has shape %s, expected %s" % (i, q, tuple(t.shape), want))
                arr[i].channels[q] = c
                arr[i].data[q] = t.data_ptr()
        return arr

    def _outs(self, out, want28):
        """The three logits buffers: fresh ones, or the caller's (out7, out14, out28) -- out28 None means no 28 head."""
        shape = (self.out_rows(), self.num_classes)
        if out is None:
            out7 = torch.empty(shape, dtype=torch.float32, device=self.device)
            return out7, torch.empty_like(out7), torch.empty_like(out7) if want28 else None
        out7, out14, out28 = out
        return (_given(out7, shape, "out7", self.device), _given(out14, shape, "out14", self.device),
                _given(out28, shape, "out28", self.device) if out28 is not None else None)

    def forward(self, feats, want28=True, out=None):
        """feats: nine fp32 maps, or nine bf16 / fp16 maps of one dtype (split-fp32 handles: offk_forward_typed, the values of
        the same maps upcast); each map a tensor or a list of its channel groups.  Logits are fp32 either way.
        out: the caller's (out7, out14, out28) instead of fresh tensors (out28 None: no 28 head).
        torch.channels_last maps of any of the three dtypes (all nine, logical shape as ever) are taken as they are on a split-fp32
        handle (offk_forward_cl) and give the values of their contiguous copies."""
        r = self._route(feats, "infer")
        if r.route == "cl":
            return self._forward_cl(feats, want28, **({} if out is None else {"out": out}))
        return self._forward(feats, want28, out, r)

    def _forward(self, feats, want28, out, r):
        op = "forward_parts" if r.parts else "forward"
        arr = (self._parts_array if r.parts else self._feat_array)(feats, _ENTRIES[op][r.route][1])
        out7, out14, out28 = self._outs(out, want28)
        self._call(op, r, arr, _ptr(out7), _ptr(out14), _ptr(out28), _ptr(self.workspace))
        return out7, out14, out28

    def _forward_cl(self, feats, want28, out=None):
        """forward() of nine channels_last maps, under a name of its own: what the mirror class's test hooks to see them arrive"""
        return self._forward(feats, want28, out, self._route(feats, "infer"))

    def forward_into(self, feat_array, out7, out14, out28):
        """Launch-only variant for benchmarking: pre-validated ctypes array + outputs."""
        _lib.check(self.lib.offk_forward(self._h, _stream(self.device), feat_array, _ptr(out7), _ptr(out14), _ptr(out28),
                                         _ptr(self.workspace)), self._h)

    def off_units(self, feats, arith="fp32"):
        """K1 + K2 into the workspace.  feats: nine fp32 maps, or nine bf16 / fp16 maps of one dtype (offk_off_units_typed: the values
        of the same maps upcast, on any handle).  Nine torch.channels_last maps of any of the three dtypes are taken as they are
        (offk_off_units_cl, any handle) and give the values of their contiguous copies.
        arith: "fp32" (the default: the entries above) or "f32split" (offk_off_units_train_split with drop_p = 0: K1 in split-fp32
        arithmetic on the bf16 matrix pipe, for every dtype and layout of the maps; G / D get bits of their own)."""
        _check_fwd_arith(arith)
        if arith == "f32split":
            return self._units_split(feats, 0, 0.0)
        self._units_call("off_units", feats)

    def off_units_fused(self, feats):
        """The units as forward() runs them (fused K1T + S-blocks, the handle's arithmetic); results in the fusion_* / D_* regions.
        bf16 / fp16 maps (split-fp32 handles): offk_off_units_fused_typed; torch.channels_last maps: offk_off_units_fused_cl."""
        self._units_call("off_units_fused", feats)

    # ---- training side of the units ----------------------------
    def off_units_train(self, feats, drop_seed=0, drop_p=0.8, arith="fp32"):
        """K1+K2 in training mode: nn.Dropout(p) (RGB_OFF.py:356, :612) on the spatial gradients with the
        reproducible mask of synth.dropout_keep; leaves G/D in the workspace for off_units_backward.
        bf16 / fp16 maps of one dtype are taken as they are (offk_off_units_train_typed), and so are nine torch.channels_last maps
        of any of the three dtypes (offk_off_units_train_cl).
        arith: "fp32" (the default: the entries above) or "f32split" (offk_off_units_train_split: K1 in split-fp32 arithmetic on the
        bf16 matrix pipe, for every dtype and layout of the maps; G / D get bits of their own, K2 and the backward run unchanged)."""
        _check_fwd_arith(arith)
        if arith == "f32split":
            return self._units_split(feats, drop_seed, drop_p)
        self._units_call("off_units_train", feats, ctypes.c_uint64(int(drop_seed)), float(drop_p))

    def _units_split(self, feats, drop_seed, drop_p):
        """offk_off_units_train_split with the dtype and layout the route found (plain: contiguous fp32 -> NCHW)"""
        r = self._route(feats, "train")
        arr = self._feat_array(feats, _ENTRIES["off_units_train"][r.route][1])
        _lib.check(self.lib.offk_off_units_train_split(self._h, _stream(self.device), r.fdt, _lib.FEAT_NHWC if r.route == "cl" else _lib.FEAT_NCHW,
                                                       arr, _ptr(self.workspace), ctypes.c_uint64(int(drop_seed)), float(drop_p)), self._h)

    def unit_grad_slots(self):
        """OrderedDict key -> (offset, shape) of every unit parameter in the flat gradient buffer."""
        from collections import OrderedDict
        out = OrderedDict()
        for key, shape in spec.weight_shapes(self.variant).items():
            if not key.startswith(spec.UNIT_PARAM_PREFIXES):
                continue
            off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(self.lib.offk_unit_grad_slot(self._h, key.encode(), ctypes.byref(off), ctypes.byref(cnt)), self._h)
            assert cnt.value == int(np.prod(shape))
            out[key] = (off.value, shape)
        return out

    def new_unit_grads(self):
        return torch.zeros(int(self.lib.offk_unit_grad_floats(self._h)), dtype=torch.float32, device=self.device)

    def off_units_backward(self, feats, grad_views, drop_seed=0, drop_p=0.0, grads=None, accumulate=False, arith="fp32"):
        """Gradients of the units' parameters.  grad_views: nine (tensor, coff) pairs -- a channels-last
        gradient buffer [P, H, W, Cs] (or [P*H*W, Cs]) and the first of the unit's 160 channels in it.
        Needs training=True (workspace superset) and the G/D state of the matching forward call.
        feats: the maps of the matching forward call, fp32 or bf16 / fp16 of one dtype (offk_off_units_backward_typed; gradients
        are fp32 and equal those from the upcast maps), contiguous or all nine torch.channels_last (offk_off_units_backward_cl;
        equal to the gradients from the contiguous copies).
        arith: "fp32" (the default: the entries above, the weight-gradient GEMM on the fp32 matrix pipe) or "f32split"
        (offk_off_units_backward_split: that GEMM in split-fp32 arithmetic on the bf16 matrix pipe, for every dtype and layout of
        the maps; the two weight matrices get bits of their own, every other gradient and dG / dD keep the default's).
        Returns (flat grads tensor, dict key -> view in the reference's parameter shape)."""
        if arith not in WGRAD_ARITHS:
            raise ValueError("arith must be one of %s, got %r" % (", ".join(repr(a) for a in WGRAD_ARITHS), arith))
        if not self.training:
            raise _lib.OffkError("create the handle with training=True for the units' backward")
        r = self._route(feats, "train")
        arr = self._feat_array(feats, _ENTRIES["off_units_backward"][r.route][1])
        gv = (_lib.OffkGradView * spec.NUM_SITES)()
        for i, ((t, coff), (_n, _c, H)) in enumerate(zip(grad_views, spec.SITES)):
            _check_dev(t, "grad_views[%d]" % i, self.device)
            if t.numel() != self.P * H * H * t.shape[-1]:
                raise ValueError("grad_views[%d] has %d elements, expected P*H*W*%d" % (i, t.numel(), t.shape[-1]))
            gv[i].data, gv[i].cstride, gv[i].coff = t.data_ptr(), t.shape[-1], int(coff)
        if grads is None:
            grads = self.new_unit_grads()
        _check_dev(grads, "grads", self.device)
        tail = (arr, gv, _ptr(self.workspace), ctypes.c_uint64(int(drop_seed)), float(drop_p), _ptr(grads), int(bool(accumulate)))
        if arith == "f32split":    # layout and dtype of the call: what the route found (plain: contiguous fp32 -> NCHW)
            _lib.check(self.lib.offk_off_units_backward_split(self._h, _stream(self.device), r.fdt, _lib.FEAT_NHWC if r.route == "cl" else _lib.FEAT_NCHW,
                                                              *tail), self._h)
        else:
            self._call("off_units_backward", r, *tail)
        views = dict((k, grads[off:off + int(np.prod(shape))].view(shape)) for k, (off, shape) in self.unit_grad_slots().items())
        return grads, views

    def off_units_backward_feats(self, sites=None, layout="nchw", out=None, accumulate=False, dtype=torch.float32, arith="fp32"):
        """Gradient w.r.t. the feature maps (offk_off_units_backward_feats): one launch, from what the LAST off_units_backward on this
        handle left in the workspace and the gen / down weights as they are now (bound weights: call it before the optimizer step).
        sites: the site indices wanted (None: all nine).  layout "nchw": contiguous [B*L, C, H, H] tensors; "cl": the same logical
        shape with torch.channels_last strides.  out: nine entries (None where a site is skipped) to write -- or, accumulate=True,
        add -- into instead of fresh tensors.  dtype: torch.float32 (offk_off_units_backward_feats), or torch.bfloat16 / torch.float16
        (offk_off_units_backward_feats_typed: the kernel rounds each fp32 sum once, to nearest-even -- bit-equal to the fp32 result's
        .to(dtype); accumulate: (old.float() + dx32).to(dtype)); fresh tensors and `out` tensors are of that dtype.  Returns a list of
        nine, None for the skipped sites.
        arith: "fp32" (the default: the entries above, exact fp32 on the fp32 matrix pipe) or "f32split"
        (offk_off_units_backward_feats_split: split-fp32 arithmetic on the bf16 matrix pipe for every dtype, a weight pre-pass plus
        the GEMM; its own bits, reproducible, the 16-bit forms bit-equal to ITS fp32 result's .to(dtype))."""
        if arith not in FEAT_GRAD_ARITHS:
            raise ValueError("arith must be one of %s, got %r" % (", ".join(repr(a) for a in FEAT_GRAD_ARITHS), arith))
        if not self.training:
            raise _lib.OffkError("create the handle with training=True for the units' backward")
        if layout not in ("nchw", "cl"):
            raise ValueError("layout must be \"nchw\" or \"cl\", got %r" % (layout,))
        if dtype not in _CL_DTYPES:
            raise ValueError("dtype must be torch.float32, torch.bfloat16 or torch.float16, got %r" % (dtype,))
        dname = {torch.float32: "an fp32", torch.bfloat16: "a bf16", torch.float16: "an fp16"}[dtype]
        want = feat_grad_sites_mask(sites)
        if out is not None and len(out) != spec.NUM_SITES:
            raise ValueError("out must have nine entries (None for a skipped site)")
        if accumulate and out is None:
            raise ValueError("accumulate=True needs the tensors to add to (out)")
        res = [None] * spec.NUM_SITES
        for i, (n, c, h, _w) in enumerate(spec.feature_shapes(self.batch, self.length)):
            if not want[i]:
                continue
            t = out[i] if out is not None else None
            if t is None:
                if accumulate:
                    raise ValueError("accumulate=True: out[%d] is None but site %d is asked for" % (i, i))
                t = torch.empty((n, c, h, h) if layout == "nchw" else (n, h, h, c), dtype=dtype, device=self.device)
                t = t if layout == "nchw" else t.permute(0, 3, 1, 2)
            dense = t.is_contiguous() if layout == "nchw" else _is_channels_last(t)
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 4 and dense):
                raise ValueError("out[%d] must be %s CUDA/HIP tensor, %s" % (i, dname, "contiguous" if layout == "nchw" else "torch.channels_last"))
            if t.device != self.device:
                raise ValueError("out[%d] lives on %s, handle on %s" % (i, t.device, self.device))
            if tuple(t.shape) != (n, c, h, h):
                raise ValueError("out[%d] has shape %s, expected %s" % (i, tuple(t.shape), (n, c, h, h)))
            res[i] = t
        arr = (ctypes.c_void_p * spec.NUM_SITES)(*[t.data_ptr() if t is not None else None for t in res])
        lay = _lib.FEAT_NCHW if layout == "nchw" else _lib.FEAT_NHWC
        if arith == "f32split":
            _lib.check(self.lib.offk_off_units_backward_feats_split(self._h, _stream(self.device), _ptr(self.workspace), _CL_DTYPES[dtype], arr,
                                                                    lay, int(bool(accumulate))), self._h)
        elif dtype == torch.float32:
            _lib.check(self.lib.offk_off_units_backward_feats(self._h, _stream(self.device), _ptr(self.workspace), arr, lay,
                                                              int(bool(accumulate))), self._h)
        else:
            _lib.check(self.lib.offk_off_units_backward_feats_typed(self._h, _stream(self.device), _ptr(self.workspace), _CL_DTYPES[dtype], arr,
                                                                    lay, int(bool(accumulate))), self._h)
        return res

    # ---- stage entry points -----------------------------------------------------------
    def pw_reduce(self, site, feat, G=None, D=None):
        """K1 of one site.  feat: the site's map, fp32 / bf16 / fp16, contiguous or torch.channels_last (offk_pw_reduce_cl).
        G / D: the caller's buffers instead of fresh ones."""
        _name, C, H = spec.SITES[site]
        G = _given(G, (self.N * H * H, spec.GEN_CH), "G", self.device)
        D = _given(D, (self.P * H * H, spec.DOWN_CH), "D", self.device)
        tensor = torch.is_tensor(feat)                 # one map: the ladder of feat_route's training side on it alone
        route = "cl" if tensor and not feat.is_contiguous() and _is_channels_last(feat) else "typed" if tensor and feat.dtype in _FEAT_DTYPES else "plain"
        _ENTRIES["pw_reduce"][route][1](feat, "feat", self.device)
        if route == "cl" and tuple(feat.shape) != (self.N, C, H, H):
            raise ValueError("feat is channels_last with logical shape %s, expected %s" % (tuple(feat.shape), (self.N, C, H, H)))
        self._call("pw_reduce", Route(route, _CL_DTYPES.get(feat.dtype), False), site, _ptr(feat), _ptr(G), _ptr(D))
        return G, D

    def sobel_tdiff(self, site, G, D, M, m_coff, algo=0):
        _check_dev(G, "G", self.device)
        _check_dev(D, "D", self.device)
        _check_dev(M, "M", self.device)
        _lib.check(self.lib.offk_sobel_tdiff(self._h, _stream(self.device), site, _ptr(G), _ptr(D), _ptr(M),
                                             M.shape[-1], m_coff, algo), self._h)

    def sobel_tdiff_all(self, algo=0):
        """Grouped K2 launch over the workspace G/D regions (after off_units / forward)."""
        _lib.check(self.lib.offk_sobel_tdiff_all(self._h, _stream(self.device), _ptr(self.workspace), algo), self._h)

    def set_conv_plan(self, conv_key, tile_cfg, splitk):
        _lib.check(self.lib.offk_set_conv_plan(self._h, conv_key.encode(), tile_cfg, splitk), self._h)

    # ---- profiling ---------------------------------------------------------------------
    def set_profiling(self, on):
        """False / 0 off, True / 1 per-stage events (stage_times), 2 per-launch trace (launch_times)."""
        _lib.check(self.lib.offk_set_profiling(self._h, int(on)), self._h)

    def launch_times(self, reset=True, max_entries=128):
        """Per-launch trace: OrderedDict name -> (accumulated ms, calls), in first-launch order."""
        from collections import OrderedDict
        ms = (ctypes.c_double * max_entries)()
        calls = (ctypes.c_int64 * max_entries)()
        buf = ctypes.create_string_buffer(64 * max_entries)
        n = self.lib.offk_launch_times(self._h, buf, len(buf), ms, calls, max_entries, int(reset))
        if n < 0:
            _lib.check(n, self._h)
        names = buf.value.decode().split("\n")
        return OrderedDict((names[i], (ms[i], int(calls[i]))) for i in range(min(n, max_entries)))

    def stage_times(self, reset=True):
        ms = (ctypes.c_double * _lib.NUM_STAGES)()
        calls = (ctypes.c_int64 * _lib.NUM_STAGES)()
        _lib.check(self.lib.offk_stage_times(self._h, ms, calls, int(reset)), self._h)
        return dict((n, (ms[i], int(calls[i]))) for i, n in enumerate(_lib.STAGE_NAMES))


def segment_consensus_backward(grad_out, length_m1, out=None):
    """basic_ops.py:29-33: grad_out [B, C] -> grad_in [B*(L-1), C] = grad_out / (L-1), repeated."""
    lib = _lib.load()
    B, C = grad_out.shape
    gi = _given(out, (B * length_m1, C), "out", grad_out.device)
    _lib.check(lib.offk_segment_consensus_backward(_stream(grad_out.device), _ptr(grad_out.contiguous()), B, int(length_m1), C, _ptr(gi)))
    return gi


# ---- handle-less stage kernels (channels-last tensors) ----------------------------------
def conv2d_nhwc(x, w_oihw, bias, stride, pad, res=None, flags=0, x_coff=0, ci=None, y=None, y_coff=0,
                tile_cfg=-1, splitk=0, w_packed=None, precision=0, partial=None):
    """x: [n, H, W, Cs] fp32 CUDA; uses channels [x_coff, x_coff+Ci).  Returns y [n, Ho, Wo, Co]
    (or writes channels [y_coff, y_coff+Co) of the given y).  partial: the caller's split-K slab buffer, exactly
    splitk * M * Co floats (splitk > 1)."""
    lib = _lib.load()
    n, H, W, cs = x.shape
    Co, Ci, KH, KW = w_oihw.shape
    wp = w_packed
    if wp is None:
        wp = torch.empty(Co, KH, KW, Ci, dtype=torch.float32, device=x.device)   # library K order [Co][Ci/32][KH*KW][32]
        _lib.check(lib.offk_pack_conv_weight(_stream(x.device), _ptr(w_oihw.contiguous()), Co, Ci, KH, KW, _ptr(wp)))
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    if y is None:
        y = torch.empty(n, Ho, Wo, Co, dtype=torch.float32, device=x.device)
    part, nfl = None, 0
    if splitk > 1:
        nfl = splitk * n * Ho * Wo * Co
        part = _given(partial, (nfl,), "partial", x.device)
    _lib.check(lib.offk_conv2d_ex(_stream(x.device), _ptr(x), cs, x_coff, n, H, W, Ci, _ptr(wp), _ptr(bias), Co, KH, KW,
                                  stride, pad, _ptr(res), res.shape[-1] if res is not None else 0, 0, flags,
                                  _ptr(y), y.shape[-1], y_coff, tile_cfg, splitk, _ptr(part), nfl, precision))
    return y


def pack_conv_weight(w_oihw, out=None):
    """[Co][Ci][KH][KW] -> the library's K order [Co][Ci/32][KH*KW][32] (device tensor; out: the caller's buffer of that size)."""
    lib = _lib.load()
    Co, Ci, KH, KW = w_oihw.shape
    wp = _given(out, (Co, KH, KW, Ci), "out", w_oihw.device)
    _lib.check(lib.offk_pack_conv_weight(_stream(w_oihw.device), _ptr(w_oihw.contiguous()), Co, Ci, KH, KW, _ptr(wp)))
    return wp


# ---- backward of one fusion conv: stride 1 (csrc/conv_bwd.hip) and stride 2 (csrc/conv_bwd_s2.hip), exact fp32 or split-fp32 ----
def _nhwc(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 4):
        raise ValueError("%s must be a contiguous fp32 CUDA/HIP tensor [n, H, W, Cs]" % name)
    return t


def _plan(entry, kinds, n_img, H, W, ci, co, ksize):
    """One plan entry of the conv backward (host code): its outputs, of the ctypes types `kinds`, as a tuple -- or alone where it has one."""
    outs = [kind() for kind in kinds]
    k = int(ksize)
    _lib.check(getattr(_lib.load(), entry)(int(n_img), int(H), int(W), int(ci), int(co), k, k, *[ctypes.byref(o) for o in outs]))
    return outs[0].value if len(outs) == 1 else tuple([o.value for o in outs])


def conv2d_backward_plan(n_img, H, W, ci, co, ksize):
    """offk_conv2d_backward_plan: (data_scratch_bytes, weight_scratch_bytes, weight_chunks) of one conv's backward -- host code, a function
    of these integers only.  The weight gradient's K chunks hold ceil(n_img / weight_chunks) images each, the last one what is left."""
    return _plan("offk_conv2d_backward_plan", (ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int), n_img, H, W, ci, co, ksize)


def conv2d_backward_plan_split(n_img, H, W, ci, co, ksize):
    """offk_conv2d_backward_plan_split: (weight_scratch_bytes, weight_chunks) of the split-fp32 weight gradient
    (conv2d_backward_weight(arith="f32split")) -- host code, a function of these integers only; the chunks are the split kernel's own."""
    return _plan("offk_conv2d_backward_plan_split", (ctypes.c_size_t, ctypes.c_int), n_img, H, W, ci, co, ksize)


def relu_backward(dy, y, out=None, accumulate=False, dy_coff=0, y_coff=0, out_coff=0, c=None):
    """out = dy * [y > 0] (exactly 0 where y <= 0, -0.0 or NaN), or out += that.  dy, y, out: [n, H, W, Cs] fp32 CUDA, channels
    [coff, coff + c) of each (c: what dy holds behind dy_coff); out=None: a new dense tensor; out may be dy itself (in place)."""
    lib = _lib.load()
    _nhwc(dy, "dy"), _nhwc(y, "y")
    n, H, W, cs = dy.shape
    C = cs - dy_coff if c is None else int(c)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the tensor to add to (out)")
        out = torch.empty(n, H, W, C, dtype=torch.float32, device=dy.device)
    _nhwc(out, "out")
    if y.shape[:3] != dy.shape[:3] or out.shape[:3] != dy.shape[:3]:
        raise ValueError("dy, y and out must agree in [n, H, W]")
    _lib.check(lib.offk_relu_backward(_stream(dy.device), _ptr(dy), cs, dy_coff, _ptr(y), y.shape[-1], y_coff, n * H * W, C, _ptr(out),
                                      out.shape[-1], out_coff, int(bool(accumulate))))
    return out


def conv2d_backward_data_plan_split(n_img, H, W, ci, co, ksize):
    """offk_conv2d_backward_data_plan_split: data_scratch_bytes of the split-fp32 data gradient (conv2d_backward_data(arith="f32split")) --
    host code, a function of these integers only: the three bf16 planes of the packed weight, then those of g, each rounded up to 256."""
    return _plan("offk_conv2d_backward_data_plan_split", (ctypes.c_size_t,), n_img, H, W, ci, co, ksize)


def conv2d_backward_data_form_split(n_img, H, W, ci, co, ksize):
    """offk_conv2d_backward_data_form_split: (ci_per_block, pixels_per_block) of the split-fp32 data gradient's GEMM -- host code, a function
    of these integers only; the result's bits do not depend on it."""
    return _plan("offk_conv2d_backward_data_form_split", (ctypes.c_int, ctypes.c_int), n_img, H, W, ci, co, ksize)


# the compute entries by (stride, arith)
_DATA_ENTRIES = {(1, "fp32"): "offk_conv2d_backward_data", (1, "f32split"): "offk_conv2d_backward_data_split",
                 (2, "fp32"): "offk_conv2d_s2_backward_data", (2, "f32split"): "offk_conv2d_s2_backward_data_split"}
_WEIGHT_ENTRIES = {(1, "fp32"): "offk_conv2d_backward_weight", (1, "f32split"): "offk_conv2d_backward_weight_split",
                   (2, "fp32"): "offk_conv2d_s2_backward_weight", (2, "f32split"): "offk_conv2d_s2_backward_weight_split"}


def _conv_backward_data(stride, g, w_oihw, pad, dx, dx_coff, accumulate, scratch, g_coff, arith):
    """conv2d_backward_data (stride 1) and conv2d_s2_backward_data (stride 2): g's map is dx's divided by the stride."""
    if arith not in DGRAD_ARITHS:
        raise ValueError("arith must be one of %s, got %r" % (", ".join(repr(a) for a in DGRAD_ARITHS), arith))
    lib = _lib.load()
    _nhwc(g, "g")
    n, OH, OW, gs = g.shape
    H, W = stride * OH, stride * OW
    Co, Ci, KH, KW = w_oihw.shape
    if not (w_oihw.is_cuda and w_oihw.dtype == torch.float32 and w_oihw.is_contiguous()):
        raise ValueError("w_oihw must be a contiguous fp32 CUDA/HIP tensor")
    if dx is None:
        if accumulate:
            raise ValueError("accumulate needs the tensor to add to (dx)")
        dx = torch.empty(n, H, W, Ci, dtype=torch.float32, device=g.device)
    _nhwc(dx, "dx")
    if stride == 2 and tuple(dx.shape[:3]) != (n, H, W):
        raise ValueError("dx must be [n, 2 * g's H, 2 * g's W, Cs]")
    split = arith == "f32split"
    if KH != KW:
        nbytes = 0
    elif stride == 1:
        nbytes = conv2d_backward_data_plan_split(n, H, W, Ci, Co, KH) if split else conv2d_backward_plan(n, H, W, Ci, Co, KH)[0]
    else:
        nbytes = conv2d_s2_backward_plan_split(n, H, W, Ci, Co, KH) if split else conv2d_s2_backward_plan(n, H, W, Ci, Co, KH)[0]
    scratch = _given(scratch, (nbytes,), "scratch", g.device, torch.uint8)
    entry = getattr(lib, _DATA_ENTRIES[stride, arith])
    _lib.check(entry(_stream(g.device), _ptr(g), gs, g_coff, n, H, W, Co, _ptr(w_oihw), Ci, KH, KW, int(pad), _ptr(dx),
                     dx.shape[-1], dx_coff, int(bool(accumulate)), _ptr(scratch), scratch.numel()))
    return dx


def _conv_backward_weight(stride, x, g, ksize, pad, relu_in, x_coff, ci, g_coff, co, dw, db, accumulate, scratch, want_db, arith):
    """conv2d_backward_weight (stride 1) and conv2d_s2_backward_weight (stride 2): g's map is x's divided by the stride."""
    if arith not in WGRAD_ARITHS:
        raise ValueError("arith must be one of %s, got %r" % (", ".join(repr(a) for a in WGRAD_ARITHS), arith))
    lib = _lib.load()
    _nhwc(x, "x"), _nhwc(g, "g")
    n, H, W, xs = x.shape
    if stride == 1:
        if g.shape[:3] != x.shape[:3]:
            raise ValueError("x and g must agree in [n, H, W]")
    elif tuple(g.shape[:3]) != (n, H // 2, W // 2) or H % 2 or W % 2:
        raise ValueError("x must be [n, H, W, Xs] with even H and W, g [n, H / 2, W / 2, Gs]")
    Ci = xs - x_coff if ci is None else int(ci)
    Co = g.shape[-1] - g_coff if co is None else int(co)
    k = int(ksize)
    if accumulate and (dw is None or (want_db and db is None)):
        raise ValueError("accumulate needs the tensors to add to (dw, db)")
    if dw is None:
        dw = torch.empty(Co, Ci, k, k, dtype=torch.float32, device=x.device)
    if db is None and want_db:
        db = torch.empty(Co, dtype=torch.float32, device=x.device)
    for t, name, numel in ((dw, "dw", Co * Ci * k * k), (db, "db", Co)):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel):
            raise ValueError("%s must be a contiguous fp32 CUDA/HIP tensor of %d elements" % (name, numel))
    split = arith == "f32split"
    if stride == 1:
        nbytes = conv2d_backward_plan_split(n, H, W, Ci, Co, k)[0] if split else conv2d_backward_plan(n, H, W, Ci, Co, k)[1]
    else:
        nbytes = conv2d_s2_backward_weight_plan_split(n, H, W, Ci, Co, k)[0] if split else conv2d_s2_backward_plan(n, H, W, Ci, Co, k)[1]
    scratch = _given(scratch, (nbytes,), "scratch", x.device, torch.uint8)
    entry = getattr(lib, _WEIGHT_ENTRIES[stride, arith])
    _lib.check(entry(_stream(x.device), _ptr(x), xs, x_coff, _ptr(g), g.shape[-1], g_coff, n, H, W, Ci, Co, k, k,
                     int(pad), int(bool(relu_in)), _ptr(dw), _ptr(db), int(bool(accumulate)), _ptr(scratch), scratch.numel()))
    return dw, db


def conv2d_backward_data(g, w_oihw, pad, dx=None, dx_coff=0, accumulate=False, scratch=None, g_coff=0, arith="fp32"):
    """dx (+)= the gradient of a stride-1 conv's input.  g: [n, H, W, Gs] fp32 CUDA, channels [g_coff, g_coff + Co); w_oihw [Co, Ci, k, k]
    (read in place); returns dx [n, H, W, Ci] (or writes channels [dx_coff, dx_coff + Ci) of the given dx).  scratch: the caller's uint8
    buffer of exactly conv2d_backward_plan's data_scratch_bytes.  arith: "fp32" (offk_conv2d_backward_data, exact fp32 on the fp32 matrix
    pipe) or "f32split" (offk_conv2d_backward_data_split: three bf16 planes per operand, six products on the bf16 pipe, include/offk.h has
    the bound; its scratch is conv2d_backward_data_plan_split's bytes)."""
    return _conv_backward_data(1, g, w_oihw, pad, dx, dx_coff, accumulate, scratch, g_coff, arith)


def conv2d_backward_weight(x, g, ksize, pad, relu_in=False, x_coff=0, ci=None, g_coff=0, co=None, dw=None, db=None, accumulate=False,
                           scratch=None, want_db=True, arith="fp32"):
    """(dw, db) (+)= the weight and bias gradient of a stride-1 k x k conv.  x: [n, H, W, Xs], channels [x_coff, x_coff + ci) (relu_in: the conv
    read max(x, 0)); g: [n, H, W, Gs], channels [g_coff, g_coff + co); dw [co, ci, k, k] and db [co]: e.g. the parameters' .grad, written in
    place (None: new tensors; want_db=False: no bias gradient, db comes back None).  scratch: the caller's uint8 buffer of exactly
    conv2d_backward_plan's weight_scratch_bytes.  arith: "fp32" (offk_conv2d_backward_weight, exact fp32 on the fp32 matrix pipe) or
    "f32split" (offk_conv2d_backward_weight_split: three bf16 planes per operand, six products on the bf16 pipe, include/offk.h has the
    bound; its scratch is conv2d_backward_plan_split's weight_scratch_bytes)."""
    return _conv_backward_weight(1, x, g, ksize, pad, relu_in, x_coff, ci, g_coff, co, dw, db, accumulate, scratch, want_db, arith)


def conv2d_s2_backward_plan(n_img, H, W, ci, co, ksize):
    """offk_conv2d_s2_backward_plan: (data_scratch_bytes, weight_scratch_bytes, weight_chunks) of one stride-2 conv's backward -- host code, a
    function of these integers only.  H, W: the INPUT map.  The weight gradient's K chunks hold ceil(n_img / weight_chunks) images each."""
    return _plan("offk_conv2d_s2_backward_plan", (ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int), n_img, H, W, ci, co, ksize)


def conv2d_s2_backward_plan_split(n_img, H, W, ci, co, ksize):
    """offk_conv2d_s2_backward_plan_split: data_scratch_bytes of the split-fp32 data gradient (conv2d_s2_backward_data(arith="f32split")) --
    host code, a function of these integers only: the three bf16 planes of the packed weight, then those of g, each rounded up to 256."""
    return _plan("offk_conv2d_s2_backward_plan_split", (ctypes.c_size_t,), n_img, H, W, ci, co, ksize)


def conv2d_s2_backward_data(g, w_oihw, pad, dx=None, dx_coff=0, accumulate=False, scratch=None, g_coff=0, arith="fp32"):
    """dx (+)= the gradient of a stride-2 conv's input.  g: [n, H/2, W/2, Gs] fp32 CUDA, channels [g_coff, g_coff + Co); w_oihw [Co, Ci, k, k]
    (read in place); returns dx [n, H, W, Ci] (or writes channels [dx_coff, dx_coff + Ci) of the given dx, whose map is twice g's).
    scratch: the caller's uint8 buffer of exactly conv2d_s2_backward_plan's data_scratch_bytes.  arith: "fp32"
    (offk_conv2d_s2_backward_data, exact fp32 on the fp32 matrix pipe) or "f32split" (offk_conv2d_s2_backward_data_split: three bf16 planes
    per operand, six products on the bf16 pipe, include/offk.h has the bound; its scratch is conv2d_s2_backward_plan_split's bytes)."""
    return _conv_backward_data(2, g, w_oihw, pad, dx, dx_coff, accumulate, scratch, g_coff, arith)


def conv2d_s2_backward_weight_plan_split(n_img, H, W, ci, co, ksize):
    """offk_conv2d_s2_backward_weight_plan_split: (weight_scratch_bytes, weight_chunks) of the split-fp32 weight gradient of a stride-2 conv
    (conv2d_s2_backward_weight(arith="f32split")) -- host code, a function of these integers only; the chunks are the split kernel's own."""
    return _plan("offk_conv2d_s2_backward_weight_plan_split", (ctypes.c_size_t, ctypes.c_int), n_img, H, W, ci, co, ksize)


def conv2d_s2_backward_weight(x, g, ksize, pad, relu_in=False, x_coff=0, ci=None, g_coff=0, co=None, dw=None, db=None, accumulate=False,
                              scratch=None, want_db=True, arith="fp32"):
    """(dw, db) (+)= the weight and bias gradient of a stride-2 k x k conv.  x: [n, H, W, Xs], channels [x_coff, x_coff + ci) (relu_in: the conv
    read max(x, 0)); g: [n, H/2, W/2, Gs], channels [g_coff, g_coff + co); dw [co, ci, k, k] and db [co] as in conv2d_backward_weight.
    scratch: the caller's uint8 buffer of exactly conv2d_s2_backward_plan's weight_scratch_bytes.  arith: "fp32"
    (offk_conv2d_s2_backward_weight, exact fp32 on the fp32 matrix pipe) or "f32split" (offk_conv2d_s2_backward_weight_split: three bf16
    planes per operand, six products on the bf16 pipe, include/offk.h has the K layout and the bound; its scratch is
    conv2d_s2_backward_weight_plan_split's weight_scratch_bytes)."""
    return _conv_backward_weight(2, x, g, ksize, pad, relu_in, x_coff, ci, g_coff, co, dw, db, accumulate, scratch, want_db, arith)


def bottleneck_chain14(x, w1, b1, w2_oihw, b2, w3, b3, res=None, relu_in=False, x_coff=0, y=None, y_coff=0, w2_packed=None):
    """One 1x1 -> 3x3 -> 1x1 (+ residual) chain of fusion@28 in one launch (offk_bottleneck_chain14).  x: [n, 14, 14, Cs] fp32 CUDA,
    the chain reads channels [x_coff, x_coff + Cin); w1 [64, Cin], w2_oihw [64, 64, 3, 3], w3 [256, K3] (K3 = 128: contracts
    [t2 | x]); res: [n, 14, 14, 256] or None.  Returns y [n, 14, 14, 256] (or writes channels [y_coff, y_coff + 256) of y).
    w2_packed: pack_conv_weight(w2_oihw) where the caller already holds it."""
    lib = _lib.load()
    n, H, W, cs = x.shape
    assert H == 14 and W == 14
    Cin, K3 = w1.shape[1], w3.shape[1]
    if y is None:
        y = torch.empty(n, 14, 14, 256, dtype=torch.float32, device=x.device)
    w2p = pack_conv_weight(w2_oihw) if w2_packed is None else w2_packed
    _lib.check(lib.offk_bottleneck_chain14(_stream(x.device), _ptr(x), cs, x_coff, n, Cin, int(relu_in), _ptr(w1.contiguous()),
                                           _ptr(b1), _ptr(w2p), _ptr(b2), _ptr(w3.contiguous()), _ptr(b3), K3, _ptr(res),
                                           res.shape[-1] if res is not None else 0, 0, _ptr(y), y.shape[-1], y_coff))
    return y


def bottleneck_chain14_split(x, w1, b1, w2_oihw, b2, w3, b3, res=None, branch=None, relu_in=False, x_coff=0, y=None, y_coff=0,
                             w2_packed=None, scratch=None):
    """offk_bottleneck_chain14_split: the chain in split-fp32 arithmetic (chain_split.hip).  w3 [256, 64]; branch = (w [256, 64], b [256]):
    chain 28a's branch 1x1 on the chain input before relu_in's ReLU (then Cin = 64 and no res).  scratch: the caller's uint8 buffer
    of exactly the header's 6 * (64 * Cin + 64 * 576 + 2 * 256 * 64) bytes; w2_packed: pack_conv_weight(w2_oihw)."""
    lib = _lib.load()
    n, H, W, cs = x.shape
    assert H == 14 and W == 14 and w3.shape[1] == 64
    Cin = w1.shape[1]
    if y is None:
        y = torch.empty(n, 14, 14, 256, dtype=torch.float32, device=x.device)
    w2p = pack_conv_weight(w2_oihw) if w2_packed is None else w2_packed
    scratch = _given(scratch, (6 * (64 * Cin + 64 * 576 + 2 * 256 * 64),), "scratch", x.device, torch.uint8)
    bw, bb = (branch[0].contiguous(), branch[1].contiguous()) if branch is not None else (None, None)
    _lib.check(lib.offk_bottleneck_chain14_split(_stream(x.device), _ptr(x), cs, x_coff, n, Cin, int(relu_in), _ptr(w1.contiguous()), _ptr(b1),
                                                 _ptr(w2p), _ptr(b2), _ptr(w3.contiguous()), _ptr(b3), _ptr(bw), _ptr(bb), _ptr(res),
                                                 res.shape[-1] if res is not None else 0, 0, _ptr(y), y.shape[-1], y_coff,
                                                 _ptr(scratch), scratch.numel()))
    return y


def winograd_conv3x3(x, w_oihw, bias, res=None, flags=0, x_coff=0, y=None, y_coff=0, want_pool=False, w_packed=None, scratch=None,
                     pool=None):
    """3x3 / stride 1 / pad 1 conv on 7x7 maps as Winograd F(4x4, 3x3) (offk_winograd_conv3x3).  x: [n, 7, 7, Cs]; returns y
    [n, 7, 7, Co] (and, want_pool, the per-tile sums [4 n, Co]).  w_packed / scratch / pool: the caller's packed weight, scratch
    (exactly the header's 121 * (Co * Ci + n * (Ci + Co)) floats) and pool buffer ([4 n, Co]) instead of fresh ones."""
    lib = _lib.load()
    n, H, W, cs = x.shape
    assert H == 7 and W == 7
    Co, Ci = w_oihw.shape[:2]
    if y is None:
        y = torch.empty(n, 7, 7, Co, dtype=torch.float32, device=x.device)
    nfl = 121 * (Co * Ci + n * (Ci + Co))
    scratch = _given(scratch, (nfl,), "scratch", x.device)
    pool = _given(pool, (4 * n, Co), "pool", x.device) if want_pool else None
    wp = pack_conv_weight(w_oihw) if w_packed is None else w_packed
    _lib.check(lib.offk_winograd_conv3x3(_stream(x.device), _ptr(x), cs, x_coff, n, Ci, _ptr(wp), _ptr(bias), Co,
                                         _ptr(res), res.shape[-1] if res is not None else 0, 0, flags, _ptr(y), y.shape[-1], y_coff,
                                         _ptr(scratch), nfl, _ptr(pool)))
    return (y, pool) if want_pool else y


def winograd_conv5x5s2(x, w_oihw, bias, flags=0, x_coff=0, y=None, y_coff=0, w_packed=None, scratch=None):
    """5x5 / stride 2 / pad 2 conv on 14x14 maps in polyphase Winograd form (offk_winograd_conv5x5s2).  x: [n, 14, 14, Cs]; returns
    y [n, 7, 7, Co].  w_packed / scratch (exactly the header's 400 * Ci * (Co + n) + 121 * n * Co floats): the caller's."""
    lib = _lib.load()
    n, H, W, cs = x.shape
    assert H == 14 and W == 14
    Co, Ci = w_oihw.shape[:2]
    if y is None:
        y = torch.empty(n, 7, 7, Co, dtype=torch.float32, device=x.device)
    nfl = 400 * Ci * (Co + n) + 121 * n * Co
    scratch = _given(scratch, (nfl,), "scratch", x.device)
    wp = pack_conv_weight(w_oihw) if w_packed is None else w_packed
    _lib.check(lib.offk_winograd_conv5x5s2(_stream(x.device), _ptr(x), cs, x_coff, n, Ci, _ptr(wp), _ptr(bias), Co,
                                           None, 0, 0, flags, _ptr(y), y.shape[-1], y_coff, _ptr(scratch), nfl))
    return y


def winograd_conv7x7s2(x, w_oihw, bias, flags=0, x_coff=0, y=None, y_coff=0, w_packed=None, scratch=None):
    """7x7 / stride 2 / pad 3 conv on 28x28 maps in polyphase Winograd form F(5x5, 4x4) (offk_winograd_conv7x7s2).
    x: [n, 28, 28, Cs]; returns y [n, 14, 14, Co].  w_packed / scratch (exactly the header's 225 * Ci * (Co + 9 n) + 64 * 9 n * Co floats):
    the caller's."""
    lib = _lib.load()
    n, H, W, cs = x.shape
    assert H == 28 and W == 28
    Co, Ci = w_oihw.shape[:2]
    if y is None:
        y = torch.empty(n, 14, 14, Co, dtype=torch.float32, device=x.device)
    nfl = 225 * Ci * (Co + 9 * n) + 64 * 9 * n * Co
    scratch = _given(scratch, (nfl,), "scratch", x.device)
    wp = pack_conv_weight(w_oihw) if w_packed is None else w_packed
    _lib.check(lib.offk_winograd_conv7x7s2(_stream(x.device), _ptr(x), cs, x_coff, n, Ci, _ptr(wp), _ptr(bias), Co,
                                           flags, _ptr(y), y.shape[-1], y_coff, _ptr(scratch), nfl))
    return y


def winograd_between(M, bias_in, phases_in, w1=None, b1=None, x=None, x_coff=0, precision="fp32", V=None, scratch=None):
    """offk_winograd_between: M [121, n, Cin] (Winograd-domain GEMM output of the conv in front) -> V [121, n, Cmid] (GEMM input of
    the conv behind), through relu(A^T M A + bias_in), optionally a 1x1 conv w1 [Cmid, Cin] + b1 + ReLU, and B^T . B.  x: optional
    [n, 7, 7, Cs] buffer that also receives relu(A^T M A + bias_in) at channels [x_coff, x_coff + Cin).  V / scratch (split-fp32: exactly
    the header's Cmid * Cin * 6 bytes): the caller's buffers instead of fresh ones."""
    lib = _lib.load()
    pts, n, cin = M.shape
    assert pts == 121
    cmid = w1.shape[0] if w1 is not None else cin
    V = _given(V, (121, n, cmid), "V", M.device)
    if precision == "f32split":      # offk_winograd_between_ex: stage B (the 1x1 conv) in split-fp32 arithmetic
        scratch = _given(scratch, (cmid * cin * 6,), "scratch", M.device, torch.uint8)
        _lib.check(lib.offk_winograd_between_ex(_stream(M.device), _ptr(M.contiguous()), _ptr(bias_in), int(phases_in), n, cin, _ptr(x),
                                                x.shape[-1] if x is not None else 0, x_coff, _ptr(w1.contiguous()), _ptr(b1), cmid, _ptr(V),
                                                _lib.PRECISIONS[precision], _ptr(scratch), scratch.numel()))
        return V
    _lib.check(lib.offk_winograd_between(_stream(M.device), _ptr(M.contiguous()), _ptr(bias_in), int(phases_in), n, cin, _ptr(x),
                                         x.shape[-1] if x is not None else 0, x_coff, _ptr(w1.contiguous() if w1 is not None else None),
                                         _ptr(b1), cmid, _ptr(V)))
    return V


def batched_gemm_nt(x, w, precision="fp32", y=None, scratch=None):
    """offk_batched_gemm_nt: y[b] = x[b] @ w[b].T for x [batch, M, K], w [batch, Co, K] (the GEMMs of a conv on a Winograd path);
    precision "f32split": split-fp32 arithmetic on the bf16 matrix pipe (wino_gemm_split.hip).  y / scratch (split-fp32: exactly the
    header's batch * Co * K * 6 bytes): the caller's buffers instead of fresh ones."""
    lib = _lib.load()
    batch, m, k = x.shape
    co = w.shape[1]
    assert w.shape == (batch, co, k)
    y = _given(y, (batch, m, co), "y", x.device)
    if precision == "f32split":
        scratch = _given(scratch, (batch * co * k * 6,), "scratch", x.device, torch.uint8)
    else:
        scratch = torch.empty(16, dtype=torch.uint8, device=x.device)      # (the fp32 form takes none)
    _lib.check(lib.offk_batched_gemm_nt(_stream(x.device), _ptr(x.contiguous()), _ptr(w.contiguous()), _ptr(y), batch, m, k, co,
                                        _lib.PRECISIONS[precision], _ptr(scratch), scratch.numel()))
    return y


def head(x, fc_w, fc_b, maxpool, x_coff=0, c=None, out=None):
    lib = _lib.load()
    n, H, W, cs = x.shape
    C = cs if c is None else c
    out = _given(out, (n, fc_w.shape[0]), "out", x.device)
    _lib.check(lib.offk_head(_stream(x.device), _ptr(x), cs, x_coff, n, H, W, C, int(maxpool), _ptr(fc_w.contiguous()),
                             _ptr(fc_b.contiguous()), fc_w.shape[0], _ptr(out)))
    return out


# ---- training side of one classifier head (offk_head_train / offk_head_backward; csrc/head_bwd.hip) ----
def _fc_param(t, name, numel):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel):
        raise ValueError("%s must be a contiguous fp32 CUDA/HIP tensor of %d elements" % (name, numel))
    return t


def head_backward_plan(n_img, c, num_classes):
    """offk_head_backward_plan: (scratch_bytes, chunks) of one head's weight and bias gradient -- host code, a function of these integers
    only.  The chunks hold ceil(n_img / chunks) images each, the last one what is left."""
    lib = _lib.load()
    s, ch = ctypes.c_size_t(0), ctypes.c_int(0)
    _lib.check(lib.offk_head_backward_plan(int(n_img), int(c), int(num_classes), ctypes.byref(s), ctypes.byref(ch)))
    return s.value, ch.value


def head_train(x, fc_w, fc_b, maxpool, head_index, drop=(0, 0.0), x_coff=0, c=None, z=None, out=None):
    """(out, z) of one head in training arithmetic: z = pooled * keep * scale [n, c], out = z . fc_w^T + fc_b [n, classes].  x: [n, H, W, Xs]
    fp32 CUDA, channels [x_coff, x_coff + c); fc_w [classes, c] and fc_b [classes] are read in place; drop = (seed, p), the mask is
    synth.head_dropout_keep(seed, head_index, n, c, p); (0, 0.0) is eval arithmetic.  z is what head_backward reads."""
    lib = _lib.load()
    _nhwc(x, "x")
    n, H, W, xs = x.shape
    C = xs - x_coff if c is None else int(c)
    ncls = fc_w.shape[0]
    _fc_param(fc_w, "fc_w", ncls * C), _fc_param(fc_b, "fc_b", ncls)
    z = _given(z, (n, C), "z", x.device)
    out = _given(out, (n, ncls), "out", x.device)
    seed, p = drop
    _lib.check(lib.offk_head_train(_stream(x.device), _ptr(x), xs, x_coff, n, H, W, C, int(bool(maxpool)), _ptr(fc_w), _ptr(fc_b), ncls,
                                   int(head_index), int(seed), float(p), _ptr(z), _ptr(out)))
    return out, z


def head_backward(g, x, fc_w, z, maxpool, head_index, drop=(0, 0.0), x_coff=0, c=None, dx=None, dx_coff=0, accumulate_dx=False, dw=None,
                  db=None, accumulate_w=False, scratch=None, want_dx=True, want_dw=True, want_db=True):
    """(dx, dw, db) of one head; g: [n, classes] = d loss / d out, x / fc_w / z / drop as in head_train (z: what it returned).  dx comes back
    as [n, H, W, c] (or channels [dx_coff, dx_coff + c) of the given dx are written, added to with accumulate_dx); dw [classes, c] and
    db [classes]: e.g. the parameters' .grad, written in place (accumulate_w: added to).  want_* = False: that gradient is not launched
    and comes back None.  scratch: the caller's uint8 buffer of exactly head_backward_plan's scratch_bytes."""
    lib = _lib.load()
    _nhwc(x, "x")
    n, H, W, xs = x.shape
    C = xs - x_coff if c is None else int(c)
    ncls = fc_w.shape[0]
    _fc_param(fc_w, "fc_w", ncls * C), _fc_param(g, "g", n * ncls), _fc_param(z, "z", n * C)
    if (accumulate_dx and want_dx and dx is None) or (accumulate_w and ((want_dw and dw is None) or (want_db and db is None))):
        raise ValueError("accumulate needs the tensors to add to")
    if want_dx:
        if dx is None:
            dx = torch.empty(n, H, W, C, dtype=torch.float32, device=x.device)
        _nhwc(dx, "dx")
        if tuple(dx.shape[:3]) != (n, H, W):
            raise ValueError("dx must agree with x in [n, H, W]")
    else:
        dx = None
    dw = (torch.empty(ncls, C, dtype=torch.float32, device=x.device) if dw is None else _fc_param(dw, "dw", ncls * C)) if want_dw else None
    db = (torch.empty(ncls, dtype=torch.float32, device=x.device) if db is None else _fc_param(db, "db", ncls)) if want_db else None
    nbytes = head_backward_plan(n, C, ncls)[0] if (want_dw or want_db) else 0
    scratch = _given(scratch, (nbytes,), "scratch", x.device, torch.uint8)
    seed, p = drop
    _lib.check(lib.offk_head_backward(_stream(x.device), _ptr(g), _ptr(x), xs, x_coff, n, H, W, C, int(bool(maxpool)), _ptr(fc_w), ncls, _ptr(z),
                                      int(head_index), int(seed), float(p), _ptr(dx), dx.shape[-1] if dx is not None else 0, dx_coff,
                                      int(bool(accumulate_dx)), _ptr(dw), _ptr(db), int(bool(accumulate_w)),
                                      _ptr(scratch) if nbytes else ctypes.c_void_p(0), scratch.numel()))
    return dx, dw, db


def segment_consensus(x, batch, out=None):
    lib = _lib.load()
    T = x.shape[0] // batch
    out = _given(out, (batch, x.shape[1]), "out", x.device)
    _lib.check(lib.offk_segment_consensus(_stream(x.device), _ptr(x.contiguous()), batch, T, x.shape[1], _ptr(out)))
    return out


def nchw_to_nhwc(x, out=None):
    lib = _lib.load()
    n, C, H, W = x.shape
    out = _given(out, (n, H, W, C), "out", x.device)
    _lib.check(lib.offk_nchw_to_nhwc(_stream(x.device), _ptr(x.contiguous()), n, C, H * W, _ptr(out)))
    return out


def nhwc_to_nchw(x, coff=0, c=None, out=None):
    lib = _lib.load()
    n, H, W, cs = x.shape
    C = cs - coff if c is None else c
    out = _given(out, (n, C, H, W), "out", x.device)
    _lib.check(lib.offk_nhwc_to_nchw(_stream(x.device), _ptr(x), cs, coff, n, C, H * W, _ptr(out)))
    return out


def score_fusion(score_sets, weights, want_pred=True, out=None):
    """score_sets: list of [videos, crops, classes] (or [videos, classes]) fp32 CUDA tensors.
    Returns (fused [videos, classes], pred [videos] int32 or None) -- K7, include/offk.h.  out: the caller's (fused, pred)."""
    lib = _lib.load()
    sets = [s.contiguous() if s.dim() == 3 else s.contiguous().unsqueeze(1) for s in score_sets]
    v, k, c = sets[0].shape
    for s in sets:
        if tuple(s.shape) != (v, k, c) or not s.is_cuda or s.dtype != torch.float32:
            raise ValueError("score sets must be same-shape fp32 CUDA tensors")
    fused = _given(out[0] if out is not None else None, (v, c), "fused", sets[0].device)
    pred = _given(out[1] if out is not None else None, (v,), "pred", sets[0].device, torch.int32) if want_pred else None
    ptrs = (ctypes.c_void_p * len(sets))(*[s.data_ptr() for s in sets])
    w = (ctypes.c_float * len(sets))(*[float(x) for x in weights])
    _lib.check(lib.offk_score_fusion(_stream(sets[0].device), ptrs, w, len(sets), v, k, c, _ptr(fused), _ptr(pred)))
    return fused, pred
