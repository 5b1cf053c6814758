"""Host-side mirror of the reference's model interface for the OFF path.

The reference has no module boundary around the OFF sub-network (it is inline in
BNInception_OFF.RGB_OFF_forward, RGB_OFF.py:360-860, and BNInception_OFF.forward,
Flow_OFF.py:370-887).  This file provides

* ``OFFSubNetwork`` -- an nn.Module that owns the OFF parameters under the reference's
  exact state_dict key names (so reference-format checkpoints load) and whose forward
  takes the nine tapped feature maps and runs liboffk;
* ``BNInception_OFF`` / ``bninception_off`` -- same constructor arguments, attributes
  (``batch``, ``length``, ``modality_fuse``, ``consensus_type``) and return conventions
  as the reference classes (RGB_OFF.py:32,860,1346-1360; Flow_OFF.py:45,879-884,
  1371-1385; RGB_OFF_v2.py:891), with the TSN backbone supplied by the caller as an
  ordinary PyTorch module (it is out of scope and stays on stock PyTorch-ROCm).

The nn.Conv2d / nn.Linear children are parameter containers only: they are never
called.  All arithmetic happens in the HIP library; without it every forward raises.
"""
import os

import torch
import torch.nn as nn

from . import runtime, spec

_VARIANTS = {"rgb": spec.VARIANT_RGB, "flow": spec.VARIANT_FLOW, "rgb_v2": spec.VARIANT_FLOW}


class _SobelHolder(nn.Module):
    """state_dict key 'sobel_edge_diagonal.conv.weight' (util.py:52-77): frozen diagonal kernel."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(spec.DOWN_CH, spec.DOWN_CH, 3, 1, 1, bias=False, groups=spec.DOWN_CH)
        k = torch.tensor(spec.DIAG_SOBEL, dtype=torch.float32)
        self.conv.weight = nn.Parameter(k.expand(spec.DOWN_CH, 1, 3, 3).clone(), requires_grad=False)


class OFFSubNetwork(nn.Module):
    def __init__(self, num_classes=spec.NUM_CLASSES, batch=16, length=7, variant="rgb",
                 slice_mode=spec.SLICE_FLAT, consensus=None, feat_layout=0, precision="fp32"):
        super().__init__()
        self.precision = precision
        if variant not in _VARIANTS:
            raise ValueError("variant must be one of %s" % sorted(_VARIANTS))
        self.variant_name = variant
        self.variant = _VARIANTS[variant]
        self.batch, self.length, self.num_classes = batch, length, num_classes
        self.slice_mode, self.feat_layout = slice_mode, feat_layout
        self.consensus_avg = (self.variant == spec.VARIANT_FLOW) if consensus is None else bool(consensus)
        # parameter containers, names and shapes as in the reference (RGB_OFF.py:265-334, Flow_OFF.py:51)
        for name, C, _H in spec.SITES:
            setattr(self, "motion_conv_gen_" + name, nn.Conv2d(C, spec.GEN_CH, 1, 1))
            setattr(self, "motion_spatial_down_" + name, nn.Conv2d(C, spec.DOWN_CH, 1, 1))
            if self.variant == spec.VARIANT_RGB:
                setattr(self, "motion_spatial_grad_" + name,
                        nn.Conv2d(spec.DOWN_CH, spec.DOWN_CH, 3, 1, 1, groups=spec.DOWN_CH, bias=True))
        if self.variant == spec.VARIANT_FLOW:
            self.sobel_edge_diagonal = _SobelHolder()
        for key, co, ci, k, s, p in spec.FUSION_CONVS:
            setattr(self, key, nn.Conv2d(ci, co, k, s, p))
        for key, cin in spec.HEADS:
            setattr(self, key, nn.Linear(cin, num_classes))
        self._rt = None
        self._rt_key = None
        self._pushed = {}      # key -> (data_ptr, _version) of the tensor the library last copied

    # -- weights -> library ---------------------------------------------------------
    def mark_weights_dirty(self):
        """Force a re-push of every weight on the next forward.  Needed after writing a parameter through a path that
        bypasses the parameter's version counter: a raw-pointer write by foreign code, and IN-PLACE WRITES THROUGH
        ``.data`` (``p.data.copy_(w)``, ``p.data.mul_(0.9)`` -- common in TSN-era code; ``.data`` is a tensor with its own
        version counter, so ``p._version`` does not move and the storage pointer stays the same).  ``p.copy_`` / ``p.mul_``
        under ``torch.no_grad()``, optimizer steps, ``load_state_dict`` and ``p.data = new_tensor`` are all seen without this
        call.  OFFK_ALWAYS_PUSH=1 in the environment re-pushes everything on every forward (debugging stale weights; slow).
        The same blind spot exists for the parameter-written-between-forward-and-backward check of OFFUnits."""
        self._pushed = {}

    def load_state_dict(self, state_dict, strict=True, **kw):
        own = set(self.state_dict().keys())
        sd = {}
        for k, v in state_dict.items():
            kk = k[7:] if k.startswith("module.") else k     # DataParallel checkpoints (test_flow_off.py:52-58)
            if kk in own:
                sd[kk] = v
        missing = sorted(own - set(sd))
        if strict and missing:
            raise KeyError("missing OFF weights: %s" % ", ".join(missing[:5]))
        return super().load_state_dict(sd, strict=False, **kw)

    def _handle(self, device):
        key = (self.batch, self.length, self.variant, self.slice_mode, self.consensus_avg, self.feat_layout, str(device), self.precision)
        if self._rt is None or self._rt_key != key:
            self._rt = runtime.OffForward(self.batch, self.length, self.variant, self.slice_mode,
                                          self.consensus_avg, self.num_classes, self.feat_layout, device, self.precision)
            self._rt_key = key
            self._pushed = {}
        # liboffk keeps packed copies: push every tensor that is new or was written since the last push.  Any writer
        # that goes through torch -- load_state_dict of this module OR of a parent (which calls _load_from_state_dict
        # and never reaches the override above), optimizer steps, param.copy_(), param.data = ... -- either bumps the
        # tensor's version counter or replaces its storage, and both are part of the tag.
        if os.environ.get("OFFK_ALWAYS_PUSH") == "1":
            self._pushed = {}
        for k, v in self.state_dict(keep_vars=True).items():
            tag = (v.data_ptr(), v._version)
            if self._pushed.get(k) != tag:
                self._rt.set_weight(k, v)
                self._pushed[k] = tag
        return self._rt

    # -- forward ----------------------------------------------------------------------
    def _as_handed_over(self, feats):
        """A channels_last backbone's nine maps on a precision="f32split" module: the handle takes them with no copy
        (runtime.feat_route decides); everything else is made contiguous as ever."""
        try:
            return runtime.feat_route(feats, self.batch, self.length, self.feat_layout, self.precision, "infer").route == "cl"
        except ValueError:          # a mix of layouts or dtypes, an fp32-pipe module: the contiguous copies settle it, as ever
            return False

    def forward(self, feats, want28=True):
        """feats: the nine ``inception_{3a..5b}_output_out`` maps [B*L, C, H, H] fp32 on a HIP
        device -- each either the concatenated tensor or the list of its inception branches in
        torch.cat order (then the concat never has to exist, offk_forward_parts).  bf16 / fp16 maps of one dtype (an autocast
        backbone's) go through as they are on a precision="f32split" module (offk_forward_typed: the values of the maps upcast), and so
        do the torch.channels_last maps of a channels_last backbone, in any of the three dtypes (offk_forward_cl: no copy, no cast).  Returns (fc_action_motion_7, fc_action_motion_14, fc_action_motion_28):
        [B*(L-1), classes] each, or [B, classes] with the consensus average."""
        first = feats[0] if torch.is_tensor(feats[0]) else feats[0][0]
        if not first.is_cuda:
            raise runtime._lib.OffkError("OFFSubNetwork has no CPU path: feature maps must live on an MI355X")
        rt = self._handle(first.device)
        if not self._as_handed_over(feats):
            feats = [f.contiguous() if torch.is_tensor(f) else [g.contiguous() for g in f] for f in feats]
        with torch.no_grad():
            return rt.forward(feats, want28=want28)


class _OFFUnitsFn(torch.autograd.Function):
    """autograd node around offk_off_units(_train) / offk_off_units_backward.  Inputs after the three
    bookkeeping arguments are the unit parameters in ``OFFUnits.param_keys`` order; the feature maps come from
    the frozen backbone (train_off.py:39-56) and get no gradient; they are kept in ``ctx.feats`` in the dtype they came in
    (fp32, or bf16 / fp16 from an autocast backbone -- the typed entries read those without an fp32 copy) and in the layout
    they came in where all nine are torch.channels_last (the _cl training entries read those without a contiguous copy)."""

    @staticmethod
    def forward(ctx, mod, feats, drop, *params):
        rt = mod._handle(feats[0].device, params)
        mod._run_units(rt, feats, drop)
        ctx.mod, ctx.feats, ctx.drop = mod, feats, drop
        # the backward reads the G / D activations this call leaves in the handle's ONE workspace: remember which
        # call that was (and which parameter values it used) so that a later forward through the same module
        # -- an eval pass, a second micro-batch, a checkpoint recompute -- is detected instead of silently used
        ctx.gen = mod._generation
        ctx.versions = dict((k, (prm.data_ptr(), prm._version)) for k, prm in zip(mod.param_keys, params))
        P = rt.P
        # copies: the workspace is rewritten by the next forward, autograd consumers may outlive it.  (clone, not .contiguous():
        # fusion_28 is all unit channels, so its slice is contiguous already and .contiguous() handed out the workspace itself --
        # a forward between this one and the use of its m28 changed the values under the caller)
        outs = []
        for name, H, C, width in (("fusion_28", 28, 320, 320), ("fusion_14", 14, 1056, 800), ("fusion_7", 7, 832, 320)):
            buf = rt.region(name, C).view(P, H, H, C)[..., :width].clone(memory_format=torch.contiguous_format)
            outs.append(buf.permute(0, 3, 1, 2))       # NCHW view of channels-last memory
        return tuple(outs)

    @staticmethod
    def backward(ctx, g28, g14, g7):
        mod, feats, (seed, p) = ctx.mod, ctx.feats, ctx.drop
        rt = mod._rt
        if rt is None or any((mod._param(k).data_ptr(), mod._param(k)._version) != v for k, v in ctx.versions.items()):
            raise RuntimeError("OFFUnits: a parameter was modified (or the module moved) between this forward and its "
                               "backward; the saved activations no longer belong to the current weights")
        if mod._generation != ctx.gen:
            # another forward has overwritten G / D since: recompute them (K1 + K2 only, same seed => same mask)
            mod._run_units(rt, feats, ctx.drop)
            # G / D are this call's again: a further backward through the same graph (train_off.py:144-146 makes three, two of them
            # with retain_graph=True) finds them and does not recompute a second and a third time
            ctx.gen = mod._generation
        bufs =[g.permute(0, 2, 3, 1).contiguous() for g in (g28, g14, g7)]      # channels-last rows
        views = [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]
        # (the default arithmetic makes today's call, argument for argument)
        arith = {} if mod.wgrad_arith == "fp32" else {"arith": mod.wgrad_arith}
        _flat, grads = rt.off_units_backward(feats, views, seed, p, **arith)
        return (None, None, None) + tuple(grads[k] for k in mod.param_keys)


class _OFFUnitsFeatFn(torch.autograd.Function):
    """_OFFUnitsFn for ``OFFUnits(feat_grad=True)``: the nine maps are tensor inputs of the node (after ``mod`` and ``drop``), so
    autograd sees them, and the backward returns their gradients too -- offk_off_units_backward_feats, one launch behind the
    parameter backward, for the sites in ``ctx.needs_input_grad`` only (none required: no launch).  Forward, the stale-generation
    recompute and the parameter-version check are _OFFUnitsFn's own code."""

    @staticmethod
    def forward(ctx, mod, drop, *maps_and_params):
        feats, params = tuple(maps_and_params[:spec.NUM_SITES]), maps_and_params[spec.NUM_SITES:]
        return _OFFUnitsFn.forward(ctx, mod, feats, drop, *params)

    @staticmethod
    def backward(ctx, g28, g14, g7):
        pgrads = _OFFUnitsFn.backward(ctx, g28, g14, g7)[3:]
        sites = runtime.feat_grad_sites(ctx.needs_input_grad, first=2)
        dx = [None] * spec.NUM_SITES
        if sites:
            # the layout the maps came in: all nine channels_last (the route the forward took) -> channels_last gradients
            layout = "cl" if ctx.mod._as_handed_over(ctx.feats) else "nchw"
            # torch wants a gradient in its input's dtype.  Nine maps of one dtype (always so on the typed / cl routes): the kernel
            # stores that dtype itself, each fp32 sum rounded once.  A mix of dtypes (the plain route): fp32 dX, cast per map
            dts = set(f.dtype for f in ctx.feats)
            dtype = dts.pop() if len(dts) == 1 else torch.float32
            dtype = dtype if dtype in (torch.bfloat16, torch.float16) else torch.float32
            # (the default arithmetic makes today's call, argument for argument)
            arith = {} if ctx.mod.feat_grad_arith == "fp32" else {"arith": ctx.mod.feat_grad_arith}
            dx = ctx.mod._rt.off_units_backward_feats(sites, layout, dtype=dtype, **arith)
            if dtype == torch.float32:
                dx = [g if g is None or g.dtype == f.dtype else g.to(f.dtype) for g, f in zip(dx, ctx.feats)]
        return (None, None) + tuple(dx) + tuple(pgrads)


class OFFUnits(nn.Module):
    """The nine OFF units as a trainable module on liboffk: parameters under the
    reference's state_dict keys (``motion_conv_gen_*``, ``motion_spatial_down_*``, ``motion_spatial_grad_*``;
    the Sobel weight of the Flow variant is frozen, util.py:72), forward = K1 + K2 (in ``train()`` mode with
    nn.Dropout(p=0.8) on the spatial gradients, RGB_OFF.py:356/:612, reproducible from ``drop_seed``), backward
    = offk_off_units_backward.  Returns the three motion maps the fusion stages start from
    (cat(motion_3a, motion_3b) [P,320,28,28], cat(motion_3c..4d) [P,800,14,14], cat(motion_5a, motion_5b)
    [P,320,7,7]; RGB_OFF.py:656, :760, :832), channels-last in memory.  The fusion convolutions that
    follow -- the two stride-2 stage openers included -- can be built from ``FusionConv2d`` (below: forward and backward on
    liboffk, one conv per module) and the three heads from ``MotionHead`` (below: pooling, dropout and the Linear, forward and
    backward on liboffk), so the whole branch train_off.py un-freezes trains on the library.

    The nine maps may be fp32, or bf16 / fp16 of one dtype -- what a frozen backbone under ``torch.autocast`` emits.
    16-bit maps are neither cast nor copied: the kernels read them as they are (offk_off_units_train_typed,
    offk_off_units_backward_typed), the autograd node keeps the 16-bit tensors for its backward and for the
    recompute of a stale generation, and outputs and gradients are fp32 and equal those from ``x.float()``.

    Nine ``torch.channels_last`` maps (logical shape as ever, any of the three dtypes) -- what a backbone run in channels_last
    emits -- are not made contiguous either: offk_off_units_train_cl / offk_off_units_backward_cl read them as they are, the
    autograd node keeps those very tensors, and outputs and gradients equal those from the contiguous copies.  Any other
    layout, a mix included, is made contiguous as ever.

    ``feat_grad=False`` (the default) is the reference's training setup: the backbone is frozen (train_off.py:39-56), the maps are
    no inputs of the autograd node and get no gradient, whatever their ``requires_grad``.  ``feat_grad=True`` is for an un-frozen
    backbone (inception_5a / 5b of a TSN partial fine-tune, or all of it): the maps become inputs of the node and every map that
    requires grad gets its gradient from offk_off_units_backward_feats -- one more launch per backward, for those sites only, in
    the maps' layout (contiguous, or channels_last where all nine came so).  The gradient is computed in fp32; a bf16 / fp16 map
    receives it rounded once in the kernel to its dtype (nearest-even, offk_off_units_backward_feats_typed: no fp32 buffer, no cast).  Parameter gradients are the same bits either way.
    ``feat_grad_arith="f32split"`` (default ``"fp32"``) computes that gradient in split-fp32 arithmetic on the bf16 matrix pipe instead
    (offk_off_units_backward_feats_split: dropped part below (2^-21 + 2^-30) sum|a w| per element, reproducible, its own bits); it
    changes nothing else -- the parameter gradients are the same bits.
    ``wgrad_arith="f32split"`` (default ``"fp32"``) runs the backward's largest kernel, the weight-gradient GEMM of the stacked 1x1
    reduces, in the same split-fp32 arithmetic (offk_off_units_backward_split, for every dtype and layout of the maps): the
    ``motion_conv_gen_*.weight`` / ``motion_spatial_down_*.weight`` gradients get bits of their own (dropped part below
    (2^-21 + 2^-30) sum|a x| per element, nothing dropped on bf16 maps), every other gradient keeps the default's bits.  It is
    independent of ``feat_grad_arith``.
    ``fwd_arith="f32split"`` (default ``"fp32"``) runs the forward's largest kernel, the stacked 1x1 reduces K1, in the same split-fp32
    arithmetic (offk_off_units_train_split, for every dtype and layout of the maps; dropped part below (2^-21 + 2^-30) sum|w x| per
    element, nothing dropped on bf16 maps): the outputs and the saved G / D get bits of their own, the backward runs behind it
    unchanged, and the recompute of a stale generation inside the backward uses the same arithmetic.  It is independent of the other
    two switches."""

    def __init__(self, batch=16, length=7, variant="rgb", slice_mode=spec.SLICE_FLAT, precision="fp32", drop_p=0.8, feat_grad=False,
                 feat_grad_arith="fp32", wgrad_arith="fp32", fwd_arith="fp32"):
        super().__init__()
        if fwd_arith not in runtime.FWD_ARITHS:
            raise ValueError("fwd_arith must be one of %s, got %r" % (", ".join(repr(a) for a in runtime.FWD_ARITHS), fwd_arith))
        self.fwd_arith = fwd_arith
        if wgrad_arith not in runtime.WGRAD_ARITHS:
            raise ValueError("wgrad_arith must be one of %s, got %r" % (", ".join(repr(a) for a in runtime.WGRAD_ARITHS), wgrad_arith))
        self.wgrad_arith = wgrad_arith
        if feat_grad_arith not in runtime.FEAT_GRAD_ARITHS:
            raise ValueError("feat_grad_arith must be one of %s, got %r" % (", ".join(repr(a) for a in runtime.FEAT_GRAD_ARITHS), feat_grad_arith))
        self.feat_grad, self.feat_grad_arith = bool(feat_grad), feat_grad_arith
        if variant not in _VARIANTS:
            raise ValueError("variant must be one of %s" % sorted(_VARIANTS))
        self.variant = _VARIANTS[variant]
        self.batch, self.length, self.slice_mode, self.precision, self.drop_p = batch, length, slice_mode, precision, float(drop_p)
        for name, C, _H in spec.SITES:
            setattr(self, "motion_conv_gen_" + name, nn.Conv2d(C, spec.GEN_CH, 1, 1))
            setattr(self, "motion_spatial_down_" + name, nn.Conv2d(C, spec.DOWN_CH, 1, 1))
            if self.variant == spec.VARIANT_RGB:
                setattr(self, "motion_spatial_grad_" + name,
                        nn.Conv2d(spec.DOWN_CH, spec.DOWN_CH, 3, 1, 1, groups=spec.DOWN_CH, bias=True))
        if self.variant == spec.VARIANT_FLOW:
            self.sobel_edge_diagonal = _SobelHolder()
        self.param_keys = [k for k in spec.weight_shapes(self.variant) if k.startswith(spec.UNIT_PARAM_PREFIXES)]
        self._rt, self._bound, self._sobel_pushed, self.drop_seed = None, {}, None, 0
        self._generation = 0    # bumped by every units forward: tells a backward whether G / D in the workspace are its own

    def _run_units(self, rt, feats, drop):
        seed, p = drop
        # (the default arithmetic makes today's calls, argument for argument)
        arith = {} if self.fwd_arith == "fp32" else {"arith": self.fwd_arith}
        if p > 0.0:
            rt.off_units_train(feats, seed, p, **arith)
        else:
            rt.off_units(feats, **arith)
        self._generation += 1

    def _param(self, key):
        mod, attr = key.rsplit(".", 1)
        return getattr(getattr(self, mod), attr)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Takes a reference-format checkpoint: the unit keys are used, every other key (backbone, fusion stages,
        heads) is ignored; a DataParallel 'module.' prefix is accepted (test_flow_off.py:52-58)."""
        own = set(self.state_dict().keys())
        sd = {}
        for k, v in state_dict.items():
            kk = k[7:] if k.startswith("module.") else k
            if kk in own:
                sd[kk] = v
        missing = sorted(own - set(sd))
        if strict and missing:
            raise KeyError("missing OFF unit weights: %s" % ", ".join(missing[:5]))
        return super().load_state_dict(sd, strict=False, **kw)

    def _handle(self, device, params):
        if self._rt is None or self._rt.device != torch.device(device):
            self._rt = runtime.OffForward(self.batch, self.length, self.variant, self.slice_mode, False,
                                          device=device, precision=self.precision, training=True)
            self._bound = {}
            self._sobel_pushed = None
        if self.variant == spec.VARIANT_FLOW:
            # frozen (util.py:72) and therefore copied, not bound -- but it travels in checkpoints: one loaded after the first forward
            # moves its (data_ptr, _version) tag, like the parameters OFFSubNetwork pushes.  The tag has that class's blind spot too: an
            # in-place write through .data (sobel.data.copy_(w)) moves neither half of it; OFFK_ALWAYS_PUSH=1 copies on every forward.
            sobel = self.sobel_edge_diagonal.conv.weight
            tag = (sobel.data_ptr(), sobel._version)
            if self._sobel_pushed != tag or os.environ.get("OFFK_ALWAYS_PUSH") == "1":
                self._rt.set_weight(spec.SOBEL_KEY, sobel)
                self._sobel_pushed = tag
        # The trainable tensors are BOUND, not copied (offk_bind_weight): liboffk reads the parameters' own storage at
        # launch time, so an optimizer step costs the library nothing -- no 54 blocking copies per step, no staging, no
        # re-packing -- and is ordered like any other kernel on the stream.  Only a re-allocated parameter is re-bound.
        for key, prm in zip(self.param_keys, params):
            if not prm.is_contiguous():
                raise ValueError("OFFUnits parameter %s must be contiguous" % key)
            if self._bound.get(key) != prm.data_ptr():
                self._rt.bind_weight(key, prm)
                self._bound[key] = prm.data_ptr()
        return self._rt

    def _as_handed_over(self, feats):
        """Nine channels_last maps of the reference's logical shape and one fp32 / bf16 / fp16 dtype: the _cl training entries take
        them without a copy."""
        try:                      # (training side: the handle plays no part in the route)
            return runtime.feat_route(feats, self.batch, self.length, 0, 0, "train").route == "cl"
        except ValueError:        # a mix of layouts or dtypes, a wrong shape or count: the contiguous path and its checks
            return False

    def forward(self, feats, drop_seed=None):
        feats = tuple(feats)
        if not self._as_handed_over(feats):
            feats = tuple(f.contiguous() for f in feats)
        if not feats[0].is_cuda:
            raise runtime._lib.OffkError("OFFUnits has no CPU path: feature maps must live on an MI355X")
        if self.training and self.drop_p > 0.0:
            if drop_seed is None:
                self.drop_seed += 1
                drop_seed = self.drop_seed
            drop = (int(drop_seed), self.drop_p)
        else:
            drop = (0, 0.0)
        params = [self._param(k) for k in self.param_keys]
        if self.feat_grad:
            return _OFFUnitsFeatFn.apply(self, drop, *(feats + tuple(params)))
        return _OFFUnitsFn.apply(self, feats, drop, *params)


class _FusionConvFn(torch.autograd.Function):
    """autograd node of one ``FusionConv2d``: forward = offk_conv2d (direct fp32), backward = offk_relu_backward, then
    offk_conv2d_backward_weight (weight and bias) and offk_conv2d_backward_data -- the offk_conv2d_s2_backward_* entries for a stride-2
    module, the *_split entries where the module's wgrad_arith / s2_wgrad_arith / dgrad_arith / bwd_arith ask --, each only where ``ctx.needs_input_grad`` asks.
    Tensors cross the node as logical NCHW in channels-last memory; inside they are the [n, H, W, C] rows the library reads."""

    @staticmethod
    def forward(ctx, mod, x, res, weight, bias):
        xr = x.permute(0, 2, 3, 1).contiguous()                    # no copy where x is channels-last already
        rr = res.permute(0, 2, 3, 1).contiguous() if res is not None else None
        flags = (runtime._lib.CONV_RELU_IN if mod.relu_in else 0) | (runtime._lib.CONV_RELU_POST if mod.relu else 0)
        y = runtime.conv2d_nhwc(xr, weight, bias, mod.stride[0], mod.padding[0], res=rr, flags=flags)
        out = y.permute(0, 3, 1, 2)
        ctx.mod = mod
        ctx.save_for_backward(xr, weight, out)
        return out

    @staticmethod
    def backward(ctx, gy):
        mod = ctx.mod
        xr, weight, out = ctx.saved_tensors
        need_x, need_res, need_w, need_b = ctx.needs_input_grad[1:5]
        g = gy.permute(0, 2, 3, 1).contiguous()
        s2 = mod.stride[0] == 2
        if mod.relu:
            g = runtime.relu_backward(g, out.permute(0, 2, 3, 1))
        dx = dw = db = None
        if need_w or need_b:
            FusionConv2d.weight_grad_launches += 1
            if s2:
                dw, db = runtime.conv2d_s2_backward_weight(xr, g, mod.kernel_size[0], mod.padding[0], relu_in=mod.relu_in, want_db=bool(need_b),
                                                           arith=mod.s2_wgrad_arith)
            elif mod.wgrad_arith == "fp32" and mod.bwd_arith == "fp32":
                dw, db = runtime.conv2d_backward_weight(xr, g, mod.kernel_size[0], mod.padding[0], relu_in=mod.relu_in, want_db=bool(need_b))
            else:
                dw, db = runtime.conv2d_backward_weight(xr, g, mod.kernel_size[0], mod.padding[0], relu_in=mod.relu_in, want_db=bool(need_b),
                                                        arith="f32split")
        if need_x:
            split = mod.dgrad_arith == "f32split" or mod.bwd_arith == "f32split"
            if not s2 and not split:
                dx = runtime.conv2d_backward_data(g, weight, mod.padding[0])
            elif not s2:
                dx = runtime.conv2d_backward_data(g, weight, mod.padding[0], arith="f32split")
            elif not split:
                dx = runtime.conv2d_s2_backward_data(g, weight, mod.padding[0])
            else:
                dx = runtime.conv2d_s2_backward_data(g, weight, mod.padding[0], arith="f32split")
            if mod.relu_in:
                runtime.relu_backward(dx, xr, out=dx)
            dx = dx.permute(0, 3, 1, 2)
        return None, dx, (g.permute(0, 3, 1, 2) if need_res else None), (dw if need_w else None), db


class FusionConv2d(nn.Conv2d):
    """One fusion convolution of the OFF sub-network as a trainable module on liboffk: ``nn.Conv2d``'s constructor
    arguments, parameters and state_dict keys (reference checkpoints load into a stage built from these under the
    reference's names), plus ``relu`` (a ReLU behind the conv and its residual add) and ``relu_in`` (the conv reads
    ``max(x, 0)``: RGB_OFF.py:658, conv1 of chain 28a).  ``forward(x, res=None)`` returns
    ``post(conv(in(x)) + bias + res)``; x (and res) are fp32, logical NCHW in channels-last memory -- what ``OFFUnits``
    returns; any other layout is made so once -- and so is the result.  Exact fp32, direct sums in a fixed order: forward
    and every gradient are the same bits on every run.  The parameters are read in place on each call, nothing is
    cached across optimizer steps.  Covers what offk_conv2d_backward_* cover: kernel 1 or 3, stride 1, padding
    (k - 1) / 2, channels in multiples of 64; and what offk_conv2d_s2_backward_* cover, the two stage openers: exactly
    (kernel 7, stride 2, padding 3) and (kernel 5, stride 2, padding 2) on even maps, in_channels a multiple of 32,
    out_channels of 64.  Anything else raises ValueError at construction.

    ``wgrad_arith`` ("fp32", the default: nothing changes) or "f32split": the module's weight and bias gradient run on
    offk_conv2d_backward_weight_split -- both operands cut into three bf16 planes, six of the nine plane products on the
    bf16 matrix pipe (include/offk.h has the bound: the dropped products are at most (2^-21 + 2^-30) sum |g x| per element,
    beside an fp32 accumulation error; integer data stays exact), still bit-reproducible; the forward, the ReLU masks
    and the data gradient are untouched.  Stride-1 modules only (the two stride-2 forms have no split entry: ValueError).
    At n_img = 384 it takes the weight gradient of the 22 stride-1 convs from 3.76 to 2.66 ms (3x3 shapes 0.55 - 0.73 x the
    fp32 entry's time, 1x1 shapes 0.79 - 1.0 x; one shape is NOT faster: 128 -> 128 1x1 on 7x7 maps, 0.036 ms in both;
    DESIGN.md 8.4).

    ``dgrad_arith`` ("fp32", the default: nothing changes) or "f32split": the data gradient of a STRIDE-2 module runs on
    offk_conv2d_s2_backward_data_split -- the conv weight and g cut into three bf16 planes in two pre-pass launches, six of
    the nine plane products on the bf16 matrix pipe (include/offk.h has the K order and the bound: the dropped products are
    at most (2^-21 + 2^-30) sum |g w| per element of dx, beside an fp32 accumulation error; integer data stays exact), still
    bit-reproducible; the forward, the ReLU masks, dW and db are untouched.  Stride-2 modules only (at stride 1 this keyword
    has no split entry: ValueError; ``bwd_arith`` below reaches the stride-1 data gradient).  At n_img = 384 the entry (two pre-passes and the GEMM) takes
    0.99 against 1.36 ms (7x7, 320 -> 64) and 0.91 against 1.18 ms (5x5, 1056 -> 128) on the fp32 entry, same session, interleaved:
    both faster by more than the spread of three repeats.

    ``bwd_arith`` ("fp32", the default: nothing changes) or "f32split": ONE switch that sends every gradient GEMM of the
    module to its split entry where the library has one.  Stride 1: dX on offk_conv2d_backward_data_split (the same
    arithmetic and bound as above with K = (tap = kh k + kw, co); include/offk.h), dW / db on
    offk_conv2d_backward_weight_split.  Stride 2: dX on offk_conv2d_s2_backward_data_split; dW / db stay on the fp32 entry
    under this switch, bit for bit (the stride-2 weight gradient's split entry, offk_conv2d_s2_backward_weight_split, is
    reached by ``s2_wgrad_arith`` below, which combines with this switch).  Together with a non-default ``wgrad_arith`` or
    ``dgrad_arith`` it is a ValueError: there is one way to say it.  The forward and the ReLU masks are untouched.  Measured
    at n_img = 384 (same session, interleaved): the stride-1 split data gradient is NOT faster than the fp32 entry on any of
    the 13 stride-1 shapes -- 1.02 x its time on 832 -> 256 3x3 (0.547 against 0.539 ms), 1.19 - 1.70 x on the other 3x3
    shapes, 1.6 - 2.7 x on the 1x1 shapes; 2.77 against 1.86 ms over the 22 convs, 1.60 against 1.27 ms over the eight 3x3
    convs.  At stride 1 this switch therefore buys the weight gradient's gain (3.76 -> 2.66 ms) and pays 0.91 ms for the
    data gradient; ``wgrad_arith="f32split"`` alone is the faster stride-1 setting today.

    ``s2_wgrad_arith`` ("fp32", the default: nothing changes) or "f32split": the weight and bias gradient of a STRIDE-2
    module run on offk_conv2d_s2_backward_weight_split -- g and in(x) cut into three bf16 planes, six of the nine plane
    products on the bf16 matrix pipe over K = the output pixels, the taps that leave the map zeros on the x side
    (include/offk.h has the K layout and the bound: the dropped products are at most (2^-21 + 2^-30) sum |g x| per element of
    dw, beside an fp32 accumulation error; integer data stays exact), still bit-reproducible; the forward, the ReLU masks and
    the data gradient are untouched.  Stride-2 modules only (at stride 1 it is a ValueError: ``wgrad_arith`` is the stride-1
    weight gradient's switch).  It is a keyword of its own because the two older ones are pinned: ``wgrad_arith="f32split"``
    on a stride-2 module stays a ValueError, and ``bwd_arith="f32split"`` keeps a stride-2 module's dW / db on the fp32 entry.
    It combines freely with ``dgrad_arith`` and with ``bwd_arith``.  At n_img = 384 the entry (the GEMM and the reduce) takes
    1.14 against 1.55 ms (7x7, 320 -> 64) and 1.00 against 1.30 ms (5x5, 1056 -> 128) on the fp32 entry, same session,
    interleaved: both faster by more than the spread of three repeats."""

    weight_grad_launches = 0      # calls of offk_conv2d[_s2]_backward_weight[_split] made by all modules (a frozen layer makes none)

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 padding_mode="zeros", device=None, dtype=None, relu=False, relu_in=False, wgrad_arith="fp32",
                 dgrad_arith="fp32", bwd_arith="fp32", s2_wgrad_arith="fp32"):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias, padding_mode,
                         device=device, dtype=dtype)
        k = self.kernel_size
        if wgrad_arith not in runtime.WGRAD_ARITHS:
            raise ValueError("FusionConv2d: wgrad_arith must be one of %s, got %r" % (", ".join(repr(a) for a in runtime.WGRAD_ARITHS), wgrad_arith))
        if wgrad_arith == "f32split" and self.stride == (2, 2):
            raise ValueError("FusionConv2d: wgrad_arith='f32split' needs stride 1 (the two stride-2 forms have no split entry)")
        self.wgrad_arith = wgrad_arith
        if dgrad_arith not in runtime.DGRAD_ARITHS:
            raise ValueError("FusionConv2d: dgrad_arith must be one of %s, got %r" % (", ".join(repr(a) for a in runtime.DGRAD_ARITHS), dgrad_arith))
        if dgrad_arith == "f32split" and self.stride != (2, 2):
            raise ValueError("FusionConv2d: dgrad_arith='f32split' needs stride 2 (the stride-1 forms have no split entry under this keyword: "
                             "bwd_arith='f32split' runs their data gradient on offk_conv2d_backward_data_split)")
        self.dgrad_arith = dgrad_arith
        if bwd_arith not in runtime.BWD_ARITHS:
            raise ValueError("FusionConv2d: bwd_arith must be one of %s, got %r" % (", ".join(repr(a) for a in runtime.BWD_ARITHS), bwd_arith))
        if bwd_arith == "f32split" and (wgrad_arith != "fp32" or dgrad_arith != "fp32"):
            raise ValueError("FusionConv2d: bwd_arith='f32split' already covers wgrad_arith and dgrad_arith: leave them at their default")
        self.bwd_arith = bwd_arith
        if s2_wgrad_arith not in runtime.WGRAD_ARITHS:
            raise ValueError("FusionConv2d: s2_wgrad_arith must be one of %s, got %r" % (", ".join(repr(a) for a in runtime.WGRAD_ARITHS), s2_wgrad_arith))
        if s2_wgrad_arith == "f32split" and self.stride != (2, 2):
            raise ValueError("FusionConv2d: s2_wgrad_arith='f32split' needs stride 2 (wgrad_arith is the stride-1 weight gradient's switch)")
        self.s2_wgrad_arith = s2_wgrad_arith
        if self.stride not in ((1, 1), (2, 2)) or self.dilation != (1, 1) or self.groups != 1:
            raise ValueError("FusionConv2d: dilation and groups must be 1, stride 1 (kernel 1 or 3) or 2 (kernel 7 with padding 3, "
                             "kernel 5 with padding 2)")
        s2 = self.stride == (2, 2)
        if k not in (((7, 7), (5, 5)) if s2 else ((1, 1), (3, 3))):
            raise ValueError("FusionConv2d: kernel_size must be 1 or 3 at stride 1, 7 or 5 at stride 2")
        if isinstance(self.padding, str) or self.padding != ((k[0] - 1) // 2,) * 2 or self.padding_mode != "zeros":
            raise ValueError("FusionConv2d: padding must be (kernel_size - 1) / 2 zeros")
        if in_channels % (32 if s2 else 64) or out_channels % 64:
            raise ValueError("FusionConv2d: out_channels must be a multiple of 64, in_channels of 64 (stride 1) or 32 (stride 2)")
        if self.weight.dtype != torch.float32:
            raise ValueError("FusionConv2d: fp32 parameters only")
        self.relu, self.relu_in = bool(relu), bool(relu_in)

    def forward(self, x, res=None):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            raise ValueError("FusionConv2d: x must be an fp32 CUDA/HIP tensor [n, C, H, W]")
        if self.stride == (2, 2) and (x.shape[2] % 2 or x.shape[3] % 2):
            raise ValueError("FusionConv2d: a stride-2 module needs an even map")
        if res is not None and (res.dtype != torch.float32 or res.shape != (x.shape[0], self.out_channels) + tuple(d // self.stride[0] for d in x.shape[2:])):
            raise ValueError("FusionConv2d: res must be an fp32 tensor of the output's shape")
        return _FusionConvFn.apply(self, x, res, self.weight, self.bias)

    def extra_repr(self):
        s = super().extra_repr() + ", relu=%s, relu_in=%s" % (self.relu, self.relu_in)
        s = s if self.wgrad_arith == "fp32" else s + ", wgrad_arith=%s" % self.wgrad_arith
        s = s if self.dgrad_arith == "fp32" else s + ", dgrad_arith=%s" % self.dgrad_arith
        s = s if self.bwd_arith == "fp32" else s + ", bwd_arith=%s" % self.bwd_arith
        return s if self.s2_wgrad_arith == "fp32" else s + ", s2_wgrad_arith=%s" % self.s2_wgrad_arith


class _MotionHeadFn(torch.autograd.Function):
    """autograd node of one ``MotionHead``: forward = offk_head_train, backward = offk_head_backward with each of dx, dw, db only where
    ``ctx.needs_input_grad`` asks.  Saved: the [n, H, W, C] rows of x, z (the pooled vector behind the dropout) and the seed -- the mask is
    recomputed from it, never stored."""

    @staticmethod
    def forward(ctx, mod, x, drop, weight, bias):
        xr = x.permute(0, 2, 3, 1).contiguous()                    # no copy where x is channels-last already
        out, z = runtime.head_train(xr, weight, bias, mod.maxpool, mod.head_index, drop)
        ctx.mod, ctx.drop = mod, drop
        ctx.save_for_backward(xr, weight, z)
        return out

    @staticmethod
    def backward(ctx, g):
        mod = ctx.mod
        xr, weight, z = ctx.saved_tensors
        need_x, _, need_w, need_b = ctx.needs_input_grad[1:5]
        if need_w or need_b:
            MotionHead.weight_grad_launches += 1
        dx, dw, db = runtime.head_backward(g.contiguous(), xr, weight, z, mod.maxpool, mod.head_index, ctx.drop, want_dx=bool(need_x),
                                           want_dw=bool(need_w), want_db=bool(need_b))
        return None, (dx.permute(0, 3, 1, 2) if need_x else None), None, dw, db


class MotionHead(nn.Linear):
    """One classifier head of the OFF sub-network (fc_action_motion_28 / fc_action_motion_14 / fc_action_motion, RGB_OFF.py:782-793,
    843-847) as a trainable module on liboffk: ``nn.Linear``'s parameters and state_dict keys (the reference's ``fc_action_motion*`` keys
    load), in front of it the head's pooling -- ``maxpool``: MaxPool2d(3, 2, ceil_mode) first, the 28-head -- the mean over the map and
    nn.Dropout(``drop_p``) on the pooled vector.  ``head_index`` 0 / 1 / 2 (the 28 / 14 / 7 head) picks the dropout stream.
    ``forward(x, drop_seed=None)``: x is fp32, logical [n, C, H, W] in channels-last memory -- what ``FusionConv2d`` returns; any other
    layout is made so once; returns the logits [n, out_features].  In training mode with drop_p > 0 the mask is the library's
    reproducible dropout (``synth.head_dropout_keep``) of ``drop_seed``, or of an own counter that advances per call (as ``OFFUnits``);
    eval mode and drop_p = 0 run without a mask, and where no gradient is asked for that is K5 itself (``runtime.head``).  Exact fp32,
    sums in a fixed order: forward and every gradient are the same bits on every run.  The parameters are read in place on each call,
    nothing is cached across optimizer steps.  in_features: a multiple of 4 in [4, 1024]; fp32 parameters; drop_p in [0, 1) --
    anything else raises ValueError at construction."""

    weight_grad_launches = 0      # offk_head_backward calls with a weight or bias gradient made by all modules (a frozen head makes none)

    def __init__(self, in_features, out_features=101, maxpool=False, head_index=0, drop_p=0.8, bias=True, device=None, dtype=None):
        if not (isinstance(in_features, int) and 4 <= in_features <= 1024 and in_features % 4 == 0):
            raise ValueError("MotionHead: in_features must be a multiple of 4 in [4, 1024]")
        if not bias:
            raise ValueError("MotionHead: the head has a bias (bias=True)")
        if not (0.0 <= float(drop_p) < 1.0):
            raise ValueError("MotionHead: drop_p must be in [0, 1)")
        if not (isinstance(head_index, int) and 0 <= head_index <= 239):
            raise ValueError("MotionHead: head_index must be an int in [0, 239] (0 / 1 / 2: the 28 / 14 / 7 head)")
        super().__init__(in_features, out_features, bias=True, device=device, dtype=dtype)
        if self.weight.dtype != torch.float32:
            raise ValueError("MotionHead: fp32 parameters only")
        self.maxpool, self.head_index, self.drop_p, self.drop_seed = bool(maxpool), head_index, float(drop_p), 0

    def forward(self, x, drop_seed=None):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == self.in_features):
            raise ValueError("MotionHead: x must be an fp32 CUDA/HIP tensor [n, %d, H, W]" % self.in_features)
        if self.maxpool and (x.shape[2] < 3 or x.shape[3] < 3):
            raise ValueError("MotionHead: maxpool needs a map of 3 x 3 or more")
        if self.training and self.drop_p > 0.0:
            if drop_seed is None:
                self.drop_seed += 1
                drop_seed = self.drop_seed
            drop = (int(drop_seed), self.drop_p)
        else:
            drop = (0, 0.0)
        wants_grad = torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or self.bias.requires_grad)
        if drop == (0, 0.0) and not wants_grad:
            return runtime.head(x.permute(0, 2, 3, 1).contiguous(), self.weight.detach(), self.bias.detach(), self.maxpool)
        return _MotionHeadFn.apply(self, x, drop, self.weight, self.bias)

    def extra_repr(self):
        return super().extra_repr() + ", maxpool=%s, head_index=%d, drop_p=%g" % (self.maxpool, self.head_index, self.drop_p)


class BNInception_OFF(nn.Module):
    """Drop-in for the reference class of the same name, OFF part on liboffk.

    ``backbone`` is any module mapping the frame batch [B*L, 3|10, 224, 224] to
    ``(feats, Feature_Generation_Score)`` or ``(feats, Feature_Generation_Score, conv2_relu_3x3_out)``
    -- i.e. the reference's own layers up to RGB_OFF.py:594.  Without a backbone the
    ``input`` of forward must already be the list of nine feature maps (then
    Feature_Generation_Score is returned as None).
    """

    def __init__(self, num_classes=1000, batch=16, length=7, variant="rgb", backbone=None,
                 slice_mode=spec.SLICE_FLAT, precision="fp32"):
        super().__init__()
        self.batch, self.length = batch, length
        self.modality_fuse = False                       # Flow_OFF.py:45
        self.consensus_type = "avg"                      # RGB_OFF.py:39
        self.variant_name = variant
        self.backbone = backbone
        self.off = OFFSubNetwork(num_classes, batch, length, variant, slice_mode, precision=precision)

    def state_dict(self, *a, **kw):
        sd = super().state_dict(*a, **kw)
        # flatten 'off.' so the keys are the reference's (motion_*, fc_action_motion*, sobel_edge_diagonal.*)
        return type(sd)((k[4:] if k.startswith("off.") else k, v) for k, v in sd.items())

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Reference-format checkpoints (model_utils.py:188-216, Flow_OFF.py:1398-1413): OFF keys and backbone keys side
        by side at top level, optionally under a DataParallel 'module.' prefix (test_flow_off.py:52-58).  OFF keys go to
        the OFF sub-network, everything else to the backbone (plain or 'backbone.'-prefixed names).  Returns the
        (missing_keys, unexpected_keys) named tuple of nn.Module.load_state_dict; with strict=True missing OFF keys
        raise KeyError and keys nobody takes raise RuntimeError."""
        from torch.nn.modules.module import _IncompatibleKeys
        plain = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        own = set(self.off.state_dict().keys())
        self.off.load_state_dict({k: v for k, v in plain.items() if k in own}, strict=strict)
        missing = sorted(own - set(plain))
        rest = {(k[9:] if k.startswith("backbone.") else k): v for k, v in plain.items() if k not in own}
        unexpected = []
        if self.backbone is not None:
            r = self.backbone.load_state_dict(rest, strict=False)
            missing += ["backbone." + k for k in r.missing_keys]
            unexpected = list(r.unexpected_keys)
        else:
            unexpected = sorted(rest)      # no backbone attached: nobody takes the TSN keys
        if strict and self.backbone is not None and unexpected:
            raise RuntimeError("unexpected keys in state_dict: %s" % ", ".join(unexpected[:5]))
        return _IncompatibleKeys(missing, unexpected)

    def _features(self, input):
        if self.backbone is None:
            return list(input), None, None
        r = self.backbone(input)
        return list(r[0]), r[1], (r[2] if len(r) > 2 else None)

    @staticmethod
    def _squeeze(x):
        # torch.squeeze at RGB_OFF.py:786,792,846 also drops the pair axis when P == 1
        return x[0] if x.shape[0] == 1 else x

    def RGB_OFF_forward(self, input):
        """RGB_OFF.py:360-860: returns (fc_action_motion_7, Feature_Generation_Score, fc_action_motion_14)."""
        feats, fgs, _ = self._features(input)
        fc7, fc14, _fc28 = self.off(feats, want28=False)
        return self._squeeze(fc7), fgs, self._squeeze(fc14)

    def forward(self, input):
        """Flow_OFF.py:370-887 / RGB_OFF_v2.py:377-894 for the flow / rgb_v2 variants
        (consensus average inside, optional fused score); for the rgb variant this is
        RGB_OFF_forward (the reference's plain ``forward`` there is the backbone only)."""
        if self.off.variant == spec.VARIANT_RGB:
            return self.RGB_OFF_forward(input)
        feats, fgs, conv2 = self._features(input)
        fc7, fc14, _fc28 = self.off(feats, want28=False)
        # K6 / K7 are raw library calls on data_ptr: they do not record an autograd graph.  The reference uses this path at test time
        # only (test_flow_off.py:343 under volatile=True); when a caller DOES want gradients through the backbone's score (grad mode
        # on and the score requires grad) the same arithmetic runs as torch ops so the graph stays intact.
        wants_grad = torch.is_grad_enabled() and fgs is not None and fgs.requires_grad
        if fgs is not None and fgs.shape[0] == self.batch * self.length:
            if wants_grad:
                fgs = fgs.float().reshape(self.batch, self.length, -1).mean(dim=1)          # basic_ops.py:19-21
            else:
                fgs = runtime.segment_consensus(fgs.contiguous().float(), self.batch)   # Flow_OFF.py:867,873 (K6)
        if self.modality_fuse:
            if fgs is None:
                raise ValueError("modality_fuse adds the backbone's Feature_Generation_Score (Flow_OFF.py:881): "
                                 "attach a backbone that returns it")
            if wants_grad or fc7.requires_grad or fc14.requires_grad:
                return fc7 + fgs.to(fc7.dtype) + fc14                                    # Flow_OFF.py:881, differentiable
            # Flow_OFF.py:881 `fc7 + fgs + fc14`: K7 with unit weights and one "crop" (offk_score_fusion), not a torch op
            fused, _ = runtime.score_fusion([fc7, fgs.to(fc7.dtype).contiguous(), fc14], (1.0, 1.0, 1.0), want_pred=False)
            return fused
        if self.variant_name == "rgb_v2":
            return fc7, fgs, fc14, conv2                                       # RGB_OFF_v2.py:891
        return fc7, fgs, fc14                                                  # Flow_OFF.py:884


def bninception_off(num_classes=101, batch=16, num_seg=7, variant="rgb", backbone=None, **kw):
    """RGB_OFF.py:1346-1360 / Flow_OFF.py:1371-1385 factory."""
    return BNInception_OFF(num_classes=num_classes, batch=batch, length=num_seg, variant=variant,
                           backbone=backbone, **kw)
