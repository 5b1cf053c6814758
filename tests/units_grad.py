"""What the GPU tests of the OFF units' training side share (tests/test_gpu_backward.py, test_gpu_feat_grad*.py, test_gpu_wgrad_split.py,
test_gpu_units_fwd_split.py and the files that borrow a case from them: test_gpu_sobel_taps.py, test_gpu_bound_weights.py,
test_gpu_big_batch.py, test_gpu_train_ranges.py): the constants, the layout and bit predicates, `Case` (one handle after forward +
backward on random dM) behind the one cached `case`, the shape tables of the two split GEMM files, the module helpers, the split dX
entry's operands and inequality, and the forms table of the three dX entries (DX_FORMS; the bodies written against it are
tests/units_dx_checks.py).  The `rt` fixture, the oracle-side inputs (cotangents, unit_drop, grad_views, device_relu_masks, rel_err) and
the feature-map kinds are tests/featmaps.py's and are re-exported here.  A helper module like tests/arena.py: no tests of its own."""
import ctypes
import functools

import numpy as np
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec, synth
from oracle import off_oracle as orc

from . import arena as arena_mod
from . import split_bound as sb
from .exact import down_rows  # noqa: F401  (r(n) of every frame n, -1 outside the spatial slice: the one definition)
from .featmaps import DROP_P, DROP_SEED, captured, cotangents, device_relu_masks, grad_views, rel_err, rt, to_cl, unit_drop  # noqa: F401
from .units_fwd_split import DOWN_B, DOWN_W, GEN_B, GEN_W  # noqa: F401

RTOL = 2e-4                     # gradients are sums of up to N*H*W ~ 3.5e5 products: of each tensor's max magnitude (the north_star bar is 1e-3)
U = 2.0 ** -23
FEAT = {torch.float32: _lib.FEAT_F32, torch.bfloat16: _lib.FEAT_BF16, torch.float16: _lib.FEAT_F16}

# the (B, L, variant, slice_mode) cases of the two split GEMM files (tests/test_gpu_wgrad_split.py, tests/test_gpu_units_fwd_split.py):
# (1, 2) flat -- N = 2, one partial tile at the 7x7 sites; (2, 3) flat -- quirk Q1; (3, 4) per-clip; (2, 3) flat, Flow; (8, 7) per-clip
SHAPES = [(1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT), (2, 3, spec.VARIANT_RGB, spec.SLICE_FLAT), (3, 4, spec.VARIANT_RGB, spec.SLICE_PER_CLIP),
          (2, 3, spec.VARIANT_FLOW, spec.SLICE_FLAT), (8, 7, spec.VARIANT_RGB, spec.SLICE_PER_CLIP)]
IDS = ["b1l2_flat", "b2l3_flat", "b3l4_clip", "b2l3_flat_flow", "b8l7_clip"]
DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FORMS = [(lay, dt) for lay in ("nchw", "cl") for dt in DTS]          # the six map forms


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.cuda().contiguous()


def as_form(feats, layout, dt):
    fmt = torch.contiguous_format if layout == "nchw" else torch.channels_last
    return [f.to(DTS[dt]).contiguous(memory_format=fmt) for f in feats]


def random_views(P, seed=5, scale=1.0):
    """Random gradients w.r.t. the three fusion buffers (channels-last) and the nine (tensor, coff) views of the units in them."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bufs = [scale * torch.randn(P, H, H, C, device="cuda", generator=gen) for H, C in ((28, 320), (14, 1056), (7, 832))]
    return bufs, [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]


# ---- layouts and bits ----

def as_rows(t, layout):
    """[N, C, H, H] fp32 result of either layout -> [N, HW, C] on the host."""
    assert t.dtype == torch.float32 and t.dim() == 4
    if layout == "cl":
        assert t.permute(0, 2, 3, 1).is_contiguous()
    else:
        assert t.is_contiguous()
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).cpu()


def rows_of(t):
    """[N, C, H, H] result of either layout -> [N*HW, C] (a view where the layout allows, values unchanged)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def rows16(t, layout):
    """[N, C, H, H] 16-bit result of either layout -> [N * HW, C], on the device."""
    assert t.dim() == 4 and (t.permute(0, 2, 3, 1).is_contiguous() if layout == "cl" else t.is_contiguous())
    return rows_of(t)


def bits16(t):
    return t.contiguous().view(torch.int16)


def same_bits16(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits16(a), bits16(b))


def same_bits_any(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return arena_mod.same_bits(a, b) if a.dtype == torch.float32 else torch.equal(bits16(a), bits16(b))


def region_span(h, name):
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(h.lib.offk_workspace_region(h._h, name.encode(), ctypes.byref(off), ctypes.byref(nb)), h._h)
    return off.value, nb.value


# ---- one handle after forward + backward ----

class Case:
    """One handle after forward + backward on random dM, with everything the checks share."""

    def __init__(self, rt, B, L, variant, slice_mode, seed):
        self.B, self.L, self.variant, self.slice_mode, self.seed = B, L, variant, slice_mode, seed
        self.N, self.P = B * L, B * (L - 1)
        self.h = rt.OffForward(B, L, variant, slice_mode, training=True)
        self.wnp = synth.make_weights(variant)
        assert self.h.load_state_dict(self.wnp) == []
        self.w = orc.to_torch_weights(self.wnp)
        self.feats_np = synth.make_features(B, L, 2 if B == 2 else 3)
        self.feats = [dev(f) for f in self.feats_np]
        self.bufs, self.views = random_views(self.P)
        self.drop = (0, 0.0) if seed is None else (seed, DROP_P)
        self.run()

    def forward(self, feats=None):
        feats = self.feats if feats is None else feats
        if self.seed is None:
            self.h.off_units(feats)
        else:
            self.h.off_units_train(feats, self.seed, DROP_P)

    def backward(self, feats=None, views=None, grads=None):
        return self.h.off_units_backward(self.feats if feats is None else feats, self.views if views is None else views,
                                         self.drop[0], self.drop[1], grads=grads)

    def run(self):
        self.forward()
        self.backward()

    def weights(self, si):
        site = spec.SITES[si][0]
        return (self.w[GEN_W % site].reshape(128, -1), self.w[DOWN_W % site].reshape(32, -1))

    def bind_unit_weights(self):
        """Device copies of every unit parameter, bound in place of the handle's own; {key: tensor}."""
        bound = {}
        for k, v in self.wnp.items():
            if k.startswith(spec.UNIT_PARAM_PREFIXES):
                bound[k] = dev(v)
                self.h.bind_weight(k, bound[k])
        return bound

    def reference(self, si, wg=None, wd=None):
        """fp64 product of the kernel's own inputs on the host, as [N, HW, C], its bound, and the gen part alone."""
        site, C, H = spec.SITES[si]
        HW = H * H
        dG = self.h.region("dG_" + site, 128).cpu().double().view(self.N, HW, 128)
        dD = self.h.region("dD_" + site, 32).cpu().double().view(self.P, HW, 32)
        if wg is None:
            wg, wd = self.weights(si)
        wg, wd = wg.double(), wd.double()
        rows = down_rows(self.B, self.L, self.slice_mode)
        inside = torch.tensor([r >= 0 for r in rows])
        dDn = torch.zeros(self.N, HW, 32, dtype=torch.float64)
        dDn[inside] = dD[torch.tensor([r for r in rows if r >= 0], dtype=torch.long)]
        gen = dG @ wg
        ref = gen + dDn @ wd
        bound = 160 * U * (dG.abs() @ wg.abs() + dDn.abs() @ wd.abs())
        return ref, bound, gen, inside


@functools.lru_cache(maxsize=None)
def case(rt, B, L, variant, slice_mode, seed):
    return Case(rt, B, L, variant, slice_mode, seed)


def oracle_dx(c):
    """x.grad of every site of a Case from the oracle's unit, the device's ReLU decisions on both sides."""
    tf = [torch.from_numpy(f) for f in c.feats_np]
    masks = device_relu_masks(c.h, tf, c.w, c.B, c.L)
    drops = None if c.seed is None else unit_drop(c.seed, c.P)
    out = []
    for si, ((site, _c, _h), x) in enumerate(zip(spec.SITES, tf)):
        buf, coff = c.views[si]
        dm = buf[..., coff:coff + 160].permute(0, 3, 1, 2).cpu()
        x = x.clone().requires_grad_(True)
        orc.off_unit(x, c.w, site, c.B, c.L, c.variant, c.slice_mode, None if drops is None else drops[si], masks[si]).backward(dm)
        out.append(x.grad)
    return out


@functools.lru_cache(maxsize=None)
def exact_case(B, L, variant, slice_mode):
    from . import exact_units as gx
    return gx.Case(B, L, variant, slice_mode)           # (its constructor asserts exact.check_caps on every output, dX among them)


def workspace_arena(h, maps, more_bytes=()):
    """The arena of the two split GEMM files' test_memory_discipline: room for the workspace, the maps and `more_bytes`, the handle moved onto
    its first carve.  (arena, workspace)"""
    ar = arena_mod.Arena.for_sizes([h.workspace_bytes] + list(more_bytes) + [m.numel() * m.element_size() for m in maps])
    ws = ar.carve("workspace", h.workspace_bytes)
    h.set_workspace(ws)
    return ar, ws


def guarded_maps(ar, maps, layout):
    """Copies of the maps as carves of the arena, each exactly its elements in its own layout."""
    if layout == "nchw":
        return [ar.put("map_%d" % i, m) for i, m in enumerate(maps)]
    gm = [ar.put("map_%d" % i, m.permute(0, 2, 3, 1)).permute(0, 3, 1, 2) for i, m in enumerate(maps)]
    assert all(m.is_contiguous(memory_format=torch.channels_last) for m in gm)
    return gm


# ---- the module ----

def make_units(B, L, feat_grad, variant="rgb", **kw):
    from offk_amd.off_module import OFFUnits
    wnp = synth.make_weights(spec.VARIANT_RGB if variant == "rgb" else spec.VARIANT_FLOW)
    u = OFFUnits(B, L, variant, feat_grad=feat_grad, **kw).cuda()
    u.load_state_dict({k: torch.from_numpy(a) for k, a in wnp.items() if k in u.state_dict()}, strict=True)
    u.train()
    return u, wnp


def module_cots(P, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).cuda() for s in ((P, 320, 28, 28), (P, 800, 14, 14), (P, 320, 7, 7))]


def assert_module_dx_matches_the_oracle(u, wnp, feats_np, feats, cots, B, L, seed=7):
    """x.grad of every map of a (B, L) flat RGB OFFUnits after backward(cots) against the oracle's unit, the device's ReLU decisions on
    both sides: RTOL of each tensor's max magnitude."""
    w = orc.to_torch_weights(wnp)
    tf = [torch.from_numpy(f) for f in feats_np]
    masks = device_relu_masks(u._rt, tf, w, B, L)
    drops = unit_drop(seed, B * (L - 1))
    dms = [cots[0][:, :160], cots[0][:, 160:]] + [cots[1][:, 160 * k:160 * k + 160] for k in range(5)] + [cots[2][:, :160], cots[2][:, 160:]]
    for si, ((site, _c, _h), x) in enumerate(zip(spec.SITES, tf)):
        x = x.clone().requires_grad_(True)
        orc.off_unit(x, w, site, B, L, spec.VARIANT_RGB, spec.SLICE_FLAT, drops[si], masks[si]).backward(dms[si].cpu())
        assert feats[si].grad is not None and feats[si].grad.shape == x.grad.shape
        assert rel_err(feats[si].grad, x.grad) < RTOL, site


# ---- the split dX entry: its operands and its inequality ----

def dx_operands(h, B, L, slice_mode, si, wg, wd, rows=None):
    """The dX kernel's own operands of site si on the host: a [M, 160] (the dD part at row r(n), zeros outside the slice) and w [C, 160],
    fp32 numpy; rows: an index tensor of rows of a to take (full-size case)."""
    site, C, H = spec.SITES[si]
    HW, N = H * H, B * L
    r_of = torch.tensor(down_rows(B, L, slice_mode), device="cuda")
    idx = torch.arange(N * HW, device="cuda") if rows is None else rows
    f, px = idx // HW, idx % HW
    r = r_of[f]
    a = torch.zeros(idx.numel(), 160, device="cuda")
    a[:, :128] = h.region("dG_" + site, 128)[idx]
    ins = r >= 0
    a[ins, 128:] = h.region("dD_" + site, 32)[(r * HW + px)[ins]]
    w = torch.cat((torch.as_tensor(wg).reshape(128, C), torch.as_tensor(wd).reshape(32, C))).t().contiguous()
    return a.cpu().numpy(), w.cpu().numpy()


def dx_check_inequality(tag, got, a, w, got32=None):
    """Asserts, per element and none excluded, |got - ref64| <= |dropped64| + A 2^-24 sum|a w| + 2^-24 |ref64|, A = max(1, 2 c_acc), for got
    [M, C] (fp32 tensor or array) on the operands (a, w), c_acc the CPU emulation's (form "units", K = 160); prints the emulated and the
    measured accumulation constants and the errors against fp64 (beside them the fp32 entry's, when given).  Returns (c_acc emulated, gpu)."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    ref, dropped, mag = synth.split_terms(w, a)
    assert got.shape == ref.shape
    c_emu = sb.c_acc(synth.emulate_split_dot(w, a, form="units"), ref, dropped, mag)
    A = max(1.0, 2.0 * c_emu)
    unit = np.maximum(sb.EPS * mag, 1e-300)
    err = np.abs(got - ref)
    c_gpu = float((np.abs(got - (ref - dropped)) / unit).max())
    line = "%s: c_acc emulated %.3f -> A %.3f | gpu accumulation %.3f | dropped (exact) max %.3f | err max %.3e rms %.3e" % (
        tag, c_emu, A, c_gpu, float((np.abs(dropped) / unit).max()), float(err.max()), float(np.sqrt((err ** 2).mean())))
    if got32 is not None:
        e32 = np.abs(np.asarray(got32.detach().cpu(), dtype=np.float64) - ref)
        line += " | fp32 entry: err max %.3e rms %.3e" % (float(e32.max()), float(np.sqrt((e32 ** 2).mean())))
    print(line)
    zero = mag == 0
    assert not got[zero].any(), "%s: %d elements with sum|a w| = 0 are not exactly 0" % (tag, int((got[zero] != 0).sum()))
    over = sb.excess_map(got, ref, dropped, mag, A)
    assert float(over.max()) <= 0.0, "%s: element %d misses the limit by %.3e (err %.3e)" % (tag, int(over.argmax()), float(over.max()),
                                                                                            float(err.reshape(-1)[over.argmax()]))
    return c_emu, c_gpu


# ---- the three dX entries: one host body in offk_api.hip (off_units_backward_feats), one row each here ----

def _traces(extra):
    """{(dtype, layout): trace name} of an entry, as offk_api.hip's kDxTrace / kDxsTrace spell them"""
    tail = {torch.float32: "", torch.bfloat16: ", bf16", torch.float16: ", fp16"}
    return {(dt, lay): "units:feature-map gradient (dX, %s%s%s)" % ({"nchw": "NCHW", "cl": "NHWC"}[lay], extra, tail[dt])
            for dt in tail for lay in ("nchw", "cl")}


class DxForm:
    """One dX entry.  entry: the C name, which every refusal's text begins with; takes_dtype: whether the entry has a grad_dtype argument
    (the fp32 entry has none: `grad_dtype must be` cannot be stated for it, and OFFK_FEAT_F32 is the only code it is called with);
    f32_entry: the entry that answers when grad_dtype is OFFK_FEAT_F32 (the typed entry hands that call to the fp32 one); kw: how
    runtime.off_units_backward_feats reaches it beside dtype=; dtypes: the result dtypes it is tested with (the output's element size is the
    dtype's own); same: its equality predicate; traces: its trace names."""

    def __init__(self, name, entry, takes_dtype, f32_entry, kw, dtypes, same, traces):
        self.name, self.entry, self.takes_dtype, self.f32_entry, self.kw = name, entry, takes_dtype, f32_entry, kw
        self.dtypes, self.same, self.traces = dtypes, same, traces

    def __repr__(self):
        return "DxForm(%s)" % self.name

    def call(self, h, **kw):
        """h.off_units_backward_feats through this entry; dtype= (default fp32) picks the result dtype.  The typed form at fp32 is the fp32
        entry: the result its 16-bit forms are defined by."""
        return h.off_units_backward_feats(**dict(self.kw, **kw))

    def raw(self, lib, handle, stream, ws, code, arr, layout, accumulate=0):
        """the C entry through ctypes, no Python-side checks; code: the OFFK_FEAT_* of the result dtype"""
        fn = getattr(lib, self.entry)
        if not self.takes_dtype:
            assert code == _lib.FEAT_F32
            return fn(handle, stream, ws, arr, layout, accumulate)
        return fn(handle, stream, ws, code, arr, layout, accumulate)

    def named_in(self, code):
        """the name a refusal of a call with this grad_dtype carries"""
        return self.f32_entry if code == _lib.FEAT_F32 else self.entry


DX_FP32 = DxForm("fp32", "offk_off_units_backward_feats", False, "offk_off_units_backward_feats", {}, (torch.float32,),
                 arena_mod.same_bits, _traces(""))
DX_TYPED = DxForm("typed", "offk_off_units_backward_feats_typed", True, "offk_off_units_backward_feats", {}, (torch.bfloat16, torch.float16),
                  same_bits16, _traces(""))
DX_SPLIT = DxForm("split", "offk_off_units_backward_feats_split", True, "offk_off_units_backward_feats_split", {"arith": "f32split"},
                  (torch.float32, torch.bfloat16, torch.float16), same_bits_any, _traces(", split"))
DX_FORMS = (DX_FP32, DX_TYPED, DX_SPLIT)
