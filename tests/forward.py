"""Common ground of the forward family's GPU tests (tests/test_gpu_parity.py, test_gpu_paths.py, test_gpu_switches.py, test_gpu_heads.py,
test_gpu_bounds.py and the files that build on them): the tolerances and case lists, the trace names of the launches, the path tables,
the ONE handle maker, the caches of features and oracle runs (one instance each: a shape's oracle is computed once for every file), the
per-launch trace and the ONE whole-forward check.  A helper module like tests/arena.py: no tests of its own (tests/test_forward_checks.py
checks on the CPU what has no device in it).  The `rt` fixture is tests/featmaps.py's; a test file imports it by name.

Tolerance: BASELINE.json north_star asks for 1e-3 relative fp32.  The HIP path computes in exact fp32 (v_mfma_f32_32x32x2_f32 is an fmaf
chain), so the tests hold it to RTOL = 2e-4 of the tensor's max magnitude -- five times tighter than the stated bar -- so that a wrong
bias / tap / channel offset cannot hide inside the budget."""
import contextlib
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc

RTOL_NORTH_STAR = 1e-3
RTOL = 2e-4
PRECISIONS = ["fp32"]   # (until round 4 also "bf16x3", the two-plane split mode: retired in ABI v9 in favour of the exact three-plane mode)
# handle-level arithmetic modes: f32split = fp32 operands as three bf16 planes on the bf16 pipe (round 5; its own error tests:
# tests/test_gpu_split.py); kernels without a split form run as in fp32
HANDLE_PRECISIONS = PRECISIONS + ["f32split"]
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = ["rgb_b1_l7", "rgb_b2_l3", "rgb_b3_l7", "flow_b1_l7", "flow_b2_l3", "flow_b3_l7", "rgbv2_b2_l3"]
RET_GOLDEN = ["ret_rgb_b2_l3", "ret_rgb_b1_l2", "ret_flow_b2_l3", "ret_flow_b1_l2", "ret_rgbv2_b2_l3"]
CONV_CASES = [  # (Ci, Co, k, stride, pad, H, n_img)  -- the distinct shapes of spec.FUSION_CONVS at small size
    (320, 64, 7, 2, 3, 28, 2), (64, 64, 1, 1, 0, 14, 3), (64, 64, 3, 1, 1, 14, 2), (64, 256, 1, 1, 0, 14, 2),
    (256, 64, 1, 1, 0, 14, 2), (1056, 128, 5, 2, 2, 14, 2), (128, 128, 3, 1, 1, 7, 5), (128, 512, 1, 1, 0, 7, 3),
    (512, 128, 1, 1, 0, 7, 3), (128, 512, 3, 1, 1, 7, 3), (832, 256, 3, 1, 1, 7, 2), (256, 1024, 1, 1, 0, 7, 3),
]
PATCH_CASES = [  # (k, stride, H, Ci, Co, n_img, cfg, splitk): the four shapes of the LDS-patch kernel, partial last groups
    (7, 2, 28, 320, 64, 3, 7, 1), (7, 2, 28, 64, 128, 2, 6, 2), (5, 2, 14, 1056, 128, 6, 6, 3), (5, 2, 14, 96, 64, 9, 7, 1),
    (3, 1, 14, 64, 64, 3, 7, 2), (3, 1, 14, 128, 256, 2, 6, 1), (3, 1, 7, 832, 256, 7, 6, 4), (3, 1, 7, 128, 128, 5, 7, 1),
    (3, 1, 7, 256, 256, 8, 6, 3),
]
# the stage tensors a forward leaves in the workspace: (region, channels per pixel, map size)
STAGES = (("fusion_28", 320, 28), ("fusion_14", 1056, 14), ("fusion_7", 832, 7), ("sum_7", 1024, 7))
LOGITS = ("fc7", "fc14", "fc28")
# every pair-count gate forced open (read once, at offk_create)
FORCE = {"OFFK_CHAIN": "2", "OFFK_WINOGRAD_5X5": "2", "OFFK_WINOGRAD_7X7": "2"}

# ---- names in the per-launch trace (offk_launch_times) ----
WINO, CHAINS = "[winograd", ("chain_28a", "chain_28b", "chain_28c")
FC_FOLDED, POOL_ROWS_28 = "heads (fc on folded pools, one launch)", "head_28 (max pool rows)"
POOL_FC = ("head_7 (pool + fc)", "head_14 (pool + fc)", "head_28 (pool + fc)")
W5, W7, BETWEEN = "motion_conv_trans_14 [winograd", "motion_conv_trans_28 [winograd", "[winograd: between]"


def rel_err(a, b):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(a).double()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def signal_err(a, b):
    """Error of the ROW-TO-ROW signal: the logits are bias-dominated under default init (the part that
    differs between rows is ~2.6 % of their magnitude), so rel_err admits ~1 % of the actual signal.  This removes the
    per-class mean over rows from both sides and normalises by the signal's own maximum."""
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(a).double()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(b).double()
    assert a.shape == b.shape and a.shape[0] >= 2, (a.shape, b.shape)
    da, db = a - a.mean(0, keepdim=True), b - b.mean(0, keepdim=True)
    return ((da - db).abs().max() / (db.abs().max() + 1e-30)).item()


def dev(x):
    return torch.as_tensor(x).to("cuda").contiguous()


def nhwc(x):  # logical NCHW cpu tensor -> channels-last physical, on device
    return x.permute(0, 2, 3, 1).contiguous().to("cuda")


# ---- the one handle maker ----
@contextlib.contextmanager
def switches(env):
    """The switches of INTEGRATION.md section 7 in `env`, set inside the block and put back after it, whether or not it raises."""
    saved = dict((k, os.environ.get(k)) for k in env)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def default_weights(variant):
    """synth.make_weights(variant), made once (a quarter of a second each time) and never written to."""
    return synth.make_weights(variant)


def make_handle(rt, B, L, variant, slice_mode=spec.SLICE_FLAT, consensus=None, weights=None, precision="fp32", env=None,
                num_classes=spec.NUM_CLASSES, **kw):
    """A handle with all its weights loaded -> (handle, the weights as the oracle takes them).  `env`: switches of INTEGRATION.md
    section 7, set around OffForward's construction only (they are read once, at offk_create; `switches`);
    `weights`: a numpy state dict (default: synth's for the variant); `kw`: OffForward's other arguments (feat_layout, training)."""
    with switches(env or {}):
        h = rt.OffForward(B, L, variant, slice_mode, consensus, num_classes=num_classes, precision=precision, **kw)
    w = default_weights(variant) if weights is None else weights
    unknown = h.load_state_dict(w)
    assert unknown == [], "load_state_dict left keys over: %s" % (unknown,)
    missing = h.missing_weights()
    assert missing[0] == 0, "%d weight(s) not set: %s" % (missing[0], missing[1])
    return h, orc.to_torch_weights(w)


# ---- shapes, features and oracle runs: one cache each ----
def shape_of(shape, golden_dir=GOLDEN_DIR):
    """A golden tag (variant, B, L and the feature config come from its meta) or (variant, B, L, feature config)
    -> (variant, B, L, cfg, the golden or None)."""
    if isinstance(shape, str):
        g = np.load(os.path.join(golden_dir, shape + ".npz"))
        variant, B, L, cfg = (int(v) for v in g["meta"])
        return variant, B, L, cfg, g
    return tuple(shape) + (None,)


_FEATS, _ORACLE, _ORACLE_B64 = {}, {}, {}


def features(B, L, cfg):
    """The nine maps of a shape; the last two shapes asked for are kept (the cases of one shape run one after the other)."""
    if (B, L, cfg) not in _FEATS:
        while len(_FEATS) >= 2:
            _FEATS.pop(next(iter(_FEATS)))
        _FEATS[(B, L, cfg)] = synth.make_features(B, L, cfg)
    return _FEATS[(B, L, cfg)]


def oracle(variant, B, L, cfg, w):
    """(logits, stage tensors) of the oracle on features(B, L, cfg) and the DEFAULT weights, once per shape: shared by every case and both
    arithmetic modes, never written to.  The cache key has no weights in it, so other weights than default_weights(variant) are refused."""
    w0 = default_weights(variant)
    other = [k for k in w0 if k.endswith(".bias") and not np.array_equal(w0[k], np.asarray(w[k]))]
    assert sorted(w) == sorted(w0) and not other, "oracle() caches the default weights' run; these differ: %s" % (other or sorted(set(w) ^ set(w0)))
    key = (variant, B, L, cfg)
    if key not in _ORACLE:
        with torch.no_grad():
            want, st = orc.off_forward([torch.from_numpy(f) for f in features(B, L, cfg)], w, B, L, variant, orc.SLICE_FLAT,
                                       consensus=False, return_stages=True)
        _ORACLE[key] = (want, dict((name, st[name]) for name, _ch, _H in STAGES))
    return _ORACLE[key]


def oracle_b64(variant, feats_np, w):
    """The oracle's B = 64 forward with stage tensors (~25 s of host time): once per variant, shared by both arithmetic modes."""
    if variant not in _ORACLE_B64:
        with torch.no_grad():
            _ORACLE_B64[variant] = orc.off_forward([torch.from_numpy(f) for f in feats_np], w, 64, 7, variant, orc.SLICE_FLAT, consensus=False,
                                                   return_stages=True)
    return _ORACLE_B64[variant]


# ---- the per-launch trace ----
def traced_forward(h, feats):
    """One forward with the per-launch trace on: (names of its launch groups, logits)."""
    h.set_profiling(2)
    out = h.forward(feats)
    torch.cuda.synchronize()
    names = list(h.launch_times().keys())
    h.set_profiling(0)
    return names, out


def has(names, sub):
    return any(sub in n for n in names)


def check_trace(names, must, must_not):
    for sub in must:
        assert has(names, sub), "no launch named %r in %s" % (sub, names)
    for sub in must_not:
        assert not has(names, sub), "a launch named %r in %s" % (sub, names)


# ---- the one whole-forward check ----
def stage_errs(h, st, P, rows=None):
    """Error of every STAGES region against the oracle's stage tensors (rows: the oracle holds these pair rows only)."""
    out = {}
    for name, ch, H in STAGES:
        got = h.region(name, ch).view(P, H, H, ch)
        out[name] = rel_err((got if rows is None else got[rows.to(got.device)]).permute(0, 3, 1, 2), st[name])
    return out


def check_whole_forward(h, out, shape, w, what, rows=None, oracle_run=None):
    """The logits `out` of a forward handle h has just run (consensus off), and the stage tensors it left, against the references.
    shape: a golden tag or (variant, B, L, feature config) -- the forward ran on features(B, L, cfg) with the default weights; the oracle
    comes from the cache -- or None beside oracle_run, the (logits, stage tensors) of an oracle run of the caller's own.  rows: `out` and
    the oracle hold these pair rows only.  Asserted:
      * the logits against the golden, where there is one, and against the oracle, < RTOL;
      * every STAGES tensor against the oracle, < RTOL;
      * the row-to-row signal of all three logits against both, < RTOL_NORTH_STAR (not with fewer than two rows);
      * fusion_7[:, :160] against the golden's full_motion_5a, where it has it.
    Returns the stage errors."""
    assert (shape is None) != (oracle_run is None), "one of shape and oracle_run"
    if shape is not None:
        variant, B, L, cfg, g = shape_of(shape)
        want, st = oracle(variant, B, L, cfg, w)
    else:
        (want, st), g = oracle_run, None
    P = h.P
    nrows = P if rows is None else len(rows)
    assert len(out) == 3 and all(o.shape[0] == nrows for o in out), ([tuple(o.shape) for o in out], nrows)
    lerr = [rel_err(a, b.reshape(a.shape)) for a, b in zip(out, want)]
    errs = stage_errs(h, st, P, rows)
    gerr = [rel_err(a, g[k]) for a, k in zip(out, LOGITS)] if g is not None else []
    sig, gsig = [], []
    if nrows >= 2:
        sig = [signal_err(a, b.reshape(a.shape)) for a, b in zip(out, want)]
        gsig = [signal_err(a, g[k]) for a, k in zip(out, LOGITS)] if g is not None else []
    m5a = None
    if g is not None and "full_motion_5a" in g.files:
        m5a = rel_err(h.region("fusion_7", 832).view(P, 7, 7, 832).permute(0, 3, 1, 2)[:, :160], g["full_motion_5a"])
    fmt = lambda v: " ".join("%.1e" % x for x in v) or "-"
    print("%s: logits vs oracle %s, vs golden %s; stages %s; signal vs oracle %s, vs golden %s; full_motion_5a %s"
          % (what, fmt(lerr), fmt(gerr), " ".join("%s %.1e" % kv for kv in errs.items()), fmt(sig), fmt(gsig),
             "-" if m5a is None else "%.1e" % m5a))
    assert max(lerr + gerr) < RTOL, "%s: logits vs oracle %s, vs golden %s" % (what, lerr, gerr)
    assert max(errs.values()) < RTOL, "%s: stage tensors %s" % (what, errs)
    assert max(sig + gsig + [0.0]) < RTOL_NORTH_STAR, "%s: row-to-row signal vs oracle %s, vs golden %s" % (what, sig, gsig)
    assert m5a is None or m5a < RTOL, "%s: full_motion_5a %.2e" % (what, m5a)
    return errs


def check_sobel_tdiff(h, w, B, L, site, variant, algo):
    name, _C, H = spec.SITES[site]
    g = torch.Generator().manual_seed(site + 10 * variant)
    G = torch.relu(torch.randn(B * L, 128, H, H, generator=g))
    D = torch.randn(B * (L - 1), 32, H, H, generator=g)
    t_ref = orc.temporal_diff(G, B)
    if variant == spec.VARIANT_RGB:
        s_ref = F.conv2d(D, w["motion_spatial_grad_%s.weight" % name], w["motion_spatial_grad_%s.bias" % name],
                         padding=1, groups=32)
    else:
        s_ref = F.conv2d(D, w[spec.SOBEL_KEY], None, padding=1, groups=32)
    M = torch.full((B * (L - 1) * H * H, 352), -3.0, device="cuda")
    h.sobel_tdiff(site, nhwc(G).view(-1, 128), nhwc(D).view(-1, 32), M, 160, algo)
    Mv = M.view(B * (L - 1), H, H, 352).permute(0, 3, 1, 2)
    es, et = rel_err(Mv[:, 160:192], s_ref), rel_err(Mv[:, 192:320], t_ref)
    assert es < RTOL, "site %s: S %.2e" % (name, es)
    assert et < 1e-6, "site %s: T %.2e" % (name, et)          # a single fp32 subtraction: exact
    assert torch.all(Mv[:, :160] == -3.0) and torch.all(Mv[:, 320:] == -3.0), "site %s: channels outside the unit's 160 written" % name


def chain_inputs(case, n, kind, seed):
    """Inputs of a bottleneck chain of fusion@28 (offk_bottleneck_chain14 / _split): x, the three convs and the branch conv of block 28a."""
    g = torch.Generator().manual_seed(seed)
    branch = case == "28a_branch"
    Cin = 64 if branch else 256
    x = torch.randn(n, 14, 14, Cin + (64 if branch else 0), generator=g) * (1.0 if branch else 0.5)
    if kind == "heavy_tail":
        x = x * torch.exp(1.5 * torch.randn(n, 14, 14, 1, generator=g))
    if not branch:
        x = x.clamp_min(0)                               # sa / sb are post-ReLU
    k1 = 1.0 / Cin ** 0.5
    w1 = (torch.rand(64, Cin, generator=g) * 2 - 1) * k1
    b1 = (torch.rand(64, generator=g) * 2 - 1) * k1
    w2 = (torch.rand(64, 64, 3, 3, generator=g) * 2 - 1) / 24.0
    b2 = (torch.rand(64, generator=g) * 2 - 1) / 24.0
    w3 = (torch.rand(256, 64, generator=g) * 2 - 1) / 8.0
    b3 = (torch.rand(256, generator=g) * 2 - 1) / 8.0
    wb = (torch.rand(256, 64, generator=g) * 2 - 1) / 8.0
    bb = (torch.rand(256, generator=g) * 2 - 1) / 8.0
    return x.float().contiguous(), w1, b1, w2, b2, w3, b3, wb, bb


class StubBackbone(torch.nn.Module):
    """Stands for the TSN backbone (out of scope, RGB_OFF.py:362-594): hands back the nine tap maps, the per-frame
    Feature_Generation_Score the golden captured from the reference's own backbone and, for RGB_OFF_v2, conv2."""

    def __init__(self, feats, fgs, conv2=None):
        super().__init__()
        self.feats, self.fgs, self.conv2 = feats, fgs, conv2

    def forward(self, frames):
        assert frames.shape[0] == self.fgs.shape[0], (frames.shape, self.fgs.shape)
        return (self.feats, self.fgs) if self.conv2 is None else (self.feats, self.fgs, self.conv2)


# ---- the path tables: a new forward path is a row here ----
# test_gpu_heads: switches, launches that must be there, launches that must not
HEAD_PATHS = {
    "default": ({}, (POOL_ROWS_28, FC_FOLDED, "motion_conv3_trans_14b [winograd: output transform]"), ("(pool + fc)",)),
    "winograd0": ({"OFFK_WINOGRAD": "0"}, (POOL_ROWS_28, FC_FOLDED), ("(pool + fc)", WINO)),
    "fold_pool0": ({"OFFK_FOLD_POOL": "0"}, POOL_FC, ("heads (fc on folded", "(max pool rows)")),
}
# test_gpu_bounds: switches
BOUNDS_PATHS = {"default": {}, "unfused_units": {"OFFK_FUSED_UNITS": "0"}, "direct_convs": {"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0"},
                "separate_pools": {"OFFK_FOLD_POOL": "0"}, "gates_open": FORCE}

# test_gpu_switches / test_gpu_forward_plan.  shapes: a golden tag or (variant, B, L, feature config)
P18, P18_FLOW, P4 = "rgb_b3_l7", "flow_b3_l7", "rgb_b2_l3"
P42 = (spec.VARIANT_RGB, 7, 7, 2)
P72 = (spec.VARIANT_RGB, 12, 7, 2)
# id -> (switches, shape, arithmetic modes, launches that must be there, launches that must not,
#        launches the DEFAULT handle of the same shape must show (None: not compared), region that must differ bitwise from the default handle's)
FP32, SPLIT, BOTH = ("fp32",), ("f32split",), tuple(HANDLE_PRECISIONS)
NO_WINO_CHAIN = {"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0"}


def winograd0(shape):
    """OFFK_WINOGRAD=0, per arithmetic mode: fp32 handles sit below their chain gate (72 pairs); split-fp32 handles keep theirs at the first
    pair and, with no plane images packed for chain_split.hip, run chain_fused.hip's direct 3x3 form (OFFK_WINOGRAD row)."""
    return ({"OFFK_WINOGRAD": "0"}, shape, BOTH, {"fp32": (FC_FOLDED,), "f32split": (FC_FOLDED,) + CHAINS},
            {"fp32": (WINO, "head_14 (pool + fc)", "chain_28"), "f32split": (WINO, "head_14 (pool + fc)")}, None, None)


SWITCH_CASES = {
    # direct implicit GEMMs everywhere, the 14-head's pool in conv_igemm's epilogue + fc_pooled in slab mode (winograd0 above)
    "winograd0": winograd0(P18), "winograd0-flow": winograd0(P18_FLOW), "winograd0-p4": winograd0(P4),
    # the documented pin of INTEGRATION.md section 7
    "winograd0-chain0-p18": (NO_WINO_CHAIN, P18, BOTH, ("motion_conv2_trans_28a",), (WINO, "chain_28"), None, None),
    "winograd0-chain0-p72": (NO_WINO_CHAIN, P72, BOTH, ("motion_conv2_trans_28a",), (WINO, "chain_28"), None, None),
    # pool_kernel + fc_kernel for all three heads
    "fold_pool0": ({"OFFK_FOLD_POOL": "0"}, P18, BOTH, POOL_FC, ("heads (fc on folded", POOL_ROWS_28), (FC_FOLDED, POOL_ROWS_28), None),
    "fold_pool0-winograd0": ({"OFFK_FOLD_POOL": "0", "OFFK_WINOGRAD": "0"}, P18, BOTH, POOL_FC, ("heads (fc on folded", POOL_ROWS_28, WINO), None, None),
    "chain0-p72": ({"OFFK_CHAIN": "0"}, P72, BOTH, ("motion_conv2_trans_28a", WINO), ("chain_28",), CHAINS, None),
    "winograd_5x5_0": ({"OFFK_WINOGRAD_5X5": "0"}, P42, BOTH, (W7, "motion_conv2_trans_14a [winograd", "motion_conv_trans [winograd"), (W5,), (W5, W7), None),
    "winograd_7x7_0": ({"OFFK_WINOGRAD_7X7": "0"}, P42, BOTH, (W5, "motion_conv2_trans_14a [winograd", "motion_conv_trans [winograd"), (W7,), (W5, W7), None),
    # split-fp32 handles: the chain gate back at 72 pairs; chain_fused.hip in place of chain_split.hip; wino_mid's 1x1 convs on the fp32 pipe
    "split_chain0": ({"OFFK_SPLIT_CHAIN": "0"}, P18, SPLIT, ("motion_conv2_trans_28a",), ("chain_28",), CHAINS, None),
    "chain2-split_chain0": ({"OFFK_CHAIN": "2", "OFFK_SPLIT_CHAIN": "0"}, P18, SPLIT, CHAINS, (), CHAINS, ("sa_28", 256)),
    "split_mid0": ({"OFFK_SPLIT_MID": "0"}, P18, SPLIT, (BETWEEN,), (), (BETWEEN,), ("xv_7", 512)),
    # switches other modules already turn, without saying which path ran: K1 + K2 apart; the Winograd GEMMs and the 1x1 convs on 7x7 maps
    # of a split-fp32 handle on the fp32 pipe.  (OFFK_WINO_GEMM=0 leaves the same launch names AND the same bits --
    # test_wino_gemm_persistent_matches_generic -- so nothing a test can read tells its two kernels apart.)
    "fused_units0": ({"OFFK_FUSED_UNITS": "0"}, P18, BOTH, ("units:pw_reduce (K1)", "units:sobel_tdiff (K2)"), ("units:pw_tdiff",), ("units:pw_tdiff (K1T)",), None),
    "split_gemm0": ({"OFFK_SPLIT_GEMM": "0"}, P18, SPLIT, (WINO,), (), (WINO,), ("sum_7", 1024)),
}

# ---- the heads' own weights ----
HEAD_CH = {"7": 1024, "14": 512, "28": 256}
HEAD_KEY = {"7": "fc_action_motion", "14": "fc_action_motion_14", "28": "fc_action_motion_28"}
_HEAD_WEIGHTS = {}


def head_weights(ncls):
    """synth's weights with the three FCs replaced: N(0, 1) / sqrt(C), biases N(0, 0.1) -- and `ncls` classes."""
    if ncls not in _HEAD_WEIGHTS:
        w = dict(synth.make_weights(spec.VARIANT_RGB))
        g = np.random.default_rng(4100 + ncls)
        for k, C in HEAD_CH.items():
            w[HEAD_KEY[k] + ".weight"] = (g.standard_normal((ncls, C)) / C ** 0.5).astype(np.float32)
            w[HEAD_KEY[k] + ".bias"] = (g.standard_normal(ncls) * 0.1).astype(np.float32)
        _HEAD_WEIGHTS[ncls] = w
    return _HEAD_WEIGHTS[ncls]


def head_handle(rt, env, B, L, prec, ncls=spec.NUM_CLASSES, consensus=False):
    """-> (RGB handle holding head_weights(ncls), those weights as numpy arrays)"""
    w = head_weights(ncls)
    h, _ = make_handle(rt, B, L, spec.VARIANT_RGB, consensus=consensus, weights=w, precision=prec, env=env, num_classes=ncls)
    return h, w
