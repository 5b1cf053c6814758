"""One weight key updated after a first forward, every key, every configuration: does every kernel that reads the weight see it?

A handle keeps a weight up to four times over, and three dirty flags (pw_dirty, merged_dirty, derived_dirty) decide when the copies
behind the plain one are made again.  The images, and where each is PACKED AND READ at B = 1, L = 3 (P = 2), by configuration
(CONFIGS below) and arithmetic mode of the handle -- "fp32", "split" (f32split) or "both":

  image (csrc/offk_api.hip)                                  packed and read in
  pw_wt16                                                     default, gates_open, direct_convs: fp32 (the fused units kernel)
  pw_wt16s                                                    default, gates_open, direct_convs, split_on_fp32_pipe: split
  (pw_w itself, by K1)                                        unfused_units: both
  merged_w / merged_b  merged_28a                             default, unfused_units: fp32; direct_convs: both (a conv of its own);
                                                              gates_open: fp32, split_on_fp32_pipe (c3's K inside chain_28a)
                       merged_14a, merged_7                   every configuration (gates_open: merged_7 through the composed head and,
                                                              for sum_7, offk_stage_tensors)
  kDerived, its 33 rows (7 u, 7 u_planes, 3 gemm_planes, 3 u2, 12 planes, 1 head):
  u         motion_conv3_trans_14b, motion_conv_trans,        default, unfused_units, gates_open, split_on_fp32_pipe: both
            motion_conv2_trans, motion_conv2_trans_14a,
            motion_conv2_trans_14b  (F(4x4, 3x3))
  u         motion_conv_trans_14  (polyphase 5x5)             gates_open, split_on_fp32_pipe: both
  u         motion_conv_trans_28  (polyphase 7x7)             gates_open, split_on_fp32_pipe: both
  u_planes  the same five 3x3 convs                           default, unfused_units, gates_open: split
  u_planes  motion_conv_trans_14, motion_conv_trans_28        gates_open: split
  gemm_planes  merged_14a, motion_conv1_trans_14b             default, unfused_units, gates_open: split
  gemm_planes  merged_7                                       default, unfused_units: split; gates_open: split (offk_stage_tensors)
  u2        motion_conv2_trans_28a / 28b / 28c                gates_open: fp32; split_on_fp32_pipe
  planes    conv1 / conv2 / conv3 of chains 28a, 28b, 28c     default, unfused_units, gates_open: split (split handles chain from the
            and motion_conv_branch_28a  (ten rows)            first pair)
  planes    motion_conv1_trans  (inside wino_mid)             default, unfused_units, gates_open: split
  planes    motion_conv1_trans_14a  (inside wino_mid, behind  gates_open: split
            the polyphase 5x5)
  head      merged_7 composed with fc_action_motion           gates_open, split_on_fp32_pipe: both
  (none of them: OFFK_WINOGRAD=0 allocates no derived image)  direct_convs: both

test_the_configurations_run_the_paths_the_table_names holds each configuration to the launch groups behind this table (the per-launch
trace), so a gate whose default moves makes that test fail instead of leaving a row of the table unread.  The trace names launch
groups, not kernels: that a split handle's GEMMs leave the bf16 pipe under split_on_fp32_pipe shows in the bits (asserted there too).

Protocol, per configuration, two handles `live` and `reload` that have both run a forward on the synth weights w0.  For every key k:
  1. live.set_weight(k, perturbed(k, w0[k])), forward; the three heads, fusion_28 / fusion_14 / fusion_7, D_<site> and sum_7 are read back;
  2. reload.load_state_dict(w1) -- every key set, every flag dirty: the path every other test trusts -- forward: equal bits everywhere;
  3. against live's w0 results exactly the heads of feeds(k) differ, the others are bit-equal;
  4. live.set_weight(k, w0[k]), forward: the bits of the first w0 forward again.
Once per group the key goes in under its "module." spelling, and at the end of a group a freshly created handle loaded with the last w1
must give reload's bits.  No assertion here is a tolerance.

Wall time of this module on an MI355X: 25.8 s on the first run (281 items then), 45.4 s for today's 285 on another machine of the pool; the
slowest item 0.5 s (the first, which loads the library).
"""
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import weight_updates as wu
from .arena import same_bits
from .featmaps import rt  # noqa: F401
from .forward import BETWEEN, CHAINS, FC_FOLDED, HANDLE_PRECISIONS, W5, W7, WINO, check_trace, dev, make_handle, traced_forward
from .weight_updates import CONFIGS, SPLIT, differing, feats, run

pytestmark = pytest.mark.gpu

SETUPS = [(c, p, v) for c, (_env, precs) in CONFIGS.items() for p in precs for v in wu.VARIANTS]


def setup_id(c, p, v):
    return "%s-%s-%s" % (c, p, wu.VARIANT_TAGS[v])


def new_handle(rt, config, prec, variant, weights):
    return make_handle(rt, wu.B, wu.L, variant, consensus=False, weights=weights, precision=prec, env=CONFIGS[config][0])[0]


class Setup:
    """live and reload of one (configuration, arithmetic mode, variant), both after one forward on w0."""

    def __init__(self, rt, config, prec, variant):
        self.config, self.prec, self.variant = config, prec, variant
        self.w0 = synth.make_weights(variant)
        self.live = new_handle(rt, config, prec, variant, self.w0)
        self.reload = new_handle(rt, config, prec, variant, self.w0)
        self.base = run(self.live)
        assert differing(run(self.reload), self.base) == []
        self.clean = True

    def ready(self):
        """Called first by every case: after a case that failed in mid-protocol both handles go back to w0 by the trusted path."""
        if not self.clean:
            for h in (self.live, self.reload):
                assert h.load_state_dict(self.w0) == []
                assert differing(run(h), self.base) == []
            self.clean = True
        return self


@pytest.fixture(scope="module")
def setup(request, rt):
    """One Setup per (configuration, arithmetic mode, variant), shared by the cases of that setup (module scope and parametrised
    indirectly, like `case` in tests/test_gpu_exact.py: pytest keeps the value while the parameter stays the same)."""
    return Setup(rt, *request.param)


def setup_params(with_groups=False):
    if with_groups:
        return [pytest.param((c, p, v), g, id="%s-%s" % (setup_id(c, p, v), g)) for c, p, v in SETUPS for g in wu.groups(v)]
    return [pytest.param((c, p, v), id=setup_id(c, p, v)) for c, p, v in SETUPS]


def update_and_check(s, pairs, spelling=lambda k: k):
    """Steps 1 - 4 for the keys of `pairs` (key -> new value), all set before the one forward.  Returns (w1, reload's results)."""
    w1 = dict(s.w0)
    w1.update(pairs)
    s.clean = False
    for k, v in pairs.items():
        s.live.set_weight(spelling(k), v)
    got = run(s.live)                                                                  # 1
    assert s.reload.load_state_dict(w1) == []
    want = run(s.reload)                                                               # 2
    assert differing(got, want) == [], sorted(pairs)
    moved = set(n for n in wu.HEAD_ORDER if not same_bits(got[n], s.base[n]))          # 3
    assert moved == set().union(*(wu.feeds(k) for k in pairs)), (sorted(pairs), sorted(moved))
    for k in pairs:
        s.live.set_weight(k, s.w0[k])
    assert differing(run(s.live), s.base) == [], sorted(pairs)                         # 4
    s.clean = True
    return w1, want


@pytest.mark.parametrize("setup,grp", setup_params(with_groups=True), indirect=["setup"])
def test_one_key_updated_after_a_forward(rt, setup, grp):
    s = setup.ready()
    group_keys = wu.keys_of(s.variant, grp)
    for i, k in enumerate(group_keys):
        spelling = (lambda key: "module." + key) if i == 0 else (lambda key: key)
        w1, want = update_and_check(s, {k: wu.perturbed(k, s.w0[k])}, spelling)
    # the full reload against a handle that has never held anything else
    fresh = new_handle(rt, s.config, s.prec, s.variant, w1)
    assert differing(run(fresh), want) == [], group_keys[-1]


def _shared_image_pairs():
    main, branch = wu.MERGED_PAIRS[0]
    main7, branch7 = wu.MERGED_PAIRS[2]
    return {"merged-weights-28a": (main + ".weight", branch + ".weight"), "merged-biases-28a": (main + ".bias", branch + ".bias"),
            "merged-weights-7": (main7 + ".weight", branch7 + ".weight"), "merged-biases-7": (main7 + ".bias", branch7 + ".bias"),
            "merged-biases-14a": (wu.MERGED_PAIRS[1][0] + ".bias", wu.MERGED_PAIRS[1][1] + ".bias"),
            "gen-down-3c": ("motion_conv_gen_3c.weight", "motion_spatial_down_3c.weight"),
            "gen-down-5b": ("motion_conv_gen_5b.weight", "motion_spatial_down_5b.weight")}


@pytest.mark.parametrize("setup", setup_params(), indirect=True)
def test_two_keys_that_share_an_image(rt, setup):
    """Main and branch weight of a merged conv, main and branch bias (merged_b is their SUM), gen and down weight of one site (one
    pw_wt16 image): both keys set before the one forward."""
    s = setup.ready()
    for _name, (ka, kb) in _shared_image_pairs().items():
        update_and_check(s, {ka: wu.perturbed(ka, s.w0[ka]), kb: wu.perturbed(kb, s.w0[kb])})


# ---- the launch groups behind the table of the module docstring ---------------------------------------------------------------------
K1T, SBLOCKS, K1, K2 = "units:pw_tdiff (K1T)", "units:sobel S-blocks (K2 spatial half)", "units:pw_reduce (K1)", "units:sobel_tdiff (K2)"
WINO3 = tuple(k + " [winograd: 121 GEMMs]" for k in ("motion_conv_trans", "motion_conv2_trans", "motion_conv2_trans_14a", "motion_conv2_trans_14b",
                                                     "motion_conv3_trans_14b"))
CHAIN_CONVS = tuple("motion_conv%d_trans_28%s" % (i, c) for c in "abc" for i in (1, 2, 3) if (i, c) != (3, "a"))      # (3, a): inside merged_28a
MERGED = ("merged_28a", "merged_14a", "merged_7")


def expected_launches(config, prec):
    """(launch groups that must be there, by exact name; ... that must not; substrings that must; ... that must not)"""
    fused = (K1T, SBLOCKS) if config != "unfused_units" else (K1, K2)
    not_fused = (K1, K2) if config != "unfused_units" else (K1T, SBLOCKS)
    if config == "direct_convs":
        convs = tuple(k for k, _co, _ci, _k, _s, _p in spec.FUSION_CONVS if k not in sum(wu.MERGED_PAIRS, ()))
        return fused + convs + MERGED, not_fused, (FC_FOLDED,), (WINO, "chain_28", "head_7 (pool + fc)")
    if config in ("gates_open", "split_on_fp32_pipe"):
        return (fused + WINO3 + ("merged_14a", "motion_conv1_trans_14b"),
                not_fused + CHAIN_CONVS + ("merged_28a", "merged_7", "motion_conv_trans_28", "motion_conv_trans_14"),
                (W5, W7, BETWEEN, FC_FOLDED) + CHAINS, ())
    chained = prec == SPLIT          # default, unfused_units: below every gate but the split handles' chain gate (the first pair)
    return (fused + WINO3 + ("motion_conv_trans_28", "motion_conv_trans_14", "merged_14a", "merged_7", "motion_conv1_trans_14b")
            + (() if chained else CHAIN_CONVS + ("merged_28a",)),
            not_fused + (CHAIN_CONVS + ("merged_28a",) if chained else ()),
            (BETWEEN, FC_FOLDED) + (CHAINS if chained else ()), (W5, W7) + (() if chained else ("chain_28",)))


@pytest.mark.parametrize("setup", setup_params(), indirect=True)
def test_the_configurations_run_the_paths_the_table_names(rt, setup):
    s = setup.ready()
    config, prec, variant = s.config, s.prec, s.variant
    names, _out = traced_forward(s.live, feats())
    exact, exact_not, sub, sub_not = expected_launches(config, prec)
    for n in exact:
        assert n in names, (n, names)
    for n in exact_not:
        assert n not in names, (n, names)
    check_trace(names, sub, sub_not)
    if config == "split_on_fp32_pipe":
        # same launch groups as gates_open, other kernels behind them: the Winograd GEMMs, the chains and wino_mid's 1x1 convs leave the
        # bits of the fp32 pipe, which are not those of the plane images
        other = new_handle(rt, "gates_open", prec, variant, s.w0)
        on_planes = run(other)
        for name in ("fusion_14", "fusion_7", "sum_7"):
            assert not same_bits(on_planes[name], s.base[name]), name


# ---- a captured forward and a later offk_set_weight -----------------------------------------------------------------------------------
def captured(h, arr, out):
    """A graph of one forward into `out`, by the rules of test_forward_is_stream_capturable (the warm-up off the default stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h.forward_into(arr, *out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h.forward_into(arr, *out)
    return g


def replayed(g, out):
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def eager(h):
    res = [o.clone() for o in h.forward(feats())]
    torch.cuda.synchronize()
    return res


def same(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
def test_graph_replay_sees_a_weight_update_after_one_eager_forward(rt, prec):
    """include/offk.h, offk_set_weight: the copies and the images are handle-owned and made again IN PLACE, by the first forward
    behind the update -- a captured forward holds no packing launch (it was captured clean), so it reads the new images once one
    eager forward has passed through the library, and the replay then gives that forward's bits."""
    variant, key = spec.VARIANT_RGB, "motion_conv_trans_14.weight"          # Winograd u (and u_planes) with the gates open
    w0 = synth.make_weights(variant)
    h = new_handle(rt, "gates_open", prec, variant, w0)
    out = [torch.empty(h.out_rows(), spec.NUM_CLASSES, device="cuda") for _ in range(3)]
    g = captured(h, h._feat_array(feats()), out)
    before = eager(h)
    assert same(replayed(g, out), before)
    h.set_weight(key, wu.perturbed(key, w0[key]))
    after = eager(h)
    got = replayed(g, out)
    assert same(got, after)
    moved = set(n for n, a, b in zip(wu.HEAD_ORDER, before, got) if not same_bits(a, b))
    assert moved == wu.feeds(key), sorted(moved)
    assert same(eager(new_handle(rt, "gates_open", prec, variant, wu.with_key(w0, key))), got)


def _dense_sobel(rt, prec):
    """A Flow handle on the four-tap kernel, and the dense weight set on it."""
    variant = spec.VARIANT_FLOW
    w0 = synth.make_weights(variant)
    h = new_handle(rt, "default", prec, variant, w0)
    return h, lambda: h.set_weight(spec.SOBEL_KEY, wu.perturbed(spec.SOBEL_KEY, w0[spec.SOBEL_KEY])), wu.with_key(w0, spec.SOBEL_KEY), []


def _set_on_bound_keys(rt, prec):
    """An RGB handle with a contraction weight and a depthwise bias bound in place, and offk_set_weight on both keys."""
    variant, keys = spec.VARIANT_RGB, ("motion_conv_gen_3a.weight", "motion_spatial_grad_3b.bias")      # (28x28 sites: all three heads)
    w0 = synth.make_weights(variant)
    h = new_handle(rt, "default", prec, variant, w0)
    bound = [dev(w0[k]).clone() for k in keys]
    for k, t in zip(keys, bound):
        h.bind_weight(k, t)
    w1 = dict(w0)
    w1.update((k, wu.perturbed(k, w0[k])) for k in keys)

    def update():
        for k in keys:
            h.set_weight(k, w1[k])
    return h, update, w1, bound


@pytest.mark.parametrize("prec", HANDLE_PRECISIONS)
@pytest.mark.parametrize("case", [_dense_sobel, _set_on_bound_keys], ids=["sobel-four-tap-to-dense", "set-replaces-a-binding"])
def test_graph_needs_a_recapture_when_an_update_changes_the_launches(rt, case, prec):
    """include/offk.h, offk_set_weight: two updates change the LAUNCHES, not only the values behind them, and launches are fixed at
    capture.  A Sobel weight that leaves (or enters) the four-tap form of util.py:61 selects another instantiation of K2 on the host,
    and offk_set_weight on a bound key takes the bound pointer (and, for a contraction weight, the register-staged units kernel) out
    of every later launch.  The graph captured before goes on running what it captured -- the four-tap kernel over the nine-tap
    weights, the old bound tensors -- whatever runs eagerly in between; a graph captured after the update gives the eager bits, which
    are those of a fresh handle that holds the new values."""
    h, update, w1, keep_alive = case(rt, prec)
    arr = h._feat_array(feats())
    out = [torch.empty(h.out_rows(), spec.NUM_CLASSES, device="cuda") for _ in range(3)]
    g0 = captured(h, arr, out)
    assert same(replayed(g0, out), eager(h))
    update()
    after = eager(h)
    assert same(eager(new_handle(rt, "default", prec, h.variant, w1)), after)
    assert not any(same_bits(a, b) for a, b in zip(replayed(g0, out), after))       # the documented limit: the old launches
    out1 = [torch.empty_like(o) for o in out]
    g1 = captured(h, arr, out1)
    assert same(replayed(g1, out1), after)
    del keep_alive
