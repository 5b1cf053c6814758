"""What the forward family's helper modules (tests/forward.py, tests/wino_ref.py) promise, checked on the CPU -- nothing here has a device in
it: the import graph of tests/ and tools/ (no module imports a test module; one `rt` fixture), rel_err / signal_err on written-out
tensors, the folded point numbering against its two earlier spellings, between_reference against a direct conv2d form, check_trace,
shape_of, the handle maker against a stub runtime, and the values of every constant the GPU files now take from tests/forward.py."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import offk_amd  # noqa: F401
from offk_amd import spec, synth

from . import forward as fw
from . import wino_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the import graph ----
def python_files():
    out = []
    for top in ("tests", "tools"):
        for d, _dirs, files in os.walk(os.path.join(ROOT, top)):
            out += [os.path.join(d, f) for f in files if f.endswith(".py")]
    return sorted(out)


def imported_modules(tree):
    """every dotted module name an import statement of the tree names: `import a.b`, `from a import b` (a and a.b), `from . import b`"""
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                yield a.name
        elif isinstance(node, ast.ImportFrom):
            if node.module:
                yield node.module
            for a in node.names:
                yield (node.module + "." if node.module else "") + a.name


def test_no_module_imports_a_test_module():
    files = python_files()
    assert len(files) > 100 and any(f.endswith(os.path.join("tools", "record_forward_plans.py")) for f in files)
    bad = []
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        bad += ["%s: %s" % (os.path.relpath(path, ROOT), m) for m in imported_modules(tree) if m.rsplit(".", 1)[-1].startswith("test_")]
    assert not bad, bad


def test_the_rt_fixture_is_defined_once():
    where = []
    for path in python_files():
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.FunctionDef) and node.name == "rt" and any("fixture" in ast.dump(d) for d in node.decorator_list):
                where.append(os.path.relpath(path, ROOT))
    assert where == [os.path.join("tests", "featmaps.py")], where


# ---- rel_err, signal_err ----
def test_rel_err_and_signal_err_on_written_out_tensors():
    a = torch.tensor([[1.0, 2.0], [3.0, 5.0]])
    b = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    assert fw.rel_err(a, b) == pytest.approx(0.25)                     # max |a - b| = 1 over max |b| = 4
    assert fw.rel_err(a.numpy(), b) == pytest.approx(0.25) and fw.rel_err(b, b) == 0.0
    with pytest.raises(AssertionError):
        fw.rel_err(a, b[:1])
    # the signal: b's rows differ from their mean by +-1 in both classes, a's by (+-1, +-1.5): error 0.5 of a signal of 1
    assert fw.signal_err(a, b) == pytest.approx(0.5)
    # blind to a per-class offset, which rel_err is not
    off = b + torch.tensor([[100.0, -7.0]])
    assert fw.signal_err(off, b) == pytest.approx(0.0, abs=1e-12) and fw.rel_err(off, b) > 1.0
    with pytest.raises(AssertionError):
        fw.signal_err(a[:1], b[:1])                                     # a single row has no row-to-row signal
    with pytest.raises(AssertionError):
        fw.signal_err(a, b[:, :1])


# ---- the point numbering: the two spellings wino_ref.mindex replaced ----
def mindex_of_test_gpu_paths(phases, cy, cx, i, j):
    ny, nx, cls = (5 if cy else 6), (5 if cx else 6), 2 * cy + cx
    if phases == 1:
        return (0, 36, 66, 96)[cls] + i * nx + j
    offa, offb, offc = (0, 25, 45, 65), (0, 5, 9, 14), (0, 5, 10, 14)
    if i < ny - 1 and j < nx - 1:
        return offa[cls] + i * (nx - 1) + j
    if i == ny - 1 and j < nx - 1:
        return 81 + offb[cls] + j
    if j == nx - 1 and i < ny - 1:
        return 99 + offc[cls] + i
    return 117 + cls


OLD_OFFSETS = {"off1": (0, 36, 66, 96), "offA": (0, 25, 45, 65), "offB": (0, 5, 9, 14), "offC": (0, 5, 10, 14)}


def mindex_of_exact_wino(phases, cy, cx, i, j, offs=OLD_OFFSETS):
    ny, nx, cls = (5 if cy else 6), (5 if cx else 6), 2 * cy + cx
    if phases == 1:
        return offs["off1"][cls] + i * nx + j
    if i < ny - 1 and j < nx - 1:
        return offs["offA"][cls] + i * (nx - 1) + j
    if i == ny - 1 and j < nx - 1:
        return 81 + offs["offB"][cls] + j
    if j == nx - 1 and i < ny - 1:
        return 99 + offs["offC"][cls] + i
    return 117 + cls


def test_mindex_equals_both_earlier_spellings():
    from . import exact_fusion, exact_wino
    assert exact_wino.mindex is wino_ref.mindex and exact_fusion._mindex is wino_ref.mindex
    assert wino_ref.OFFSETS == OLD_OFFSETS
    shifted = dict(OLD_OFFSETS, offA=(0, 25, 46, 65))                   # (the mutation tests/test_exact_wino_inputs.py passes in)
    for phases in (1, 4):
        seen = set()
        for cy in (0, 1):
            for cx in (0, 1):
                for i in range(5 if cy else 6):
                    for j in range(5 if cx else 6):
                        m = wino_ref.mindex(phases, cy, cx, i, j)
                        assert m == mindex_of_test_gpu_paths(phases, cy, cx, i, j) == mindex_of_exact_wino(phases, cy, cx, i, j), (phases, cy, cx, i, j)
                        assert wino_ref.mindex(phases, cy, cx, i, j, shifted) == mindex_of_exact_wino(phases, cy, cx, i, j, shifted)
                        seen.add(m)
        assert seen == set(range(121)), phases


@pytest.mark.parametrize("phases", [1, 4])
def test_between_reference_agrees_with_a_direct_form(phases):
    """n = 2, cin = 64.  M is MADE from a known 7x7 map y: per class M = E y E^T with E a right inverse of A^T (its pseudo-inverse: A^T has
    full row rank), so A^T M A = y by construction.  Then x must be relu(y + bias), and V the B^T . B transform, written out tap by tap, of
    every overlapping window of relu(conv2d 1x1 (x)) zero-padded by one.  What is independent here is relu(y + bias), the 1x1 conv2d and the
    placement of classes, windows and points; M and the expected V are built from wino_ref's own AT / BT / mindex, so a wrong transform matrix
    would pass -- the matrices are held to exact fractions by tests/test_exact_wino_inputs.py, the numbering by the test above."""
    n, cin = 2, 64
    g = np.random.default_rng(5 + phases)
    y = g.standard_normal((n, 7, 7, cin))

    def evaluate(npts):
        e = np.linalg.pinv(wino_ref.AT[npts - 2])                          # [npts, outs]
        assert np.allclose(wino_ref.AT[npts - 2] @ e, np.eye(npts - 2), atol=1e-12)
        return e

    M = np.zeros((121, n, cin))
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = (5 if cy else 6), (5 if cx else 6)
            oy, ox = (4 if cy else 0), (4 if cx else 0)
            m = np.einsum("po,nouc,qu->pqnc", evaluate(ny), y[:, oy:oy + ny - 2, ox:ox + nx - 2], evaluate(nx))
            for i in range(ny):
                for j in range(nx):
                    M[wino_ref.mindex(phases, cy, cx, i, j)] = m[i, j]
    bias = g.standard_normal(cin) * 0.5
    w1, b1 = g.standard_normal((cin, cin)) / 8.0, g.standard_normal(cin) * 0.1
    x, V = wino_ref.between_reference(M, bias, phases, w1, b1)
    x_want = np.maximum(y + bias, 0.0)
    assert np.abs(x - x_want).max() < 1e-11 * np.abs(x_want).max()
    t = F.relu(F.conv2d(torch.from_numpy(x_want).permute(0, 3, 1, 2), torch.from_numpy(w1)[:, :, None, None], torch.from_numpy(b1)))
    tp = F.pad(t, (1, 1, 1, 1)).permute(0, 2, 3, 1).numpy()                # [n, 9, 9, c]
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = (5 if cy else 6), (5 if cx else 6)
            oy, ox = (4 if cy else 0), (4 if cx else 0)
            for i in range(ny):
                for j in range(nx):
                    want = sum(wino_ref.BT[ny][i, a] * wino_ref.BT[nx][j, b] * tp[:, oy + a, ox + b] for a in range(ny) for b in range(nx))
                    assert np.abs(V[wino_ref.mindex(1, cy, cx, i, j)] - want).max() < 1e-12 * max(1.0, np.abs(want).max()), (cy, cx, i, j)
    # without the 1x1 conv the second transform takes x itself
    x2, V2 = wino_ref.between_reference(M, bias, phases, None, None)
    assert np.array_equal(x2, x)
    assert np.allclose(V2[wino_ref.mindex(1, 0, 0, 0, 0)], sum(wino_ref.BT[6][0, a] * wino_ref.BT[6][0, b] * np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))[:, a, b]
                                                                for a in range(6) for b in range(6)))


# ---- check_trace, shape_of ----
def test_check_trace_passes_and_fails_as_its_arguments_say():
    names = ["units:pw_tdiff (K1T)", "motion_conv_trans_28 [winograd: input transform]", "chain_28a", fw.FC_FOLDED]
    assert fw.has(names, fw.WINO) and fw.has(names, "K1T") and not fw.has(names, "pool + fc")
    fw.check_trace(names, (fw.W7, "chain_28a", fw.FC_FOLDED), (fw.W5, "(pool + fc)"))
    fw.check_trace(names, (), ())
    with pytest.raises(AssertionError, match="no launch named"):
        fw.check_trace(names, (fw.W5,), ())
    with pytest.raises(AssertionError, match="a launch named"):
        fw.check_trace(names, (), ("chain_28",))


def test_shape_of_a_golden_tag_and_of_a_tuple(golden_dir):
    variant, B, L, cfg, g = fw.shape_of("rgb_b3_l7")
    assert (variant, B, L) == (spec.VARIANT_RGB, 3, 7) and cfg == int(g["meta"][3])
    assert g["fc7"].shape == (18, 101) and "full_motion_5a" in fw.shape_of("rgb_b2_l3", golden_dir)[4].files
    assert fw.shape_of("flow_b1_l7")[:3] == (spec.VARIANT_FLOW, 1, 7)
    assert fw.shape_of((spec.VARIANT_RGB, 12, 7, 2)) == (spec.VARIANT_RGB, 12, 7, 2, None)
    assert fw.GOLDEN_DIR == golden_dir
    for tag in fw.GOLDEN + fw.RET_GOLDEN:
        assert os.path.exists(os.path.join(golden_dir, tag + ".npz")), tag


# ---- the handle maker ----
class StubRuntime:
    """A runtime whose OffForward records os.environ and its arguments at construction."""

    def __init__(self, left_over=(), missing=0, fail=False):
        stub = self
        stub.seen, stub.args, stub.loaded = [], [], []

        class OffForward:
            def __init__(self, *args, **kw):
                stub.seen.append(dict(os.environ))
                stub.args.append((args, kw))
                if fail:
                    raise RuntimeError("offk_create failed")

            def load_state_dict(self, w):
                stub.seen.append(dict(os.environ))
                stub.loaded.append(w)
                return list(left_over)

            def missing_weights(self):
                return missing, "fc_action_motion.bias" if missing else ""

        self.OffForward = OffForward


def test_make_handle_sets_the_switches_around_construction_only(monkeypatch):
    monkeypatch.setenv("OFFK_CHAIN", "1")                                # a value of the caller's own comes back
    monkeypatch.delenv("OFFK_WINOGRAD", raising=False)
    env = {"OFFK_CHAIN": "0", "OFFK_WINOGRAD": "0"}
    w = {"fc_action_motion.bias": np.zeros(101, dtype=np.float32)}
    rt = StubRuntime()
    h, tw = fw.make_handle(rt, 2, 3, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP, False, w, "f32split", env=env, num_classes=51, feat_layout=1)
    at_create, at_load = rt.seen
    assert at_create["OFFK_CHAIN"] == "0" and at_create["OFFK_WINOGRAD"] == "0"
    assert at_load["OFFK_CHAIN"] == "1" and "OFFK_WINOGRAD" not in at_load
    assert os.environ["OFFK_CHAIN"] == "1" and "OFFK_WINOGRAD" not in os.environ
    assert rt.args == [((2, 3, spec.VARIANT_FLOW, spec.SLICE_PER_CLIP, False), dict(num_classes=51, precision="f32split", feat_layout=1))]
    assert isinstance(h, rt.OffForward) and rt.loaded == [w]
    assert sorted(tw) == sorted(w) and torch.is_tensor(tw["fc_action_motion.bias"])
    # no switches, default weights: synth's for the variant
    rt = StubRuntime()
    _h, tw = fw.make_handle(rt, 1, 2, spec.VARIANT_RGB)
    assert rt.args == [((1, 2, spec.VARIANT_RGB, spec.SLICE_FLAT, None), dict(num_classes=spec.NUM_CLASSES, precision="fp32"))]
    assert sorted(tw) == sorted(spec.weight_shapes(spec.VARIANT_RGB))
    assert np.array_equal(rt.loaded[0]["fc_action_motion.bias"], synth.make_weights(spec.VARIANT_RGB)["fc_action_motion.bias"])


def test_make_handle_unsets_the_switches_when_construction_raises(monkeypatch):
    monkeypatch.delenv("OFFK_FOLD_POOL", raising=False)
    rt = StubRuntime(fail=True)
    with pytest.raises(RuntimeError, match="offk_create failed"):
        fw.make_handle(rt, 1, 2, spec.VARIANT_RGB, env={"OFFK_FOLD_POOL": "0"})
    assert rt.seen[0]["OFFK_FOLD_POOL"] == "0" and "OFFK_FOLD_POOL" not in os.environ


def test_make_handle_fails_on_left_over_keys_and_on_a_missing_weight():
    with pytest.raises(AssertionError, match="load_state_dict left keys over"):
        fw.make_handle(StubRuntime(left_over=["conv1_7x7_s2.weight"]), 1, 2, spec.VARIANT_RGB)
    with pytest.raises(AssertionError, match="1 weight.s. not set: fc_action_motion.bias"):
        fw.make_handle(StubRuntime(missing=1), 1, 2, spec.VARIANT_RGB)
    with pytest.raises(AssertionError):
        fw.head_handle(StubRuntime(missing=2), {}, 1, 2, "fp32")
    rt = StubRuntime()
    _h, w = fw.head_handle(rt, {"OFFK_FOLD_POOL": "0"}, 3, 7, "f32split", ncls=51, consensus=True)
    assert rt.seen[0]["OFFK_FOLD_POOL"] == "0" and "OFFK_FOLD_POOL" not in os.environ
    assert rt.args[0][1]["num_classes"] == 51 and w["fc_action_motion_14.weight"].shape == (51, 512) and rt.loaded == [w]


# ---- the constants, written out ----
def test_the_moved_constants_keep_their_values():
    assert (fw.RTOL, fw.RTOL_NORTH_STAR) == (2e-4, 1e-3)
    assert fw.PRECISIONS == ["fp32"] and fw.HANDLE_PRECISIONS == ["fp32", "f32split"]
    assert fw.GOLDEN == ["rgb_b1_l7", "rgb_b2_l3", "rgb_b3_l7", "flow_b1_l7", "flow_b2_l3", "flow_b3_l7", "rgbv2_b2_l3"]
    assert fw.RET_GOLDEN == ["ret_rgb_b2_l3", "ret_rgb_b1_l2", "ret_flow_b2_l3", "ret_flow_b1_l2", "ret_rgbv2_b2_l3"]
    assert fw.CONV_CASES == [(320, 64, 7, 2, 3, 28, 2), (64, 64, 1, 1, 0, 14, 3), (64, 64, 3, 1, 1, 14, 2), (64, 256, 1, 1, 0, 14, 2),
                             (256, 64, 1, 1, 0, 14, 2), (1056, 128, 5, 2, 2, 14, 2), (128, 128, 3, 1, 1, 7, 5), (128, 512, 1, 1, 0, 7, 3),
                             (512, 128, 1, 1, 0, 7, 3), (128, 512, 3, 1, 1, 7, 3), (832, 256, 3, 1, 1, 7, 2), (256, 1024, 1, 1, 0, 7, 3)]
    assert fw.PATCH_CASES == [(7, 2, 28, 320, 64, 3, 7, 1), (7, 2, 28, 64, 128, 2, 6, 2), (5, 2, 14, 1056, 128, 6, 6, 3), (5, 2, 14, 96, 64, 9, 7, 1),
                              (3, 1, 14, 64, 64, 3, 7, 2), (3, 1, 14, 128, 256, 2, 6, 1), (3, 1, 7, 832, 256, 7, 6, 4), (3, 1, 7, 128, 128, 5, 7, 1),
                              (3, 1, 7, 256, 256, 8, 6, 3)]
    assert fw.STAGES == (("fusion_28", 320, 28), ("fusion_14", 1056, 14), ("fusion_7", 832, 7), ("sum_7", 1024, 7))
    assert fw.FORCE == {"OFFK_CHAIN": "2", "OFFK_WINOGRAD_5X5": "2", "OFFK_WINOGRAD_7X7": "2"}
    assert (fw.WINO, fw.CHAINS) == ("[winograd", ("chain_28a", "chain_28b", "chain_28c"))
    assert (fw.FC_FOLDED, fw.POOL_ROWS_28) == ("heads (fc on folded pools, one launch)", "head_28 (max pool rows)")
    assert fw.POOL_FC == ("head_7 (pool + fc)", "head_14 (pool + fc)", "head_28 (pool + fc)")
    assert (fw.W5, fw.W7, fw.BETWEEN) == ("motion_conv_trans_14 [winograd", "motion_conv_trans_28 [winograd", "[winograd: between]")
    assert fw.HEAD_PATHS == {
        "default": ({}, ("head_28 (max pool rows)", "heads (fc on folded pools, one launch)", "motion_conv3_trans_14b [winograd: output transform]"),
                    ("(pool + fc)",)),
        "winograd0": ({"OFFK_WINOGRAD": "0"}, ("head_28 (max pool rows)", "heads (fc on folded pools, one launch)"), ("(pool + fc)", "[winograd")),
        "fold_pool0": ({"OFFK_FOLD_POOL": "0"}, ("head_7 (pool + fc)", "head_14 (pool + fc)", "head_28 (pool + fc)"),
                       ("heads (fc on folded", "(max pool rows)")),
    }
    # ("gates_open" was None beside a call of forced_handle: the same three switches)
    assert fw.BOUNDS_PATHS == {"default": {}, "unfused_units": {"OFFK_FUSED_UNITS": "0"}, "direct_convs": {"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0"},
                               "separate_pools": {"OFFK_FOLD_POOL": "0"},
                               "gates_open": {"OFFK_CHAIN": "2", "OFFK_WINOGRAD_5X5": "2", "OFFK_WINOGRAD_7X7": "2"}}
    assert (fw.HEAD_CH, fw.HEAD_KEY) == ({"7": 1024, "14": 512, "28": 256},
                                         {"7": "fc_action_motion", "14": "fc_action_motion_14", "28": "fc_action_motion_28"})


def test_the_switch_cases_keep_their_values():
    rgb = spec.VARIANT_RGB
    both, split = ("fp32", "f32split"), ("f32split",)
    chains = ("chain_28a", "chain_28b", "chain_28c")
    pool_fc = ("head_7 (pool + fc)", "head_14 (pool + fc)", "head_28 (pool + fc)")
    fc_folded, rows28 = "heads (fc on folded pools, one launch)", "head_28 (max pool rows)"
    w5, w7 = "motion_conv_trans_14 [winograd", "motion_conv_trans_28 [winograd"

    def winograd0(shape):
        return ({"OFFK_WINOGRAD": "0"}, shape, both, {"fp32": (fc_folded,), "f32split": (fc_folded,) + chains},
                {"fp32": ("[winograd", "head_14 (pool + fc)", "chain_28"), "f32split": ("[winograd", "head_14 (pool + fc)")}, None, None)

    assert fw.SWITCH_CASES == {
        "winograd0": winograd0("rgb_b3_l7"), "winograd0-flow": winograd0("flow_b3_l7"), "winograd0-p4": winograd0("rgb_b2_l3"),
        "winograd0-chain0-p18": ({"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0"}, "rgb_b3_l7", both, ("motion_conv2_trans_28a",), ("[winograd", "chain_28"), None, None),
        "winograd0-chain0-p72": ({"OFFK_WINOGRAD": "0", "OFFK_CHAIN": "0"}, (rgb, 12, 7, 2), both, ("motion_conv2_trans_28a",), ("[winograd", "chain_28"), None, None),
        "fold_pool0": ({"OFFK_FOLD_POOL": "0"}, "rgb_b3_l7", both, pool_fc, ("heads (fc on folded", rows28), (fc_folded, rows28), None),
        "fold_pool0-winograd0": ({"OFFK_FOLD_POOL": "0", "OFFK_WINOGRAD": "0"}, "rgb_b3_l7", both, pool_fc, ("heads (fc on folded", rows28, "[winograd"), None, None),
        "chain0-p72": ({"OFFK_CHAIN": "0"}, (rgb, 12, 7, 2), both, ("motion_conv2_trans_28a", "[winograd"), ("chain_28",), chains, None),
        "winograd_5x5_0": ({"OFFK_WINOGRAD_5X5": "0"}, (rgb, 7, 7, 2), both, (w7, "motion_conv2_trans_14a [winograd", "motion_conv_trans [winograd"), (w5,), (w5, w7), None),
        "winograd_7x7_0": ({"OFFK_WINOGRAD_7X7": "0"}, (rgb, 7, 7, 2), both, (w5, "motion_conv2_trans_14a [winograd", "motion_conv_trans [winograd"), (w7,), (w5, w7), None),
        "split_chain0": ({"OFFK_SPLIT_CHAIN": "0"}, "rgb_b3_l7", split, ("motion_conv2_trans_28a",), ("chain_28",), chains, None),
        "chain2-split_chain0": ({"OFFK_CHAIN": "2", "OFFK_SPLIT_CHAIN": "0"}, "rgb_b3_l7", split, chains, (), chains, ("sa_28", 256)),
        "split_mid0": ({"OFFK_SPLIT_MID": "0"}, "rgb_b3_l7", split, ("[winograd: between]",), (), ("[winograd: between]",), ("xv_7", 512)),
        "fused_units0": ({"OFFK_FUSED_UNITS": "0"}, "rgb_b3_l7", both, ("units:pw_reduce (K1)", "units:sobel_tdiff (K2)"), ("units:pw_tdiff",), ("units:pw_tdiff (K1T)",), None),
        "split_gemm0": ({"OFFK_SPLIT_GEMM": "0"}, "rgb_b3_l7", split, ("[winograd",), (), ("[winograd",), ("sum_7", 1024)),
    }
    assert list(fw.SWITCH_CASES) == ["winograd0", "winograd0-flow", "winograd0-p4", "winograd0-chain0-p18", "winograd0-chain0-p72", "fold_pool0",
                                     "fold_pool0-winograd0", "chain0-p72", "winograd_5x5_0", "winograd_7x7_0", "split_chain0", "chain2-split_chain0",
                                     "split_mid0", "fused_units0", "split_gemm0"]
