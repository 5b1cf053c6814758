"""Where nine feature maps go: the routing rule of the Python wrapper (runtime.feat_route) over dtypes, layouts, malformed inputs, both
sides and every handle setting, against a literal table.  The table was taken from the three-way ladders the wrapper's methods spelled out
before there was one function (takes_channels_last / _cl_dtype / _feat16 on the inference side, train_takes_channels_last / _cl_dtype /
_train16 on the training side, called unbound on a stub); where the module has no feat_route the test walks those ladders itself, so the
table holds either way.  CPU tensors throughout: the rule looks at dtype, shape and strides only.  B = 1, L = 2."""
import types

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, runtime, spec

B, L = 1, 2
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
OTHER = {"f32": torch.float16, "bf16": torch.float32, "f16": torch.bfloat16}       # the second dtype of a mixed-dtype input
PRECISIONS = {"fp32": _lib.PRECISION_FP32, "split": _lib.PRECISION_F32SPLIT}
SETTINGS = [(side, prec, layout) for side in ("infer", "train") for prec in PRECISIONS for layout in (0, 1)]


def _maps(dtype, fmt=torch.contiguous_format, batch=B):
    return [torch.zeros(batch * L, C, H, H, dtype=dtype).contiguous(memory_format=fmt) for _, C, H in spec.SITES]


def _groups(maps, fmt):
    """Every map as two channel groups (multiples of 32), each a tensor of its own in `fmt`."""
    return [[t[:, :64].contiguous(memory_format=fmt), t[:, 64:].contiguous(memory_format=fmt)] for t in maps]


def _with(maps, i, t):
    out = list(maps)
    out[i] = t
    return out


CL = torch.channels_last
INPUTS = {
    "contiguous": lambda dt: _maps(dt),
    "cl": lambda dt: _maps(dt, CL),
    "groups_contiguous": lambda dt: _groups(_maps(dt), torch.contiguous_format),
    "groups_cl": lambda dt: _groups(_maps(dt), CL),
    "one_map_in_groups_cl": lambda dt: _with(_maps(dt, CL), 2, _groups(_maps(dt), CL)[2]),
    "last_cl_rest_contiguous": lambda dt: _maps(dt)[:8] + _maps(dt, CL)[8:],
    "first_contiguous_rest_cl": lambda dt: _maps(dt)[:1] + _maps(dt, CL)[1:],
    "groups_mixed_layouts": lambda dt: _with(_groups(_maps(dt), CL), 5, _groups(_maps(dt), torch.contiguous_format)[5]),
    "contiguous_mixed_dtypes": lambda dt: _with(_maps(dt), 6, _maps(OTHER[dt_name(dt)])[6]),
    "cl_mixed_dtypes": lambda dt: _with(_maps(dt, CL), 6, _maps(OTHER[dt_name(dt)], CL)[6]),
    "cl_fp64": lambda dt: _maps(torch.float64, CL),
    "contiguous_fp64": lambda dt: _maps(torch.float64),
    "contiguous_non_tensor": lambda dt: _with(_maps(dt), 2, np.zeros((2, 3), np.float32)),
    "cl_non_tensor": lambda dt: _with(_maps(dt, CL), 2, np.zeros((2, 3), np.float32)),
    "eight_contiguous": lambda dt: _maps(dt)[:8],
    "eight_cl": lambda dt: _maps(dt, CL)[:8],
    "cl_wrong_batch": lambda dt: _with(_maps(dt, CL), 3, _maps(dt, CL, batch=B + 1)[3]),
    "contiguous_wrong_batch": lambda dt: _with(_maps(dt), 3, _maps(dt, batch=B + 1)[3]),
    "cl_one_permuted": lambda dt: _with(_maps(dt, CL), 8, _maps(dt)[8].permute(0, 1, 3, 2)),
    "contiguous_one_permuted": lambda dt: _with(_maps(dt), 8, _maps(dt)[8].permute(0, 1, 3, 2)),
    "nhwc_shaped_contiguous": lambda dt: [t.permute(0, 2, 3, 1).contiguous() for t in _maps(dt)],
}


def dt_name(dtype):
    return [k for k, v in DTYPES.items() if v == dtype][0]


def ladder(feats, side, precision, layout):
    """(route, enum offk_feat_dtype, any map in channel groups) or "ValueError: <text>"."""
    try:
        if hasattr(runtime, "feat_route"):
            return tuple(runtime.feat_route(feats, B, L, layout, precision, side))
        h = types.SimpleNamespace(batch=B, length=L, precision=precision, feat_layout=layout)
        O = runtime.OffForward
        parts = any(not torch.is_tensor(f) for f in feats)
        if (O.takes_channels_last if side == "infer" else O.train_takes_channels_last)(h, feats):
            return ("cl", O._cl_dtype(h, feats), parts)
        fdt = (O._feat16 if side == "infer" else O._train16)(h, feats)
        return ("plain", _lib.FEAT_F32, parts) if fdt is None else ("typed", fdt, parts)
    except ValueError as e:
        return "ValueError: %s" % e


F32, BF16, F16 = _lib.FEAT_F32, _lib.FEAT_BF16, _lib.FEAT_F16
NEED_SPLIT_16 = 'ValueError: bf16 / fp16 feature maps need a split-fp32 handle (precision="f32split"); this one runs the fp32 pipe'
NEED_SPLIT_CL = ('ValueError: feature maps must be contiguous fp32 CUDA/HIP tensors on this handle (the fp32 pipe): channels_last maps need a '
                 'split-fp32 handle (precision="f32split")')
ONE_LAYOUT = "ValueError: feature maps must all have one layout (all contiguous or all torch.channels_last), got a mix"
NINE = "ValueError: need nine feature maps"

# EXPECTED[(input, dtype)] = outcome, or {(side, precision, handle layout): outcome} where the handle or the side matters; "*" stands for
# every value of that position, the first matching key in the order written counts
EXPECTED = {
    ('contiguous', 'f32'): ('plain', 0, False),
    ('contiguous', 'bf16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 1, False),
        ('train', '*', '*'): ('typed', 1, False)},
    ('contiguous', 'f16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 2, False),
        ('train', '*', '*'): ('typed', 2, False)},
    ('cl', 'f32'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): ('cl', 0, False),
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): ('cl', 0, False)},
    ('cl', 'bf16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ('cl', 1, False),
        ('infer', 'split', 1): ('typed', 1, False),
        ('train', '*', '*'): ('cl', 1, False)},
    ('cl', 'f16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ('cl', 2, False),
        ('infer', 'split', 1): ('typed', 2, False),
        ('train', '*', '*'): ('cl', 2, False)},
    ('groups_contiguous', 'f32'): ('plain', 0, True),
    ('groups_contiguous', 'bf16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 1, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('groups_contiguous', 'f16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 2, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('groups_cl', 'f32'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): ('plain', 0, True),
        ('infer', 'split', 0): ('cl', 0, True),
        ('infer', 'split', 1): ('plain', 0, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('groups_cl', 'bf16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ('cl', 1, True),
        ('infer', 'split', 1): ('typed', 1, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('groups_cl', 'f16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ('cl', 2, True),
        ('infer', 'split', 1): ('typed', 2, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('one_map_in_groups_cl', 'f32'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): ('plain', 0, True),
        ('infer', 'split', 0): ('cl', 0, True),
        ('infer', 'split', 1): ('plain', 0, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('one_map_in_groups_cl', 'bf16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ('cl', 1, True),
        ('infer', 'split', 1): ('typed', 1, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('one_map_in_groups_cl', 'f16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ('cl', 2, True),
        ('infer', 'split', 1): ('typed', 2, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('last_cl_rest_contiguous', 'f32'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): ONE_LAYOUT},
    ('last_cl_rest_contiguous', 'bf16'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('typed', 1, False),
        ('train', '*', '*'): ONE_LAYOUT},
    ('last_cl_rest_contiguous', 'f16'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('typed', 2, False),
        ('train', '*', '*'): ONE_LAYOUT},
    ('first_contiguous_rest_cl', 'f32'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): ONE_LAYOUT},
    ('first_contiguous_rest_cl', 'bf16'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('typed', 1, False),
        ('train', '*', '*'): ONE_LAYOUT},
    ('first_contiguous_rest_cl', 'f16'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('typed', 2, False),
        ('train', '*', '*'): ONE_LAYOUT},
    ('groups_mixed_layouts', 'f32'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): ('plain', 0, True),
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('plain', 0, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('groups_mixed_layouts', 'bf16'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('typed', 1, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('groups_mixed_layouts', 'f16'): {
        ('infer', 'fp32', 0): ONE_LAYOUT,
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): ONE_LAYOUT,
        ('infer', 'split', 1): ('typed', 2, True),
        ('train', '*', '*'): ('plain', 0, True)},
    ('contiguous_mixed_dtypes', 'f32'): "ValueError: feature maps must all have one dtype, got ['torch.float16', 'torch.float32']",
    ('contiguous_mixed_dtypes', 'bf16'): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float32']",
    ('contiguous_mixed_dtypes', 'f16'): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float16']",
    ('cl_mixed_dtypes', 'f32'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): "ValueError: feature maps must all have one dtype, got ['torch.float16', 'torch.float32']",
        ('infer', 'split', '*'): "ValueError: feature maps must all have one dtype, got ['torch.float16', 'torch.float32']",
        ('train', '*', '*'): "ValueError: feature maps must all have one dtype, got ['torch.float16', 'torch.float32']"},
    ('cl_mixed_dtypes', 'bf16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float32']",
        ('infer', 'split', '*'): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float32']",
        ('train', '*', '*'): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float32']"},
    ('cl_mixed_dtypes', 'f16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float16']",
        ('infer', 'split', '*'): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float16']",
        ('train', '*', '*'): "ValueError: feature maps must all have one dtype, got ['torch.bfloat16', 'torch.float16']"},
    ('cl_fp64', 'f32'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): 'ValueError: channels_last feature maps must be fp32, bf16 or fp16, got torch.float64',
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): 'ValueError: channels_last feature maps must be fp32, bf16 or fp16, got torch.float64'},
    ('cl_fp64', 'bf16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): 'ValueError: channels_last feature maps must be fp32, bf16 or fp16, got torch.float64',
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): 'ValueError: channels_last feature maps must be fp32, bf16 or fp16, got torch.float64'},
    ('cl_fp64', 'f16'): {
        ('infer', 'fp32', 0): NEED_SPLIT_CL,
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): 'ValueError: channels_last feature maps must be fp32, bf16 or fp16, got torch.float64',
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): 'ValueError: channels_last feature maps must be fp32, bf16 or fp16, got torch.float64'},
    ('contiguous_fp64', 'f32'): ('plain', 0, False),
    ('contiguous_fp64', 'bf16'): ('plain', 0, False),
    ('contiguous_fp64', 'f16'): ('plain', 0, False),
    ('contiguous_non_tensor', 'f32'): {
        ('infer', '*', '*'): 'ValueError: feature maps must all have one dtype, got ["<class \'numpy.ndarray\'>", \'torch.float32\']',
        ('train', '*', '*'): ('plain', 0, True)},
    ('contiguous_non_tensor', 'bf16'): {
        ('infer', '*', '*'): 'ValueError: feature maps must all have one dtype, got ["<class \'numpy.ndarray\'>", \'torch.bfloat16\']',
        ('train', '*', '*'): ('plain', 0, True)},
    ('contiguous_non_tensor', 'f16'): {
        ('infer', '*', '*'): 'ValueError: feature maps must all have one dtype, got ["<class \'numpy.ndarray\'>", \'torch.float16\']',
        ('train', '*', '*'): ('plain', 0, True)},
    ('cl_non_tensor', 'f32'): {
        ('infer', '*', '*'): 'ValueError: feature maps must all have one dtype, got ["<class \'numpy.ndarray\'>", \'torch.float32\']',
        ('train', '*', '*'): ('plain', 0, True)},
    ('cl_non_tensor', 'bf16'): {
        ('infer', '*', '*'): 'ValueError: feature maps must all have one dtype, got ["<class \'numpy.ndarray\'>", \'torch.bfloat16\']',
        ('train', '*', '*'): ('plain', 0, True)},
    ('cl_non_tensor', 'f16'): {
        ('infer', '*', '*'): 'ValueError: feature maps must all have one dtype, got ["<class \'numpy.ndarray\'>", \'torch.float16\']',
        ('train', '*', '*'): ('plain', 0, True)},
    ('eight_contiguous', 'f32'): NINE,
    ('eight_contiguous', 'bf16'): NINE,
    ('eight_contiguous', 'f16'): NINE,
    ('eight_cl', 'f32'): NINE,
    ('eight_cl', 'bf16'): NINE,
    ('eight_cl', 'f16'): NINE,
    ('cl_wrong_batch', 'f32'): {
        ('infer', 'fp32', 0): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)',
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)',
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)'},
    ('cl_wrong_batch', 'bf16'): {
        ('infer', 'fp32', 0): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)',
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)',
        ('infer', 'split', 1): ('typed', 1, False),
        ('train', '*', '*'): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)'},
    ('cl_wrong_batch', 'f16'): {
        ('infer', 'fp32', 0): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)',
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)',
        ('infer', 'split', 1): ('typed', 2, False),
        ('train', '*', '*'): 'ValueError: feats[3] is channels_last with logical shape (4, 576, 14, 14), expected (2, 576, 14, 14)'},
    ('contiguous_wrong_batch', 'f32'): ('plain', 0, False),
    ('contiguous_wrong_batch', 'bf16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 1, False),
        ('train', '*', '*'): ('typed', 1, False)},
    ('contiguous_wrong_batch', 'f16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 2, False),
        ('train', '*', '*'): ('typed', 2, False)},
    ('cl_one_permuted', 'f32'): {
        ('infer', 'fp32', 0): 'ValueError: feats[8] is neither contiguous nor torch.channels_last',
        ('infer', 'fp32', 1): ('plain', 0, False),
        ('infer', 'split', 0): 'ValueError: feats[8] is neither contiguous nor torch.channels_last',
        ('infer', 'split', 1): ('plain', 0, False),
        ('train', '*', '*'): 'ValueError: feats[8] is neither contiguous nor torch.channels_last'},
    ('cl_one_permuted', 'bf16'): {
        ('infer', 'fp32', 0): 'ValueError: feats[8] is neither contiguous nor torch.channels_last',
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): 'ValueError: feats[8] is neither contiguous nor torch.channels_last',
        ('infer', 'split', 1): ('typed', 1, False),
        ('train', '*', '*'): 'ValueError: feats[8] is neither contiguous nor torch.channels_last'},
    ('cl_one_permuted', 'f16'): {
        ('infer', 'fp32', 0): 'ValueError: feats[8] is neither contiguous nor torch.channels_last',
        ('infer', 'fp32', 1): NEED_SPLIT_16,
        ('infer', 'split', 0): 'ValueError: feats[8] is neither contiguous nor torch.channels_last',
        ('infer', 'split', 1): ('typed', 2, False),
        ('train', '*', '*'): 'ValueError: feats[8] is neither contiguous nor torch.channels_last'},
    ('contiguous_one_permuted', 'f32'): ('plain', 0, False),
    ('contiguous_one_permuted', 'bf16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 1, False),
        ('train', '*', '*'): ('typed', 1, False)},
    ('contiguous_one_permuted', 'f16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 2, False),
        ('train', '*', '*'): ('typed', 2, False)},
    ('nhwc_shaped_contiguous', 'f32'): ('plain', 0, False),
    ('nhwc_shaped_contiguous', 'bf16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 1, False),
        ('train', '*', '*'): ('typed', 1, False)},
    ('nhwc_shaped_contiguous', 'f16'): {
        ('infer', 'fp32', '*'): NEED_SPLIT_16,
        ('infer', 'split', '*'): ('typed', 2, False),
        ('train', '*', '*'): ('typed', 2, False)},
}


def expected(name, dt, side, prec, layout):
    e = EXPECTED[(name, dt)]
    if not isinstance(e, dict):
        return e
    for (s, p, lay), outcome in e.items():
        if s in ("*", side) and p in ("*", prec) and lay in ("*", layout):
            return outcome
    raise KeyError((name, dt, side, prec, layout))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(INPUTS))
def test_route_table(name, dt):
    feats = INPUTS[name](DTYPES[dt])
    for side, prec, layout in SETTINGS:
        got = ladder(feats, side, PRECISIONS[prec], layout)
        assert got == expected(name, dt, side, prec, layout), (name, dt, side, prec, layout, got)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(INPUTS))
def test_names_other_code_uses_follow_the_route(name, dt):
    """OffForward.takes_channels_last / train_takes_channels_last (unbound, on a stub) and train_feat_layout say "cl" exactly where the
    route does; where the route raises they raise the same text or leave it to the rungs behind them."""
    feats = INPUTS[name](DTYPES[dt])
    for side, prec, layout in SETTINGS:
        h = types.SimpleNamespace(batch=B, length=L, precision=PRECISIONS[prec], feat_layout=layout)
        want = expected(name, dt, side, prec, layout)
        fn = runtime.OffForward.takes_channels_last if side == "infer" else runtime.OffForward.train_takes_channels_last
        if isinstance(want, tuple):
            assert fn(h, feats) is (want[0] == "cl")
            if side == "train":
                assert runtime.train_feat_layout(feats, B, L) == ("cl" if want[0] == "cl" else "nchw")
        else:
            try:
                cl = fn(h, feats)
            except ValueError as e:
                assert "ValueError: %s" % e == want
            else:                                      # a later rung raises: the count of maps; behind "cl", the dtype rules alone
                assert not cl or "one dtype" in want or "must be fp32, bf16 or fp16" in want
