"""The generated inputs of the conv backward tests held to a recorded golden, tests/golden/conv_bwd_cases.json (tools/record_conv_bwd_cases.py
wrote it from the case modules as they were before the two strides were folded onto tests/conv_bwd.py's forms): one sha256 over the bytes of
int_inputs(c) and of normal_inputs(c) for every case of both forms (a plan-chosen case at n = 3), of the data gradient's worst-case
operands on every pattern / sign combination at every shape its tests use, and of the wide-integer operand of both recipes at the shapes
and seeds their tests use.  No library, no device.

References are not hashed (an fp64 conv on the CPU may sum in another order on another machine); instead reference() of three small
cases per form -- the 1x1 and 2x2 maps and a non-square one -- must EQUAL a conv2d + autograd call written out here, on one thread."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from . import conv_grad_checks as chk
from .conv_bwd import S1, S2

GOLDEN_FILE = "conv_bwd_cases.json"
FORMS = (("S1", S1), ("S2", S2))
SMALL = {"S1": [S1.Case(3, 1, 1, 1, 64, 64), S1.Case(3, 1, 2, 2, 64, 64), S1.Case(3, 2, 5, 3, 128, 128)],
         "S2": [S2.Case(7, 1, 2, 2, 32, 64), S2.Case(5, 1, 2, 2, 32, 64), S2.Case(5, 2, 6, 4, 160, 64)]}


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def worst_shapes(form):
    """(k, n, H, W, ci, co) of every shape the data gradient's worst-case tests use: the CPU test's, and on the GPU the 13 fusion shapes at
    n = 1 (stride 1) or the same two again (stride 2)"""
    return list(form.WORST) + [(k, 1, H, H, ci, co) for H, ci, co, k in getattr(form, "FUSION_SHAPES", ())]


def jobs():
    """[(id, a function that returns the arrays to hash)]"""
    out = []
    for name, form in FORMS:
        for c in form.cases():
            c3 = c._replace(n=3) if c.n is None else c
            out.append(("%s/int/%s" % (name, form.case_id(c)), lambda form=form, c=c3: [form.int_inputs(c)[k] for k in ("x", "g", "w", "dx0", "dw0", "db0")]))
            out.append(("%s/normal/%s" % (name, form.case_id(c)), lambda form=form, c=c3: [form.normal_inputs(c)[k] for k in ("x", "g", "w")]))
        for shape in worst_shapes(form):
            for pattern, signs in chk.ADV:
                out.append(("%s/worst/%s/0x%06X_%s" % (name, form.case_id(form.Case(*shape)), pattern, signs),
                            lambda form=form, a=(shape, pattern, signs): form.worst_inputs(*a)))
        for split, sides in (("dgrad", "gw"), ("wgrad", "gx")):
            for c in chk.WIDE[form.stride, split][1]:
                for side in sides:
                    out.append(("%s/wide_%s/%s/%s" % (name, split, form.case_id(c), side),
                                lambda form=form, a=(c, side, split): [chk.wide_inputs(form, *a)[a[1]]]))
    return out


def record():
    """what the golden file holds, from the modules in the tree"""
    return dict((jid, digest(make())) for jid, make in jobs())


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, GOLDEN_FILE)) as f:
        return json.load(f)


def test_golden_lists_the_cases(golden):
    ids = [jid for jid, _make in jobs()]
    assert len(ids) == len(set(ids)) and sorted(golden) == sorted(ids)
    assert len(set(golden.values())) == len(golden), "no two entries hold the same bytes"


def test_generated_inputs_keep_their_bytes(golden):
    wrong = [jid for jid, make in jobs() if digest(make()) != golden[jid]]
    assert not wrong, wrong


@pytest.mark.parametrize("relu_in", [False, True], ids=["plain", "relu_in"])
@pytest.mark.parametrize("name,c", [(n, c) for n, _f in FORMS for c in SMALL[n]], ids=[f.case_id(c) for n, f in FORMS for c in SMALL[n]])
def test_reference_is_conv2d_and_autograd(name, c, relu_in):
    form = dict(FORMS)[name]
    assert c in form.cases()
    inp = form.int_inputs(c)

    def grads(x, g, w):
        x = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        w = w.double().clone().requires_grad_(True)
        b = torch.zeros(c.co, dtype=torch.float64, requires_grad=True)
        F.conv2d(x, w, b, stride=form.stride, padding=(c.k - 1) // 2).backward(g.double().permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1).contiguous(), w.grad, b.grad

    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref = form.reference(c, inp, relu_in)
        xin = torch.relu(inp["x"]) if relu_in else inp["x"]
        mask = (inp["x"] > 0).double() if relu_in else 1.0
        dx, dw, db = grads(xin, inp["g"], inp["w"])                       # the gradient w.r.t. relu(x), then the mask: conv(relu(x))'s dX
        dxa, dwa, dba = grads(xin.abs(), inp["g"].abs(), inp["w"].abs())
    finally:
        torch.set_num_threads(threads)
    for key, want in (("dX", dx * mask), ("dW", dw), ("db", db), ("dX_abs", dxa * mask), ("dW_abs", dwa), ("db_abs", dba)):
        assert ref[key].shape == want.shape and torch.equal(ref[key], want), key
    assert ref["dX"].shape == (c.n, c.H, c.W, c.ci) and inp["g"].shape == (c.n, c.H // form.stride, c.W // form.stride, c.co)
