"""The generated inputs of the conv backward tests held to a recorded golden, tests/golden/conv_bwd_cases.json (tools/record_conv_bwd_cases.py
wrote it from the case modules as they were before the two strides were folded onto tests/conv_bwd.py's forms): one sha256 over the bytes of
int_inputs(c) and of normal_inputs(c) for every case of both forms (a plan-chosen case at n = 3), of the data gradient's worst-case
operands on every pattern / sign combination at every shape its tests use, and of the wide-integer operand of both recipes at the shapes
and seeds their tests use.  No library, no device.

References are not hashed (an fp64 conv on the CPU may sum in another order on another machine); instead reference() of three small
cases per form -- the 1x1 and 2x2 maps and a non-square one -- must EQUAL a conv2d + autograd call written out here, on one thread."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from .conv_bwd_cases import digest, FORMS, GOLDEN_FILE, jobs, SMALL


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
