"""The job list of tests/test_conv_bwd_cases.py (tools/record_conv_bwd_cases.py writes tests/golden/conv_bwd_cases.json from it): one
sha256 per generated input of the conv backward tests.  A helper module: no tests of its own."""
import hashlib

import numpy as np
import torch

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
