"""Records tests/golden/forward_plans.json: the ordered launch-group names of one forward for every case of
tests/forward_plan.py (the list tests/test_gpu_forward_plan.py holds later builds to), from the library in the tree (or OFFK_LIB).  Run on an MI355X, from the repository root:

    python tools/record_forward_plans.py

    python tools/record_forward_plans.py --digests OUT.txt
        writes no golden; OUT.txt gets the bytes of device memory offk_create takes for three handles and one line per case: SHA-256
        (first 16 hex digits each) of the launch names, the three logit tensors and the stage regions (tests/forward_plan.py REGIONS).
        For a one-off A/B of two builds on one box (OFFK_LIB=<the other liboffk.so>): the files of two builds that compute the same
        are identical.  Digests are not committed as goldens: split-K depths follow the device's grid (tests/test_gpu_switches.py).
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import offk_amd  # noqa: E402,F401
from offk_amd import runtime, spec  # noqa: E402
from tests import forward_plan as t  # noqa: E402
from tests.forward import switches  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def sha(x):
    data = x.encode() if isinstance(x, str) else x.detach().contiguous().cpu().numpy().tobytes()
    return hashlib.sha256(data).hexdigest()[:16]


def create_bytes():
    """hipMemGetInfo's free bytes before minus after offk_create (B = 3, L = 7, RGB), per handle."""
    out = {}
    for name, prec, env in (("fp32", "fp32", {}), ("f32split", "f32split", {}), ("f32split-winograd0", "f32split", {"OFFK_WINOGRAD": "0"})):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        with switches(env):
            h = runtime.OffForward(3, 7, spec.VARIANT_RGB, consensus=False, precision=prec)
        out[name] = before - torch.cuda.mem_get_info()[0]
        del h
    return out


def main():
    digests = sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--digests" else None
    if len(sys.argv) > 1 and not digests:
        sys.exit(__doc__)
    torch.zeros(1, device="cuda")                      # (the context and torch's own first allocations, before anything is measured)
    lines = ["create_bytes %s" % " ".join("%s=%d" % kv for kv in sorted(create_bytes().items())),
             "# case: names out7 out14 out28 " + " ".join(name for name, _ch in t.REGIONS)] if digests else []
    plans = {}
    for case, prec in t.CASE_PARAMS:
        h, names, traced, plain = t.run_case(runtime, GOLDEN_DIR, case, prec)
        for a, b in zip(traced, plain):
            if a is not None and not torch.equal(a, b):
                sys.exit("traced and untraced logits differ: %s" % t.case_id(case, prec))
        plans[t.case_id(case, prec)] = names
        if digests:
            d = [sha("\n".join(names))] + ["-" if x is None else sha(x) for x in plain] + [sha(h.region(name, ch)) for name, ch in t.REGIONS]
            lines.append("%s: %s" % (t.case_id(case, prec), " ".join(d)))
        del h
    path = digests or os.path.join(GOLDEN_DIR, t.GOLDEN_FILE)
    if digests:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        t.dump_golden(plans, path)
    print("%d cases -> %s" % (len(t.CASE_PARAMS), path))


if __name__ == "__main__":
    main()
