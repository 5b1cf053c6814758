"""Records tests/golden/conv_bwd_entries.json: what every conv backward entry of include/offk.h refuses (return code and the full
offk_last_error text, fp32 entry and split twin, for every rule of the refusal tables of tests/conv_bwd_abi.py and tests/conv_bwd_s2_abi.py) and what its six plan
entries return over a sweep of n_img, from the library in the tree (or OFFK_LIB).  The case lists are tests/conv_bwd_entries.py's;
tests/test_conv_bwd_entries.py holds later builds to the file.  Needs no GPU (every refusal fires before the first HIP call, the plans are host code); from the
repository root:

    [OFFK_LIB=<an earlier build's liboffk.so>] python tools/record_conv_bwd_entries.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import offk_amd  # noqa: E402,F401
from offk_amd import _lib  # noqa: E402
from tests import conv_bwd_entries as t  # noqa: E402


def main():
    out = t.record(_lib.load())
    accepted = [cid for cid, (rc, msg) in out["refusals"].items() if rc != -1 or not msg]
    if accepted:
        sys.exit("NOT REFUSED: %s" % accepted)
    path = os.path.join(ROOT, "tests", "golden", t.GOLDEN_FILE)
    with open(path, "w") as f:          # one record per line
        sections = ["%s: {\n%s\n}" % (json.dumps(name), ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                                                  for k, v in sorted(sec.items()))) for name, sec in sorted(out.items())]
        f.write("{\n%s\n}\n" % ",\n".join(sections))
    print("%d refusals, %d plan sweeps from %s -> %s" % (len(out["refusals"]), len(out["plans"]), _lib.LIB_PATH, path))


if __name__ == "__main__":
    main()
