"""Records tests/golden/feat_entry_refusals.json: what every feature-map entry of include/offk.h refuses (return code and
offk_last_error text) and the launch names of its good calls, from the library in the tree (or OFFK_LIB).  The case lists are
tests/feat_entries.py's; tests/test_gpu_feat_entries.py holds later builds to the file.  Run on an MI355X, from the repository root:

    python tools/record_feat_entries.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import offk_amd  # noqa: E402,F401
from offk_amd import runtime  # noqa: E402
from tests import feat_entries as t  # noqa: E402


def main():
    world = t.World(runtime)
    out = {"refusals": {}, "traces": {}}
    for h in world.handles.values():
        world.fill(h)
    for case in t.refusal_cases():
        got = world.refused(case)
        if got[0] == 0:
            sys.exit("NOT REFUSED (nothing further is run): %s" % t.case_id(*case))
        out["refusals"][t.case_id(*case)] = got
    dirty = [name for name, h in world.handles.items() if not world.untouched(h)]
    if dirty:
        sys.exit("a refused call wrote to the buffers of handle(s) %s" % dirty)
    for case in t.trace_cases():
        out["traces"][t.case_id(*case)] = world.traced(*case)
    path = os.path.join(ROOT, "tests", "golden", t.GOLDEN_FILE)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d refusals, %d traces -> %s" % (len(out["refusals"]), len(out["traces"]), path))


if __name__ == "__main__":
    main()
