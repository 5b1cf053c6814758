"""Records tests/golden/handle_layout.json: per handle of tests/handle_layout.py's list the workspace sizes, every workspace
region and unit-gradient slot by name (or the code and text with which the handle says it has none), and on the smallest handles what the
unit entries answer while one weight is missing and what binding a parameter returns -- from the library in the tree (or OFFK_LIB).  The
case lists are those tests/test_gpu_handle_layout.py holds later builds to.  Run on an MI355X, from the repository root:

    [OFFK_LIB=<an earlier build's liboffk.so>] python tools/record_handle_layout.py [output path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import offk_amd  # noqa: E402,F401
from offk_amd import _lib  # noqa: E402
from tests import handle_layout as t  # noqa: E402


def main():
    out = t.record(_lib.load())
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.GOLDEN_FILE)
    line = lambda v: json.dumps(v, separators=(",", ":"), sort_keys=True)      # noqa: E731
    with open(path, "w") as f:          # one handle's section per line
        sections = ["%s: {\n%s\n}" % (json.dumps(name), ",\n".join("%s: %s" % (json.dumps(k), line(v)) for k, v in sorted(sec.items())))
                    for name, sec in sorted(out.items())]
        f.write("{\n%s\n}\n" % ",\n".join(sections))
    print("%d handle layouts, %d trails from %s -> %s" % (len(out["layout"]), len(out["trail"]), _lib.LIB_PATH, path))


if __name__ == "__main__":
    main()
