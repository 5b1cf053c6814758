"""Records tests/golden/conv_bwd_cases.json: one sha256 per generated input of the conv backward tests (integer and normal inputs of every
case of both strides, the data gradient's worst-case operands, the wide-integer operands), from the case modules in the tree.  The job list
is tests/conv_bwd_cases.py's; tests/test_conv_bwd_cases.py holds later trees to the file.  Needs no library and no GPU; from the repository root:

    python tools/record_conv_bwd_cases.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import conv_bwd_cases as t  # noqa: E402


def main():
    out = t.record()
    path = os.path.join(ROOT, "tests", "golden", t.GOLDEN_FILE)
    with open(path, "w") as f:          # one record per line
        f.write("{\n%s\n}\n" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(out.items())))
    print("%d inputs -> %s" % (len(out), path))


if __name__ == "__main__":
    main()
