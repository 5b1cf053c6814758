"""Does every translation unit of this tree compile to the same gfx950 device code as another tree's?
    python tools/same_device_code.py <other csrc dir> [source.hip ...]
Compiles each source of build.py's SOURCES (or the ones named) from both directories, device side only, with the product flags,
and compares the disassembly (`llvm-objdump -d`, the line that names the file dropped) and what build.kernel_resources reads
from the code object's metadata (registers, spills, scratch) plus each kernel's LDS size.  Prints one line per source:
source, kernels, identical; exits 1 unless all are identical.  A refactor's speed argument: needs no GPU."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("offk_build", os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "build.py"))
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)


def device_code(csrc, src, out_dir):
    """(disassembly lines, kernel resources) of one source of one tree; (None, None) where it has no device code."""
    co = os.path.join(out_dir, src.replace(".hip", ".co"))
    cmd = [b._hipcc(), "-c", os.path.join(csrc, src), "-o", co, "--cuda-device-only", "--no-gpu-bundle-output"] + b.FLAGS + b.EXTRA_FLAGS.get(src, [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit("hipcc failed for %s:\n%s" % (os.path.join(csrc, src), r.stderr))
    d = subprocess.run([b._llvm_objdump(), "-d", co], capture_output=True, text=True, check=True).stdout
    text = [ln for ln in d.splitlines() if "file format" not in ln]
    res = b.kernel_resources(co)
    notes = subprocess.run([b._llvm_readelf(), "--notes", co], capture_output=True, text=True, check=True).stdout
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)
    for k, size in zip(res, lds):
        k["group_segment_fixed_size"] = int(size)
    if len(lds) != len(res):
        raise SystemExit("%s: %d LDS sizes for %d kernels" % (src, len(lds), len(res)))
    return text, res


def compare(other, src, out_dir):
    mine = device_code(b.CSRC, src, os.path.join(out_dir, "here"))
    theirs = device_code(other, src, os.path.join(out_dir, "other"))
    return src, len(mine[1]), mine[0] == theirs[0], mine[1] == theirs[1]


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    other = os.path.abspath(sys.argv[1])
    sources = sys.argv[2:] or list(b.SOURCES)                                     # offk_api.hip: no kernels, an empty code object
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "here"))
        os.makedirs(os.path.join(tmp, "other"))
        with ThreadPoolExecutor(max_workers=4) as ex:
            rows = list(ex.map(lambda s: compare(other, s, tmp), sources))
    print("%-28s %7s  %s" % ("source", "kernels", "identical"))
    for src, n, same_text, same_res in rows:
        print("%-28s %7d  %s" % (src, n, "yes" if same_text and same_res else
                                 "NO (%s)" % ", ".join(w for w, ok in (("instructions", same_text), ("resources", same_res)) if not ok)))
    bad = [r[0] for r in rows if not (r[2] and r[3])]
    print("%d of %d sources identical" % (len(rows) - len(bad), len(rows)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
