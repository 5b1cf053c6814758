"""Does every translation unit of this tree compile to the same gfx950 device code as another tree's?
    python tools/same_device_code.py <other csrc dir> [source.hip ...]
Compiles each source of build.py's SOURCES (or the ones named) from both directories, device side only, with the product flags,
and compares the disassembly (`llvm-objdump -d`, the line that names the file dropped) and what build.kernel_resources reads
from the code object's metadata (registers, spills, scratch) plus each kernel's LDS size.  Prints one line per source:
source, kernels and one of three verdicts:
  identical   the same disassembly and the same resources;
  same loop   per kernel: equal resources, an equal count of every mnemonic, and the same sequence of mnemonics among the
              non-scalar instructions (all whose mnemonic does not begin with `s_`): what differs is scalar register
              allocation, scalar order and operands;
  differs     anything else, followed by the per-mnemonic count differences (other -> here) of each kernel that differs.
Exits 1 unless all are identical: an identical source needs no GPU for its speed argument, the other two need a timing."""
import collections
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


def mnemonics(text):
    """{symbol: [mnemonic, ...]} of a disassembly: a symbol line is `<address> <name>:`, an instruction line begins with a tab."""
    out, cur = {}, None
    for ln in text:
        m = re.match(r"[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.startswith("\t"):
            cur.append(ln.split()[0])
    return out


def compare(other, src, out_dir):
    """(source, kernels, verdict, [difference lines])"""
    mine = device_code(b.CSRC, src, os.path.join(out_dir, "here"))
    theirs = device_code(other, src, os.path.join(out_dir, "other"))
    if mine == theirs:
        return src, len(mine[1]), "identical", []
    res = [{k["mangled"]: k for k in r} for r in (mine[1], theirs[1])]
    ops = [mnemonics(t) for t in (mine[0], theirs[0])]
    verdict, notes = "same loop", []
    for name in sorted(set(ops[0]) | set(ops[1])):
        if name not in ops[0] or name not in ops[1]:
            verdict = "differs"
            notes.append("%s: only %s" % (name, "here" if name in ops[0] else "in the other tree"))
            continue
        if res[0].get(name) != res[1].get(name):
            verdict = "differs"
            a, c = res[1].get(name) or {}, res[0].get(name) or {}
            notes.append("%s: resources %s" % (name, ", ".join("%s %s -> %s" % (f, a.get(f), c.get(f)) for f in sorted(set(a) | set(c)) if a.get(f) != c.get(f))))
        here, there = collections.Counter(ops[0][name]), collections.Counter(ops[1][name])
        if here != there:
            verdict = "differs"
            notes.append("%s: %s" % (name, ", ".join("%s %d -> %d" % (m, there[m], here[m]) for m in sorted(set(here) | set(there)) if here[m] != there[m])))
        elif [m for m in ops[0][name] if not m.startswith("s_")] != [m for m in ops[1][name] if not m.startswith("s_")]:
            verdict = "differs"
            notes.append("%s: equal mnemonic counts, another order of the non-scalar instructions" % name)
    return src, len(mine[1]), verdict, notes


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
    print("%-28s %7s  %s" % ("source", "kernels", "verdict"))
    for src, n, verdict, notes in rows:
        print("%-28s %7d  %s" % (src, n, verdict))
        for note in notes:
            print("    " + note)
    bad = [r[0] for r in rows if r[2] != "identical"]
    print(", ".join("%d %s" % (sum(r[2] == v for r in rows), v) for v in ("identical", "same loop", "differs")) + " of %d sources" % len(rows))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
