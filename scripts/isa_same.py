"""Is the device code of two trees the same?  The parent-against-new check of a change that must not touch a kernel.

usage: python scripts/isa_same.py PARENT_TREE TREE [unit.hip ...]      (default: every .hip of cal_amd/csrc in either tree)

Compiles each unit of both trees for the device only, to assembly (cal_amd.build.FLAGS + --cuda-device-only -S: both sides the
same way -- a --save-temps build prints block names that -S does not), drops the lines that hold the compilation-unit id
(__hip_cuid_*: it differs whenever the source text does) and compares the rest as plain text.  Per unit: the number of kernels and
of differing lines; exit status 1 if any unit differs.  Needs hipcc, no GPU.  At most 8 compiles at a time.
"""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from cal_amd.build import FLAGS, _hipcc  # noqa: E402


def assembly(tree, unit, out):
    """Filtered device assembly of tree/cal_amd/csrc/unit as a list of lines, or None where the tree has no such unit."""
    src = os.path.join(tree, "cal_amd", "csrc", unit)
    if not os.path.exists(src):
        return None
    cmd = [_hipcc()] + FLAGS + ["-I", os.path.join(tree, "include"), "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr))
    with open(out) as fh:
        lines = [ln for ln in fh if "__hip_cuid_" not in ln]
    os.remove(out)
    return lines


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    trees = argv[1:3]
    units = argv[3:] or sorted({f for t in trees for f in os.listdir(os.path.join(t, "cal_amd", "csrc")) if f.endswith(".hip")})
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as ex:
        jobs = {(u, k): ex.submit(assembly, trees[k], u, os.path.join(tmp, "%d_%s.s" % (k, u))) for u in units for k in (0, 1)}
        differ = 0
        for u in units:
            a, b = jobs[u, 0].result(), jobs[u, 1].result()
            if a is None or b is None:
                print("%-20s only in %s" % (u, trees[1] if a is None else trees[0]))
                differ += 1
                continue
            n = 0
            if a != b:
                pa, pb = os.path.join(tmp, "a.s"), os.path.join(tmp, "b.s")
                for p, lines in ((pa, a), (pb, b)):
                    with open(p, "w") as fh:
                        fh.writelines(lines)
                d = subprocess.run(["diff", pa, pb], capture_output=True, text=True).stdout
                n = sum(ln[:1] in ("<", ">") for ln in d.splitlines())
                differ += 1
            kernels = [sum(".amdhsa_kernel " in ln for ln in x) for x in (a, b)]
            print("%-20s kernels %3d / %3d   lines %7d / %7d   differing lines %d" % (u, kernels[0], kernels[1], len(a), len(b), n))
    print("SAME" if not differ else "%d unit(s) differ" % differ)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
