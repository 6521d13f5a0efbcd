#!/usr/bin/env python
"""Device assembly of two source trees, file by file: python tools/dev/isa_diff.py <tree A> <tree B> [file.hip ...]
Compiles every mgnns_amd/csrc/*.hip of both trees with the flags of mgnns_amd/build.py (this tree's) plus
--cuda-device-only -S, drops what cannot be equal (.file / .ident / .loc directives, comment lines, the __hip_cuid_* symbol,
lines naming the source path) and prints per file "identical" or the kernels whose text differs.  Exit status 1 on any
difference.  A refactor that moves helpers between files proves itself with it: same assembly, same behaviour, same speed.
It compares two texts and looks for nothing inside them.  Needs hipcc, no GPU."""
import glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mgnns_amd import build


def assembly(tree, name, out):
    """{function name: its lines}; what precedes the first function and the metadata note go under names in parentheses."""
    csrc = os.path.join(os.path.abspath(tree), "mgnns_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc if os.path.exists(hipcc) else "hipcc"] + build.FLAGS + build.FILE_FLAGS.get(name, [])
    r = subprocess.run(cmd + ["--cuda-device-only", "-S", os.path.join(csrc, name), "-o", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s of %s:\n%s" % (name, tree, r.stdout))
    parts, cur = {}, "(head)"
    for line in open(out):
        s = line.strip()
        if not s or s.startswith(";") or s.startswith("//") or re.match(r"\.(file|ident|loc)\b", s) or "__hip_cuid_" in s or csrc in s:
            continue
        m = re.match(r"\.type\s+(\S+),@function", s)
        cur = m.group(1) if m else "(metadata)" if s.startswith(".amdgpu_metadata") else cur
        parts.setdefault(cur, []).append(s)
    return parts


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = sys.argv[1], sys.argv[2]
    names = [sorted(os.path.basename(f) for f in glob.glob(os.path.join(t, "mgnns_amd", "csrc", "*.hip"))) for t in (a, b)]
    if sys.argv[3:]:
        names = [[n for n in ns if n in sys.argv[3:]] for ns in names]
    both = [n for n in names[0] if n in names[1]]
    bad = sorted(set(names[0]) ^ set(names[1]))
    for n in bad:
        print("%-28s only in %s" % (n, a if n in names[0] else b))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        jobs = [(n, pool.submit(assembly, a, n, os.path.join(tmp, "a_" + n + ".s")), pool.submit(assembly, b, n, os.path.join(tmp, "b_" + n + ".s")))
                for n in both]
        for n, fa, fb in jobs:
            pa, pb = fa.result(), fb.result()
            diff = [k for k in sorted(set(pa) | set(pb)) if pa.get(k) != pb.get(k)]
            bad += diff
            print("%-28s %s" % (n, "identical" if not diff else "DIFFERENT: " + ", ".join(diff)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
