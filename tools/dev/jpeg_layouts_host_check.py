"""Build tools/dev/jpeg_layouts_host_check.cpp with the host compiler under AddressSanitizer + UBSan and run it over every file of
tests/golden/jpeg_layouts.npz: the accepted ones must decode to Pillow's pixels, the refused ones get their recorded reasons and the
corrupt ones their recorded statuses; the two smallest accepted files are cut at every length, and every file takes 10 000 seeded
mutations.  CPU only (a stand-alone program run as a child; nothing is loaded into Python) -- never run it on a GPU machine.

    python tools/dev/jpeg_layouts_host_check.py [--mutations 10000] [--cxx c++]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutations", type=int, default=10000)
    ap.add_argument("--cxx", default=os.environ.get("CXX", "c++"))
    a = ap.parse_args()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "jpeg_layouts.npz")))
    want_reason = dict(zip((str(n) for n in g["refused"]), (int(r) for r in g["refused_reason"])))
    want_status = dict(zip((str(n) for n in g["corrupt"]), (int(s) for s in g["corrupt_status"])))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "jpeg_layouts_host_check")
        cmd = [a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
               os.path.join(ROOT, "tools", "dev", "jpeg_layouts_host_check.cpp"), "-o", exe]
        print(" ".join(cmd))
        subprocess.check_call(cmd)
        names = [k[5:] for k in g if k.startswith("file_")]
        smallest = sorted((k for k in names if "pix_" + k in g), key=lambda k: g["file_" + k].size)[:2]
        inputs = 0
        for name in sorted(names):
            path = os.path.join(tmp, name + ".jpg")
            g["file_" + name].tofile(path)
            args = [exe, path]
            if "pix_" + name in g:
                g["pix_" + name].tofile(path[:-4] + ".rgb")
                args.append(path[:-4] + ".rgb")
            if name in smallest:
                args.append("--truncate")
            r = subprocess.run(args + ["--mutations", str(a.mutations)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            print(r.stdout.strip().replace(tmp + os.sep, ""))
            if r.returncode != 0:
                sys.exit("FAILED on %s (exit status %d)" % (name, r.returncode))
            m = re.search(r"reason (\d+), .* worst status (\d+)", r.stdout)
            if int(m.group(1)) != want_reason.get(name, 0) or int(m.group(2)) != want_status.get(name, 0):
                sys.exit("FAILED on %s: reason %s, worst status %s" % (name, m.group(1), m.group(2)))
            inputs += int(re.search(r"(\d+) inputs,", r.stdout).group(1))
    print("clean: %d files, the smallest accepted ones (%s) cut at every length, %d mutations each, %d inputs, no sanitizer report"
          % (len(names), ", ".join(smallest), a.mutations, inputs))


if __name__ == "__main__":
    main()
