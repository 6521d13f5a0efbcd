"""Build tools/dev/jpeg_host_check.cpp with the host compiler under AddressSanitizer + UBSan and run it over every file of
tests/golden/jpeg_decode.npz: the accepted ones must give Pillow's pixels, the two smallest files and the two smallest accepted ones are cut at every length, and every file
takes 10 000 seeded mutations.  CPU only (a stand-alone program; nothing is loaded into Python) -- never run it on a GPU machine.

    python tools/dev/jpeg_host_check.py [--mutations 10000] [--cxx c++]
"""
import argparse
import os
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
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "jpeg_host_check")
        cmd = [a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
               os.path.join(ROOT, "tools", "dev", "jpeg_host_check.cpp"), "-o", exe]
        print(" ".join(cmd))
        subprocess.check_call(cmd)
        names = [k[5:] for k in g if k.startswith("file_")]
        by_size = sorted(names, key=lambda k: g["file_" + k].size)
        smallest = by_size[:2] + [k for k in by_size if "pix_" + k in g][:2]          # of all files, and of the accepted ones
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
    print("clean: %d files, the smallest (%s) cut at every length, %d mutations each, no sanitizer report" % (len(names), ", ".join(smallest), a.mutations))


if __name__ == "__main__":
    main()
