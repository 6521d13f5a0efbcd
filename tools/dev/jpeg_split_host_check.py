"""Build tools/dev/jpeg_split_host_check.cpp with the host compiler under AddressSanitizer + UBSan and run it over every baseline
file of tests/golden/jpeg_decode.npz and tests/golden/jpeg_split.npz with chunk sizes 8 and 64: every input must decode to the
serial decoder's coefficients and status byte for byte, the accepted ones to Pillow's pixels; the two smallest accepted files are
cut at every length, and every file takes 10 000 seeded mutations per chunk size.  CPU only (a stand-alone program run as a
child; nothing is loaded into Python) -- never run it on a GPU machine.

    python tools/dev/jpeg_split_host_check.py [--mutations 10000] [--lanes 1024] [--cxx c++]
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
    ap.add_argument("--lanes", default="1024")
    ap.add_argument("--cxx", default=os.environ.get("CXX", "c++"))
    a = ap.parse_args()
    g = {}
    for f in ("jpeg_decode.npz", "jpeg_split.npz"):
        g.update(np.load(os.path.join(ROOT, "tests", "golden", f)))
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "jpeg_split_host_check")
        cmd = [a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wno-unknown-pragmas",
               os.path.join(ROOT, "tools", "dev", "jpeg_split_host_check.cpp"), "-o", exe]
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
            r = subprocess.run(args + ["--chunks", "8,64", "--lanes", a.lanes, "--mutations", str(a.mutations)], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True)
            print(r.stdout.strip().replace(tmp + os.sep, ""))
            if r.returncode != 0:
                sys.exit("FAILED on %s (exit status %d)" % (name, r.returncode))
            inputs += int(r.stdout.split(" inputs equal")[0].split()[-1])
    print("clean: %d files, the smallest accepted ones (%s) cut at every length, %d mutations each per chunk size, %d inputs, "
          "all equal to the serial decoder, no sanitizer report" % (len(names), ", ".join(smallest), a.mutations, inputs))


if __name__ == "__main__":
    main()
