"""Build the host pass of csrc/step_tail.hip (with csrc/api.hip for the error text) under AddressSanitizer + UBSan, link it with
tools/dev/step_tail_host_check.cpp and run that program: the size getters and every argument check of the step tail's entry points
(null pointers, NL = 0, negative counts, misaligned tables), each of which must return its error code before anything reaches a
device.  CPU only (a stand-alone program run as a child; nothing is loaded into Python) -- never run it on a GPU machine.

    python tools/dev/step_tail_host_check.py [--hipcc /opt/rocm/bin/hipcc]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    a = ap.parse_args()
    csrc = os.path.join(ROOT, "mgnns_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for name in ("step_tail.hip", "api.hip"):
            obj = os.path.join(tmp, name[:-4] + ".o")
            cmd = [a.hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off"] + SAN + ["-c", os.path.join(csrc, name), "-o", obj]
            print(" ".join(cmd))
            subprocess.check_call(cmd)
            objs.append(obj)
        # the program itself is plain C++: compiled and linked by the host compiler hipcc drives, so that no device code is instrumented
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(a.hipcc)))
        cxx = os.path.join(rocm, "lib", "llvm", "bin", "clang++")
        exe = os.path.join(tmp, "step_tail_host_check")
        cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               os.path.join(ROOT, "tools", "dev", "step_tail_host_check.cpp")] + objs + \
              ["-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe]
        print(" ".join(cmd))
        subprocess.check_call(cmd)
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout.strip())
        if r.returncode != 0 or "clean:" not in r.stdout:
            sys.exit("FAILED (exit status %d)" % r.returncode)


if __name__ == "__main__":
    main()
