"""Builds the TEST-ONLY device probe, tests/device_probe/_build/libzr_probe.so (git-ignored): probe.hip's kernels call the product's device
functions (csrc/zr_math.h, zr_dev.h, zr_shade.h) one case per thread, so tests/test_gpu_device_functions.py can hold each to the CPU oracle.

The compile flags are the product's own (zeldaengine_amd.build.FLAGS): -ffp-contract=off and -fno-fast-math are the numerics contract, and
a probe compiled otherwise would test another arithmetic.  It is linked like the product: plain g++ against libamdhip64's SONAME, so in a
torch process it binds to the HIP runtime already loaded.  zeldaengine_amd/ never names this directory.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "_build")
LIB = os.path.join(OUT, "libzr_probe.so")
SRC = os.path.join(HERE, "probe.hip")


def stale():
    from zeldaengine_amd import build as zbuild
    return not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in zbuild._deps(SRC) | {os.path.abspath(__file__)})


def build(force=False):
    from zeldaengine_amd import build as zbuild
    if not force and not stale():
        return LIB
    os.makedirs(OUT, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.join(OUT, "probe.o")
    subprocess.check_call([hipcc, "-x", "hip"] + zbuild.FLAGS + ["-c", SRC, "-o", obj])
    hip_dir = "/opt/rocm/lib"
    try:
        import torch
        cand = os.path.join(os.path.dirname(torch.__file__), "lib")
        if os.path.exists(os.path.join(cand, "libamdhip64.so")):
            hip_dir = cand
    except Exception:      # noqa: BLE001
        pass
    subprocess.check_call(["g++", "-shared", "-fPIC", "-o", LIB, obj, "-L" + hip_dir, "-l:libamdhip64.so", "-Wl,-rpath,/opt/rocm/lib",
                           "-Wl,--no-as-needed", "-lpthread", "-ldl"])
    return LIB


if __name__ == "__main__":
    print(build(force=True))
