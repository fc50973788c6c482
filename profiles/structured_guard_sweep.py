"""The bound of the structured solve's guard (csrc/se3_math.h kStructuredSolveBound) against how far the frame
is from the origin: for each bound 2^-e, se3_math.h is compiled for the host with that bound and random weighted
frames (tests/test_structured_solve.py) at growing offsets are solved both ways — how many the guard accepts,
and the worst relative difference to ldlt_solve6 among those.  CPU only.
    python profiles/structured_guard_sweep.py"""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_structured_solve as T  # noqa: E402

tmp = tempfile.mkdtemp()
for e in (12, 16, 20, 24, 30):
    d = os.path.join(tmp, "h%d" % e)
    shutil.copytree(os.path.join(ROOT, "sage-icp_amd", "csrc"), d)
    p = os.path.join(d, "se3_math.h")
    s = open(p).read()
    assert "kStructuredSolveBound = 1.0 / 65536.0" in s
    open(p, "w").write(s.replace("kStructuredSolveBound = 1.0 / 65536.0", "kStructuredSolveBound = %r" % (2.0 ** -e)))
    open(os.path.join(d, "w.cpp"), "w").write(T.SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I", d,
                           os.path.join(d, "w.cpp"), "-o", os.path.join(d, "l.so")])
    L = C.CDLL(os.path.join(d, "l.so"))
    dp = C.POINTER(C.c_double)
    for f in (L.sst_structured, L.sst_solve, L.sst_ldlt):
        f.argtypes = [dp, dp]
    for off in (0.0, 1e2, 1e3, 1e4, 1e5):
        rng = np.random.default_rng(7)
        worst, acc = 0.0, 0
        for n in (6, 10, 100, 1000, 20000):
            for k in range(20):
                S = T.sums(*T.frame(rng, n, rng.normal(size=3) * off))
                xl, _ = T._call(L.sst_ldlt, S)
                xs, ok = T._call(L.sst_structured, S)
                if ok:
                    acc += 1
                    worst = max(worst, np.linalg.norm(xs - xl) / np.linalg.norm(xl))
        print("2^-%d offset %g m: accepted %d/100, worst relative difference %.2e" % (e, off, acc, worst), flush=True)
shutil.rmtree(tmp, ignore_errors=True)
