"""ctypes front of tests/deskew_ref.cpp, the independent CPU restatement of DeSkewScan (core/Deskew.cpp:31-50) and of
the Sophus SE(3) arithmetic it uses.  Compiled once per process with g++ -O2 -ffp-contract=off into a temporary
directory (nothing is written into the tree)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "deskew_ref.cpp")
_lib = []
_dp = C.POINTER(C.c_double)


def lib():
    if not _lib:
        d = tempfile.mkdtemp(prefix="deskewref_")
        so = os.path.join(d, "deskewref.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra",
                               "-Werror", SRC, "-o", so])
        L = C.CDLL(so)
        for name, args in (("dsr_exp", [_dp, _dp]), ("dsr_log", [_dp, _dp]), ("dsr_inv", [_dp, _dp]),
                           ("dsr_mul", [_dp, _dp, _dp]), ("dsr_apply", [_dp, _dp, _dp]),
                           ("dsr_delta", [_dp, _dp, _dp]),
                           ("dsr_deskew_delta", [_dp, _dp, C.c_uint64, _dp, _dp]),
                           ("dsr_deskew", [_dp, _dp, C.c_uint64, _dp, _dp, _dp])):
            fn = getattr(L, name)
            fn.restype = None
            fn.argtypes = args
        _lib.append(L)
    return _lib[0]


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _unary(name, x, m):
    x, xp = _d(x)
    o = np.empty(m)
    getattr(lib(), name)(xp, o.ctypes.data_as(_dp))
    return o


def exp(a):
    return _unary("dsr_exp", a, 7)


def log(T):
    return _unary("dsr_log", T, 6)


def inv(T):
    return _unary("dsr_inv", T, 7)


def mul(A, B):
    A, ap = _d(A)
    B, bp = _d(B)
    o = np.empty(7)
    lib().dsr_mul(ap, bp, o.ctypes.data_as(_dp))
    return o


def apply(T, p):
    T, tp = _d(T)
    p, pp = _d(p)
    o = np.empty(3)
    lib().dsr_apply(tp, pp, o.ctypes.data_as(_dp))
    return o


def delta(start, finish):
    """(start.inverse() * finish).log()"""
    a, ap = _d(start)
    b, bp = _d(finish)
    o = np.empty(6)
    lib().dsr_delta(ap, bp, o.ctypes.data_as(_dp))
    return o


def deskew(frame, timestamps, start, finish):
    """DeSkewScan(frame, timestamps, start, finish)"""
    f, fp = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 4))
    t, tp = _d(timestamps)
    assert t.size == len(f)
    a, ap = _d(start)
    b, bp = _d(finish)
    out = np.empty((len(f), 4))
    lib().dsr_deskew(fp, tp, len(f), ap, bp, out.ctypes.data_as(_dp))
    return out


def deskew_delta(frame, timestamps, delta_):
    """DeSkewScan's per-point step with a given tangent"""
    f, fp = _d(np.asarray(frame, dtype=np.float64).reshape(-1, 4))
    t, tp = _d(timestamps)
    assert t.size == len(f)
    d, dp = _d(delta_)
    out = np.empty((len(f), 4))
    lib().dsr_deskew_delta(fp, tp, len(f), dp, out.ctypes.data_as(_dp))
    return out
