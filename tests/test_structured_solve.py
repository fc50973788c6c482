"""The block-structured solve of the normal equations (csrc/se3_math.h structured_solve_t) against the
generic 6x6 LDL^T it replaces on the device (ldlt_solve6): the header compiled by g++ into a small
ctypes library.  Well-posed systems agree to 1e-10 relative; wherever the guard refuses a system, the
answer of solve_normal_equations is ldlt_solve6's bit for bit.  CPU only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage-icp_amd", "csrc")

SRC = r'''
#include "se3_math.h"
using namespace sageicp;
extern "C" int sst_structured(const double *S, double *x) { return structured_solve(S, x) ? 1 : 0; }
extern "C" void sst_solve(const double *S, double *x) { solve_normal_equations(S, x); }
extern "C" void sst_ldlt(const double *S, double *x) {
    double JTJ[36], JTr[6], neg[6];
    assemble_normal_equations(S, JTJ, JTr);
    for (int i = 0; i < 6; ++i) neg[i] = -JTr[i];
    ldlt_solve6(JTJ, neg, x);
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile se3_math.h for the host")
    d = tmp_path_factory.mktemp("sst")
    src, out = d / "sst.cpp", d / "libsst.so"
    src.write_text(SRC)
    # the flags of the product's fp64 arithmetic (build.py): no contraction into fused multiply-adds
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC,
                           str(src), "-o", str(out)])
    L = C.CDLL(str(out))
    dp = C.POINTER(C.c_double)
    L.sst_structured.argtypes = [dp, dp]
    L.sst_structured.restype = C.c_int
    L.sst_solve.argtypes = [dp, dp]
    L.sst_ldlt.argtypes = [dp, dp]
    return L


def _call(fn, S):
    S = np.ascontiguousarray(S, dtype=np.float64)
    x = np.zeros(6)
    r = fn(S.ctypes.data_as(C.POINTER(C.c_double)), x.ctypes.data_as(C.POINTER(C.c_double)))
    return x, r


def sums(s, q, w):
    """the 16 closed-form sums of sageicp_types.h (Sum) of source points s, targets q, weights w"""
    r = s - q
    S = np.zeros(20)
    S[0] = w.sum()
    S[1:4] = (w[:, None] * s).sum(0)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    S[4:10] = [np.sum(w * x * x), np.sum(w * x * y), np.sum(w * x * z), np.sum(w * y * y), np.sum(w * y * z),
               np.sum(w * z * z)]
    S[10:13] = (w[:, None] * r).sum(0)
    S[13:16] = (w[:, None] * np.cross(s, r)).sum(0)
    S[16] = len(s)
    return S


def frame(rng, n, offset, spread=30.0, noise=0.05):
    s = rng.normal(scale=spread, size=(n, 3)) * [1.0, 1.0, 0.2] + offset
    q = s + rng.normal(scale=noise, size=(n, 3)) + [0.02, -0.01, 0.005]
    w = rng.uniform(0.05, 1.0, size=n)
    return s, q, w


def check(lib, S):
    """-> whether the guard accepted; asserts the contract either way"""
    xl, _ = _call(lib.sst_ldlt, S)
    xs, ok = _call(lib.sst_structured, S)
    x, _ = _call(lib.sst_solve, S)
    if ok:
        assert np.array_equal(x, xs)
        assert np.linalg.norm(xs - xl) <= 1e-10 * np.linalg.norm(xl), (xs, xl)
    else:
        assert np.array_equal(x, xl)          # the fall-back, bit for bit
    return bool(ok)


@pytest.mark.parametrize("offset", [0.0, 1e2, 1e4])
@pytest.mark.parametrize("n", [6, 10, 100, 1000, 100_000])
def test_well_posed_systems_agree(lib, n, offset):
    rng = np.random.default_rng(n + int(offset))
    accepted = 0
    for k in range(20):
        off = rng.normal(size=3) * offset
        accepted += check(lib, sums(*frame(rng, n, off)))
    if offset <= 1e2:
        assert accepted == 20        # near the origin every such frame takes the structured solve


def test_no_pairs_is_zero(lib):
    S = np.zeros(20)
    x, ok = _call(lib.sst_structured, S)
    assert not ok
    x, _ = _call(lib.sst_solve, S)
    assert np.array_equal(x, np.zeros(6))
    check(lib, S)


@pytest.mark.parametrize("offset", [0.0, 1e2, 1e4])
def test_one_point_falls_back(lib, offset):
    rng = np.random.default_rng(1)
    for _ in range(10):
        s, q, w = frame(rng, 1, rng.normal(size=3) * offset)
        S = sums(s, q, w)
        assert not check(lib, S)


@pytest.mark.parametrize("offset", [0.0, 1e2, 1e4])
def test_collinear_points_fall_back(lib, offset):
    rng = np.random.default_rng(2)
    for n in (2, 3, 50, 5000):
        d = rng.normal(size=3)
        s = rng.normal(size=(n, 1)) * 20.0 * d / np.linalg.norm(d) + rng.normal(size=3) * offset
        q = s + rng.normal(scale=0.05, size=(n, 3))
        w = rng.uniform(0.05, 1.0, size=n)
        assert not check(lib, sums(s, q, w))


@pytest.mark.parametrize("offset", [0.0, 1e2, 1e4])
def test_exactly_planar_points(lib, offset):
    """point-to-point ICP on a plane is still well posed (the inertia of a lamina is not singular)"""
    rng = np.random.default_rng(3)
    for n in (3, 10, 1000, 50_000):
        s = np.zeros((n, 3))
        s[:, :2] = rng.uniform(-40, 40, size=(n, 2))
        s += np.array([1.0, -2.0, 0.0]) * offset
        q = s + rng.normal(scale=0.05, size=(n, 3))
        w = rng.uniform(0.05, 1.0, size=n)
        ok = check(lib, sums(s, q, w))
        if offset == 0.0:
            assert ok


def test_frame_at_utm_coordinates_falls_back(lib):
    """4e6 m northing, tens of metres of spread: S_ii keeps fewer than 2^-16 of M_ii's bits"""
    rng = np.random.default_rng(4)
    for n in (10, 1000, 100_000):
        s, q, w = frame(rng, n, np.array([5e5, 4e6, 0.0]))
        assert not check(lib, sums(s, q, w))


def test_non_finite_sums_fall_back(lib):
    rng = np.random.default_rng(5)
    S = sums(*frame(rng, 100, np.zeros(3)))
    for k in (0, 1, 4, 10, 13):
        for v in (np.nan, np.inf):
            T = S.copy()
            T[k] = v
            xs, ok = _call(lib.sst_structured, T)
            assert not ok
            x, _ = _call(lib.sst_solve, T)
            xl, _ = _call(lib.sst_ldlt, T)
            assert np.array_equal(x, xl, equal_nan=True)
