"""accept_threshold (csrc/accept.h: "the largest double whose IEEE sqrt is below max_dist") against exact arithmetic, and
the boundary scenes of tests/acceptscenes.py against the oracle.  CPU only.

The header is compiled by g++ into a small ctypes library, with the flags of the product's fp64 arithmetic.  The truth is
acceptscenes.threshold: fractions.Fraction, no square root.  Every comparison is for equality.

The scenes: each states, from its own arithmetic and the exact threshold, which rows are accepted and which map point
answers; the oracle — which takes the square root, sqrt(r2) < max_dist — must say the same before the GPU tests
(tests/test_accept_boundary_gpu.py) hold the library to the oracle.  Both follow SAGE_SQNORM3_ORDER."""
import ctypes as C
import math
import shutil
import subprocess
import os

import numpy as np
import pytest

import acceptscenes as acs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage-icp_amd", "csrc")
DBL_MAX = acs.DBL_MAX
DBL_MIN = float(np.finfo(np.float64).tiny)          # the smallest normal

SRC = r'''
#include "accept.h"
extern "C" double sat_accept_threshold(double max_dist) { return sageicp_impl::accept_threshold(max_dist); }
'''


@pytest.fixture(scope="module")
def accept_threshold(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile accept.h for the host")
    d = tmp_path_factory.mktemp("sat")
    src, out = d / "sat.cpp", d / "libsat.so"
    src.write_text(SRC)
    subprocess.check_call([cxx, "-std=c++17", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, str(src), "-o",
                           str(out)])
    L = C.CDLL(str(out))
    L.sat_accept_threshold.argtypes = [C.c_double]
    L.sat_accept_threshold.restype = C.c_double
    return L.sat_accept_threshold


def _same(fn, values):
    bad = [(m, fn(m), acs.threshold(m)) for m in values if fn(m) != acs.threshold(m)]
    assert not bad, bad[:5]


# ---- the truth itself: the characterisation agrees with the square root wherever the square root can be asked ---------------
def test_the_exact_threshold_is_where_the_ieee_sqrt_crosses():
    rng = np.random.default_rng(7)
    for m in [0.3, 0.7, 0.81, 0.9, 3.0, 6.0, 1e-3, 1e-7, 1e3, 4.0, 1e-150] + list(rng.uniform(0.01, 10.0, size=200)):
        t = acs.threshold(m)
        assert math.sqrt(t) < m and not math.sqrt(math.nextafter(t, math.inf)) < m, m


# ---- the function ------------------------------------------------------------------------------------------------------------
def test_the_values_the_suite_and_the_pipeline_use(accept_threshold):
    _same(accept_threshold, [0.3, 0.7, 0.81, 0.9, 3.0, 6.0, 1e-3, 1e-7, 1e3, 0.8, 0.25, 2.0, 2.0 / 3.0, 0.1, 0.4])


def test_random_doubles(accept_threshold):
    rng = np.random.default_rng(1)
    _same(accept_threshold, rng.uniform(0.01, 10.0, size=3000).tolist())


def test_random_mantissas_at_every_exponent(accept_threshold):
    rng = np.random.default_rng(2)
    _same(accept_threshold, [math.ldexp(1.0 + rng.random(), e) for e in range(-40, 41) for _ in range(10)])
    # ... and the ends of every binade: 2^e, its two neighbours
    ends = [math.ldexp(1.0, e) for e in range(-40, 41)]
    _same(accept_threshold, ends + [math.nextafter(x, 0.0) for x in ends] + [math.nextafter(x, math.inf) for x in ends])


def test_perfect_squares_and_their_neighbours(accept_threshold):
    """max_dist = k or k^2 (and k / 8, k^2 / 64): max_dist^2 is exact, its root is max_dist itself and does not pass"""
    vals = []
    for k in range(1, 41):
        for x in (float(k), float(k * k), k / 8.0, k * k / 64.0):
            vals += [x, math.nextafter(x, 0.0), math.nextafter(x, math.inf)]
    _same(accept_threshold, vals)
    for k in (1.0, 2.0, 3.0, 0.5, 7.0):
        assert accept_threshold(k) == math.nextafter(k * k, 0.0)


def test_tiny_radii(accept_threshold):
    _same(accept_threshold, [1e-150, 1e-170, DBL_MIN, math.nextafter(DBL_MIN, 1.0), 1e-160, 1.5e-154, 1e-162])
    # the square underflows: only a distance of exactly zero passes
    assert accept_threshold(1e-170) == 0.0 and accept_threshold(DBL_MIN) == 0.0


def test_huge_radii_accept_every_finite_distance(accept_threshold):
    for m in (1e200, math.inf, DBL_MAX, 1e155):
        assert accept_threshold(m) == DBL_MAX, m
        assert acs.threshold(m) == DBL_MAX
    # 1e150 squares to a finite double (1e300): the threshold there is an ordinary one, not DBL_MAX
    assert accept_threshold(1e150) == acs.threshold(1e150) < DBL_MAX
    _same(accept_threshold, [1e150, 1e153, 1.3e154, 1.34e154, 1.35e154])


def test_nothing_passes_a_radius_that_is_not_positive(accept_threshold):
    for m in (0.0, -0.0, -1.0, -math.inf, math.nan):
        assert accept_threshold(m) == -1.0
        assert acs.threshold(m) == -1.0


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
CASES = [(name, None) for name in acs.CONFIGS] + [("v1.0_d0.7", acs.POSE)]


@pytest.mark.parametrize("name,pose", CASES, ids=[n + ("" if p is None else "-posed") for n, p in CASES])
def test_the_oracle_answers_the_scene_as_its_arithmetic_says(oracle, name, pose):
    sc = acs.scene(name, pose)                    # (its own preconditions are asserted as it is built)
    om = oracle.Map(sc.voxel, 100.0)
    om.add_points(sc.map)
    n = max(sc.sizes)
    want = sc.expect(n)
    src, tgt, idx = om.get_correspondences(sc.moved[:n], sc.max_dist, sc.sem_th, with_index=True)
    print(name, "rows", len(sc.rows), "accepted %.3f" % sc.accept.mean(), "r2 == T", int((sc.r2 == sc.T).sum()),
          "r2 == next(T)", int((sc.r2 == np.nextafter(sc.T, np.inf)).sum()), "deciders", int(sc.deciders().sum()))
    assert np.array_equal(idx, want[2])
    assert np.array_equal(src, want[0]) and np.array_equal(tgt, want[1])


def test_the_deciders_decide(oracle):
    """the rows whose two associations land on different sides of T: evaluated the other way, the answer differs at them
    and nowhere else — what the run of these tests on the other build (tests/test_sqnorm3_variant.py) relies on"""
    sc = acs.scene("v1.0_d0.7")
    d = sc.moved[:, :3] - sc.own[:, :3]
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    a, b = xx + (yy + zz), (xx + yy) + zz
    mine, other = (a, b) if acs.SQNORM3_ORDER == 0 else (b, a)
    assert np.array_equal(mine, sc.r2) and np.array_equal(other, sc.r2_other)
    assert np.array_equal((mine <= sc.T) != (other <= sc.T), sc.deciders()) and sc.deciders().sum() >= 20
