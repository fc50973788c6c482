"""One Gauss-Newton step against extended precision, on the host: the truth against itself (tests/gnref.py), the fp64
oracle within the truth's error budget on every pair set and scene of tests/gnstep_cases.py (its worst ratio over the
detector cases is RHO_REF, from which the GPU tests' bound TAU follows), two deliberately wrong restatements that must
exceed the budget on every detector case, and csrc/se3_math.h compiled by g++ (solve_normal_equations + se3_exp over the
exact sums rounded once).  CPU only; prints the figures it asserts on (run with -s to see them)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import gnref
import gnstep_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sage-icp_amd", "csrc")
U = gnref.U
TINY = Fraction(1, 1 << (gnref.FRAC - 40))       # what the fixed point's own roundings may leave


# ---- gnref against itself ---------------------------------------------------------------------------------------------
def test_pure_translation_of_a_symmetric_cloud():
    rng = np.random.default_rng(1)
    half = np.round(rng.normal(scale=10.0, size=(20, 3)) * 1024.0) / 1024.0
    s = np.concatenate([half, -half])
    d = np.array([0.25, -0.125, 0.0625])
    q = s + d
    assert np.array_equal(q - s, np.broadcast_to(d, s.shape))          # (multiples of 2^-10: the sum is exact)
    st = gnref.Step(s, q, 1 / 3)
    assert st.full_rank
    for got, want in zip(st.x, list(d) + [0, 0, 0]):
        assert abs(got - Fraction(float(want))) < TINY
    assert all(abs(st.t[i] - Fraction(float(d[i]))) < TINY for i in range(3))
    assert all(abs(st.R[i][j] - int(i == j)) < TINY for i in range(3) for j in range(3))


def test_zero_residual_is_the_identity():
    rng = np.random.default_rng(2)
    s = rng.normal(scale=10.0, size=(30, 3)) + [4321.0, -2750.0, 12.0]
    st = gnref.Step(s, s, 1 / 3)
    assert st.full_rank and all(v == 0 for v in st.b) and all(v == 0 for v in st.x)
    assert st.R == [[int(i == j) for j in range(3)] for i in range(3)] and st.t == [0, 0, 0] and st.theta == 0.0
    assert st.ratio(np.array([0, 0, 0, 1.0, 0, 0, 0]), gnref.spread(s.mean(0), 10.0), 16 * U) == 0.0


def test_one_pair():
    s, q = np.array([[3.0, -2.0, 0.5]]), np.array([[3.25, -2.5, 0.75]])
    st = gnref.Step(s, q, 0.5)
    assert not st.full_rank and st.n == 1
    r = s[0] - q[0]
    w = Fraction(1, 4) / (Fraction(1, 2) + sum(Fraction(float(v)) ** 2 for v in r)) ** 2
    assert abs(st.A[0][0] - w) < TINY and abs(st.A[0][4] - w * Fraction(0.5)) < TINY and abs(st.b[1] - w * Fraction(0.5)) < TINY
    assert abs(st.A[3][3] - w * (4 + Fraction(1, 4))) < TINY and abs(st.EA[3][4] - w * 6) < TINY
    # the translation by -r solves the normal equations; nothing else is asked of a rank-3 system
    assert st.residual_ratio([-float(v) for v in r] + [0, 0, 0], 16 * U) < 1e-100
    assert st.residual_ratio([0, 0, 0, 0, 0, 0], 16 * U) > 1e10


def test_multiplicities_equal_explicit_tiling():
    s, q, k, (bs, bq), mult, pts = cases.pair_case("km4", 3 * cases.BASE + 100)
    explicit = gnref.Step(s, q, k)
    tiled = gnref.Step(bs, bq, k, mult)
    assert explicit.n == tiled.n == 3 * cases.BASE + 100 and sum(mult) == explicit.n
    for i in range(6):
        assert abs(explicit.x[i] - tiled.x[i]) < TINY * 10 ** 12
        for j in range(6):
            assert abs(explicit.A[i][j] - tiled.A[i][j]) < TINY and abs(explicit.EA[i][j] - tiled.EA[i][j]) < TINY


def test_exponential_and_logarithm():
    # a rotation about z with a translation along z commutes: R = Rz(th), t = u
    R, t, th = gnref.exp_se3([Fraction(0), Fraction(0), Fraction(3, 2), Fraction(0), Fraction(0), Fraction(7, 10)])
    assert th == 0.7 and abs(float(R[0][0]) - math.cos(0.7)) < 2 * U and abs(float(R[1][0]) - math.sin(0.7)) < 2 * U
    assert abs(R[0][0] ** 2 + R[1][0] ** 2 - 1) < TINY and t[0] == 0 and t[1] == 0 and abs(t[2] - Fraction(3, 2)) < TINY
    # exp(log(T)) acts as T does, for a pose of fp64 numbers with a quaternion that is not quite a unit
    T = np.array([0.01, -0.02, 0.03, 0.9993, 4.0, -5.0, 6.0])
    x = gnref.log_se3(T)
    Rx, tx, _ = gnref.exp_se3(x)
    Tn = T.copy()
    Rn, tn = gnref.pose_parts(Tn)
    n2 = sum(Fraction(float(v)) ** 2 for v in T[:4])
    # (pose_parts does not renormalise: R_n = I + (R - I) / |q|^2)
    for i in range(3):
        assert abs(tx[i] - tn[i]) < TINY * 10 ** 6
        for j in range(3):
            assert abs(Rx[i][j] - (int(i == j) + (Rn[i][j] - int(i == j)) / n2)) < TINY * 10 ** 6


# ---- the oracle within budget; the wrong restatements outside it -----------------------------------------------------
def _report(title, rows):
    print("\n" + title)
    for name, fig in rows.items():
        print("  %-12s %s" % (name, "  ".join("%s=%.3g" % kv for kv in fig.items())))


@pytest.fixture(scope="module")
def pair_figures(oracle):
    """per pair set: the oracle's worst ratios, and the smallest ratio of each wrong restatement, over the sizes"""
    fig = {}
    for name, kernel, _ in cases.PAIR_SETS:
        f = dict(oracle=0.0, oracle_sums=0.0, oracle_residual=0.0, weight=math.inf, sign=math.inf)
        for n in cases.PAIR_N:
            s, q, k, (bs, bq), mult, pts = cases.pair_case(name, n)
            st = cases.pair_truth(name, n)
            T, JTJ, JTr = oracle.align_clouds(s, q, k, nthreads=1)
            g = gnref.gamma_serial(n)
            f["oracle_sums"] = max(f["oracle_sums"], st.sums_ratio(JTJ, JTr, g))
            if not st.full_rank:
                if st.turn < cases.MAX_TURN:
                    f["oracle_residual"] = max(f["oracle_residual"], st.residual_ratio(gnref.log_se3(T), g, of_pose=True))
                continue
            f["oracle"] = max(f["oracle"], st.ratio(T, pts, g))
            if n in (3, 7, cases.BASE, cases.PAIR_N[-1]):
                gd = gnref.gamma_partials(n)                 # the budget the device is held to
                for v in ("weight", "sign"):
                    bad = gnref.Step(bs, bq, k, mult, variant=v)
                    f[v] = min(f[v], st.ratio((bad.R, bad.t), pts, gd))
        fig[name] = f
    _report("pair sets: the oracle's worst error / budget, the wrong restatements' smallest", fig)
    return fig


@pytest.fixture(scope="module")
def scene_figures(oracle):
    fig = {}
    for name, kernel, _ in cases.SCENES:
        f = dict(oracle=0.0, weight=math.inf, sign=math.inf, theta_min=math.inf, theta_max=0.0, clear=1.0)
        for n in cases.FRAMES:
            sc = cases.Scene(oracle, name, n)
            st = sc.truth1
            f["clear"] = min(f["clear"], float(sc.clear1))
            T, stats = sc.om.register_frame(sc.frame, sc.guess, cases.MAX_DIST, sc.kernel, cases.SEM_TH, nthreads=1, max_iter=1)
            assert stats.n_corr_first == st.n
            if not st.full_rank:
                assert st.n == 0 and np.array_equal(T, sc.guess)
                continue
            # (the oracle composes est * identity and then * guess: the budget of se3_mul for every scene with a guess)
            f["oracle"] = max(f["oracle"], st.ratio(T, sc.points, gnref.gamma_serial(st.n), guess=sc.guess, extra=sc.extra1()))
            f["theta_min"], f["theta_max"] = min(f["theta_min"], st.theta), max(f["theta_max"], st.theta)
            for v in ("weight", "sign"):
                bad = gnref.Step(*sc.pairs1, sc.kernel, variant=v)
                wrong = gnref.compose((bad.R, bad.t), gnref.pose_parts(sc.guess))
                f[v] = min(f[v], st.ratio(wrong, sc.points, gnref.GAMMA_EPILOGUE, guess=sc.guess, extra=sc.extra1()))
            # iteration 2, after the oracle's own first pose: its budget is the wider one (every s perturbed by 4u |s|)
            if sc.two_iterations():
                P1 = np.array(T)
                P2, _ = sc.om.register_frame(sc.frame, sc.guess, cases.MAX_DIST, sc.kernel, cases.SEM_TH, nthreads=1, max_iter=2)
                st2, clear2 = sc.truth2(P1)
                f["clear"] = min(f["clear"], float(clear2))
                f["oracle2"] = max(f.get("oracle2", 0.0), sc.ratio2(P1, P2, gnref.gamma_serial(st2.n)))
                src2, tgt2, _ = cases.pairs_clear_of_edge(sc.om, sc.oracle.transform_points(P1, sc.frame))
                for v in ("weight", "sign"):
                    bad = gnref.Step(src2, tgt2, sc.kernel, variant=v)
                    wrong = gnref.compose((bad.R, bad.t), gnref.pose_parts(P1))
                    f[v + "2"] = min(f.get(v + "2", math.inf), sc.ratio2(P1, wrong, gnref.GAMMA_EPILOGUE))
        fig[name] = f
    _report("scenes, iterations 1 and 2: the oracle's worst error / budget, the wrong restatements' smallest", fig)
    return fig


def test_oracle_within_budget_and_rho_ref(pair_figures, scene_figures):
    rho = 0.0
    for fig, detector in ((pair_figures, cases.PAIR_DETECTOR), (scene_figures, cases.SCENE_DETECTOR)):
        for name, f in fig.items():
            assert f["oracle"] <= 1.0 and f.get("oracle2", 0.0) <= 1.0, (name, f)
            assert f.get("oracle_sums", 0.0) <= 1.0 and f.get("oracle_residual", 0.0) <= 1.0, (name, f)
            if detector[name]:
                rho = max(rho, f["oracle"], f.get("oracle2", 0.0))
    tau = min(1.0, 2.0 ** math.ceil(math.log2(4 * rho)))
    print("\nrho_ref = %.4g (recorded %.4g), tau = %g (recorded %g)" % (rho, cases.RHO_REF, tau, cases.TAU))
    assert rho <= cases.RHO_REF and tau == cases.TAU == min(1.0, 2.0 ** math.ceil(math.log2(4 * cases.RHO_REF)))


def test_wrong_restatements_exceed_the_budget_on_every_detector(pair_figures, scene_figures):
    for fig, detector in ((pair_figures, cases.PAIR_DETECTOR), (scene_figures, cases.SCENE_DETECTOR)):
        for name, f in fig.items():
            if detector[name]:
                assert f["weight"] > 1.0 and f["sign"] > 1.0, (name, f)
                assert f.get("weight2", math.inf) > 1.0 and f.get("sign2", math.inf) > 1.0, (name, f)      # (scenes: iteration 2)
    # these stay detectors, whatever else is added
    for name in ("origin", "km4", "km12"):
        assert cases.PAIR_DETECTOR[name] and cases.SCENE_DETECTOR[name]
    assert cases.SCENE_DETECTOR["trans"]


def test_no_pair_at_the_edge_of_the_search_radius(scene_figures):
    assert all(f["clear"] == 1.0 for f in scene_figures.values())


# ---- se3_math.h by g++ ------------------------------------------------------------------------------------------------
SRC = r'''
#include "se3_math.h"
using namespace sageicp;
extern "C" void gns_step(const double *S, double *x, double *T) { solve_normal_equations(S, x); se3_exp(x, T); }
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile se3_math.h for the host")
    d = tmp_path_factory.mktemp("gns")
    src, out = d / "gns.cpp", d / "libgns.so"
    src.write_text(SRC)
    # the flags of the product's fp64 arithmetic (build.py): no contraction into fused multiply-adds
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(out)])
    L = C.CDLL(str(out))
    dp = C.POINTER(C.c_double)
    L.gns_step.argtypes = [dp, dp, dp]
    return L


def _host_step(lib, st):
    S = np.ascontiguousarray(st.sums16())
    x, T = np.zeros(6), np.zeros(7)
    dp = C.POINTER(C.c_double)
    lib.gns_step(S.ctypes.data_as(dp), x.ctypes.data_as(dp), T.ctypes.data_as(dp))
    return x, T


@pytest.mark.parametrize("name", [s[0] for s in cases.PAIR_SETS])
def test_host_solve_and_exp_within_budget(lib, name):
    """the sums are exact but for one rounding each: what is left of the budget is the solve and the exponential"""
    worst = worst_res = 0.0
    for n in cases.PAIR_N:
        st = cases.pair_truth(name, n)
        x, T = _host_step(lib, st)
        if st.full_rank:
            worst = max(worst, st.ratio(T, cases.pair_case(name, n)[5], gnref.GAMMA_EPILOGUE))
        else:
            worst_res = max(worst_res, st.residual_ratio(x, gnref.GAMMA_EPILOGUE))
    print("%s: solve_normal_equations + se3_exp by g++: error / budget %.3g, residual / bound %.3g" % (name, worst, worst_res))
    assert worst_res <= 1.0
    if name == "identical":
        assert np.array_equal(T, [0, 0, 0, 1, 0, 0, 0])
    if name != "utm":
        assert worst <= 1.0


def test_host_solve_on_scenes(lib, oracle):
    for name, _, _ in cases.SCENES:
        for n in (17, 1000):
            sc = cases.Scene(oracle, name, n)
            if not sc.truth1.full_rank:
                continue
            x, T = _host_step(lib, sc.truth1)
            ratio = sc.truth1.ratio(T, [p + sc.guess[4:] for p in sc.points], gnref.GAMMA_EPILOGUE)
            print("%s n=%d: error / budget %.3g" % (name, n, ratio))
            if name != "utm":
                assert ratio <= 1.0
