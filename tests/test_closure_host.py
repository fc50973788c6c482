"""The corrections of a loop closure on the CPU (include/sageicp.h "loop closure"): the symbols and the struct,
the two exact ends, the shares of path length, every refusal, translation equivariance, and C_k / poses_out against the
restatement (tests/closureref.py); the header shim's member.  Host arithmetic only: no test here needs a GPU.

Tolerances of the two comparisons that are not exact (MEASURED below).  The restatement is evaluated once in np.longdouble
(x87 extended, 64-bit mantissa) and once in np.float64, in the operation order of csrc/se3_math.h; the fp64 restatement's
own error against the extended one is measured over the cases of each group, for quaternion components and for
translation components apart, and the library is allowed FOUR times that against the extended restatement (its sin, cos
and atan2 are libm's, the restatement's numpy's: they differ by ulps).  Measured on the cases below:

    group    fp64 restatement vs extended (max abs)      the library vs extended (max abs)
             quaternion     translation [m]              quaternion     translation [m]
    local    2.29e-16       2.50e-14                     2.29e-16       2.50e-14
    utm      2.29e-16       2.37e-09                     2.29e-16       2.37e-09

(local: trajectories within 100 m of the origin; utm: the same shifted by (5e5, 5e6, 0), where one ulp of a coordinate
is 9.3e-10 m; every translation of the cases lies on a grid of 2^-10 m, so the shift is exact.)  The library's worst
difference from the extended evaluation equals the fp64 restatement's in both groups: it needed none of the factor
four.  The figures are recomputed by every run and printed; the bound is always 4 x the run's own measurement,
never these numbers."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import closureref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTM = np.array([5.0e5, 5.0e6, 0.0])


def _quat(rpy_deg):
    r, p, y = (math.radians(v) / 2.0 for v in rpy_deg)
    cr_, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    return np.array([sr * cp * cy - cr_ * sp * sy, cr_ * sp * cy + sr * cp * sy, cr_ * cp * sy - sr * sp * cy,
                     cr_ * cp * cy + sr * sp * sy])


def _grid(t):
    """translations on a grid of 2^-10 m: adding UTM to them is exact, so the shifted trajectory IS the same trajectory
    (its steps, and with them the shares of path length, have the same bits)"""
    return np.round(np.asarray(t, dtype=np.float64) * 1024.0) / 1024.0


def _pose(rpy_deg, t):
    return np.concatenate([_quat(rpy_deg), _grid(t)])


def _arc(n=40, seed=5):
    """a curved drive: the heading turns, the steps differ in length"""
    rng = np.random.default_rng(seed)
    poses, t, yaw = [], np.zeros(3), 0.0
    for k in range(n):
        poses.append(_pose((rng.normal(0, 0.5), rng.normal(0, 0.5), yaw), t))
        yaw += rng.uniform(2.0, 9.0)
        step = rng.uniform(0.5, 2.5)
        t = t + np.array([step * math.cos(math.radians(yaw)), step * math.sin(math.radians(yaw)), rng.normal(0, 0.02)])
    return np.array(poses)


def _closed_from(poses, j, rpy_deg, shift):
    """pose j moved by a small world-frame transform: what a relocalisation would say"""
    c = cr.se3_mul(_pose(rpy_deg, shift), poses[j])
    c[4:] = _grid(c[4:])
    return c


def _cases():
    arc = _arc()
    line = np.array([_pose((0, 0, 0), (1.5 * k, 0.0, 0.0)) for k in range(30)])
    still = np.array([_pose((0, 0, 3.0 * k), (4.0, -2.0, 1.0)) for k in range(12)])
    out = {
        "arc, drift in rotation and translation": (arc, 3, 36, _closed_from(arc, 36, (0.8, -0.6, 4.0), (1.7, -2.2, 0.3))),
        "arc, the whole trajectory": (arc, 0, 39, _closed_from(arc, 39, (0.0, 0.0, -7.0), (-3.0, 1.0, 0.0))),
        "line, translation only": (line, 2, 27, line[27] + np.array([0, 0, 0, 0, 0.875, -1.375, 0.25])),
        "line, a large turn": (line, 0, 29, _closed_from(line, 29, (0.0, 0.0, 150.0), (0.5, 0.5, 0.0))),
        "standing still: no path": (still, 2, 9, _closed_from(still, 9, (0.0, 0.0, 2.0), (0.3, 0.1, 0.0))),
        "neighbours": (arc, 10, 11, _closed_from(arc, 11, (0.0, 0.0, 0.5), (0.05, 0.0, 0.0))),
    }
    return out


CASES = _cases()


def _shifted(poses, closed):
    p, c = np.array(poses), np.array(closed)
    p[:, 4:] += UTM
    c[4:] += UTM
    return p, c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


_REF = {}


def _reference(name, utm):
    """the two restatements of a case, computed once"""
    key = (name, utm)
    if key not in _REF:
        poses, i, j, closed = CASES[name]
        if utm:
            poses, closed = _shifted(poses, closed)
        _REF[key] = (poses, i, j, closed, cr.corrections(poses, i, j, closed, np.float64),
                     cr.corrections(poses, i, j, closed, np.longdouble))
    return _REF[key]


def _err(a, ext):
    """(max abs over quaternion components, over translation components) of a against the extended evaluation"""
    d = np.abs(np.asarray(a, dtype=np.longdouble) - ext)
    return float(d[:, :4].max()), float(d[:, 4:].max())


def _measured(utm):
    """the fp64 restatement's own error over the group's cases: (quaternion, translation), C_k and poses_out together"""
    q = t = 0.0
    for name in CASES:
        _, _, _, _, r64, ext = _reference(name, utm)
        for field in ("C", "poses_out"):
            eq, et = _err(r64[field], ext[field])
            q, t = max(q, eq), max(t, et)
    return q, t


# ---- the entries ------------------------------------------------------------------------------------------------------
def test_symbols_and_struct(sage, tmp_path):
    lib = sage.lib()
    for name in ("sageicp_closure_corrections", "sageicp_map_session_stays", "sageicp_map_session_corrected",
                 "sageicp_map_session_corrected_device", "sageicp_pipeline_closure", "sageicp_pipeline_session_corrected",
                 "sageicp_pipeline_session_corrected_device"):
        assert getattr(lib, name)
    assert lib.sageicp_abi_version() == 4
    fields = ["delta", "angle", "shift", "path", "i", "j"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){printf("%zu", sizeof(sageicp_closure_info));'
           + "".join('printf(" %%zu", offsetof(sageicp_closure_info, %s));' % f for f in fields) + "return 0;}")
    exe = str(tmp_path / "closure_layout_probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(sage.ClosureInfo)] + [getattr(sage.ClosureInfo, f).offset for f in fields]
    assert got == [96, 0, 56, 64, 72, 80, 88]
    header = open(os.path.join(ROOT, "include", "sageicp.h")).read()
    for name in ("sageicp_closure_corrections(", "sageicp_map_session_stays(", "sageicp_map_session_corrected(",
                 "sageicp_map_session_corrected_device(", "sageicp_pipeline_closure(", "sageicp_pipeline_session_corrected(",
                 "sageicp_pipeline_session_corrected_device("):
        assert name in header, name
    for member in ("SessionStays", "CorrectedPointcloud"):
        assert callable(getattr(sage.VoxelHashMap, member))
    for member in ("Closure", "CorrectedSessionMap"):
        assert callable(getattr(sage.SageICP, member))


def test_shim_corrected_pointcloud_type_checks():
    """the CorrectedPointcloud member of the header shim against the stand-in Eigen (tests/shim_stubs)"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_stubs", "closure_user.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- what is exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_the_two_ends_are_exact(sage, name):
    poses, i, j, closed = CASES[name]
    C, out, info = sage.closure_corrections(poses, i, j, closed, return_info=True)
    identity = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    for k in range(i + 1):
        assert _bits(C[k]) == _bits(identity), k                 # (+0.0, not -0.0)
        assert _bits(out[k]) == _bits(poses[k]), k
    for k in range(j, len(poses)):
        assert _bits(C[k]) == _bits(info["delta"]), k
    assert (info["i"], info["j"]) == (i, j)
    # delta is formed with se3_mul and se3_inv: the restatement's bits (no libm call on the way)
    assert _bits(info["delta"]) == _bits(cr.corrections(poses, i, j, closed)["delta"])


@pytest.mark.parametrize("name", list(CASES))
def test_the_last_pose_lands_on_closed(sage, name):
    """poses_out[j] = (closed * poses[j]^-1) * poses[j]: closed to the accuracy of two products — a few ulps of the
    quaternion, and of the translation a few ulps of the largest term of the products (|t_j| + |closed.t|)"""
    poses, i, j, closed = CASES[name]
    _, out = sage.closure_corrections(poses, i, j, closed)
    u = 2.0 ** -53
    scale = 1.0 + np.abs(poses[j, 4:]).max() + np.abs(closed[4:]).max()
    assert np.abs(out[j, :4] - closed[:4]).max() <= 16 * u
    assert np.abs(out[j, 4:] - closed[4:]).max() <= 32 * u * scale


def _alpha_of(C_k, ref):
    """the share a correction was built with, read back: log(Tr(-c) C_k Tr(c)) = alpha * a"""
    c = ref["c"]
    u = cr.mat_apply(cr.quat_to_mat(C_k), C_k[4:], c)
    a_k = cr.se3_log(np.concatenate([C_k[:4], u - c]))
    return float(a_k @ ref["a"] / (ref["a"] @ ref["a"]))


@pytest.mark.parametrize("name", list(CASES))
def test_the_shares_of_path_length(sage, name):
    poses, i, j, closed = CASES[name]
    C, _, info = sage.closure_corrections(poses, i, j, closed, return_info=True)
    t = poses[:, 4:]
    steps = np.linalg.norm(t[i + 1:j + 1] - t[i:j], axis=1)
    total = steps.sum()
    want = np.cumsum(steps) / total if total > 0 else np.arange(1, j - i + 1) / (j - i)
    assert info["path"] == pytest.approx(total, rel=1e-13, abs=0.0)
    if name.startswith("standing still"):
        assert total == 0.0 and info["path"] == 0.0
    c = poses[j, 4:]
    delta = np.array(info["delta"])
    u = cr.mat_apply(cr.quat_to_mat(delta), delta[4:], c)
    a = cr.se3_log(np.concatenate([delta[:4], u - c]))
    ref = dict(c=c, a=a)
    assert info["angle"] == pytest.approx(np.linalg.norm(a[3:]), rel=1e-13)
    assert info["shift"] == pytest.approx(np.linalg.norm(closed[4:] - c), rel=1e-9, abs=1e-12)
    got = [_alpha_of(C[k], ref) for k in range(i + 1, j + 1)]
    # (read back through a logarithm: the comparison is of shares, not of bits)
    assert np.allclose(got, want, rtol=0.0, atol=1e-9), (got, want)
    assert all(0.0 <= g <= 1.0 + 1e-12 for g in got) and np.all(np.diff(got) >= -1e-12)


# ---- every refusal ----------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(sage):
    lib, dp = sage.lib(), ctypes.POINTER(ctypes.c_double)
    poses, i, j, closed = CASES["arc, drift in rotation and translation"]
    n = len(poses)

    def refused(P, n_, i_, j_, c, corr=True, what=""):
        C = np.full((n, 7), 7.25)
        O = np.full((n, 7), 7.25)
        info = sage.ClosureInfo()
        info.angle = 7.25
        rc = lib.sageicp_closure_corrections(None if P is None else np.ascontiguousarray(P).ctypes.data_as(dp), n_, i_, j_,
                                             None if c is None else np.ascontiguousarray(c).ctypes.data_as(dp),
                                             C.ctypes.data_as(dp) if corr else None, O.ctypes.data_as(dp), ctypes.byref(info))
        assert rc == sage.ERR_INVALID, (what, rc)
        assert (C == 7.25).all() and (O == 7.25).all() and info.angle == 7.25, what

    refused(None, n, i, j, closed, what="poses NULL")
    refused(poses, n, i, j, None, what="closed NULL")
    refused(poses, n, i, j, closed, corr=False, what="corrections_out NULL")
    refused(poses, 0, 0, 0, closed, what="n == 0")
    refused(poses, n, 5, 5, closed, what="i == j")
    refused(poses, n, 6, 5, closed, what="i > j")
    refused(poses, n, 3, n, closed, what="j == n")
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 3, 4, 6):
            P = poses.copy()
            P[n - 1, col] = bad                          # (a pose beyond j counts too: poses_out is written for it)
            refused(P, n, i, j, closed, what="non-finite pose")
            c = closed.copy()
            c[col] = bad
            refused(poses, n, i, j, c, what="non-finite closed")
    P = poses.copy()
    P[1, :4] = 0.0
    refused(P, n, i, j, closed, what="a pose's quaternion of norm 0")
    c = closed.copy()
    c[:4] = 0.0
    refused(poses, n, i, j, c, what="closed's quaternion of norm 0")
    # a delta that turns by more than pi - 1e-6: half a turn, and just inside the limit on the other side of it
    refused(poses, n, i, j, _closed_from(poses, j, (0.0, 0.0, 180.0), (0.0, 0.0, 0.0)), what="a turn of pi")
    refused(poses, n, i, j, _closed_from(poses, j, (0.0, 0.0, math.degrees(math.pi - 5e-7)), (0.0, 0.0, 0.0)), what="pi - 5e-7")
    ok = _closed_from(poses, j, (0.0, 0.0, math.degrees(math.pi - 2e-6)), (0.0, 0.0, 0.0))
    C, _ = sage.closure_corrections(poses, i, j, ok)     # pi - 2e-6: accepted
    assert np.isfinite(C).all()
    # the optional pointers
    C = np.empty((n, 7))
    assert lib.sageicp_closure_corrections(poses.ctypes.data_as(dp), n, i, j, closed.ctypes.data_as(dp), C.ctypes.data_as(dp),
                                           None, None) == 0
    with pytest.raises(ValueError):
        sage.closure_corrections(poses[:, :6], i, j, closed)


# ---- against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("utm", [False, True], ids=["local", "utm"])
def test_corrections_against_the_restatement(sage, utm):
    mq, mt = _measured(utm)
    print("fp64 restatement vs extended, %s: quaternion %.3g translation %.3g" % ("utm" if utm else "local", mq, mt))
    assert mq > 0.0 and mt > 0.0
    worst_q = worst_t = 0.0
    for name in CASES:
        poses, i, j, closed, _, ext = _reference(name, utm)
        C, out = sage.closure_corrections(poses, i, j, closed)
        for got, field in ((C, "C"), (out, "poses_out")):
            eq, et = _err(got, ext[field])
            worst_q, worst_t = max(worst_q, eq), max(worst_t, et)
    print("the library vs extended, %s: quaternion %.3g translation %.3g (allowed %.3g / %.3g)"
          % ("utm" if utm else "local", worst_q, worst_t, 4 * mq, 4 * mt))
    assert worst_q <= 4 * mq and worst_t <= 4 * mt


@pytest.mark.parametrize("name", list(CASES))
def test_translation_equivariance(sage, name):
    """the same trajectory shifted by (5e5, 5e6, 0): the same quaternions, the shifted translations — to four times the
    fp64 restatement's own error at those coordinates (the utm group's measurement)"""
    mq, mt = _measured(True)
    poses, i, j, closed = CASES[name]
    C0, out0 = sage.closure_corrections(poses, i, j, closed)
    P, c = _shifted(poses, closed)
    C1, out1 = sage.closure_corrections(P, i, j, c)
    print("%s: quaternions differ by %.3g, translations by %.3g (allowed %.3g / %.3g)"
          % (name, np.abs(out1[:, :4] - out0[:, :4]).max(), np.abs(out1[:, 4:] - UTM - out0[:, 4:]).max(), 4 * mq, 4 * mt))
    assert np.abs(out1[:, :4] - out0[:, :4]).max() <= 4 * mq
    assert np.abs(C1[:, :4] - C0[:, :4]).max() <= 4 * mq
    assert np.abs(out1[:, 4:] - UTM - out0[:, 4:]).max() <= 4 * mt
