"""The registration quality report without a GPU: the header's struct against its ctypes mirror, the new symbols, every
refusal that happens before any device is asked for, and the truth tests/qualityref.py against a plain fp64 evaluation
and the oracle's AlignClouds."""
import ctypes
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import qualityref as qr
from gnref import U, gamma_serial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [0, 0, 10, 40, 44, 50, 70, 71, 80, 251]
_dp = ctypes.POINTER(ctypes.c_double)


def _pairs(n=50, seed=3, shift=(0.0, 0.0, 0.0)):
    """n pairs of a street-sized scene: queries, each with a map point within 0.5, labels of every kind"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-40.0, 40.0, size=(n, 4))
    src[:, 2] *= 0.1
    src[:, :3] += shift
    src[:, 3] = rng.choice(LABELS, size=n)
    src[:3, 3] = [300.0, -3.0, 10.9]
    tgt = src.copy()
    tgt[:, :3] += rng.uniform(-0.3, 0.3, size=(n, 3))
    tgt[:, 3] = rng.choice(LABELS, size=n)
    return src, tgt


def test_struct_size_matches_the_header(sage):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){' + \
          'printf("%zu %zu %zu %zu %d", sizeof(sageicp_quality), offsetof(sageicp_quality, n_queries), ' + \
          'offsetof(sageicp_quality, class_queries), offsetof(sageicp_quality, valid), SAGEICP_ABI_VERSION);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"),
                               "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    Q = sage.Quality
    assert got[0] == ctypes.sizeof(Q) == sage.QUALITY_BYTES == 5464
    assert got[1] == Q.n_queries.offset and got[2] == Q.class_queries.offset and got[3] == Q.valid.offset
    assert got[4] == 4


def test_new_symbols_and_abi_version(sage):
    L = sage.lib()
    for name in ("sageicp_registration_quality", "sageicp_registration_quality_device", "sageicp_pipeline_set_quality",
                 "sageicp_pipeline_quality"):
        assert name in sage.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.sageicp_abi_version() == 4 == sage.ABI_VERSION


def test_as_dict_shapes(sage):
    d = sage.Quality().as_dict()
    for k in ("JTJ", "info", "covariance", "covariance_pose"):
        assert d[k].shape == (6, 6) and d[k].dtype == np.float64
    assert d["class_queries"].shape == (256,) and d["class_sum_r2"].shape == (256,) and d["step"].shape == (6,)
    assert d["valid"] is False and d["covariance_valid"] is False and d["n_pairs"] == 0


def _call(sage, vmap_h, rows, pose, md, kernel, th, out):
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.float64)
    pose = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64)
    rc = sage.lib().sageicp_registration_quality(
        vmap_h, None if rows is None else rows.ctypes.data_as(_dp), 0 if rows is None else len(rows),
        None if pose is None else pose.ctypes.data_as(_dp), md, kernel, th, out)
    return rc, (sage.lib().sageicp_last_error() or b"").decode()


def test_refusals_before_any_device(sage):
    m = sage.VoxelHashMap(1.0, 100.0)
    q = sage.Quality()
    rows = np.array([[1.0, 2.0, 3.0, 40.0], [2.0, 2.0, 3.0, 0.0]])
    ok_pose = sage.IDENTITY.copy()
    rc, msg = _call(sage, None, rows, None, 1.0, 0.5, 0.4, ctypes.byref(q))
    assert rc == sage.ERR_INVALID and "map" in msg
    rc, msg = _call(sage, m._h, rows, None, 1.0, 0.5, 0.4, None)
    assert rc == sage.ERR_INVALID and "out" in msg
    for bad in (np.nan, np.inf):
        p = ok_pose.copy()
        p[5] = bad
        rc, msg = _call(sage, m._h, rows, p, 1.0, 0.5, 0.4, ctypes.byref(q))
        assert rc == sage.ERR_INVALID and "pose" in msg
    for bad in (0.0, -1.0, np.nan, np.inf):
        rc, msg = _call(sage, m._h, rows, ok_pose, 1.0, bad, 0.4, ctypes.byref(q))
        assert rc == sage.ERR_INVALID and "kernel" in msg
    for col, bad in ((0, np.nan), (2, np.inf), (3, np.nan), (3, -np.inf)):
        r = rows.copy()
        r[1, col] = bad
        rc, msg = _call(sage, m._h, r, None, 1.0, 0.5, 0.4, ctypes.byref(q))
        assert rc == sage.ERR_INVALID and "not finite" in msg
    # the device-frame entry: what it refuses before it asks for a device
    f = sage.DeviceFrame(0x1000, 32, sage.DTYPE_FLOAT64, 0, None, 0, 2)
    L = sage.lib()
    pp = ok_pose.ctypes.data_as(_dp)
    assert L.sageicp_registration_quality_device(None, ctypes.byref(f), pp, 1.0, 0.5, 0.4, None, ctypes.byref(q)) == sage.ERR_INVALID
    assert L.sageicp_registration_quality_device(m._h, ctypes.byref(f), pp, 1.0, 0.5, 0.4, None, None) == sage.ERR_INVALID
    assert L.sageicp_registration_quality_device(m._h, None, pp, 1.0, 0.5, 0.4, None, ctypes.byref(q)) == sage.ERR_INVALID
    assert "frame" in L.sageicp_last_error().decode()
    bad_pose = ok_pose.copy()
    bad_pose[0] = np.nan
    assert L.sageicp_registration_quality_device(m._h, ctypes.byref(f), bad_pose.ctypes.data_as(_dp), 1.0, 0.5, 0.4, None,
                                                 ctypes.byref(q)) == sage.ERR_INVALID
    assert "pose" in L.sageicp_last_error().decode()
    assert L.sageicp_registration_quality_device(m._h, ctypes.byref(f), pp, 1.0, -2.0, 0.4, None, ctypes.byref(q)) == sage.ERR_INVALID
    assert "kernel" in L.sageicp_last_error().decode()
    # the pipeline's switches
    assert L.sageicp_pipeline_set_quality(None, 1) == sage.ERR_INVALID
    assert L.sageicp_pipeline_quality(None, ctypes.byref(q)) == sage.ERR_INVALID


def test_empty_map_and_no_rows_are_ok_and_zero(sage):
    m = sage.VoxelHashMap(1.0, 100.0)
    q = sage.Quality()
    ctypes.memset(ctypes.byref(q), 0xAB, ctypes.sizeof(q))
    rows = np.array([[1.0, 2.0, 3.0, 40.0]])
    rc, _ = _call(sage, m._h, rows, None, 1.0, 0.5, 0.4, ctypes.byref(q))       # an empty map: no device is asked for
    assert rc == 0 and bytes(q) == bytes(ctypes.sizeof(q))
    ctypes.memset(ctypes.byref(q), 0xAB, ctypes.sizeof(q))
    rc, _ = _call(sage, m._h, None, None, 1.0, 0.5, 0.4, ctypes.byref(q))
    assert rc == 0 and bytes(q) == bytes(ctypes.sizeof(q))


def test_pipeline_switch_and_empty_report(sage):
    p = sage.SageICP(sage.make_pipeline_config())
    assert not p.quality().valid
    p.set_quality(True)
    assert bytes(p.quality()) == bytes(sage.QUALITY_BYTES)
    p.set_quality(False)
    p.reinitialize()
    assert not p.quality().valid


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), (5e5, 5.5e6, 0.0)], ids=["local", "utm"])
def test_reference_agrees_with_plain_fp64(shift):
    src, tgt = _pairs(50, shift=shift)
    ref = qr.Quality(src[:, 3], src, tgt, 0.7)
    got = qr.numpy_quality(src[:, 3], src, tgt, 0.7)
    worst, where = ref.sums_ratio(got, gamma_serial(50))
    print("worst |numpy - exact| / (gamma_serial(50) E) = %.3g at %s" % (worst, where))
    assert worst <= 1.0, where
    c = ref.counts
    assert c["n_pairs"] == 50 and c["other_queries"] == 2 and c["other_pairs"] == 2 and c["class_queries"][10] >= 1
    assert c["pairs_same_label"] + c["pairs_unlabelled"] + c["pairs_cross_label"] == 50
    assert c["pairs_same_label"] > 0 and c["pairs_unlabelled"] > 0 and c["pairs_cross_label"] > 0
    # the three residual sums are what their definitions say, and the class table adds up to sum_r2
    assert sum(ref.real["class_sum_r2"][0]) == ref.real["sum_r2"][0]
    assert ref.real["JTJ"][0][0][0] == ref.real["sum_w"][0] == ref.real["JTJ"][0][2][2]
    assert ref.real["info"][0][1][1] == 50


def test_reference_agrees_with_the_oracles_align_clouds(oracle):
    src, tgt = _pairs(50)
    ref = qr.Quality(src[:, 3], src, tgt, 0.7)
    _, JTJ, JTr = oracle.align_clouds(src, tgt, 0.7, nthreads=1)
    got = {"JTJ": JTJ, "JTr": JTr, "sum_w": JTJ[0, 0], "sum_r2": float(ref.real["sum_r2"][0]),
           "sum_w_r2": float(ref.real["sum_w_r2"][0]), "info": [[float(v) for v in row] for row in ref.real["info"][0]]}
    worst, where = ref.sums_ratio(got, gamma_serial(50))
    print("worst |oracle - exact| / (gamma_serial(50) E) = %.3g at %s" % (worst, where))
    assert worst <= 1.0, where


def test_reference_derived_values():
    src, tgt = _pairs(12)
    t = (3.0, -2.0, 0.5)
    ref = qr.Quality(src[:, 3], src, tgt, 0.7, t=t)
    A, b = ref.real["JTJ"][0], ref.real["JTr"][0]
    # JTJ step = -JTr, exactly
    for i in range(6):
        assert sum(A[i][j] * ref.step[j] for j in range(6)) == -b[i]
    # JTJ covariance = s2 I, exactly
    s2 = ref.real["sum_w_r2"][0] / (3 * 12 - 6)
    for i in range(6):
        for j in range(6):
            assert sum(A[i][k] * ref.covariance[k][j] for k in range(6)) == (s2 if i == j else 0)
    # the pose's covariance: the rotation block is kept, the translation block is that of dt = upsilon - hat(t) omega
    C, P = ref.covariance, ref.covariance_pose
    assert [row[3:] for row in P[3:]] == [row[3:] for row in C[3:]]
    H = qr.hat([Fraction(v) for v in t])
    G = [[Fraction(int(i == j)) - (H[i][j - 3] if j >= 3 else 0) for j in range(6)] for i in range(3)]
    for a in range(3):
        for c in range(3):
            assert P[a][c] == sum(G[a][i] * C[i][j] * G[c][j] for i in range(6) for j in range(6))
    P0, _ = qr.pose_covariance(C, (0.0, 0.0, 0.0))
    assert P0 == C
    # fewer than three pairs, and collinear queries: nothing derived
    assert qr.Quality(src[:2, 3], src[:2], tgt[:2], 0.7).step is None
    line = src[:5].copy()
    line[:, 1:3] = [2.0, 1.0]
    assert qr.Quality(line[:, 3], line, tgt[:5], 0.7).step is None
    assert float(ref.fitness) == 1.0 and abs(float(ref.rmse2) - np.mean(np.sum((src[:12, :3] - tgt[:12, :3]) ** 2, axis=1))) < 1e-12
    assert U == 2.0 ** -53
