"""Host-side tests of the constant-velocity deskew (core/Deskew.cpp:31-50, pipeline/sageICP.cpp:36-52): the independent
CPU restatement (tests/deskew_ref.cpp) against closed forms and the skewed generator's known answer,
normalize_timestamps against the reference node's rule, the C ABI's refusals where no device is needed, and the
reference's pipeline type-checked against the opt-in Deskew shim."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import deskewref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference/cpp"


def _ring(n=2000, seed=3):
    rng = np.random.default_rng(seed)
    f = np.empty((n, 4))
    f[:, :3] = rng.uniform(-60.0, 60.0, (n, 3))
    f[:, 3] = rng.integers(0, 100, n)
    return f, rng.uniform(0.0, 1.0, n)


def test_pure_translation_moves_points_along_the_velocity():
    f, t = _ring()
    v = np.array([1.5, -0.4, 0.2])
    start = np.array([0, 0, 0, 1, 0, 0, 0.0])
    finish = np.array([0, 0, 0, 1, *v])
    out = dr.deskew(f, t, start, finish)
    want = f[:, :3] + (t - 0.5)[:, None] * v[None, :]
    assert np.max(np.abs(out[:, :3] - want)) < 1e-13
    assert np.array_equal(out[:, 3], f[:, 3])


def test_pure_yaw_rotates_about_z():
    f, t = _ring()
    w = np.deg2rad(2.0)
    start = np.array([0, 0, 0, 1, 0, 0, 0.0])
    finish = np.array([0, 0, np.sin(w / 2), np.cos(w / 2), 0, 0, 0])
    out = dr.deskew(f, t, start, finish)
    a = (t - 0.5) * w
    c, s = np.cos(a), np.sin(a)
    want = np.stack([c * f[:, 0] - s * f[:, 1], s * f[:, 0] + c * f[:, 1], f[:, 2]], axis=1)
    assert np.max(np.abs(out[:, :3] - want)) < 1e-12
    assert np.array_equal(out[:, 3], f[:, 3])


def test_mid_scan_timestamps_give_the_identity_bit_for_bit():
    f, _ = _ring()
    start = np.array([0.01, -0.02, 0.3, 0.0, 4.0, -2.0, 0.5])
    start[:4] /= np.linalg.norm(start[:4])
    finish = np.array([0.02, 0.01, 0.33, 0.0, 5.2, -1.1, 0.4])
    finish[:4] /= np.linalg.norm(finish[:4])
    out = dr.deskew(f, np.full(len(f), 0.5), start, finish)
    assert np.array_equal(out, f)


def test_restatement_exp_log_round_trip():
    # (not between ~1e-10 and ~1e-5 rad: there Sophus's (1 - cos th) / th^2 cancels to ~1e-16 / th^2 relative, in the
    # reference and in csrc/se3_math.h alike)
    rng = np.random.default_rng(5)
    for scale in (1e-13, 1e-3, 0.3, 2.9):
        for _ in range(20):
            a = rng.normal(size=6)
            a[3:] *= scale / np.linalg.norm(a[3:])
            assert np.max(np.abs(dr.log(dr.exp(a)) - a)) < 1e-12 * max(1.0, np.linalg.norm(a)), (scale, a)


def test_true_poses_unskew_the_generated_stream():
    from sage_icp_amd import synthetic_skew as sk
    S = sk.make_skewed_stream(n_frames=3)
    P = S["poses"]
    assert np.max(np.abs(dr.delta(P[0], P[1]) - S["xi"])) < 1e-12
    for k in range(3):
        f, t = S["frames"][k], S["timestamps"][k]
        assert len(f) > 50000 and np.all((t >= 0.0) & (t < 1.0))
        # the skew is metre-scale at the ends of a turn
        assert np.max(np.abs(f[:, :3] - S["unskewed"][k][:, :3])) > 1.0
        out = dr.deskew(f, t, P[max(k - 1, 0)] if k else P[0], P[k] if k else P[1])
        assert np.max(np.abs(out[:, :3] - S["unskewed"][k][:, :3])) <= 1e-12, k
        assert np.array_equal(out[:, 3], S["unskewed"][k][:, 3])


def test_normalize_timestamps(sage):
    a = np.array([0.0, 0.25, 0.999])
    assert np.array_equal(sage.normalize_timestamps(a), a)
    b = np.array([0, 100, 400, 200], dtype=np.int64)
    assert np.array_equal(sage.normalize_timestamps(b), np.array([0.0, 0.25, 1.0, 0.5]))
    c = np.array([1.0, 0.5])                           # max == 1 is divided (by 1)
    assert np.array_equal(sage.normalize_timestamps(c), c)
    d = np.array([3.0, 6.0])
    assert np.array_equal(sage.normalize_timestamps(d), d / 6.0)
    assert sage.normalize_timestamps(np.zeros(0)).size == 0


def _p(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def test_deskew_scan_refusals_need_no_device(sage):
    L = sage.lib()
    f = np.array([[10.0, 0.0, 0.0, 40.0], [0.0, 12.0, 1.0, 44.0]])
    t = np.array([0.1, 0.9])
    I = np.array([0, 0, 0, 1, 0, 0, 0.0])
    out = np.empty((2, 4))
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    keep = [f, t, I]                                                      # (alive while the pointers are used)
    assert L.sageicp_deskew_scan(None, _p(t), 2, _p(I), _p(I), op, 0) == sage.ERR_INVALID
    assert L.sageicp_deskew_scan(_p(f), None, 2, _p(I), _p(I), op, 0) == sage.ERR_INVALID
    assert L.sageicp_deskew_scan(_p(f), _p(t), 2, None, _p(I), op, 0) == sage.ERR_INVALID
    assert L.sageicp_deskew_scan(_p(f), _p(t), 2, _p(I), None, op, 0) == sage.ERR_INVALID
    assert L.sageicp_deskew_scan(_p(f), _p(t), 2, _p(I), _p(I), None, 0) == sage.ERR_INVALID
    assert L.sageicp_deskew_scan(_p(f), _p(t), (1 << 26) - 3, _p(I), _p(I), op, 0) == sage.ERR_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        tb = t.copy(); tb[1] = bad
        keep.append(tb)
        assert L.sageicp_deskew_scan(_p(f), _p(tb), 2, _p(I), _p(I), op, 0) == sage.ERR_INVALID
        fb = f.copy(); fb[0, 1] = bad
        assert L.sageicp_deskew_scan(_p(fb), _p(t), 2, _p(I), _p(I), op, 0) == sage.ERR_INVALID
        fl = f.copy(); fl[1, 3] = bad
        assert L.sageicp_deskew_scan(_p(fl), _p(t), 2, _p(I), _p(I), op, 0) == sage.ERR_INVALID
        pb = I.copy(); pb[5] = bad
        assert L.sageicp_deskew_scan(_p(f), _p(t), 2, _p(I), _p(pb), op, 0) == sage.ERR_INVALID
    assert "not finite" in sage.lib().sageicp_last_error().decode()
    # n == 0: nothing to do, no device needed, pointers may be NULL
    assert L.sageicp_deskew_scan(None, None, 0, _p(I), _p(I), None, 0) == 0
    assert len(sage.deskew_scan(np.zeros((0, 4)), np.zeros(0), I, I)) == 0
    with pytest.raises(ValueError):
        sage.deskew_scan(f, t[:1], I, I)
    del keep


def test_pipeline_deskew_refusals_need_no_device(sage):
    L = sage.lib()
    p = sage.SageICP(sage.make_pipeline_config(deskew=True))
    f = np.array([[10.0, 0.0, 0.0, 40.0], [0.0, 12.0, 1.0, 44.0]])
    pose = np.empty(7)
    pp = pose.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    # NULL timestamps with n > 0, and non-finite ones, are refused before anything else: no pose is pushed
    rc = L.sageicp_pipeline_register_frame_timestamps(p._h, _p(f), None, 2, pp, None, None, None, None)
    assert rc == sage.ERR_INVALID
    for bad in (np.nan, np.inf):
        with pytest.raises(sage.SageIcpError) as e:
            p.RegisterFrame(f, np.array([0.2, bad]))
        assert e.value.code == sage.ERR_INVALID
    assert len(p.poses()) == 0
    with pytest.raises(ValueError):
        p.RegisterFrame(f, np.array([0.2]))
    # prefetch is refused while deskew is on; switching it off allows it again
    with pytest.raises(sage.SageIcpError) as e:
        p.prefetch(f)
    assert e.value.code == sage.ERR_INVALID and "deskew" in str(e.value)
    p.set_deskew(False)
    p.prefetch(f)
    p.set_deskew(True)          # drops the announcement
    p.prefetch_cancel()
    applied, delta = p.deskew_info()
    assert not applied and np.array_equal(delta, np.zeros(6))
    assert L.sageicp_pipeline_set_deskew(None, 1) == sage.ERR_INVALID
    assert L.sageicp_pipeline_deskew_info(p._h, None, None) == sage.ERR_INVALID
    assert L.sageicp_pipeline_register_frame_timestamps(None, _p(f), None, 2, pp, None, None, None, None) == sage.ERR_INVALID


def test_deskew_entries_need_a_device(sage):
    if sage.device_count() > 0:
        pytest.skip("a HIP device is present")
    f = np.array([[10.0, 0.0, 0.0, 40.0]])
    I = np.array([0, 0, 0, 1, 0, 0, 0.0])
    with pytest.raises(sage.SageIcpError) as e:
        sage.deskew_scan(f, [0.3], I, I)
    assert e.value.code == sage.ERR_NO_DEVICE


@pytest.mark.skipif(not os.path.exists(os.path.join(REFERENCE, "sage_icp", "pipeline", "sageICP.cpp")),
                    reason="the reference tree is only present in the build container")
def test_reference_caller_compiles_unchanged_against_the_deskew_shim():
    """pipeline/sageICP.cpp with sage_icp/core/Deskew.hpp resolved to shim_deskew: DeSkewScan(frame, timestamps,
    poses_[N-2], poses_[N-1]) type-checks against the shim's declaration"""
    src = os.path.join(REFERENCE, "sage_icp", "pipeline", "sageICP.cpp")
    inc = ["-I", os.path.join(ROOT, "tests", "shim_stubs"),
           "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
           "-I", os.path.join(ROOT, "sage-icp_amd", "shim_preprocessing"),
           "-I", os.path.join(ROOT, "sage-icp_amd", "shim_deskew"),
           "-I", os.path.join(ROOT, "include"),
           "-I", REFERENCE]
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall"] + inc + [src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    deps = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-M"] + inc + [src], capture_output=True, text=True)
    assert deps.returncode == 0
    used = deps.stdout.replace("\\\n", " ").split()
    hits = [u for u in used if u.endswith("sage_icp/core/Deskew.hpp")]
    assert hits and all(os.path.abspath(h).startswith(os.path.join(ROOT, "sage-icp_amd", "shim_deskew")) for h in hits)


def test_deskew_shim_builds_host_side(sage, tmp_path):
    exe = str(tmp_path / "deskew_user")
    lib_dir = os.path.join(ROOT, "sage-icp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "shim_stubs"),
                           "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                           "-I", os.path.join(ROOT, "sage-icp_amd", "shim_deskew"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_stubs", "deskew_user.cpp"),
                           "-L", lib_dir, "-l:libsageicp_hip.so", "-Wl,-rpath," + lib_dir, "-o", exe])
    f = np.array([[10.0, 0.0, 0.0, 40.0]])
    np.array([[0, 0, 0, 1, 0, 0, 0.0]] * 2).tofile(str(tmp_path / "poses.f64"))
    f.tofile(str(tmp_path / "frame.f64"))
    np.array([np.nan]).tofile(str(tmp_path / "ts.f64"))
    r = subprocess.run([exe, str(tmp_path / "frame.f64"), str(tmp_path / "ts.f64"), str(tmp_path / "poses.f64"),
                        str(tmp_path / "out.f64")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 4 and "DeSkewScan" in r.stdout        # a NaN timestamp throws (before any device use)
