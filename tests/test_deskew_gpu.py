"""The constant-velocity deskew on the device (csrc/deskew.hip; core/Deskew.cpp:31-50, pipeline/sageICP.cpp:36-52):
sageicp_deskew_scan against the independent CPU restatement tests/deskew_ref.cpp row for row, the pipeline against the
oracle fed restated deskewed frames, the order deskew -> dynamic filter -> down-sampling, the paths where deskew does
not apply, the entry contract, and the opt-in Deskew shim."""
import os
import subprocess

import numpy as np
import pytest

import deskewref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I7 = np.array([0, 0, 0, 1, 0, 0, 0.0])


def _pose(axis, angle, t):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)], np.asarray(t, dtype=np.float64)])


def _stream(n_frames=12, az_steps=2048, seed=0x5E):
    from sage_icp_amd import synthetic_skew as sk
    return sk.make_skewed_stream(seed=seed, n_frames=n_frames, az_steps=az_steps)


def _check_rows(sage, f, t, start, finish):
    out = sage.deskew_scan(f, t, start, finish)
    ref = dr.deskew(f, t, start, finish)
    assert out.shape == f.shape
    assert np.array_equal(out[:, 3].view(np.uint64), f[:, 3].view(np.uint64))         # labels, bit for bit, in order
    tol = 1e-13 * np.maximum(1.0, np.linalg.norm(f[:, :3], axis=1))
    err = np.max(np.abs(out[:, :3] - ref[:, :3]), axis=1)
    assert np.all(err <= tol), (np.max(err / tol), int(np.argmax(err / tol)))
    return out


@pytest.mark.gpu
def test_deskew_scan_matches_the_restatement_on_skewed_ring_scans(gpu_sage):
    S = _stream(n_frames=2, az_steps=3072)
    P = S["poses"]
    for k in range(2):
        f, t = S["frames"][k], S["timestamps"][k]
        assert len(f) > 120000
        out = _check_rows(gpu_sage, f, t, P[0], P[1])
        assert np.max(np.abs(out[:, :3] - S["unskewed"][k][:, :3])) < 1e-9         # the known answer


def _cases():
    rng = np.random.default_rng(11)
    C = {}
    moderate = (I7, _pose([0.1, -0.2, 1.0], np.deg2rad(3.0), [1.4, -0.3, 0.05]))
    for n in (1, 255, 257, 1 << 20):
        f = np.empty((n, 4))
        f[:, :3] = rng.uniform(-80.0, 80.0, (n, 3))
        f[:, 3] = rng.integers(0, 260, n)
        C["n=%d" % n] = (f, rng.uniform(0.0, 1.0, n)) + moderate
    f = np.empty((50000, 4))
    f[:, :3] = rng.uniform(-80.0, 80.0, (50000, 3))
    f[:, 3] = rng.integers(0, 260, 50000)
    wide = rng.uniform(-2.0, 3.0, 50000)
    C["t_in_-2_3"] = (f, wide) + moderate
    C["delta_170deg"] = (f, rng.uniform(0.0, 1.0, 50000), _pose([0.3, 0.5, 1.0], np.deg2rad(20.0), [2.0, 1.0, 0.0]),
                         _pose([-0.2, 0.4, -1.0], np.deg2rad(170.0), [-3.0, 4.0, 1.0]))
    C["all_below_1e-10"] = (f, wide, I7, _pose([0.3, -0.7, 0.2], 1e-12, [0.2, -0.1, 0.05]))
    C["straddling_1e-10"] = (f, wide, I7, _pose([0.3, -0.7, 0.2], 8e-11, [0.2, -0.1, 0.05]))
    A = _pose([0.0, 0.1, 1.0], 0.7, [5.0, -3.0, 1.0])
    C["start_equals_finish"] = (f, wide, A, A.copy())
    g = f.copy()
    g[:, :3] += np.array([4.1e6, 5.3e6, 120.0])                  # UTM-scale coordinates
    C["utm"] = (g, rng.uniform(0.0, 1.0, 50000)) + moderate
    return C


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_cases()))
def test_deskew_scan_adversarial_inputs(gpu_sage, name):
    f, t, start, finish = _cases()[name]
    if name == "straddling_1e-10":
        th = np.abs(t - 0.5) * np.linalg.norm(dr.delta(start, finish)[3:])
        assert np.any(th < 1e-10) and np.any(th > 1e-10)
    if name == "all_below_1e-10":
        assert np.all(np.abs(t - 0.5) * np.linalg.norm(dr.delta(start, finish)[3:]) < 1e-10)
    _check_rows(gpu_sage, f, t, start, finish)


@pytest.mark.gpu
def test_deskew_scan_mid_timestamps_in_place_and_out_of_place(gpu_sage):
    import ctypes
    sage = gpu_sage
    f, t, start, finish = _cases()["n=257"]
    same = sage.deskew_scan(f, np.full(len(f), 0.5), start, finish)
    assert np.array_equal(same, f)
    out = sage.deskew_scan(f, t, start, finish)
    g = np.ascontiguousarray(f.copy())
    dp = ctypes.POINTER(ctypes.c_double)
    ts = np.ascontiguousarray(t)
    rc = sage.lib().sageicp_deskew_scan(g.ctypes.data_as(dp), ts.ctypes.data_as(dp), len(g),
                                        np.ascontiguousarray(start).ctypes.data_as(dp),
                                        np.ascontiguousarray(finish).ctypes.data_as(dp), g.ctypes.data_as(dp), 0)
    assert rc == 0 and np.array_equal(g, out)


def _near_faces(sage, pts, eps=1e-9):
    """a point within eps of a face of its label group's voxels at either down-sampling scale (0.5, 1.5)"""
    for labels, v in zip(sage.KITTI_VOXEL_LABELS, sage.KITTI_VOXEL_SIZE):
        sel = pts[np.isin(pts[:, 3], labels), :3]
        for s in (v * 0.5, v * 1.5):
            r = sel / s
            if np.any(np.abs(r - np.round(r)) * s < eps):
                return True
    return False


@pytest.mark.gpu
def test_pipeline_with_deskew_matches_the_oracle_fed_restated_frames(gpu_sage, oracle, reference_emission_order):
    sage = gpu_sage
    S = _stream(12)
    cfg = sage.make_pipeline_config(deskew=True)
    a = sage.SageICP(cfg)
    o = oracle.Pipeline(sage.make_pipeline_config())
    opos = []
    for k, (f, t) in enumerate(zip(S["frames"], S["timestamps"])):
        g = dr.deskew(f, t, opos[-2], opos[-1]) if len(opos) > 2 else f
        # precondition: no restated coordinate on a voxel face, no range on a crop radius (else a ulp decides)
        assert not _near_faces(sage, g), k
        rng_ = np.linalg.norm(g[:, :3], axis=1)
        assert np.all(np.min(np.abs(rng_[:, None] - np.array([5.0, 50.0, 100.0])[None, :]), axis=1) > 1e-9), k
        pa, _, _, ns_a, st_a = a.RegisterFrame(f, t)
        applied, delta = a.deskew_info()
        assert applied == (k > 2), k
        if applied:
            pp = a.poses()
            assert np.max(np.abs(delta - dr.delta(pp[-3], pp[-2]))) < 1e-12, k
        else:
            assert np.array_equal(delta, np.zeros(6))
        po, ns_o, _, st_o = o.register_frame(g)
        opos.append(po)
        assert ns_o == ns_a, k
        dlog = dr.log(dr.mul(dr.inv(po), pa))
        assert np.max(np.abs(dlog[:3])) <= 1e-6 and np.max(np.abs(dlog[3:])) <= 1e-6, (k, po, pa)
        if k:
            assert st_o.iterations == st_a.iterations, k
    assert len(a.LocalMap()) == len(o.local_map())


@pytest.mark.gpu
def test_deskew_runs_before_the_dynamic_filter_and_the_down_sampling(gpu_sage):
    sage = gpu_sage
    S = _stream(10)
    a = sage.SageICP(sage.make_pipeline_config(deskew=True, dynamic_vehicle_filter=True))
    b = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
    drop = ("us_wall", "us_host", "us_device")
    for k, (f, t) in enumerate(zip(S["frames"], S["timestamps"])):
        pb_all = b.poses()
        g = sage.deskew_scan(f, t, pb_all[-2], pb_all[-1]) if len(pb_all) > 2 else f
        pa, _, _, ns_a, _ = a.RegisterFrame(f, t)
        pb, _, _, ns_b, _ = b.RegisterFrame(g)
        assert np.array_equal(pa, pb) and ns_a == ns_b, k
        ia, ib = a.dynamic_filter_info(), b.dynamic_filter_info()
        assert {x: ia[x] for x in ia if x not in drop} == {x: ib[x] for x in ib if x not in drop}, k
        assert np.array_equal(a.LocalMap(), b.LocalMap()), k
    assert a.deskew_info()[0]


@pytest.mark.gpu
def test_no_change_where_deskew_does_not_apply(gpu_sage):
    sage = gpu_sage
    S = _stream(6)
    F, T = [np.ascontiguousarray(f) for f in S["frames"]], S["timestamps"]
    on = sage.SageICP(sage.make_pipeline_config(deskew=True))
    off = sage.SageICP(sage.make_pipeline_config())
    plain_on = sage.SageICP(sage.make_pipeline_config(deskew=True))
    ts_off = sage.SageICP(sage.make_pipeline_config())          # timestamped entry, deskew off, with prefetch
    for k in range(6):
        p_off = off.RegisterFrame(F[k])[0]
        p_plain = plain_on.RegisterFrame(F[k])[0]               # the one-argument entry never deskews
        assert np.array_equal(p_plain, p_off) and not plain_on.deskew_info()[0], k
        if k + 1 < 6:
            ts_off.prefetch(F[k + 1])
        p_ts = ts_off.RegisterFrame(F[k], T[k])[0]
        assert np.array_equal(p_ts, p_off) and not ts_off.deskew_info()[0], k
        if k < 3:                                               # N <= 2: the frame passes through
            p_on = on.RegisterFrame(F[k], T[k])[0]
            assert np.array_equal(p_on, p_off) and not on.deskew_info()[0], k
    for x in (plain_on, ts_off):
        assert np.array_equal(x.LocalMap(), off.LocalMap())
    # reinitialize() clears the poses: the next three frames are not deskewed again
    on.RegisterFrame(F[3], T[3])
    assert on.deskew_info()[0]
    on.reinitialize()
    fresh = sage.SageICP(sage.make_pipeline_config())
    for k in range(3):
        p_on = on.RegisterFrame(F[3 + k], T[3 + k])[0]
        assert not on.deskew_info()[0], k
        assert np.array_equal(p_on, fresh.RegisterFrame(F[3 + k])[0]), k


@pytest.mark.gpu
def test_deskew_entry_contract(gpu_sage):
    import ctypes
    sage = gpu_sage
    S = _stream(5)
    F, T = [np.ascontiguousarray(f) for f in S["frames"]], S["timestamps"]
    p = sage.SageICP(sage.make_pipeline_config())
    q = sage.SageICP(sage.make_pipeline_config(deskew=True))
    p.RegisterFrame(F[0], T[0])
    p.prefetch(F[1])
    p.set_deskew(True)                      # drops the announced frame
    with pytest.raises(sage.SageIcpError):
        p.prefetch(F[2])
    for k in range(1, 5):
        if k == 1:
            q.RegisterFrame(F[0], T[0])
        assert np.array_equal(p.RegisterFrame(F[k], T[k])[0], q.RegisterFrame(F[k], T[k])[0]), k
    before = p.poses()
    bad = T[0].copy()
    bad[len(bad) // 2] = np.nan
    with pytest.raises(sage.SageIcpError) as e:
        p.RegisterFrame(F[0], bad)
    assert e.value.code == sage.ERR_INVALID
    dp = ctypes.POINTER(ctypes.c_double)
    pose = np.empty(7)
    rc = sage.lib().sageicp_pipeline_register_frame_timestamps(p._h, F[0].ctypes.data_as(dp), None, len(F[0]),
                                                               pose.ctypes.data_as(dp), None, None, None, None)
    assert rc == sage.ERR_INVALID
    assert np.array_equal(p.poses(), before)


@pytest.mark.gpu
def test_deskew_shim_equals_deskew_scan(gpu_sage, tmp_path):
    exe = str(tmp_path / "deskew_user")
    lib_dir = os.path.join(ROOT, "sage-icp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "shim_stubs"),
                           "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                           "-I", os.path.join(ROOT, "sage-icp_amd", "shim_deskew"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_stubs", "deskew_user.cpp"),
                           "-L", lib_dir, "-l:libsageicp_hip.so", "-Wl,-rpath," + lib_dir, "-o", exe])
    S = _stream(2)
    f, t, P = S["frames"][1], S["timestamps"][1], S["poses"]
    f.tofile(str(tmp_path / "frame.f64"))
    np.ascontiguousarray(t).tofile(str(tmp_path / "ts.f64"))
    np.concatenate([P[0], P[1]]).tofile(str(tmp_path / "poses.f64"))
    r = subprocess.run([exe, str(tmp_path / "frame.f64"), str(tmp_path / "ts.f64"), str(tmp_path / "poses.f64"),
                        str(tmp_path / "out.f64")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = np.fromfile(str(tmp_path / "out.f64"), dtype=np.float64).reshape(-1, 4)
    assert np.array_equal(out, gpu_sage.deskew_scan(f, t, P[0], P[1]))
