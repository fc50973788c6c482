"""Preprocess()'s dynamic vehicle filter on the device (csrc/dyn_filter.hip; core/Preprocessing.cpp:95-172) against the
independent CPU restatement tests/dynfilter_ref.cpp: row for row and in order, standalone, inside the pipeline (with
and without prefetch) and through the opt-in Preprocessing shim."""
import os
import subprocess

import numpy as np
import pytest

import dynref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEH = dynref.KITTI_VEHICLES


def _dev(sage, f, dy_th=0.5, dyn=VEH, lm=(44, 48), **ranges):
    r = dict(max_range=100.0, min_range=5.0, label_max_range=50.0)
    r.update(ranges)
    return sage.preprocess(f, r["max_range"], r["min_range"], r["label_max_range"], dynamic_vehicle_filter=True,
                           dy_th=dy_th, dynamic_labels=dyn, landmark_labels=lm, return_info=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(dynref.kat_scenes()))
def test_known_answer_scenes_on_device(gpu_sage, name):
    frame, dy_th, expected = dynref.kat_scenes()[name]
    out, info = _dev(gpu_sage, frame, dy_th, (10,), (44,), **dynref.KAT_RANGES)
    assert np.array_equal(out, expected)
    ref, rinfo = dynref.preprocess(frame, dy_th=dy_th, dynamic_labels=(10,), landmark_labels=(44,), **dynref.KAT_RANGES)
    assert all(info[k] == rinfo[k] for k in rinfo)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_full_scans_match_the_restatement(gpu_sage, seed):
    from sage_icp_amd import synthetic_dynamic as sd
    f = sd.make_dynamic_scan(seed)
    cases = [(th, (44, 48)) for th in (0.05, 0.1, 0.5, 0.9)] + [(0.5, ()), (0.5, (99,))]
    for th, lm in cases:
        out, info = _dev(gpu_sage, f, th, VEH, lm)
        ref, rinfo = dynref.preprocess(f, dy_th=th, landmark_labels=lm)
        assert out.shape == ref.shape and np.array_equal(out, ref), (seed, th, lm)
        assert all(info[k] == rinfo[k] for k in rinfo), (seed, th, lm, info, rinfo)
        if not lm or lm == (99,):
            assert info["clusters_kept"] == 0 and info["points_removed"] == info["vehicle_points"]


@pytest.mark.gpu
def test_info_counts_match_the_scene(gpu_sage):
    from sage_icp_amd import synthetic_dynamic as sd
    f, parts = sd.make_dynamic_scan(5, return_parts=True)
    out, info = _dev(gpu_sage, f, 0.5)
    assert info["clusters"] == 30 and info["clusters_kept"] == 20
    assert info["points_removed"] == len(parts["moving"]) + len(parts["kerb"]) + len(parts["fragment"])
    rows = {tuple(r) for r in out}
    assert all(tuple(f[i]) in rows for i in parts["parked"])                  # parked cars kept
    assert not any(tuple(f[i]) in rows for i in parts["moving"])             # moving cars removed
    assert not any(tuple(f[i]) in rows for i in parts["fragment"])           # fragments removed
    far = f[parts["far"]].copy()
    far[:, 3] = 0.0                                                           # beyond 50 m: zeroed, ordinary points
    assert all(tuple(r) in rows for r in far)


@pytest.mark.gpu
def test_without_vehicles_equals_preprocess(gpu_sage):
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(3, 1, points_per_frame=60000)
    f = frames[0]
    out, info = _dev(gpu_sage, f, 0.5, (12345,))
    assert info["vehicle_points"] == 0
    assert np.array_equal(out, gpu_sage.preprocess(f, 100.0, 5.0, 50.0))
    empty, _ = _dev(gpu_sage, np.zeros((0, 4)))
    assert len(empty) == 0


@pytest.mark.gpu
def test_non_finite_label_is_refused_as_a_whole(gpu_sage):
    from sage_icp_amd import synthetic_dynamic as sd
    f = sd.make_dynamic_scan(6, n=20000)
    g = f.copy()
    k = int(np.argmax((np.linalg.norm(g[:, :3], axis=1) > 6.0) & (np.linalg.norm(g[:, :3], axis=1) < 40.0)))
    g[k, 3] = np.nan
    with pytest.raises(gpu_sage.SageIcpError) as e:
        _dev(gpu_sage, g)
    assert e.value.code == gpu_sage.ERR_INVALID
    out, _ = _dev(gpu_sage, f)          # the next call is unaffected
    assert np.array_equal(out, dynref.preprocess(f)[0])


def _stream(n_frames=30):
    from sage_icp_amd import synthetic_dynamic as sd
    frames, _ = sd.make_dynamic_stream(21, n_frames, n=40000)
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("reference_order", [True, False])
def test_pipeline_with_filter_equals_pipeline_fed_filtered_frames(gpu_sage, oracle, reference_order):
    sage = gpu_sage
    frames = _stream()
    filtered = [dynref.preprocess(f, dy_th=0.5)[0] for f in frames]
    sage.set_downsample_order(reference_order)
    oracle.set_robin_order(1 if reference_order else 0)
    try:
        a = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
        cfg = sage.make_pipeline_config()
        b = sage.SageICP(cfg)
        o = oracle.Pipeline(cfg) if reference_order else None
        for k, (f, g) in enumerate(zip(frames, filtered)):
            pa, _, _, ns_a, st_a = a.RegisterFrame(f)
            info = a.dynamic_filter_info()
            assert info["vehicle_points"] > 0 and info["clusters_kept"] > 0, k
            pb, _, _, ns_b, st_b = b.RegisterFrame(g)         # the filter-off crop of a filtered frame changes nothing
            assert np.array_equal(pa, pb) and ns_a == ns_b and st_a.iterations == st_b.iterations, k
            if o is not None:
                po, ns_o, _, st_o = o.register_frame(g)
                assert ns_o == ns_a, k
                assert np.max(np.abs(po - pa)) < 1e-7, (k, po, pa)
                if k:
                    assert st_o.iterations == st_a.iterations, k
        assert np.array_equal(a.LocalMap(), b.LocalMap())
    finally:
        sage.set_downsample_order(True)
        oracle.set_robin_order(0)


@pytest.mark.gpu
def test_pipeline_filter_with_prefetch_is_bit_identical(gpu_sage):
    sage = gpu_sage
    frames = [np.ascontiguousarray(f) for f in _stream(12)]
    a = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
    b = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
    for k, f in enumerate(frames):
        pa, _, _, ns_a, st_a = a.RegisterFrame(f)
        if k + 1 < len(frames):
            b.prefetch(frames[k + 1])
        if k == 6:      # changing the setting drops the prepared frame; the next frame is computed afresh
            b.set_dynamic_vehicle_filter(True, 0.5, 5, (44, 48))
        pb, _, _, ns_b, st_b = b.RegisterFrame(f)
        assert np.array_equal(pa, pb) and ns_a == ns_b and st_a.iterations == st_b.iterations, k
        assert a.dynamic_filter_info()["points_removed"] == b.dynamic_filter_info()["points_removed"], k
    assert np.array_equal(a.LocalMap(), b.LocalMap())


@pytest.mark.gpu
def test_preprocessing_shim_runs_the_filter(gpu_sage, tmp_path):
    from sage_icp_amd import synthetic_dynamic as sd
    exe = str(tmp_path / "dynfilter_user")
    lib_dir = os.path.join(ROOT, "sage-icp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "shim_stubs"),
                           "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                           "-I", os.path.join(ROOT, "sage-icp_amd", "shim_preprocessing"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_stubs", "dynfilter_user.cpp"),
                           "-L", lib_dir, "-l:libsageicp_hip.so", "-Wl,-rpath," + lib_dir, "-o", exe])
    f = sd.make_dynamic_scan(7)
    src, dst = str(tmp_path / "frame.f64"), str(tmp_path / "out.f64")
    f.tofile(src)
    r = subprocess.run([exe, src, dst, "0.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = np.fromfile(dst, dtype=np.float64).reshape(-1, 4)
    assert np.array_equal(out, dynref.preprocess(f, dy_th=0.5)[0])
