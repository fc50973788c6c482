"""Parity of the HIP path (through the C ABI) against the CPU oracle and the golden vectors.
Every test here needs a real MI355X:  python -m pytest tests -m gpu

Bars: correspondences index-exact (same query indices, bit-identical targets); Gauss-Newton sums
1e-10 relative (fp64, different but fixed summation order); registration pose within the
north-star tolerance 1e-4 m / 1e-4 rad of the oracle (observed ~1e-9)."""
import glob
import os

import numpy as np
import pytest


def _examples(n):
    """SAGE_TEST_EXAMPLES=k runs k times the usual number of random examples (campaigns; profiles/README.md)"""
    return n * max(1, int(os.environ.get("SAGE_TEST_EXAMPLES", "1")))
from hypothesis import HealthCheck, given, settings, strategies as st

pytestmark = pytest.mark.gpu

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "street_*.npz")))
TOL_M = 1e-4
TOL_RAD = 1e-4


def pose_error(oracle, A, B):
    e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(A), B))
    return np.linalg.norm(e[:3]), np.linalg.norm(e[3:])


def both_maps(sage, oracle, stream, vs=1.0, md=100.0, basic=20, critical=20):
    a = sage.VoxelHashMap(vs, md, basic, critical)
    b = oracle.Map(vs, md, basic, critical)
    a.AddPoints(stream)
    b.add_points(stream)
    return a, b


def random_scene(seed, n_map=20000, n_q=3000, span=12.0, labels=(0, 40, 50, 70, 71, 80)):
    rng = np.random.default_rng(seed)
    mp = rng.uniform(-span, span, size=(n_map, 4))
    mp[:, 2] = rng.uniform(-2, 3, n_map)
    mp[:, 3] = rng.choice(labels, size=n_map)
    q = rng.uniform(-span - 1.5, span + 1.5, size=(n_q, 4))
    q[:, 2] = rng.uniform(-3, 4, n_q)
    q[:, 3] = rng.choice(labels, size=n_q)
    return mp, q


# ------------------------------------------------------------------ GetCorrespondences
@pytest.mark.parametrize("seed,vs,basic,critical,th,md", [
    (1, 1.0, 20, 20, 0.4, 6.0), (2, 0.8, 20, 20, 0.05, 0.9), (3, 1.0, 20, 20, 1.0, 2.0),
    (4, 0.5, 3, 2, 0.8, 0.4), (5, 2.5, 60, 60, 0.4, 3.0), (6, 1.0, 1, 0, 0.4, 6.0),
    (7, 3.0, 128, 127, 0.2, 6.0)])
def test_correspondences_index_exact(gpu_sage, oracle, seed, vs, basic, critical, th, md, scan_form):
    mp, q = random_scene(seed)
    a, b = both_maps(gpu_sage, oracle, mp, vs, 100.0, basic, critical)
    src, tgt, idx = a.GetCorrespondences(q, md, th, with_index=True)
    osrc, otgt, oidx = b.get_correspondences(q, md, th, with_index=True)
    assert len(oidx) > 0
    assert np.array_equal(idx, oidx)
    assert np.array_equal(tgt, otgt) and np.array_equal(src, osrc)


@settings(max_examples=_examples(150), deadline=None, suppress_health_check=list(HealthCheck))
@given(seed=st.integers(0, 2**31 - 1), vs=st.sampled_from([0.1, 0.3, 0.8, 1.0, 2.5]),
       th=st.sampled_from([0.05, 0.4, 1.0, 1.7]), md=st.sampled_from([0.2, 0.9, 2.0, 6.0]),
       basic=st.integers(0, 24), critical=st.integers(1, 24), span=st.sampled_from([1.5, 6.0, 20.0]),
       lw=st.integers(0, 4), compact=st.booleans(), n_q=st.sampled_from([1, 63, 700, 5000]), flat=st.booleans())
def test_get_correspondences_property(gpu_sage, oracle, seed, vs, th, md, basic, critical, span, lw,
                                      compact, n_q, flat):
    """random clouds, voxel sizes, capacities, thresholds, query counts, clustered queries and
    queries on voxel faces, in every kernel variant: the HIP search against the oracle, index for
    index and bit for bit (flat: the lanes of a query stride through its voxels as one sequence — a choice
    with 2 and 4 lanes per query, the rule with 8 and 16)"""
    old = {k: os.environ.get(k) for k in ("SAGEICP_LW", "SAGEICP_FILTER", "SAGEICP_FLAT")}
    os.environ["SAGEICP_LW"], os.environ["SAGEICP_FILTER"] = str(lw), "1" if compact else "0"
    os.environ["SAGEICP_FLAT"] = "1" if flat else "0"
    try:
        rng = np.random.default_rng(seed)
        labels = [0, 0, 10, 40, 44, 50, 70, 71, 80, 251]
        mp = rng.uniform(-span, span, size=(6000, 4))
        mp[:, 2] *= 0.2
        mp[:, 3] = rng.choice(labels, size=len(mp))
        q = rng.uniform(-span - vs, span + vs, size=(n_q, 4))
        q[:, 2] *= 0.2
        if seed % 4 == 1:                   # clustered queries: many share a home voxel
            q[:, :3] = q[0, :3] + rng.normal(size=(n_q, 3)) * 0.3 * vs
        q[:, 3] = rng.choice(labels, size=n_q)
        if seed % 3 == 0:                   # queries exactly on voxel faces
            q[:, :3] = np.round(q[:, :3] / vs) * vs
        a, b = both_maps(gpu_sage, oracle, mp, vs, 100.0, basic, critical)
        assert a.size() == b.size()
        src, tgt, idx = a.GetCorrespondences(q, md, th, with_index=True)
        osrc, otgt, oidx = b.get_correspondences(q, md, th, with_index=True)
        assert np.array_equal(idx, oidx)
        assert np.array_equal(tgt, otgt) and np.array_equal(src, osrc)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_golden_vectors(gpu_sage, oracle, path, scan_form):
    g = np.load(path)
    vs, md, basic, critical, th, max_dist, kernel = g["params"]
    m = gpu_sage.VoxelHashMap(vs, md, int(basic), int(critical))
    m.AddPoints(g["map_stream"])
    assert [m.size(), m.num_voxels()] == list(g["map_size"])
    src, tgt, idx = m.GetCorrespondences(g["queries"], max_dist, th, with_index=True)
    assert np.array_equal(idx, g["corr_idx"]) and np.array_equal(tgt, g["corr_tgt"])
    T, JTJ, JTr = gpu_sage.align_clouds(src, tgt, kernel)
    assert np.allclose(JTJ, g["align_JTJ"], rtol=1e-10, atol=1e-7)
    assert np.allclose(JTr, g["align_JTr"], rtol=1e-10, atol=1e-7)
    dt, dr = pose_error(oracle, g["align_pose"], T)
    assert dt < 1e-9 and dr < 1e-9
    pose, st = gpu_sage.register_frame(g["scan"], m, gpu_sage.IDENTITY, max_dist, kernel, th,
                                       return_stats=True)
    dt, dr = pose_error(oracle, g["reg_pose"], pose)
    assert dt < TOL_M and dr < TOL_RAD
    assert dt < 1e-7 and dr < 1e-7, "far looser than fp64 needs: something is off"
    assert st.iterations == g["reg_iterations"][0]
    assert [st.n_corr_first, st.n_corr_last] == list(g["reg_n_corr"])


def test_edge_cases(gpu_sage, oracle, scan_form):
    sage = gpu_sage
    m = sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints([[1.25, 0.5, 0.5, 7], [-0.25, 0.5, 0.5, 7]])
    # equidistant candidates in different voxels: x-outer enumeration -> voxel 0 before voxel 1
    _, tgt = m.GetCorrespondences([[0.5, 0.5, 0.5, 7]], 6.0, 0.4)
    assert tgt[0, 0] == -0.25
    # same voxel: insertion order
    m = sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints([[0.75, 0.5, 0.5, 7], [0.25, 0.5, 0.5, 7]])
    _, tgt = m.GetCorrespondences([[0.5, 0.5, 0.5, 7]], 6.0, 0.4)
    assert tgt[0, 0] == 0.75
    # empty query set, and an empty 27-neighbourhood (reference hazard H1 -> rejected)
    src, tgt = m.GetCorrespondences(np.zeros((0, 4)), 6.0, 0.4)
    assert src.shape == (0, 4)
    src, _ = m.GetCorrespondences([[30.5, 0.5, 0.5, 7]], 100.0, 0.4)
    assert len(src) == 0
    # acceptance uses the unscaled distance
    m = sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints([[0.9, 0.5, 0.5, 40]])
    assert len(m.GetCorrespondences([[0.1, 0.5, 0.5, 40]], 0.7, 0.05)[0]) == 0
    assert len(m.GetCorrespondences([[0.1, 0.5, 0.5, 40]], 0.81, 0.05)[0]) == 1
    # semantic preference and the unlabelled bonus
    m = sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints([[0.40, 0.5, 0.5, 50], [0.65, 0.5, 0.5, 40]])
    assert m.GetCorrespondences([[0.5, 0.5, 0.5, 40]], 6.0, 0.4)[1][0, 3] == 40
    assert m.GetCorrespondences([[0.5, 0.5, 0.5, 40]], 6.0, 1.0)[1][0, 3] == 50
    assert m.GetCorrespondences([[0.5, 0.5, 0.5, 0]], 6.0, 0.4)[1][0, 0] == 0.40
    # empty map
    e = sage.VoxelHashMap(1.0, 100.0)
    assert len(e.GetCorrespondences([[0.5, 0.5, 0.5, 40]], 6.0, 0.4)[0]) == 0


def test_zero_straddle_and_negative_coordinates(gpu_sage, oracle, scan_form):
    mp, q = random_scene(11, n_map=3000, n_q=2000, span=1.8)
    a, b = both_maps(gpu_sage, oracle, mp)
    _, tgt, idx = a.GetCorrespondences(q, 6.0, 0.4, with_index=True)
    _, otgt, oidx = b.get_correspondences(q, 6.0, 0.4, with_index=True)
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)


def test_queries_exactly_on_voxel_faces(gpu_sage, oracle, scan_form):
    rng = np.random.default_rng(12)
    mp, _ = random_scene(12, n_map=8000, span=6.0)
    q = np.round(rng.uniform(-6, 6, size=(2000, 4)) / 0.8) * 0.8      # multiples of the voxel size
    q[:, 3] = 40
    a, b = both_maps(gpu_sage, oracle, mp, vs=0.8)
    _, tgt, idx = a.GetCorrespondences(q, 2.0, 0.4, with_index=True)
    _, otgt, oidx = b.get_correspondences(q, 2.0, 0.4, with_index=True)
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)


@pytest.mark.parametrize("n_q,box", [(5000, 1.6), (700, 4.0), (64, 0.4), (33, 0.9)])
def test_dense_queries_share_voxels(gpu_sage, oracle, n_q, box, scan_form):
    """many queries per home voxel: exercises every (queries x candidates) lane split of k_nn"""
    rng = np.random.default_rng(14)
    mp, _ = random_scene(14, n_map=30000, span=5.0)
    q = rng.uniform(-box, box, size=(n_q, 4))
    q[:, 3] = rng.choice([0, 40, 50, 70, 71, 80], size=n_q)
    a, b = both_maps(gpu_sage, oracle, mp, vs=1.0)
    _, tgt, idx = a.GetCorrespondences(q, 2.0, 0.4, with_index=True)
    _, otgt, oidx = b.get_correspondences(q, 2.0, 0.4, with_index=True)
    assert len(oidx) > 0.5 * n_q
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)


def test_near_ties_and_exotic_labels_stay_exact(gpu_sage, oracle, scan_form):
    """adversarial input for k_nn's f32 filter: clusters of candidates whose distances differ by
    far less than f32 resolution (many finalists / exact fallback), exact duplicates (index
    tie-break), far-from-origin coordinates, fractional and huge labels (generic-label path)"""
    rng = np.random.default_rng(15)
    centre = np.array([4321.0, -2750.0, 12.0])
    mp = rng.uniform(-4, 4, size=(6000, 4))
    mp[:, :3] += centre
    mp[:, 3] = rng.choice([0, 40, 50, 70], size=len(mp))
    # shells of points at almost identical distance around 40 probe positions
    probes = rng.uniform(-3, 3, size=(40, 3)) + centre
    extra = []
    for c in probes:
        dirs = rng.normal(size=(12, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        r = 0.3 + rng.uniform(-1e-9, 1e-9, size=12)
        pts = c + dirs * r[:, None]
        extra.append(np.c_[pts, rng.choice([0, 40, 50], size=12)])
        extra.append(np.c_[pts[:3], [40, 40, 40]])                 # exact duplicates
    mp = np.vstack([mp] + extra)
    q = np.c_[probes, rng.choice([0, 40, 50], size=len(probes))]
    q = np.vstack([q, np.c_[rng.uniform(-4, 4, size=(3000, 3)) + centre,
                            rng.choice([0, 40, 50, 70], size=3000)]])
    for labels in ("int", "exotic"):
        m2, q2 = mp.copy(), q.copy()
        if labels == "exotic":
            m2[::7, 3] = 40.5
            m2[::11, 3] = 3.0e9
            q2[::5, 3] = 0.25
            q2[::13, 3] = -7.0
        a, b = both_maps(gpu_sage, oracle, m2, vs=1.0)
        for th in (0.4, 1.0, 2.5, 0.0):
            _, tgt, idx = a.GetCorrespondences(q2, 3.0, th, with_index=True)
            _, otgt, oidx = b.get_correspondences(q2, 3.0, th, with_index=True)
            assert len(oidx) > 2000
            assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt), (labels, th)


def test_mirror_refresh_after_updates(gpu_sage, oracle, scan_form):
    """dirty-block / table refresh: search between successive map mutations stays exact"""
    rng = np.random.default_rng(13)
    a = gpu_sage.VoxelHashMap(1.0, 18.0)
    b = oracle.Map(1.0, 18.0)
    for step in range(8):
        c = np.array([3.0 * step, 1.0 * step, 0.0])
        pts = rng.normal(size=(6000, 4)) * [8, 8, 1.5, 0] + np.append(c, 0)
        pts[:, 3] = rng.choice([0, 40, 50, 80], size=len(pts))
        a.Update(pts, c)
        b.add_points(pts)
        b.remove_far(c)
        q = rng.normal(size=(1500, 4)) * [8, 8, 1.5, 0] + np.append(c, 0)
        q[:, 3] = rng.choice([0, 40, 50, 80], size=len(q))
        _, tgt, idx = a.GetCorrespondences(q, 3.0, 0.4, with_index=True)
        _, otgt, oidx = b.get_correspondences(q, 3.0, 0.4, with_index=True)
        assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt), "step %d" % step
    c2 = a.clone()
    _, tgt2, idx2 = c2.GetCorrespondences(q, 3.0, 0.4, with_index=True)
    assert np.array_equal(idx2, oidx) and np.array_equal(tgt2, otgt)
    a.Clear()
    assert len(a.GetCorrespondences(q, 3.0, 0.4)[0]) == 0
    assert len(c2.GetCorrespondences(q, 3.0, 0.4)[0]) == len(oidx)


def test_map_of_ten_million_voxels_in_under_3_gb(gpu_sage, oracle):
    """A 0.1 m voxel map of more than 10 M voxels (KITTI-360-at-0.1-m scale; round 1 stopped at
    2^23 voxels, round 2 spent 13.8 GB of 40-point blocks on it): with size-classed regions a
    one-point voxel holds 4 point slots.  Correspondences index-exact against the oracle, a planted
    offset recovered, and the per-frame device-side update works at that size."""
    import torch
    free0 = torch.cuda.mem_get_info()[0]
    n = 222                                   # 222^3 = 10.9 M lattice points, one per 0.1 m voxel
    g = (np.arange(n, dtype=np.float64) - n // 2) * 0.1 + 0.031
    rng = np.random.default_rng(123)
    mp = np.empty((n * n * n, 4))
    mp[:, 0] = np.repeat(g, n * n)
    mp[:, 1] = np.tile(np.repeat(g, n), n)
    mp[:, 2] = np.tile(g, n * n)
    mp[:, :3] += rng.uniform(0.0, 0.035, size=(len(mp), 3))      # stays inside its voxel
    mp[:, 3] = rng.choice([0, 40, 50, 70, 71], size=len(mp))
    a = gpu_sage.VoxelHashMap(0.1, 100.0)
    a.AddPoints(mp)
    # (truncation toward zero: the two lattice layers around 0 share voxel 0 on every axis)
    assert a.num_voxels() == (n - 1) ** 3 > 10_000_000 and a.size() == len(mp)
    assert a.point_slots() * 32 < 1.6e9                 # 4 slots of 32 B per voxel, a few of 8
    a.sync()
    torch.cuda.synchronize()
    # the map in HBM: table (2^26 slots of 16 B = 1.07 GB) + points + block->region words
    assert free0 - torch.cuda.mem_get_info()[0] < 3.0e9
    b = oracle.Map(0.1, 100.0)
    b.add_points(mp)
    sel = rng.choice(len(mp), 60000, replace=False)
    q = mp[sel].copy()
    q[:, :3] += rng.normal(0.0, 0.02, size=(len(q), 3))
    _, tgt, idx = a.GetCorrespondences(q, 0.15, 0.8, with_index=True)
    _, otgt, oidx = b.get_correspondences(q, 0.15, 0.8, with_index=True)
    assert len(oidx) > 50000
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)
    T_gt = oracle.se3_exp(np.array([0.012, -0.008, 0.005, 0.0004, -0.0003, 0.0008]))
    scan = oracle.transform_points(oracle.se3_inv(T_gt), mp[sel])
    pose, st = gpu_sage.register_frame(scan, a, gpu_sage.IDENTITY, 0.3, 0.1 / 3.0, 0.8, return_stats=True)
    opose, ost = b.register_frame(scan, oracle.IDENTITY, 0.3, 0.1 / 3.0, 0.8)
    dt, dr = pose_error(oracle, opose, pose)
    assert st.converged == 1 and st.iterations == ost.iterations and dt < 1e-9 and dr < 1e-9
    dt, dr = pose_error(oracle, T_gt, pose)
    assert dt < 1e-3 and dr < 1e-4            # exact correspondences exist
    before = a.size()
    a.UpdateOnDevice(scan[:20000], pose)
    b.update(scan[:20000], pose)
    assert a.size() == b.size() >= before
    # ... with the scratch of a search, a registration and a device-side update on top
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] < 3.5e9


def test_maximum_voxel_capacity(gpu_sage, oracle, scan_form):
    """255 points per voxel (the ABI's limit): 27 x 255 candidates per query; search and
    device-side update stay exact"""
    rng = np.random.default_rng(77)
    mp = rng.uniform(-2.4, 2.4, size=(60000, 4))
    mp[:, 3] = rng.choice([0, 40, 50, 71], size=len(mp))
    a = gpu_sage.VoxelHashMap(1.0, 100.0, 200, 55)
    h = gpu_sage.VoxelHashMap(1.0, 100.0, 200, 55)
    b = oracle.Map(1.0, 100.0, 200, 55)
    a.AddPoints(mp)
    h.AddPoints(mp)
    b.add_points(mp)
    assert a.size() == b.size() and a.size() > 100 * 200
    q = rng.uniform(-2.6, 2.6, size=(900, 4))
    q[:, 3] = rng.choice([0, 40, 50, 71], size=len(q))
    _, tgt, idx = a.GetCorrespondences(q, 1.0, 0.4, with_index=True)
    _, otgt, oidx = b.get_correspondences(q, 1.0, 0.4, with_index=True)
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)
    more = rng.uniform(-3.0, 3.0, size=(20000, 4))
    more[:, 3] = rng.choice([0, 40, 50, 71, 80], size=len(more))
    a.UpdateOnDevice(more, gpu_sage.IDENTITY)
    h.Update(more, gpu_sage.IDENTITY)
    assert np.array_equal(a.Pointcloud(), h.Pointcloud())
    pose, st = gpu_sage.register_frame(q, a, gpu_sage.IDENTITY, 1.0, 0.3, 0.4, return_stats=True)
    b.add_points(more)
    opose, ost = b.register_frame(q, oracle.IDENTITY, 1.0, 0.3, 0.4)
    dt, dr = pose_error(oracle, opose, pose)
    assert st.iterations == ost.iterations and dt < 1e-9 and dr < 1e-9


# ------------------------------------------------------------------ AlignClouds / TransformPoints
@pytest.mark.parametrize("n", [0, 1, 63, 64, 1000, 70001])
def test_align_clouds_matches_oracle(gpu_sage, oracle, n):
    rng = np.random.default_rng(20 + n)
    src = rng.normal(size=(n, 4)) * 40
    tgt = src + rng.normal(size=(n, 4)) * 0.2
    T, JTJ, JTr = gpu_sage.align_clouds(src, tgt, 0.4)
    oT, oJ, orr = oracle.align_clouds(src, tgt, 0.4, nthreads=1)
    scale = max(1.0, np.abs(oJ).max())
    assert np.allclose(JTJ, oJ, rtol=1e-10, atol=1e-12 * scale)
    assert np.allclose(JTr, orr, rtol=1e-9, atol=1e-12 * scale)
    if n >= 6:       # fewer pairs leave the 6x6 system rank deficient: the step is not unique
        dt, dr = pose_error(oracle, oT, T)
        assert dt < 1e-9 and dr < 1e-9


def test_transform_points_matches_oracle(gpu_sage, oracle):
    rng = np.random.default_rng(30)
    T = oracle.se3_exp(rng.normal(size=6) * 0.5)
    pts = rng.normal(size=(5000, 4)) * 60
    out = gpu_sage.transform_points(T, pts)
    ref = oracle.transform_points(T, pts)
    assert np.array_equal(out[:, 3], pts[:, 3])
    assert np.allclose(out, ref, rtol=0, atol=1e-12)
    assert gpu_sage.transform_points(T, np.zeros((0, 4))).shape == (0, 4)


# ------------------------------------------------------------------ RegisterFrame
def _workload(gpu_sage, oracle, name, scale):
    from sage_icp_amd import synthetic as syn
    w = syn.make_workload(name, lambda: gpu_sage.VoxelHashMap(syn.WORKLOADS[name]["voxel"], 100.0),
                          scale=scale)
    om = oracle.Map(w["voxel"], 100.0)
    om.add_points(w["stream"])
    assert om.size() == w["map"].size()
    return w, om


@pytest.mark.parametrize("params", ["cold", "steady"])
def test_register_frame_pose_parity_c2_scaled(gpu_sage, oracle, params, scan_form):
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c2", 0.1)
    p = syn.PARAMS[params]
    pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                       p["kernel"], p["sem_th"], return_stats=True)
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"],
                                   p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < TOL_M and dr < TOL_RAD
    assert dt < 1e-7 and dr < 1e-7
    assert st.iterations == ost.iterations and st.converged == ost.converged == 1
    assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
    assert st.sum_candidates == ost.sum_candidates_total      # exact C_q accounting (roofline bytes)
    # resident-frame entry gives the same answer, bit for bit (deterministic reduction order)
    f = gpu_sage.Frame(w["map"], w["scan"])
    pose2 = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                    p["sem_th"])
    assert np.array_equal(pose, pose2)


@pytest.mark.parametrize("lw,flat", [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 1), (4, 1)])
def test_every_lanes_per_query_variant(gpu_sage, oracle, scan_form, lw, flat, monkeypatch):
    """k_icp is compiled for 1, 2, 4, 8 and 16 lanes per query and the library picks by frame size
    and voxel density (capi_internal.h::icp_lw), so a given workload only ever reaches one or two of the
    variants: each is forced in turn (SAGEICP_LW) in both scan forms and, with 2 and 4 lanes, in both orders
    the lanes take a query's points in (SAGEICP_FLAT; 8 and 16 lanes: always flat) — index-exact search, the
    same registration as the oracle's, the same exact candidate count."""
    from sage_icp_amd import synthetic as syn
    monkeypatch.setenv("SAGEICP_LW", str(lw))
    monkeypatch.setenv("SAGEICP_FLAT", str(flat))
    mp, q = random_scene(31 + lw)
    a, b = both_maps(gpu_sage, oracle, mp)
    for th, md in ((0.4, 6.0), (1.0, 2.0), (0.05, 0.9)):
        _, tgt, idx = a.GetCorrespondences(q, md, th, with_index=True)
        _, otgt, oidx = b.get_correspondences(q, md, th, with_index=True)
        assert len(oidx) > 0 and np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)
    w, om = _workload(gpu_sage, oracle, "c2", 0.05)
    p = syn.PARAMS["cold"]
    pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                       p["kernel"], p["sem_th"], return_stats=True)
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < 1e-7 and dr < 1e-7 and st.iterations == ost.iterations
    assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
    assert st.sum_candidates == ost.sum_candidates_total
    assert st.lanes_per_query == 1 << lw
    assert st.compact_scan == (1 if scan_form == "compact" else 0)


def test_full_size_regions_in_both_scan_forms(gpu_sage, oracle, scan_form, monkeypatch):
    """SAGEICP_SIZE_CLASSES=0: every voxel owns a region of max_points_per_voxel points (the
    layout of rounds 1-2) — the same index-exact search and the same registration as with size
    classes, in both scan forms"""
    from sage_icp_amd import synthetic as syn
    monkeypatch.setenv("SAGEICP_SIZE_CLASSES", "0")
    mp, q = random_scene(21)
    a, b = both_maps(gpu_sage, oracle, mp)
    for th in (0.4, 1.0):
        _, tgt, idx = a.GetCorrespondences(q, 6.0, th, with_index=True)
        _, otgt, oidx = b.get_correspondences(q, 6.0, th, with_index=True)
        assert len(oidx) > 0 and np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)
    w, om = _workload(gpu_sage, oracle, "c2", 0.1)
    p = syn.PARAMS["cold"]
    pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                       p["kernel"], p["sem_th"], return_stats=True)
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < 1e-7 and dr < 1e-7 and st.iterations == ost.iterations
    assert st.compact_scan == (1 if scan_form == "compact" else 0)


@pytest.mark.parametrize("params", ["dense", "dense_nosem"])
def test_register_frame_pose_parity_c5_scaled(gpu_sage, oracle, params, scan_form):
    """c5 (BASELINE configs[4]): dense scan vs a 0.1 m voxel map, semantic scaling on (0.8) / off (1.0)"""
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c5", 0.1)
    p = syn.PARAMS[params]
    pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                       p["kernel"], p["sem_th"], return_stats=True)
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"],
                                   p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < 1e-7 and dr < 1e-7
    assert st.iterations == ost.iterations and st.converged == ost.converged == 1
    assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
    assert 0 < st.n_corr_last < len(w["scan"])        # 0.1-0.2 m reach: part of the scan rejects
    assert st.sum_candidates == ost.sum_candidates_total
    gt, gr = pose_error(oracle, w["T_gt"], pose)
    assert gt < 0.03 and gr < 1e-3                    # the planted centimetre offset is recovered


def test_register_frame_pose_parity_c4_scaled(gpu_sage, oracle, scan_form):
    """c4 (BASELINE configs[3]: 500k-pt scan vs 10M-pt map, steady parameters) at one tenth of its
    size: pose, iteration count, correspondence counts and the exact C_q sum against the oracle"""
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c4", 0.1)
    assert w["map"].size() == 1_000_000 and len(w["scan"]) == 50_000
    p = syn.PARAMS["steady"]
    pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                       p["kernel"], p["sem_th"], return_stats=True)
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"],
                                   p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < TOL_M and dr < TOL_RAD
    assert dt < 1e-7 and dr < 1e-7
    assert st.iterations == ost.iterations and st.converged == ost.converged == 1
    assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
    assert st.sum_candidates == ost.sum_candidates_total
    # the two halves of the frame registered as the shards of a 2-rank run would see them give the
    # same correspondences as the whole (contiguous blocks)
    q = oracle.transform_points(pose, w["scan"])
    _, _, idx = w["map"].GetCorrespondences(q, p["max_dist"], p["sem_th"], with_index=True)
    h = len(q) // 2
    _, _, i0 = w["map"].GetCorrespondences(q[:h], p["max_dist"], p["sem_th"], with_index=True)
    _, _, i1 = w["map"].GetCorrespondences(q[h:], p["max_dist"], p["sem_th"], with_index=True)
    assert np.array_equal(idx, np.concatenate([i0, i1 + h]))


def test_c4_full_size_properties(gpu_sage, oracle):
    """c4 at full size (500k scan vs 10M map, the multi-GPU configuration) on one GPU: the oracle's FULL
    registration of this frame (minutes of CPU: run once in the build container by
    tests/golden/make_c4_golden.py, committed as tests/golden/c4_full.npz — pose, iteration count,
    correspondence counts, the exact sum of C_q; steady and cold parameters), then size-independent
    properties: convergence near the planted pose, idempotence, and index-exact correspondences against
    the oracle's search at the converged pose."""
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c4", 1.0)
    assert w["map"].size() == 10_000_000 and len(w["scan"]) == 500_000
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "c4_full.npz"))
    assert [int(x) for x in gold["map_size"]] == [w["map"].size(), om.num_voxels()]           # the same workload
    assert np.array_equal(gold["scan_checksum"], [float(np.sum(w["scan"][:, :3])), float(np.sum(w["scan"][:, 3]))])
    f = gpu_sage.Frame(w["map"], w["scan"])
    for params in ("cold", "steady"):
        p = syn.PARAMS[params]
        assert np.array_equal(gold[params + "_params"], [p["max_dist"], p["kernel"], p["sem_th"]])
        pose, st = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                           p["sem_th"], return_stats=True)
        iters, conv, nc_first, nc_last, sum_cq, _ = [int(x) for x in gold[params + "_counts"]]
        dt, dr = pose_error(oracle, gold[params + "_pose"], pose)
        assert dt < 1e-7 and dr < 1e-7, (params, dt, dr)
        assert (st.iterations, st.converged) == (iters, conv) and conv == 1
        assert (st.n_corr_first, st.n_corr_last) == (nc_first, nc_last)
        assert st.sum_candidates == sum_cq                                   # exact C_q accounting at 500k x 10M
    p = syn.PARAMS["steady"]
    assert st.converged == 1 and 0 < st.pairs_evaluated < st.sum_candidates
    dt, dr = pose_error(oracle, w["T_gt"], pose)
    assert dt < 0.05 and dr < 2e-3
    pose2, st2 = gpu_sage.register_frame(f, w["map"], pose, p["max_dist"], p["kernel"], p["sem_th"],
                                         return_stats=True)
    dt, dr = pose_error(oracle, pose, pose2)
    assert st2.iterations <= 3 and dt < 2e-4 and dr < 2e-4
    again, st3 = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                         p["sem_th"], return_stats=True)
    assert np.array_equal(again, pose) and st3.iterations == st.iterations      # bit-reproducible
    q = oracle.transform_points(pose, w["scan"])
    _, tgt, idx = w["map"].GetCorrespondences(q, p["max_dist"], p["sem_th"], with_index=True)
    _, otgt, oidx = om.get_correspondences(q, p["max_dist"], p["sem_th"], with_index=True)
    assert len(oidx) == st.n_corr_last or abs(len(oidx) - st.n_corr_last) < 50   # pose one step apart
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)


def test_register_frame_c1_plumbing(gpu_sage, oracle):
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c1", 1.0)
    p = syn.PARAMS["cold"]
    pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                       p["kernel"], p["sem_th"], return_stats=True)
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"],
                                   p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < 1e-7 and dr < 1e-7 and st.iterations == ost.iterations


def test_register_frame_with_initial_guess_and_edge_inputs(gpu_sage, oracle, scan_form):
    mp, q = random_scene(40, n_map=30000, n_q=2500, span=15.0)
    a, b = both_maps(gpu_sage, oracle, mp)
    kept = a.Pointcloud()
    rng = np.random.default_rng(41)
    T_gt = oracle.se3_exp(np.array([0.3, -0.2, 0.05, 0.004, -0.003, 0.03]))
    scan = oracle.transform_points(oracle.se3_inv(T_gt), kept[rng.choice(len(kept), 2500, False)])
    guess = oracle.se3_exp(np.array([0.25, -0.15, 0.0, 0, 0, 0.02]))
    pose, st = gpu_sage.register_frame(scan, a, guess, 3.0, 0.3, 0.4, return_stats=True)
    opose, ost = b.register_frame(scan, guess, 3.0, 0.3, 0.4)
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < 1e-7 and dr < 1e-7 and st.iterations == ost.iterations
    dt, dr = pose_error(oracle, T_gt, pose)
    assert dt < 1e-6 and dr < 1e-6          # exact correspondences exist: the planted pose
    # empty frame: one iteration, zero correspondences, pose == guess
    pose, st = gpu_sage.register_frame(np.zeros((0, 4)), a, guess, 3.0, 0.3, 0.4, return_stats=True)
    assert st.iterations == 1 and st.converged == 1 and np.allclose(pose, guess, atol=1e-15)
    # a frame with no correspondence at all
    far = np.array([[500.5, 0.5, 0.5, 1.0]])
    pose, st = gpu_sage.register_frame(far, a, gpu_sage.IDENTITY, 1.0, 0.3, 0.4, return_stats=True)
    assert st.iterations == 1 and st.n_corr_first == 0


@settings(max_examples=_examples(60), deadline=None, suppress_health_check=list(HealthCheck))
@given(seed=st.integers(0, 2**31 - 1), vs=st.sampled_from([0.3, 0.8, 1.0, 2.0]),
       sigma=st.sampled_from([0.3, 1.0, 2.0]), th=st.sampled_from([0.05, 0.4, 1.0]),
       lw=st.integers(0, 4), compact=st.booleans(), n_q=st.sampled_from([200, 3000, 12000]),
       noise=st.sampled_from([0.0, 0.02]), flat=st.booleans())
def test_register_frame_property(gpu_sage, oracle, seed, vs, sigma, th, lw, compact, n_q, noise, flat):
    """RegisterFrame on random scenes (voxel size, thresholds as the adaptive sigma gives them:
    max_corr 3 sigma, kernel sigma / 3; semantic threshold; frame size; a random planted motion and
    a random initial guess near it; with and without noise) in every kernel variant: the same
    iteration count, correspondence counts and pose as the oracle"""
    old = {k: os.environ.get(k) for k in ("SAGEICP_LW", "SAGEICP_FILTER", "SAGEICP_FLAT")}
    os.environ["SAGEICP_LW"], os.environ["SAGEICP_FILTER"] = str(lw), "1" if compact else "0"
    os.environ["SAGEICP_FLAT"] = "1" if flat else "0"
    try:
        rng = np.random.default_rng(seed)
        mp, _ = random_scene(seed % 1000, n_map=30000, n_q=10, span=15.0)
        a, b = both_maps(gpu_sage, oracle, mp, vs)
        kept = a.Pointcloud()
        T_gt = oracle.se3_exp(rng.normal(size=6) * np.array([0.2, 0.2, 0.05, 0.005, 0.005, 0.02]))
        pick = kept[rng.choice(len(kept), min(n_q, len(kept)), replace=False)]
        scan = oracle.transform_points(oracle.se3_inv(T_gt), pick)
        scan[:, :3] += rng.normal(size=(len(scan), 3)) * noise
        guess = oracle.se3_mul(T_gt, oracle.se3_exp(rng.normal(size=6) * np.array([0.05, 0.05, 0.02, 0.002, 0.002, 0.005])))
        pose, s1 = gpu_sage.register_frame(scan, a, guess, 3.0 * sigma, sigma / 3.0, th, return_stats=True)
        opose, s2 = b.register_frame(scan, guess, 3.0 * sigma, sigma / 3.0, th)
        dt, dr = pose_error(oracle, opose, pose)
        assert dt < 1e-7 and dr < 1e-7
        assert s1.iterations == s2.iterations and s1.converged == s2.converged
        assert s1.n_corr_first == s2.n_corr_first and s1.n_corr_last == s2.n_corr_last
        assert s1.sum_candidates == s2.sum_candidates_total
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("div,lw", [(1, None), (1, 1), (1, 3), (2, None), (4, None), (4, 2), (10, None), (10, 4)])
def test_ring_geometry_scene_family(gpu_sage, oracle, div, lw, monkeypatch):
    """the second scene family (synthetic.make_ring_scan: one revolution of a 64-beam sensor, by ray casting — density
    falling with range ring by ring, occlusion; a map built from such revolutions along a road): the library's own choice
    of lanes / scan form / loop and forced alternatives against the oracle's full registration — pose, iteration count,
    correspondence counts, exact C_q — at the scan's full size and at the sizes the pipeline's down-sampling leaves"""
    from sage_icp_amd import synthetic as syn
    if lw is not None:
        monkeypatch.setenv("SAGEICP_LW", str(lw))
    w = syn.make_ring_workload(lambda: gpu_sage.VoxelHashMap(1.0, 100.0), n_map_scans=12, az_steps=1024, scan_az_steps=2048)
    om = oracle.Map(1.0, 100.0)
    om.add_points(w["stream"])
    assert om.size() == w["map"].size() and om.num_voxels() == w["map"].num_voxels()
    scan = np.ascontiguousarray(w["scan"][::div])
    guess = w["T_gt"].copy()
    guess[4] -= 0.4
    for params in ("cold", "steady"):
        p = syn.PARAMS[params]
        pose, st = gpu_sage.register_frame(scan, w["map"], guess, p["max_dist"], p["kernel"], p["sem_th"], return_stats=True)
        opose, ost = om.register_frame(scan, guess, p["max_dist"], p["kernel"], p["sem_th"])
        dt, dr = pose_error(oracle, opose, pose)
        assert dt < 1e-7 and dr < 1e-7
        assert st.iterations == ost.iterations and st.converged == ost.converged == 1
        assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
        assert st.sum_candidates == ost.sum_candidates_total
        if lw is not None:
            assert st.lanes_per_query == 1 << lw
    gt, gr = pose_error(oracle, w["T_gt"], pose)
    assert gt < 0.1 and gr < 5e-3                  # the revolution is placed where it was taken


def test_streaming_frames_with_map_updates(gpu_sage, oracle, scan_form):
    """c3-style: register, update the map with the frame at the new pose, repeat — both
    backends restarted from the same state every frame."""
    from sage_icp_amd import synthetic as syn
    rng = np.random.default_rng(50)
    a = gpu_sage.VoxelHashMap(0.8, 60.0)
    b = oracle.Map(0.8, 60.0)
    pose = gpu_sage.IDENTITY.copy()
    step = syn.pose_from_rpy_t([0, 0, 0.5], [1.0, 0, 0])
    for k in range(6):
        T_true = pose if k == 0 else oracle.se3_mul(pose, step)
        frame = syn.make_scan(rng, 6000, 60.0, T_true, max_range=55.0)
        guess = T_true if k == 0 else oracle.se3_mul(pose, syn.pose_from_rpy_t([0, 0, 0.4], [0.9, 0.02, 0]))
        new_pose = gpu_sage.register_frame(frame, a, guess, 1.5, 0.17, 0.05)
        opose, _ = b.register_frame(frame, guess, 1.5, 0.17, 0.05)
        dt, dr = pose_error(oracle, opose, new_pose)
        assert dt < TOL_M and dr < TOL_RAD, "frame %d: %g m %g rad" % (k, dt, dr)
        assert dt < 1e-7 and dr < 1e-7
        a.Update(frame, opose)       # same state on both sides for the next frame
        b.update(frame, opose)
        assert a.size() == b.size()
        pose = opose


def test_rccl_refuses_two_ranks_on_one_device():
    """documented limit of this box: RCCL (like NCCL) rejects a communicator with two ranks on the
    same GPU, so the N > 1 RCCL path can only run on the driver's multi-GPU node; what runs here is
    the 1-rank RCCL path, the direct exchange between 2 processes and between 2-3 ranks of one
    process (below)"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAGEICP_BENCH_DEVICE="0", SAGEICP_NO_P2P="1", MASTER_ADDR="127.0.0.1", NCCL_DEBUG="WARN")
    run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1",
                          "--warmup", "0", "--scale", "0.05", "--no-cpu-baseline"],
                         capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode != 0      # bench.py --gpus 2 launched its own ranks; RCCL refused the pair
    # ... and it failed for THAT reason, where the communicator is created — not an import error, a
    # typo or an out-of-memory somewhere else
    text = (run.stdout + run.stderr).lower()
    print(text[-6000:])                                      # (shown by pytest when the assertions below fail)
    # (the first RCCL communicator of a rank is torch.distributed's own; RCCL names the reason itself)
    assert "duplicate gpu detected" in text and "invalid usage" in text, \
        "bench.py --gpus 2 failed, but not because RCCL refused two ranks on one device"


def test_register_frame_through_rccl_comm_world1(gpu_sage, oracle, monkeypatch):
    """the RCCL exchange path (reduce -> ncclAllReduce -> solve) with a one-rank communicator: bit for bit the
    launch-per-iteration loop without a communicator (the one-launch loop may take another number of lanes per
    query — other waves, other roundings of the per-wave sums — and is compared in tests/test_loop_kernel.py)"""
    monkeypatch.setenv("SAGEICP_LOOP", "0")
    w, om = _workload(gpu_sage, oracle, "c2", 0.05)
    f = gpu_sage.Frame(w["map"], w["scan"])
    ref = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4)
    comm = gpu_sage.Comm(gpu_sage.Comm.unique_id(), 0, 1, 0)
    got = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4, comm=comm)
    assert np.array_equal(ref, got)


def test_chunked_rccl_loop_equals_polled_loop(gpu_sage, oracle, monkeypatch):
    """the loop form every N > 1 RCCL run uses (fixed chunks of 4, 8, 16, ... iterations, one
    synchronisation per chunk, every rank enqueuing the same number of all-reduces) against the
    host-polled loop of one GPU: same bits, same iteration count — through a one-rank RCCL
    communicator, and for the plain single-GPU call forced into chunks (SAGEICP_CHUNKED=1)"""
    from sage_icp_amd import synthetic as syn
    monkeypatch.setenv("SAGEICP_LOOP", "0")     # (the launch-per-iteration loop on both sides: equal lanes per query)
    w, om = _workload(gpu_sage, oracle, "c2", 0.05)
    f = gpu_sage.Frame(w["map"], w["scan"])
    for prm in ("cold", "steady"):
        p = syn.PARAMS[prm]
        args = (f, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"])
        ref, rst = gpu_sage.register_frame(*args, return_stats=True)
        comm = gpu_sage.Comm(gpu_sage.Comm.unique_id(), 0, 1, 0)
        info = comm.describe()
        assert info["has_rccl"] == 1 and info["rccl_ranks"] == 1 and info["rccl_rank"] == 0
        assert info["p2p_enabled"] == 0 and info["nranks"] == 1
        got, gst = gpu_sage.register_frame(*args, comm=comm, return_stats=True)     # chunked: RCCL
        assert np.array_equal(ref, got) and gst.iterations == rst.iterations
        assert gst.n_corr_last == rst.n_corr_last and gst.sum_candidates == rst.sum_candidates
        monkeypatch.setenv("SAGEICP_CHUNKED", "1")
        try:
            again, ast_ = gpu_sage.register_frame(*args, return_stats=True)         # chunked: no comm
            direct = gpu_sage.Comm(None, 0, 1, 0)
            direct.p2p_connect([direct.p2p_export()])
            d, dst = gpu_sage.register_frame(*args, comm=direct, return_stats=True)  # chunked: direct exchange
        finally:
            monkeypatch.delenv("SAGEICP_CHUNKED")
        assert np.array_equal(ref, again) and ast_.iterations == rst.iterations
        assert np.array_equal(ref, d) and dst.iterations == rst.iterations
        assert direct.describe()["rccl_ranks"] == -1 and direct.describe()["p2p_enabled"] == 1


def test_register_frame_through_direct_exchange_world1(gpu_sage, oracle, monkeypatch):
    """the direct exchange path (reduce -> stores into the mapped blocks -> tags -> solve, all inside k_fin)
    with a one-rank communicator that has no RCCL side; the RCCL communicator can switch to it
    and back"""
    monkeypatch.setenv("SAGEICP_LOOP", "0")     # (the launch-per-iteration loop on both sides: equal lanes per query)
    w, om = _workload(gpu_sage, oracle, "c2", 0.05)
    f = gpu_sage.Frame(w["map"], w["scan"])
    ref, rst = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4, return_stats=True)
    comm = gpu_sage.Comm(None, 0, 1, 0)
    with pytest.raises(gpu_sage.SageIcpError):      # neither RCCL nor a connected exchange yet
        gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4, comm=comm)
    comm.p2p_connect([comm.p2p_export()])
    assert comm.p2p_enabled
    for _ in range(3):                              # the exchange counter carries over between calls
        got, st = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4, comm=comm,
                                          return_stats=True)
        assert np.array_equal(ref, got) and st.iterations == rst.iterations
    both = gpu_sage.Comm(gpu_sage.Comm.unique_id(), 0, 1, 0)
    both.p2p_connect([both.p2p_export()])
    a = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4, comm=both)
    both.p2p_enable(False)
    b = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4, comm=both)
    assert np.array_equal(a, ref) and np.array_equal(b, ref)


def test_single_process_multi_device_mode(gpu_sage, oracle):
    """sageicp_map_set_devices: one map handle spanning two ranks (both on the one GPU of this
    box), the frame sharded inside sage_icp::RegisterFrame's entry, one host thread per rank, the
    sums exchanged through peer-mapped blocks — same pose and iteration count as one device, for
    the host-buffer entry, the resident-frame entry, after a device-side Update and for a clone"""
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c2", 0.1)
    p = syn.PARAMS["cold"]
    ref, rst = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                       p["sem_th"], return_stats=True)
    m2 = gpu_sage.VoxelHashMap(1.0, 100.0)
    m2.set_devices([0, 0])
    assert m2.num_devices() == 2
    m2.AddPoints(w["stream"])
    assert m2.size() == w["map"].size()
    for frame in (w["scan"], gpu_sage.Frame(m2, w["scan"])):
        pose, st = gpu_sage.register_frame(frame, m2, gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                           p["sem_th"], return_stats=True)
        dt, dr = pose_error(oracle, ref, pose)
        assert dt < 1e-9 and dr < 1e-9 and st.iterations == rst.iterations
        assert st.n_queries == len(w["scan"]) and st.sum_candidates == rst.sum_candidates
        assert st.n_corr_last == rst.n_corr_last
    # three ranks, an uneven split, after a device-side map update on every copy; and a clone
    m3 = gpu_sage.VoxelHashMap(1.0, 100.0)
    m3.set_devices([0, 0, 0])
    m3.AddPoints(w["stream"])
    m3.UpdateOnDevice(w["scan"][:5001], ref)
    w["map"].UpdateOnDevice(w["scan"][:5001], ref)
    assert m3.size() == w["map"].size()
    one = gpu_sage.register_frame(w["scan"][:9001], w["map"], ref, p["max_dist"], p["kernel"], p["sem_th"])
    for mm in (m3, m3.clone()):
        assert mm.num_devices() == 3
        got = gpu_sage.register_frame(w["scan"][:9001], mm, ref, p["max_dist"], p["kernel"], p["sem_th"])
        dt, dr = pose_error(oracle, one, got)
        assert dt < 1e-9 and dr < 1e-9


@pytest.mark.parametrize("chunked", [0, 1])
def test_direct_exchange_between_two_processes(gpu_sage, tmp_path, chunked):
    """bench.py with two ranks on the one GPU of the box (gloo rendezvous, no RCCL): each rank
    registers half of the frame and the sums travel through the HIP-IPC mapped blocks"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # chunked: the loop form every RCCL run uses (fixed chunks of iterations, one synchronisation per
    # chunk) around the product's own exchange — two processes, the HIP path on each shard
    env = dict(os.environ, SAGEICP_BENCH_DEVICE="0", SAGEICP_BENCH_BACKEND="gloo",
               SAGEICP_P2P_TIMEOUT_S="5", MASTER_ADDR="127.0.0.1", SAGEICP_CHUNKED=str(chunked))
    common = ["--steps", "2", "--warmup", "1", "--scale", "0.1", "--no-cpu-baseline"]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(29533 + 2 * chunked),
                          os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, env=env, timeout=600)
    assert two.returncode == 0, two.stderr[-2000:]
    d2 = json.loads(two.stdout.strip().splitlines()[-1])
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common,
                         capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    assert d2["n_gpus"] == 2 and "direct exchange" in d2["config"]["parallelism"]
    assert d2["config"]["iterations_per_frame"] == d1["config"]["iterations_per_frame"]
    assert d2["config"]["converged"] and d2["config"]["pose_error_vs_planted"] == d1["config"]["pose_error_vs_planted"]
    br = d2["config"]["iteration_breakdown"]        # the first real SCALE line explains itself
    assert br and br["loop_form"]
    lp = br["launch_per_iteration"]
    assert lp["shard_compute_us_per_iteration"] > 1.0 and lp["exchange_us_per_iteration"] > 1.0
    if not chunked:        # (the polled loop: each rank's half of the frame runs in ONE launch, on its half of the CUs)
        assert "one launch" in br["loop_form"] and br["iteration_us"] > 1.0


def test_one_rank_loses_its_one_launch_loop_and_all_ranks_follow_in_step(gpu_sage):
    """under a communicator a k_loop wait that timed out used to be a hard error that poisoned the
    communicator.  Now the rank that gives up says so through the exchange it was about to make (P2pBlock::abort_tag),
    every rank leaves that exchange with it and registers the frame again through the launch-per-iteration form — same
    lanes per query, same bits: two processes on the one GPU, rank 1's solving wave gives its own workgroups 10 ns
    (SAGEICP_LOOP_COUNT_TIMEOUT_RANK=1) in every frame; the run ends normally with the registration of an untroubled run,
    and the line says what happened on which rank"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAGEICP_BENCH_DEVICE="0", SAGEICP_BENCH_BACKEND="gloo", SAGEICP_P2P_TIMEOUT_S="5",
               MASTER_ADDR="127.0.0.1", SAGEICP_LOOP_COOLDOWN="0")
    common = ["--steps", "2", "--warmup", "1", "--scale", "0.1", "--no-cpu-baseline"]

    def two_ranks(extra, port):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                            "--gpus", "2", "--exchange", "direct"] + common,
                           capture_output=True, text=True, env=dict(env, **extra), timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr

    good, _ = two_ranks({}, 29541)
    hurt, err = two_ranks({"SAGEICP_LOOP_COUNT_TIMEOUT_RANK": "1", "SAGEICP_LOOP_COUNT_TIMEOUT_TICKS": "1"}, 29543)
    assert [r["loop_form"] for r in good["config"]["per_rank"]] == ["one launch", "one launch"]
    assert good["config"]["exchange"] == hurt["config"]["exchange"] == "direct"
    # every frame of the troubled run went through the launch-per-iteration form on BOTH ranks: rank 1 because its own launch
    # gave up (TIMEOUT = 1), rank 0 because its peer said so (PEER = 4)
    pr = {r["rank"]: r for r in hurt["config"]["per_rank"]}
    assert pr[0]["loop_form"] == pr[1]["loop_form"] == "launch per iteration"
    assert pr[1]["loop_timeouts"] >= 3 and pr[1]["last_fallback"] == 1
    assert pr[0]["loop_timeouts"] == 0 and pr[0]["last_fallback"] == 4
    assert "timed out" in err
    # ... and registered the frame exactly as the untroubled run did
    assert hurt["config"]["iterations_per_frame"] == good["config"]["iterations_per_frame"]
    assert hurt["config"]["converged"] and hurt["config"]["pose_error_vs_planted"] == good["config"]["pose_error_vs_planted"]
    assert hurt["config"]["correspondences_first_last"] == good["config"]["correspondences_first_last"]


def test_chained_launches_under_a_communicator(gpu_sage):
    """frames beyond the one-launch loop under a communicator with the direct exchange (SAGEICP_CHAIN_COMM=1: off by default,
    capi_run.hip says why): the launches of the iterations chained beside each rank's resident solving wave, which makes
    the exchange (as in the one-launch loop) — no k_fin.
    Two processes on the one GPU, the one-launch loop switched off: the chained run registers the frame exactly as the
    run with k_fin between the launches; and a rank whose solving wave loses its launches (10 ns of patience) takes its
    peer out of the exchange with it, both register the frame again with k_fin, in step, and the run ends normally"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAGEICP_BENCH_DEVICE="0", SAGEICP_BENCH_BACKEND="gloo", SAGEICP_P2P_TIMEOUT_S="5",
               MASTER_ADDR="127.0.0.1", SAGEICP_LOOP="0", SAGEICP_CHAIN_COMM="1")
    common = ["--steps", "2", "--warmup", "1", "--scale", "0.1", "--no-cpu-baseline"]

    def two_ranks(extra, port):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"),
                            "--gpus", "2", "--exchange", "direct"] + common,
                           capture_output=True, text=True, env=dict(env, **extra), timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr

    chained, _ = two_ranks({}, 29551)
    with_fin, _ = two_ranks({"SAGEICP_CHAIN": "0"}, 29553)
    hurt, err = two_ranks({"SAGEICP_LOOP_COUNT_TIMEOUT_RANK": "1", "SAGEICP_LOOP_COUNT_TIMEOUT_TICKS": "1"}, 29555)
    for r in chained["config"]["per_rank"]:
        assert r["loop_form"] == "launch per iteration" and r["calls_chained"] >= 3 and r["loop_timeouts"] == 0
    for r in with_fin["config"]["per_rank"]:
        assert r["calls_chained"] == 0
    assert chained["config"]["exchange"] == with_fin["config"]["exchange"] == hurt["config"]["exchange"] == "direct"
    for other in (with_fin, hurt):
        assert other["config"]["iterations_per_frame"] == chained["config"]["iterations_per_frame"]
        assert other["config"]["converged"] and other["config"]["pose_error_vs_planted"] == chained["config"]["pose_error_vs_planted"]
        assert other["config"]["correspondences_first_last"] == chained["config"]["correspondences_first_last"]
    assert "chained ICP launches timed out" in err


def test_bench_independent_frames_mode(gpu_sage):
    """bench.py --independent (the throughput curve of BASELINE config 5): two ranks on the one GPU
    of the box, each registering the whole frame against its own map, no exchange: weak scaling,
    the frames of all ranks counted, the same registration as one rank's"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAGEICP_BENCH_DEVICE="0", SAGEICP_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    common = ["--workload", "c5", "--steps", "2", "--warmup", "1", "--scale", "0.1", "--no-cpu-baseline"]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29537",
                          os.path.join(root, "bench.py"), "--gpus", "2", "--independent"] + common,
                         capture_output=True, text=True, env=env, timeout=600)
    assert two.returncode == 0, two.stderr[-2000:]
    d2 = json.loads(two.stdout.strip().splitlines()[-1])
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common,
                         capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    assert d2["n_gpus"] == 2 and d2["scaling"] == "weak" and "independent frames x2" in d2["config"]["parallelism"]
    assert abs(d2["value"] - 2 * 1e3 / d2["ms_per_step"]) < 1e-2 * d2["value"]
    assert d2["config"]["iterations_per_frame"] == d1["config"]["iterations_per_frame"]
    assert d2["config"]["pose_error_vs_planted"] == d1["config"]["pose_error_vs_planted"]
    assert d2["roofline"]["queries_per_launch"] == d1["roofline"]["queries_per_launch"]


def test_direct_exchange_timeout_is_reported_not_hung(gpu_sage):
    """a peer whose sums do not arrive in time stops the loop with an error on every rank"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SAGEICP_BENCH_DEVICE="0", SAGEICP_BENCH_BACKEND="gloo",
               SAGEICP_P2P_TIMEOUT_TICKS="1", MASTER_ADDR="127.0.0.1")
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29534",
                          os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--scale", "0.1", "--no-cpu-baseline"],
                         capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode != 0
    assert "did not arrive in time" in run.stderr and "no RCCL side to fall back to" in run.stderr


def test_bench_dump_outputs_are_what_the_timed_path_returns(gpu_sage, tmp_path):
    """bench.py --dump-outputs DIR: the pose and statistics of the last timed step, float64, the same as the resident
    entry returns for the same seeded frame in this process; `steps` and `ms_per_step` describe the timed region"""
    import json
    import subprocess
    import sys
    from sage_icp_amd import synthetic as syn
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = tmp_path / "out"
    run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--scale", "0.05", "--no-cpu-baseline", "--dump-outputs", str(d)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    pose, stats, hist = (np.load(d / (n + ".npy")) for n in ("pose", "stats", "n_corr_hist"))
    assert pose.dtype == stats.dtype == hist.dtype == np.float64
    assert pose.shape == (7,) and stats.shape == (6,) and hist.shape == (64,)
    assert stats[0] == line["config"]["iterations_per_frame"] and stats[2] == line["config"]["scan_points"]
    assert list(stats[3:5]) == line["config"]["correspondences_first_last"]
    p = syn.PARAMS["cold"]
    w = syn.make_workload("c2", lambda: gpu_sage.VoxelHashMap(1.0, 100.0), scale=0.05)
    f = gpu_sage.Frame(w["map"], w["scan"])
    ref, st = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"],
                                      return_stats=True)
    assert stats[0] == st.iterations and stats[3] == st.n_corr_first and stats[4] == st.n_corr_last
    assert np.allclose(pose, ref, rtol=0, atol=1e-12)


def test_profiling_stats(gpu_sage, oracle, monkeypatch):
    monkeypatch.setenv("SAGEICP_LOOP", "0")       # per-kernel times of the launch-per-iteration loop (k_loop: tests/test_loop_kernel.py)
    w, om = _workload(gpu_sage, oracle, "c2", 0.05)
    gpu_sage.set_profiling(2)
    try:
        _, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4,
                                        return_stats=True)
    finally:
        gpu_sage.set_profiling(0)
    assert st.nn_launches == st.iterations and st.us_nn > 0 and st.us_fin > 0
    assert 0 < st.pairs_evaluated <= st.sum_candidates and st.lanes_per_query in (1, 2, 4, 8, 16)
    # level 1 (what bench.py runs with): k_icp bracketed in one iteration out of 8
    gpu_sage.set_profiling(1)
    try:
        _, s1 = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, 6.0, 2 / 3, 0.4,
                                        return_stats=True)
    finally:
        gpu_sage.set_profiling(0)
    assert s1.iterations == st.iterations and s1.sum_candidates == st.sum_candidates
    assert s1.nn_launches == len([k for k in range(s1.iterations) if k % 8 == 4])
    assert s1.us_nn > 0 and s1.us_fin == 0


# ------------------------------------------------------------------ full-size properties
@pytest.mark.parametrize("params", ["cold", "steady"])
def test_c2_full_size_properties(gpu_sage, oracle, params):
    """BASELINE c2 at full size (120k scan vs 1M map) at both parameter points of SURVEY 8(d) —
    `cold` is the workload bench.py times: size-independent properties (idempotence:
    re-registering from the answer is a fixed point; index-exact correspondences against the
    oracle's search at the converged pose; bit-reproducibility) and the oracle's full
    registration of the same frame (same iteration and correspondence counts, pose within 1e-7)."""
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c2", 1.0)
    assert w["map"].size() == 1_000_000 and len(w["scan"]) == 120_000
    p = syn.PARAMS[params]
    pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                       p["kernel"], p["sem_th"], return_stats=True)
    assert st.converged == 1
    dt, dr = pose_error(oracle, w["T_gt"], pose)
    assert dt < 0.05 and dr < 2e-3            # independent samples: near, not at, the planted pose
    pose2, st2 = gpu_sage.register_frame(w["scan"], w["map"], pose, p["max_dist"], p["kernel"],
                                         p["sem_th"], return_stats=True)
    dt, dr = pose_error(oracle, pose, pose2)
    assert st2.iterations <= 3 and dt < 2e-4 and dr < 2e-4
    # correspondences at the converged pose: index-exact against the oracle at full size
    q = oracle.transform_points(pose, w["scan"])
    _, tgt, idx = w["map"].GetCorrespondences(q, p["max_dist"], p["sem_th"], with_index=True)
    _, otgt, oidx = om.get_correspondences(q, p["max_dist"], p["sem_th"], with_index=True)
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)
    # full oracle registration on the same input: the headline parity bar
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"],
                                   p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < TOL_M and dr < TOL_RAD and st.iterations == ost.iterations
    assert dt < 1e-7 and dr < 1e-7
    assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
    assert st.sum_candidates == ost.sum_candidates_total
    # nothing in the loop depends on when the host looks: the same call again gives the same bits
    again, st_again = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"],
                                              p["kernel"], p["sem_th"], return_stats=True)
    assert np.array_equal(again, pose) and st_again.iterations == st.iterations


@pytest.mark.parametrize("params", ["dense", "dense_nosem"])
def test_c5_full_size_properties(gpu_sage, oracle, params):
    """BASELINE c5 at full size (200k-pt dense scan vs the 3M-pt-stream map at 0.1 m voxels, semantic
    scaling on / off): convergence to the planted centimetre offset, idempotence,
    bit-reproducibility, index-exact correspondences against the oracle's search at the converged
    pose, and the oracle's full registration of the same frame (31 candidates per query: it takes
    the oracle seconds)."""
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c5", 1.0)
    assert len(w["scan"]) == 200_000 and w["map"].num_voxels() > 1_000_000
    p = syn.PARAMS[params]
    f = gpu_sage.Frame(w["map"], w["scan"])
    pose, st = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                       p["sem_th"], return_stats=True)
    assert st.converged == 1 and 0 < st.n_corr_last < len(w["scan"])
    gt, gr = pose_error(oracle, w["T_gt"], pose)
    assert gt < 0.03 and gr < 1e-3
    pose2, st2 = gpu_sage.register_frame(f, w["map"], pose, p["max_dist"], p["kernel"], p["sem_th"],
                                         return_stats=True)
    dt, dr = pose_error(oracle, pose, pose2)
    assert st2.iterations <= 3 and dt < 2e-4 and dr < 2e-4
    again, st3 = gpu_sage.register_frame(f, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                         p["sem_th"], return_stats=True)
    assert np.array_equal(again, pose) and st3.iterations == st.iterations
    q = oracle.transform_points(pose, w["scan"])
    _, tgt, idx = w["map"].GetCorrespondences(q, p["max_dist"], p["sem_th"], with_index=True)
    _, otgt, oidx = om.get_correspondences(q, p["max_dist"], p["sem_th"], with_index=True)
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt)
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"])
    dt, dr = pose_error(oracle, opose, pose)
    assert dt < 1e-7 and dr < 1e-7 and st.iterations == ost.iterations
    assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
    assert st.sum_candidates == ost.sum_candidates_total


def test_sums_beyond_the_fixed_point_range_are_accumulated_at_a_coarser_scale(gpu_sage, oracle, monkeypatch):
    """|sum over four queries| >= 2^46 (2^40 in the one-launch loop: coordinates of millions of metres,
    georeferenced clouds) does not fit the fixed-point accumulators; the reference has no such limit, so the
    frame is registered again with the sums accumulated at 2^-24 of their value instead of failing — the same
    answer as asking for that scale, in either loop"""
    rng = np.random.default_rng(3)
    off = np.array([8.0e6, -3.0e6, 0.0, 0.0])
    mp = rng.uniform(-60, 60, size=(30000, 4))
    mp[:, 2] = rng.uniform(-2, 2, 30000)
    mp[:, 3] = rng.choice([0, 40, 50], 30000)
    q = mp[rng.choice(30000, 4000, replace=False)] + [0.3, -0.2, 0.05, 0]
    m = gpu_sage.VoxelHashMap(8.0, 1e9)
    m.AddPoints(mp + off)
    frame = np.ascontiguousarray(q + off)
    pose, st = gpu_sage.register_frame(frame, m, gpu_sage.IDENTITY, 6.0, 0.5, 0.4, return_stats=True)
    assert st.iterations >= 1 and np.all(np.isfinite(pose))
    monkeypatch.setenv("SAGEICP_LOOP", "0")
    pose0, st0 = gpu_sage.register_frame(frame, m, gpu_sage.IDENTITY, 6.0, 0.5, 0.4, return_stats=True)
    assert np.array_equal(pose, pose0) and st.iterations == st0.iterations
    monkeypatch.setenv("SAGEICP_ACC_SHIFT", "1")
    ref, sr = gpu_sage.register_frame(frame, m, gpu_sage.IDENTITY, 6.0, 0.5, 0.4, return_stats=True)
    assert np.array_equal(pose, ref) and st.iterations == sr.iterations


def test_big_frame_at_utm_coordinates_does_not_wrap_the_accumulators(gpu_sage, oracle, monkeypatch):
    """k_fin adds the 32 copies of k_icp's accumulators in 64-bit integers, so what must fit is the sum
    over ALL the blocks of the frame, not one block: 1.05M points at y = 4e6 m (UTM northing) keep every block of
    four under the old fixed limit (4 x 1.6e13 < 2^46) while sum(w y^2) ~ 1.7e19 passes 2^63.  The limit of a block
    now follows from the size of the frame (2^62 / blocks), the frame is registered at the coarser scale, and the
    answer is that of asking for the coarser scale by name."""
    rng = np.random.default_rng(5)
    off = np.array([5.0e5, 4.0e6, 0.0, 0.0])
    mp = rng.uniform(-60, 60, size=(30000, 4))
    mp[:, 2] = rng.uniform(-2, 2, 30000)
    mp[:, 3] = rng.choice([0, 40, 50], 30000)
    plant = np.array([0.3, -0.2, 0.05, 0.0])
    q = mp[rng.integers(0, 30000, 1_050_000)] + plant
    m = gpu_sage.VoxelHashMap(4.0, 1e9)
    m.AddPoints(mp + off)
    frame = np.ascontiguousarray(q + off)
    pose, st = gpu_sage.register_frame(frame, m, gpu_sage.IDENTITY, 6.0, 0.5, 0.4, return_stats=True)
    assert st.single_launch == 0 and st.converged == 1 and np.all(np.isfinite(pose))
    monkeypatch.setenv("SAGEICP_ACC_SHIFT", "1")
    ref, sr = gpu_sage.register_frame(frame, m, gpu_sage.IDENTITY, 6.0, 0.5, 0.4, return_stats=True)
    assert np.array_equal(pose, ref) and st.iterations == sr.iterations
    # the planted shift is found (the frame is the map's own points moved by `plant`)
    moved = oracle.transform_points(pose, frame[:2000])
    assert np.abs(moved[:, :3] - (frame[:2000, :3] - plant[:3])).max() < 1e-2       # (stops at |step| < 1e-4 with a lever of 4e6 m)


def test_association_decider_scene(gpu_sage, oracle):
    """tests/sqnorm3_decider.py (the scene that settles SAGE_SQNORM3_ORDER wherever the reference builds): the product
    returns the neighbour its build's association keeps — the oracle's of the same build, the one the construction predicts"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from sqnorm3_decider import decider_scene
    pts, qs, picks = decider_scene()
    a, b = both_maps(gpu_sage, oracle, pts)
    _, tgt, idx = a.GetCorrespondences(qs, 1.0, 0.4, with_index=True)
    _, otgt, oidx = b.get_correspondences(qs, 1.0, 0.4, with_index=True)
    assert np.array_equal(idx, oidx) and np.array_equal(tgt, otgt) and len(tgt) == len(qs)
    got = [int(np.flatnonzero((pts == t).all(1))[0]) for t in tgt]
    assert got == picks[oracle.SQNORM3_ORDER].tolist()


def test_counters_can_be_switched_off(gpu_sage, oracle):
    """sageicp_set_counting(0): a call that returns statistics no longer counts candidates and pairs (what bench.py's
    timed region does: the C++ shim's calls never count) — same pose to the bit, the other statistics unchanged"""
    from sage_icp_amd import synthetic as syn
    w = syn.make_workload("c2", lambda: gpu_sage.VoxelHashMap(syn.WORKLOADS["c2"]["voxel"], 100.0), scale=0.1)
    p = syn.PARAMS["cold"]
    for loop in (0, 2):
        os.environ["SAGEICP_LOOP"] = str(loop)
        try:
            a, sa = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"],
                                            return_stats=True)
            gpu_sage.set_counting(False)
            b, sb = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"],
                                            return_stats=True)
        finally:
            gpu_sage.set_counting(True)
            os.environ.pop("SAGEICP_LOOP", None)
        assert np.array_equal(a, b)
        assert sa.sum_candidates > 0 and sa.pairs_evaluated > 0
        assert sb.sum_candidates == 0 and sb.pairs_evaluated == 0
        assert (sa.iterations, sa.converged, sa.n_corr_first, sa.n_corr_last) == (sb.iterations, sb.converged, sb.n_corr_first, sb.n_corr_last)


@pytest.mark.parametrize("n", [16383, 16384])
def test_small_frames_are_searched_as_they_came(gpu_sage, oracle, monkeypatch, n):
    """kSortFrameFrom (kernels.h): below 16,384 points the frame is not sorted (its launches cost more than the order
    buys), from there on it is.  Either side of the limit: the oracle's registration (Registration.cpp:113-141) within
    1e-7, its iteration and correspondence counts; the one-launch loop and the launch-per-iteration loop bit for bit;
    and the other order of the same frame (SAGEICP_SORT_FROM) within 1e-9 with the same iterations — the order moves
    which four queries share a block of the exact sums, i.e. ulps, never the search"""
    from sage_icp_amd import synthetic as syn
    w, om = _workload(gpu_sage, oracle, "c2", 0.15)
    p = syn.PARAMS["cold"]
    scan = np.ascontiguousarray(w["scan"][:n])
    assert len(scan) == n
    pose, st = gpu_sage.register_frame(scan, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"], return_stats=True)
    opose, ost = om.register_frame(scan, oracle.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"])
    assert st.single_launch == 1 and st.converged == 1
    assert np.abs(pose - opose).max() < 1e-7 and st.iterations == ost.iterations
    assert st.n_corr_first == ost.n_corr_first and st.n_corr_last == ost.n_corr_last
    monkeypatch.setenv("SAGEICP_LOOP", "0")
    per_it, sp = gpu_sage.register_frame(scan, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"], return_stats=True)
    assert sp.single_launch == 0 and np.array_equal(per_it, pose) and sp.iterations == st.iterations
    monkeypatch.delenv("SAGEICP_LOOP")
    monkeypatch.setenv("SAGEICP_SORT_FROM", "0" if n < 16384 else "1000000")
    other, so = gpu_sage.register_frame(scan, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"], return_stats=True)
    assert np.abs(other - pose).max() < 1e-9 and so.iterations == st.iterations and so.n_corr_last == st.n_corr_last
    # a non-finite point in a frame that is not sorted is refused by the launch that stands in for the sort
    bad = scan.copy()
    bad[n // 2, 1] = np.nan
    monkeypatch.delenv("SAGEICP_SORT_FROM")
    with pytest.raises(gpu_sage.SageIcpError):
        gpu_sage.register_frame(bad, w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"])
