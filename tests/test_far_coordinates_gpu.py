"""The search held to the oracle at the far end of the voxel domain (tests/farscenes.py; tests/test_far_scenes_host.py
asserts that the scenes decide).  The map takes voxel indices in (-2^20, 2^20): 1e5 m at 0.1 m voxels, 1e8 m at 100 m.
Three parts of the search carry a term that grows with the coordinate — the fp32 filter's slack (icp_body.h, FILT), the
face gaps' slack (icp_body.h, axis_gaps), the guard of the reciprocal voxel index (kernels.hip, voxel_index) — and behind
them sit the i32 keys of the slot table, the home-voxel words of a row, the row shift and the 21-bit packed keys of the
device update.  Every comparison here is equality of indices, or of rows bit for bit.

Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch        # (before the library's first call: both bind to one HIP runtime, sage_icp_amd._check_one_hip_runtime)

import farscenes as fs
import gnstep_cases as gc
from test_loop_kernel import Env, _same, pose_error

pytestmark = pytest.mark.gpu

OCT_IDS = [fs.octant_id(o) for o in fs.OCTANTS]

_scenes = {}


def _scene(oracle, kind, vs, octant, labels):
    """-> map points, queries as the product gets them, the pose that goes with them (or None), {sem_th: the oracle's
    (src, tgt, idx)}; computed once per scene and shared by the scan forms"""
    key = (kind, vs, octant, labels)
    if key not in _scenes:
        pose = None
        if kind == "edge":
            mp, q, c, _ = fs.edge(vs, octant, labels)
            world = q
        else:
            mp, q, c = fs.corner(vs, octant, labels)
            world = q
            if kind == "offset":
                # the queries relative to the centre, the centre carried by the pose: R = I, so the device forms
                # fl(f + t), one rounding
                q = q.copy()
                q[:, :3] -= c
                world = q.copy()
                world[:, :3] += c
                pose = np.r_[0.0, 0.0, 0.0, 1.0, c]
        om = oracle.Map(vs, 100.0)
        om.add_points(mp)
        want = {th: om.get_correspondences(world, fs.MAX_DIST_VOXELS * vs, th, with_index=True) for th in fs.SEM_THS}
        assert all(len(w[2]) > len(q) // 2 for w in want.values())
        _scenes[key] = (mp, q, pose, want)
    return _scenes[key]


def _equal(got, want, what):
    src, tgt, idx = got
    assert np.array_equal(idx, want[2]), what
    assert np.array_equal(tgt, want[1]) and np.array_equal(src, want[0]), what


def _hold_to_the_oracle(sage, oracle, kind, vs, octant):
    """every kernel variant of GetCorrespondences (1 - 16 lanes per query, the lanes restarting in every voxel or striding
    through the voxels as one sequence), every sem_th, both label variants"""
    for labels in fs.LABEL_VARIANTS:
        mp, q, _, want = _scene(oracle, kind, vs, octant, labels)
        m = sage.VoxelHashMap(vs, 100.0)
        m.AddPoints(mp)
        assert m.size() > 0
        for lw in range(5):
            for flat in (0, 1):
                with Env(SAGEICP_LW=lw, SAGEICP_FLAT=flat):
                    for th in fs.SEM_THS:
                        got = m.GetCorrespondences(q, fs.MAX_DIST_VOXELS * vs, th, with_index=True)
                        _equal(got, want[th], (labels, lw, flat, th))


# ---- 1. GetCorrespondences at the corners ----------------------------------------------------------------------------
@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
@pytest.mark.parametrize("vs", fs.VOXELS)
def test_get_correspondences_at_the_corners_of_the_domain(gpu_sage, oracle, vs, octant, scan_form):
    """the near-tie scene at voxel index 2^20 - 6 on every axis: the coordinate term of the filter's slack is all of its
    threshold there (E is a quarter of a metre at 1e6 m), and fp32 alone picks another neighbour for hundreds of queries"""
    _hold_to_the_oracle(gpu_sage, oracle, "corner", vs, octant)


# ---- 2. the edge of the domain -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
@pytest.mark.parametrize("vs", fs.VOXELS)
def test_queries_at_and_beyond_the_edge_of_the_domain(gpu_sage, oracle, vs, octant, scan_form):
    """a map that ends at index +-(2^20 - 1) and queries whose home voxels lie up to two voxels beyond it: the map refuses
    such points, the search has no domain of its own — the oracle defines the answer"""
    _hold_to_the_oracle(gpu_sage, oracle, "edge", vs, octant)


# ---- 3. face deciders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1, -1], ids=["+", "-"])
@pytest.mark.parametrize("vs", fs.DECIDER_VOXELS)
def test_face_deciders_get_the_quotients_home_voxel(gpu_sage, oracle, vs, sign, scan_form, monkeypatch):
    """x on or one ulp beside a voxel face near index 2^20, where x * fl(1 / vs) truncates to another voxel than
    fl(x / vs): the one map point of every query is in reach of the right home voxel only"""
    d = fs.face_deciders(vs, sign)
    n = len(d["queries"])
    om = oracle.Map(vs, 100.0)
    om.add_points(d["map"])
    want = om.get_correspondences(d["queries"], d["max_dist"], 0.4, with_index=True)
    assert n >= 100 and np.array_equal(want[2], np.arange(n))
    m = gpu_sage.VoxelHashMap(vs, 100.0)
    m.AddPoints(d["map"])
    monkeypatch.delenv("SAGEICP_EXACT_DIVIDE", raising=False)
    for lw in range(5):
        for env in ({}, {"SAGEICP_EXACT_DIVIDE": 1}):
            with Env(SAGEICP_LW=lw, **env):
                got = m.GetCorrespondences(d["queries"], d["max_dist"], 0.4, with_index=True)
            assert len(got[2]) == n, (lw, env, "%d of %d deciders paired" % (len(got[2]), n))
            _equal(got, want, (lw, env))


# ---- 3b. slack deciders ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
def test_slack_deciders_keep_their_neighbour(gpu_sage, oracle, octant, scan_form):
    """two candidates per query on a diagonal, the nearer one scanned last and one fp32 ulp further away on every axis
    than it is: the filter's threshold has to carry the coordinate term of its slack at close to full size (the corner
    scenes, whose neighbours are a third of a voxel away, pass with a slack 256 times too small)"""
    d = fs.slack_deciders(octant)
    n = len(d["queries"])
    om = oracle.Map(fs.SLACK_VOXEL, 100.0)
    om.add_points(d["map"])
    m = gpu_sage.VoxelHashMap(fs.SLACK_VOXEL, 100.0)
    m.AddPoints(d["map"])
    for th in (0.4, 1.0):
        want = om.get_correspondences(d["queries"], d["max_dist"], th, with_index=True)
        assert np.array_equal(want[2], np.arange(n)) and np.array_equal(want[1], d["map"][d["winner"]])
        for lw in range(5):
            for flat in (0, 1):
                with Env(SAGEICP_LW=lw, SAGEICP_FLAT=flat):
                    got = m.GetCorrespondences(d["queries"], d["max_dist"], th, with_index=True)
                _equal(got, want, (th, lw, flat))


# ---- 4. the offset carried by the pose ---------------------------------------------------------------------------------
@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
@pytest.mark.parametrize("vs", fs.VOXELS)
def test_the_offset_carried_by_the_pose(gpu_sage, oracle, vs, octant, scan_form):
    """the corner's queries relative to its centre, the centre as the translation of the pose of the device-frame entry:
    the oracle gets fl(f + t)"""
    for labels in fs.LABEL_VARIANTS:
        mp, f, pose, want = _scene(oracle, "offset", vs, octant, labels)
        m = gpu_sage.VoxelHashMap(vs, 100.0)
        m.AddPoints(mp)
        ft = torch.from_numpy(f).cuda()
        for th in fs.SEM_THS:
            got = m.GetCorrespondences(ft, fs.MAX_DIST_VOXELS * vs, th, with_index=True, pose=pose)
            _equal([x.cpu().numpy() for x in got], want[th], (labels, th))


# ---- 5. a resident map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", fs.RESIDENT_KEEPS)
@pytest.mark.parametrize("vs,octant", fs.RESIDENT_CASES, ids=["%g%s" % (v, fs.octant_id(o)) for v, o in fs.RESIDENT_CASES])
def test_a_resident_map_at_the_corner(gpu_sage, oracle, vs, octant, keep, scan_form):
    """the corner's map built and then changed by device updates alone (packed 21-bit keys, evictions that leave
    tombstones, keys inserted again over them), searched where it lives after each"""
    md, updates = fs.resident_updates(vs, octant, keep)
    _, q, _ = fs.corner(vs, octant)
    qt = torch.from_numpy(q).cuda()
    m = gpu_sage.VoxelHashMap(vs, md)
    om = oracle.Map(vs, md)
    for step, (frame, pose, world) in enumerate(updates):
        m.UpdateOnDevice(frame, pose)
        assert m.resident(), step
        om.add_points(world)
        om.remove_far(pose[4:])
        assert (m.size(), m.num_voxels()) == (om.size(), om.num_voxels()), step
        cap, used, voxels = m.table_stats()
        print("step %d: %d points in %d voxels, %d slots of %d used" % (step, m.size(), voxels, used, cap))
        assert voxels == om.num_voxels() and used >= voxels, step
        if step == 1 or keep == "half":
            assert used > voxels, "step %d evicts voxels: their slots stay behind as tombstones" % step
        for th in (0.4, 1.0):
            want = om.get_correspondences(q, fs.MAX_DIST_VOXELS * vs, th, with_index=True)
            assert len(want[2]) > 1000
            for lw in (0, 2, 4):
                with Env(SAGEICP_LW=lw):
                    got = m.GetCorrespondences(qt, fs.MAX_DIST_VOXELS * vs, th, with_index=True)
                _equal([x.cpu().numpy() for x in got], want, (step, th, lw))
        assert m.resident(), step


# ---- 6. RegisterFrame at the corners -----------------------------------------------------------------------------------
FORMS = [dict(SAGEICP_LOOP=loop, SAGEICP_LW=lw, SAGEICP_FILTER=f) for loop in (0, 2) for lw in (1, 2, 3, 4) for f in (0, 1)]


@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
@pytest.mark.parametrize("vs", fs.FRAME_VOXELS)
def test_register_frame_at_the_corners_of_the_domain(gpu_sage, oracle, vs, octant):
    mp, _, c = fs.corner(vs, octant)
    frame, guess, _ = fs.planted_frame(vs, octant)
    kernel = gc.SCENE_KERNEL["origin"]
    m = gpu_sage.VoxelHashMap(vs, 100.0)
    om = oracle.Map(vs, 100.0)
    m.AddPoints(mp)
    om.add_points(mp)
    src, _, clear = gc.pairs_clear_of_edge(om, gc.first_source(frame, guess))
    assert clear and len(src) > len(frame) // 2

    def run(form, **more):
        with Env(**form, **more):
            T, st = gpu_sage.register_frame(frame, m, guess, gc.MAX_DIST, kernel, gc.SEM_TH, return_stats=True)
        assert st.single_launch == (1 if form["SAGEICP_LOOP"] == 2 else 0), form
        assert st.lanes_per_query == 1 << form["SAGEICP_LW"] and st.compact_scan == form["SAGEICP_FILTER"], form
        return T, st

    # the pairs of the first iteration: the home voxels, the rows and the search of every form, at the guess
    for form in FORMS:
        T, st = run(form, SAGEICP_MAX_ITER=1)
        assert st.iterations == 1 and st.n_corr_hist[0] == len(src), (form, st.n_corr_hist[0], len(src))
    # to convergence: 1.5 voxels and 0.02 rad away, every query changes its home voxel on the way (row shifts, rebuilt
    # rows).  SAGEICP_ACC_SHIFT=1 in every form: at 1e6 m the two loops would otherwise pick different accumulator scales
    #  — with one scale the Gauss-Newton sums are the same integers, and the poses one pose to the bit.
    runs = [run(form, SAGEICP_ACC_SHIFT=1) for form in
            FORMS + [dict(SAGEICP_LOOP=0, SAGEICP_LW=0, SAGEICP_FILTER=f) for f in (0, 1)]]
    T0, st0 = runs[0]
    assert st0.converged == 1 and st0.iterations > 10
    for T, st in runs[1:]:
        assert np.array_equal(T, T0) and T.tobytes() == T0.tobytes()
        _same(st, st0)
    opose, ost = om.register_frame(frame, guess, gc.MAX_DIST, kernel, gc.SEM_TH)
    dt, dr = pose_error(oracle, opose, T0)
    print("vs %g octant %s: %d iterations (oracle %d), pairs %d -> %d (oracle %d -> %d), pose against the oracle's "
          "%.3e m %.3e rad (not asserted: fp64 is ill-conditioned %g m from the origin)"
          % (vs, fs.octant_id(octant), st0.iterations, ost.iterations, st0.n_corr_first, st0.n_corr_last,
             ost.n_corr_first, ost.n_corr_last, dt, dr, np.linalg.norm(c)))
