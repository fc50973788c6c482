"""The scenes of tests/farscenes.py decide: each holds what makes a wrong search show, by the oracle and numpy alone.  A
scene that stops deciding fails here instead of passing silently in tests/test_far_coordinates_gpu.py.  No GPU."""
import numpy as np
import pytest

import farscenes as fs
import gnstep_cases as gc
from farscenes import LIM

OCT_IDS = [fs.octant_id(o) for o in fs.OCTANTS]


def _oracle_map(oracle, vs, mp):
    om = oracle.Map(vs, 100.0)
    om.add_points(mp)
    return om


@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
@pytest.mark.parametrize("vs", fs.VOXELS)
def test_corner_fp32_alone_gets_it_wrong_and_the_oracle_is_the_brute_force(oracle, vs, octant):
    mp, q, c = fs.corner(vs, octant)
    assert len(mp) == 6600 and len(q) == 3040
    k = np.abs(fs.voxel_of(np.vstack([mp, q]), vs))
    assert k.max() < LIM and k.min() >= LIM - 11                 # inside the domain, at its corner, on every axis
    om = _oracle_map(oracle, vs, mp)
    stored = om.pointcloud()
    md, th = fs.MAX_DIST_VOXELS * vs, 0.4
    w64, a64 = fs.brute_force(stored, q, vs, th, md, np.float64, oracle.SQNORM3_ORDER)
    w32, _ = fs.brute_force(stored, q, vs, th, md, np.float32, oracle.SQNORM3_ORDER)
    wrong = int((w32 != w64).sum())
    print("vs %g octant %s: fp32 alone returns another neighbour for %d of %d queries" % (vs, fs.octant_id(octant), wrong, len(q)))
    assert wrong >= 150
    src, tgt, idx = om.get_correspondences(q, md, th, with_index=True)
    assert len(idx) > 2000
    assert np.array_equal(idx, np.flatnonzero(a64))
    assert np.array_equal(tgt, stored[w64[a64]]) and np.array_equal(src, q[a64])


@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
@pytest.mark.parametrize("vs", fs.VOXELS)
def test_edge_has_queries_beyond_the_domain_and_a_map_that_ends_at_it(oracle, vs, octant):
    mp, q, c, dropped = fs.edge(vs, octant)
    assert dropped >= 100 and len(mp) + dropped == 6600
    assert np.abs(fs.voxel_of(mp, vs)).max() == LIM - 1          # the map reaches the last voxel of the domain
    home = np.abs(fs.voxel_of(q, vs))
    beyond = int((home >= LIM).any(axis=1).sum())
    print("vs %g octant %s: %d map points dropped, %d queries at or beyond +-LIM, furthest home index LIM + %d"
          % (vs, fs.octant_id(octant), dropped, beyond, home.max() - LIM))
    assert beyond >= 100 and home.max() <= LIM + 1
    om = _oracle_map(oracle, vs, mp)
    assert om.size() > 0
    _, _, idx = om.get_correspondences(q, fs.MAX_DIST_VOXELS * vs, 0.4, with_index=True)
    assert len(idx) > len(q) // 2
    assert (home[idx] >= LIM).any(axis=1).sum() >= 50            # ... queries beyond the edge among the paired ones


@pytest.mark.parametrize("sign", [1, -1], ids=["+", "-"])
@pytest.mark.parametrize("vs", fs.DECIDER_VOXELS)
def test_face_deciders_need_the_quotients_home_voxel(oracle, vs, sign):
    d = fs.face_deciders(vs, sign)
    mp, q, h, hp = d["map"], d["queries"], d["h"], d["hp"]
    n = len(q)
    print("vs %g sign %+d: %d deciders" % (vs, sign, n))
    assert n >= 100
    assert (np.abs(h - hp) == 1).all()
    assert np.array_equal(fs.voxel_of(q, vs)[:, 0], h)
    assert (np.abs(h) >= LIM - 3001).all() and (np.abs(h) < LIM - 3).all()
    assert len(set(d["ky"].tolist())) == n and (np.abs(np.diff(d["ky"])) == 4).all()
    planted = fs.voxel_of(mp, vs)
    assert np.array_equal(planted[:, 0], d["planted"]) and np.array_equal(planted[:, 0], 2 * h - hp)
    assert np.array_equal(planted[:, 1], d["ky"]) and (planted[:, 2] == 5).all()
    assert np.array_equal(planted[:, 1:], fs.voxel_of(q, vs)[:, 1:])
    assert np.abs(planted).max() < LIM
    om = _oracle_map(oracle, vs, mp)
    assert om.size() == n
    src, tgt, idx = om.get_correspondences(q, d["max_dist"], 0.4, with_index=True)
    assert np.array_equal(idx, np.arange(n))                      # the oracle pairs every decider ...
    assert np.array_equal(tgt, mp)                                # ... with its own map point,
    dist = np.abs(tgt[:, 0] - src[:, 0]) / vs
    assert np.allclose(dist, 1.5, rtol=0, atol=1e-6)              # 1.5 voxels away
    stored = om.pointcloud()
    right, acc = fs.brute_force(stored, q, vs, 0.4, d["max_dist"], order=oracle.SQNORM3_ORDER)
    assert acc.all() and np.array_equal(stored[right], mp)
    homes = fs.voxel_of(q, vs)
    homes[:, 0] = hp                                              # the home voxel of x * fl(1 / vs): nothing in reach
    wrong, acc = fs.brute_force(stored, q, vs, 0.4, d["max_dist"], order=oracle.SQNORM3_ORDER, homes=homes)
    assert (wrong == -1).all() and not acc.any()


@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
@pytest.mark.parametrize("vs", fs.FRAME_VOXELS)
def test_planted_frame_moves_across_voxels_and_its_first_pairs_are_clear_of_the_edge(oracle, vs, octant):
    mp, _, c = fs.corner(vs, octant)
    frame, guess, c2 = fs.planted_frame(vs, octant)
    assert np.array_equal(c, c2) and len(frame) == fs.FRAME_POINTS and np.array_equal(guess, oracle.IDENTITY)
    assert np.abs(fs.voxel_of(frame, vs)).max() < LIM
    om = _oracle_map(oracle, vs, mp)
    src, tgt, clear = gc.pairs_clear_of_edge(om, gc.first_source(frame, guess))
    assert clear and len(src) > fs.FRAME_POINTS // 2
    pose, st = om.register_frame(frame, guess, gc.MAX_DIST, gc.SCENE_KERNEL["origin"], gc.SEM_TH)
    moved = oracle.transform_points(pose, frame)
    crossed = (fs.voxel_of(moved, vs) != fs.voxel_of(frame, vs)).any(axis=1).mean()
    step = np.linalg.norm(moved[:, :3] - frame[:, :3], axis=1)
    print("vs %g octant %s: %d pairs at the guess, %d iterations, converged %d, %.1f %% of the points change their home "
          "voxel, moved by %.3f .. %.3f voxels" % (vs, fs.octant_id(octant), len(src), st.iterations, st.converged,
                                                   100 * crossed, step.min() / vs, step.max() / vs))
    assert st.converged == 1
    assert crossed >= 0.10


@pytest.mark.parametrize("keep", fs.RESIDENT_KEEPS)
@pytest.mark.parametrize("vs,octant", fs.RESIDENT_CASES, ids=["%g%s" % (v, fs.octant_id(o)) for v, o in fs.RESIDENT_CASES])
def test_resident_updates_evict_part_of_the_map_and_fill_evicted_voxels_again(oracle, vs, octant, keep):
    md, updates = fs.resident_updates(vs, octant, keep)
    om = oracle.Map(vs, md)
    counts, evicted = [], []
    for frame, pose, world in updates:
        assert np.array_equal(pose[:4], [0.0, 0.0, 0.0, 1.0]) and np.array_equal(frame[:, :3] + pose[4:], world[:, :3])
        om.add_points(world)
        before = {tuple(v) for v in fs.voxel_of(om.pointcloud(), vs)}
        om.remove_far(pose[4:])
        after = {tuple(v) for v in fs.voxel_of(om.pointcloud(), vs)}
        assert after <= before and om.size() > 1000
        counts.append((len(before), len(after)))
        evicted.append(before - after)
    print("vs %g octant %s %s: voxels before / after each update's eviction %s" % (vs, fs.octant_id(octant), keep, counts))
    if keep == "whole":
        assert not evicted[0] and len(evicted[1]) >= 5
    else:
        assert len(evicted[0]) >= 100 and len(evicted[1]) >= 200
        filled = {tuple(v) for v in fs.voxel_of(updates[1][2], vs)} & evicted[0]
        assert len(filled) >= 50                                      # update 2 inserts keys that update 1 evicted



@pytest.mark.parametrize("octant", fs.OCTANTS, ids=OCT_IDS)
def test_slack_deciders_lose_their_neighbour_to_a_slack_16_times_too_small_in_E(oracle, octant):
    vs = fs.SLACK_VOXEL
    d = fs.slack_deciders(octant)
    mp, q = d["map"], d["queries"]
    A, B = mp[d["first"]], mp[d["winner"]]
    n = len(q)
    assert n == fs.SLACK_DECIDERS and len(mp) == 2 * n
    # the coordinates lie just above 2^19 m (fp32 rounds by up to half an ulp of 2^-4 m, 2^-24 |x|) and inside the domain
    assert np.abs(mp[:, :3]).min() > 2.0 ** 19 and np.abs(mp[:, :3]).max() < 1.05 * 2.0 ** 19
    hq, ha, hb = fs.voxel_of(q, vs), fs.voxel_of(A, vs), fs.voxel_of(B, vs)
    assert np.array_equal(ha, hq - 1) and np.array_equal(hb, hq + 1) and max(np.abs(ha).max(), np.abs(hb).max()) < LIM
    assert len({tuple(v) for v in np.vstack([ha, hb])}) == 2 * n         # a voxel per point: A first, B last in the enumeration
    om = _oracle_map(oracle, vs, mp)
    src, tgt, idx = om.get_correspondences(q, d["max_dist"], 0.4, with_index=True)
    assert np.array_equal(idx, np.arange(n)) and np.array_equal(tgt, B)   # B is the neighbour, by 1e-6 of the distance
    dA, dB = np.linalg.norm(A[:, :3] - q[:, :3], axis=1), np.linalg.norm(B[:, :3] - q[:, :3], axis=1)
    assert (dA > dB).all() and (dA < dB * (1 + 2e-6)).all() and (dA < d["max_dist"]).all()
    stored = om.pointcloud()
    win, acc = fs.brute_force(stored, q, vs, 0.4, d["max_dist"], order=oracle.SQNORM3_ORDER)
    assert acc.all() and np.array_equal(stored[win], B)
    # the fp32 errors are all but the largest there are: one ulp further on every axis
    e = np.abs(B[:, :3].astype(np.float32).astype(np.float64) - q[:, :3].astype(np.float32).astype(np.float64)) - np.abs(B[:, :3] - q[:, :3])
    assert (e > 0.99 * 2.0 ** -4).all()
    # a lane that holds A: the product's slack keeps B, 2^-8 of it (E 16 times too small) drops it, for every decider
    keeps, drops = fs.filter_margin(q, A, B, vs), fs.filter_margin(q, A, B, vs, 2.0 ** -8)
    need = -fs.filter_margin(q, A, B, vs, 0.0) / ((4.0 * fs.U32 * (np.abs(q[:, :3]) + 4.0 * vs)) ** 2).sum(axis=1)
    print("octant %s: the slack these deciders need: %.2f .. %.2f |E|^2 (the product's: 1025 |E|^2)" % (fs.octant_id(octant), need.min(), need.max()))
    assert (keeps > 0).all() and (drops < -0.04).all()
