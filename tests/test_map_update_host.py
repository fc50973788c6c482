"""The adversarial map-update scenes (tests/mapscenes.py) on the CPU: the plain restatement with the block pool
(tests/mapref.py) against the library's host map — Pointcloud() byte for byte, size(), num_voxels() after every pass —
and against the oracle's Map as a sorted point set.  This pins the restatement the device tests
(test_map_update_adversarial.py) compare against before a GPU is involved.  Every comparison is exact."""
import numpy as np
import pytest

import mapref
import mapscenes
from mapscenes import make_map


def _sorted(a):
    a = np.asarray(a).reshape(-1, 4)
    return a[np.lexsort(a.T)]


def run_host(sage, s, ref, host, orc=None):
    for k, ((pts, pose, refused), (cloud, size, nvox, _)) in enumerate(zip(s["passes"], ref)):
        if refused:
            with pytest.raises(sage.SageIcpError) as e:
                host.Update(pts, pose)
            assert e.value.code == sage.ERR_CAPACITY
        else:
            host.Update(pts, pose)
            if orc is not None:
                orc.add_points(np.array(mapref.transform(pose, pts)).reshape(-1, 4))
                orc.remove_far(pose[4:])
        got = host.Pointcloud()
        assert got.tobytes() == cloud.tobytes(), "pass %d: blocks differ from the restatement (content or order)" % (k + 1)
        assert (host.size(), host.num_voxels()) == (size, nvox), "pass %d" % (k + 1)
        if orc is not None:
            assert orc.size() == size and orc.num_voxels() == nvox, "pass %d" % (k + 1)
            assert np.array_equal(_sorted(got), _sorted(orc.pointcloud())), "pass %d: the oracle holds other points" % (k + 1)
        if s["check"]:
            s["check"](k, got)


@pytest.mark.parametrize("name", mapscenes.ALL_NAMES)
def test_host_update_equals_the_restatement_and_the_oracle(sage, oracle, name):
    s = mapscenes.scene(name, sage)
    p = s["params"]
    orc = oracle.Map(p["voxel_size"], p["max_distance"], p["basic"], p["critical"])
    host = make_map(sage, s)
    run_host(sage, s, mapscenes.reference(name, sage), host, orc)
    if s["extra"] is not None:          # a host-side entry on top: the restatement's AddPoints
        m = mapref.MapRef(**p)
        for pts, pose, refused in s["passes"]:
            m.update(pts, pose)
        m.add_points(s["extra"])
        host.AddPoints(s["extra"])
        assert host.Pointcloud().tobytes() == m.pointcloud().tobytes()


@pytest.mark.parametrize("name", mapscenes.CLASS_NAMES)
def test_host_map_with_one_full_size_class(sage, monkeypatch, name):
    """SAGEICP_SIZE_CLASSES=0: every voxel in a region of the capacity — the same map, byte for byte"""
    s = mapscenes.scene(name, sage)
    monkeypatch.setenv("SAGEICP_SIZE_CLASSES", "0")
    flat = make_map(sage, s)
    monkeypatch.delenv("SAGEICP_SIZE_CLASSES")
    run_host(sage, s, mapscenes.reference(name, sage), flat)
    assert flat.point_slots() >= (s["params"]["basic"] + s["params"]["critical"]) * flat.num_voxels()


def test_the_hash_and_the_table_stats_entries(sage):
    L = sage.lib()
    ck = mapscenes.colliding_keys(sage)
    for low, boxes in ck.items():
        for keys in boxes:
            assert len(keys) >= 12
            assert all(sage.voxel_hash(*k) & 0xFFFF == low for k in keys)
    assert sage.voxel_hash(0, 0, 0) == sage.voxel_hash(0, 0, 0) and 0 <= sage.voxel_hash(-5, 7, -(1 << 20) + 1) < 2 ** 32
    m = sage.VoxelHashMap(1.0, 100.0)
    assert m.table_stats() == (1024, 0, 0)
    m.AddPoints(np.array([[x + 0.5, 0.5, 0.5, 0.0] for x in range(300)]))
    cap, used, live = m.table_stats()
    assert (used, live) == (300, 300) and cap >= 4 * 300 and cap & (cap - 1) == 0
    m.Update(np.zeros((0, 4)), [1000.0, 0.0, 0.0])         # everything goes: the host table keeps no tombstones
    assert m.table_stats()[1:] == (0, 0)
    assert L.sageicp_map_table_stats(None, None) == sage.ERR_INVALID
    assert L.sageicp_map_table_stats(m._h, None) == sage.ERR_INVALID


def test_restatement_known_answers():
    """the restatement itself on hand-derived cases: the policy (VoxelHashMap.hpp:45-70) and the pool rules"""
    m = mapref.MapRef(1.0, 10.0, basic=2, critical=1, basic_labels=(40,))
    I = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    m.update([(0.5, 0.5, 0.5, 0.0), (0.6, 0.5, 0.5, 0.0), (0.7, 0.5, 0.5, 0.0),      # third unlabelled: dropped
              (0.8, 0.5, 0.5, 71.0), (0.9, 0.5, 0.5, 40.0), (0.4, 0.5, 0.5, 80.0),   # appended / replaces #0 / full: replaces #1
              (0.3, 0.5, 0.5, 99.0),                                                   # no unlabelled point left: dropped
              (-0.5, 0.5, 0.5, 0.0), (5.5, 0.5, 0.5, 0.0), (20.5, 0.5, 0.5, 0.0)], I)  # voxel 0 again (dropped), two new
    assert m.pointcloud().tolist() == [[0.9, 0.5, 0.5, 40.0], [0.4, 0.5, 0.5, 80.0], [0.8, 0.5, 0.5, 71.0], [5.5, 0.5, 0.5, 0.0]]
    assert (m.size(), m.num_voxels(), m.free) == (4, 2, [2])
    m.update([(-4.5, 0.5, 0.5, 0.0), (-3.5, 0.5, 0.5, 0.0)], [0.0, 0.0, 0.0, 1.0, 12.0, 0.0, 0.0])     # 7.5 and 8.5 in the map frame
    # blocks 0 and 1 ((0,0,0) and (5,0,0): 11.1 and 6.5 from the origin) -> block 0 goes; 7.5 took block 2, 8.5 block 3
    assert m.pointcloud().tolist() == [[5.5, 0.5, 0.5, 0.0], [7.5, 0.5, 0.5, 0.0], [8.5, 0.5, 0.5, 0.0]]
    assert m.free == [0]
    with pytest.raises(mapref.RefusedUpdate):
        m.update([(1.5, 0.5, 0.5, 0.0), (1048576.0, 0.0, 0.0, 0.0)], I)
    assert m.size() == 3
    # a half turn about z and a shift: (1, 2, 3) -> (-1, -2, 3) + (10, 20, 30)
    assert mapref.transform([0.0, 0.0, 1.0, 0.0, 10.0, 20.0, 30.0], [(1.0, 2.0, 3.0, 7.0)]) == [(9.0, 18.0, 33.0, 7.0)]
