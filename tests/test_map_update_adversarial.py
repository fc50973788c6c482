"""The device-side VoxelHashMap::Update (csrc/map_update.hip) on the adversarial scenes of tests/mapscenes.py: runs of
equal voxels against the 256-position LDS stage, counts on the size-class boundaries, hash chains with tombstones that
wrap around the table, a table rebuilt because of tombstones alone, the edges of the key and label domain.  After every
pass the resident map must equal the plain restatement (tests/mapref.py, pinned on the CPU by test_map_update_host.py)
and the library's host map: Pointcloud() byte for byte and in order, size(), num_voxels().  Everything is integer and
byte work: every comparison is exact.  Needs the MI355X."""
import numpy as np
import pytest

import mapref
import mapscenes
from mapscenes import make_map

pytestmark = pytest.mark.gpu


def _update(sage, m, device, pts, pose, refused, k):
    if refused:
        with pytest.raises(sage.SageIcpError) as e:
            (m.UpdateOnDevice if device else m.Update)(pts, pose)
        assert e.value.code == sage.ERR_CAPACITY, "pass %d" % (k + 1)
    else:
        (m.UpdateOnDevice if device else m.Update)(pts, pose)


def _same(dev, host, k, ref=None):
    a = dev.Pointcloud()
    assert dev.resident(), "pass %d: Pointcloud() moved the authority" % (k + 1)
    assert a.tobytes() == host.Pointcloud().tobytes(), "pass %d: blocks differ from the host map (content or order)" % (k + 1)
    assert (dev.size(), dev.num_voxels()) == (host.size(), host.num_voxels()), "pass %d" % (k + 1)
    if ref is not None:
        cloud, size, nvox, _ = ref
        assert a.tobytes() == cloud.tobytes(), "pass %d: blocks differ from the restatement" % (k + 1)
        assert (dev.size(), dev.num_voxels()) == (size, nvox), "pass %d" % (k + 1)
    return a


def _pow2_for(voxels):
    cap = 1024
    while voxels * 4 > cap:
        cap *= 2
    return cap


def _hand_back(dev, host, extra):
    """AddPoints on both: the device map downloads the table, regions and free stacks its passes left"""
    dev.AddPoints(extra)
    host.AddPoints(extra)
    assert not dev.resident()
    assert dev.Pointcloud().tobytes() == host.Pointcloud().tobytes()
    assert (dev.size(), dev.num_voxels()) == (host.size(), host.num_voxels())


def _run(sage, name, flat=None):
    s = mapscenes.scene(name, sage)
    ref = mapscenes.reference(name, sage)
    dev, host = make_map(sage, s), make_map(sage, s)
    for k, (pts, pose, refused) in enumerate(s["passes"]):
        for m, on_device in ((dev, True), (host, False)) + (((flat, True),) if flat is not None else ()):
            _update(sage, m, on_device, pts, pose, refused, k)
        assert dev.resident()
        a = _same(dev, host, k, ref[k])
        if flat is not None:
            assert flat.resident() and flat.Pointcloud().tobytes() == a.tobytes(), "pass %d: one full-size class" % (k + 1)
        if s["check"]:
            s["check"](k, a)
    return s, dev, host


@pytest.mark.parametrize("name", mapscenes.STAGE_NAMES + mapscenes.EDGE_NAMES)
def test_device_update_on_stage_and_domain_scenes(gpu_sage, name):
    _run(gpu_sage, name)


@pytest.mark.parametrize("name", mapscenes.CLASS_NAMES)
def test_device_update_on_class_boundaries(gpu_sage, monkeypatch, name):
    sage = gpu_sage
    monkeypatch.setenv("SAGEICP_SIZE_CLASSES", "0")
    flat = make_map(sage, mapscenes.scene(name, sage))
    monkeypatch.delenv("SAGEICP_SIZE_CLASSES")
    s, dev, host = _run(sage, name, flat)
    assert dev.point_slots() <= flat.point_slots()
    _hand_back(dev, host, s["extra"])


@pytest.mark.parametrize("name", mapscenes.CHAIN_NAMES)
def test_device_update_on_hash_chains(gpu_sage, oracle, name):
    """the chain keys share the last slot as home: lookups that must pass tombstones, claims behind them, chains that
    wrap to slot 0, k_rebuild with the chain in it — and the searches (k_rows, k_icp) over such a table"""
    sage = gpu_sage
    s = mapscenes.scene(name, sage)
    ref = mapscenes.reference(name, sage)
    p = s["params"]
    dev, host = make_map(sage, s), make_map(sage, s)
    orc = oracle.Map(p["voxel_size"], p["max_distance"], p["basic"], p["critical"])
    box1, box2, held = s["chain"]
    for cap in (1024, 2048, 65536):         # what the scene rests on, from the product's hash
        assert len({sage.voxel_hash(*k) & (cap - 1) for k in box1[:17] + box2[:17]}) <= 2
    stats = dev.table_stats()
    for k, (pts, pose, _) in enumerate(s["passes"]):
        before = stats
        dev.UpdateOnDevice(pts, pose)
        host.Update(pts, pose)
        orc.add_points(np.array(mapref.transform(pose, pts)).reshape(-1, 4))
        orc.remove_far(pose[4:])
        assert dev.resident()
        _same(dev, host, k, ref[k])
        stats = cap, used, live = dev.table_stats()
        assert live == dev.num_voxels() and used * 4 <= cap
        if s["table"].get(k) == "same":
            assert cap == before[0], "pass %d rebuilt the table: the scene wants its tombstones kept" % (k + 1)
        if s["table"].get(k) == "grown":
            assert cap > before[0] and cap <= 65536
        if k in s["tombstones"]:
            assert used > live, "pass %d: no tombstone in the table" % (k + 1)
        if k in s["queries"]:
            q = s["queries"][k]
            assert len(q) <= 2000
            guess = np.array([0.0, 0.0, 0.0, 1.0, 0.05, -0.03, 0.02])
            Ta, sa = sage.register_frame(q, dev, guess, 3.0, 0.5, 0.4, return_stats=True)
            Tb, sb = sage.register_frame(q, host, guess, 3.0, 0.5, 0.4, return_stats=True)
            assert dev.resident() and Ta.tobytes() == Tb.tobytes(), "pass %d" % (k + 1)
            assert (sa.iterations, sa.n_corr_first, sa.n_corr_last) == (sb.iterations, sb.n_corr_first, sb.n_corr_last)
            assert sa.n_corr_first > 0
            c = dev.clone()                  # (device to device; GetCorrespondences downloads the copy it is given)
            _, tgt, idx = c.GetCorrespondences(q, 3.0, 0.4, with_index=True)
            _, otgt, oidx = orc.get_correspondences(q, 3.0, 0.4, with_index=True)
            assert dev.resident() and np.array_equal(idx, oidx) and tgt.tobytes() == otgt.tobytes(), "pass %d" % (k + 1)
    _hand_back(dev, host, s["extra"])


def test_device_update_rebuilds_on_tombstones_alone(gpu_sage):
    """~370 live voxels while every pass leaves ~300 tombstones: the table is rebuilt at its size, never grown"""
    sage = gpu_sage
    s = mapscenes.scene("d_tombstones", sage)
    ref = mapscenes.reference("d_tombstones", sage)
    dev, host = make_map(sage, s), make_map(sage, s)
    stats, bound, rebuilt_in_place = dev.table_stats(), 1024, 0
    for k, (pts, pose, _) in enumerate(s["passes"]):
        cap0, used0, live0 = stats
        bound = max(bound, _pow2_for(live0 + len(pts)))
        rebuilds = (used0 + len(pts)) * 4 > cap0            # the rule of the device-side update
        dev.UpdateOnDevice(pts, pose)
        host.Update(pts, pose)
        _same(dev, host, k, ref[k])
        stats = cap, used, live = dev.table_stats()
        assert live == dev.num_voxels()
        assert used * 4 <= cap, "pass %d: load beyond a quarter" % (k + 1)
        assert cap <= bound, "pass %d: tombstones grew the table (%d slots, %d would do)" % (k + 1, cap, bound)
        # voxels the pass opened and evicted: the points are one per new voxel, plus the runs into live voxels
        evicted = ref[k - 1][2] + s["new_voxels"][k] - ref[k][2] if k else s["new_voxels"][0] - ref[0][2]
        if rebuilds:
            # no older tombstone survives a rebuild: the used slots are the live voxels plus what THIS pass evicted
            # (used == live where it evicted nothing)
            assert used == live + evicted, "pass %d" % (k + 1)
            rebuilt_in_place += cap == cap0 and k > 0
        else:
            assert used == used0 + s["new_voxels"][k]
    assert rebuilt_in_place >= 2, "the scene never rebuilt the table on tombstones alone"
    _hand_back(dev, host, s["extra"])


@pytest.mark.parametrize("name", mapscenes.CHAIN_NAMES + ["d_tombstones"])
def test_device_update_in_reference_order_mode(gpu_sage, name):
    """maps in reference-order mode: the device inserts and finds the far voxels, the host replays the bucket array
    and the device evicts what its sweep reached (map_update_insert_find_far, map_evict_listed)"""
    sage = gpu_sage
    s = mapscenes.scene(name, sage)
    dev, host = make_map(sage, s).set_reference_order(), make_map(sage, s).set_reference_order()
    for k, (pts, pose, _) in enumerate(s["passes"]):
        dev.UpdateOnDevice(pts, pose)
        host.Update(pts, pose)
        assert dev.resident() and dev.reference_order() == host.reference_order() == 1
        _same(dev, host, k)
        cap, used, live = dev.table_stats()
        assert used * 4 <= cap and live == dev.num_voxels()
    _hand_back(dev, host, s["extra"])
