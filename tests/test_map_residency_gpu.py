"""One map walked through every transition between its two copies (csrc/map_device.h: nothing valid in HBM, mirror of
the host copy, HBM copy the authority, host copy downloaded again) beside a twin that holds the same contents and is
only ever changed through host entries.  After every step the two answer alike: the counts, Pointcloud() row for row,
and a RegisterFrame of one fixed frame bit for bit — under both forms of the scan, so that a compact copy left over
from before a change of the HBM copy shows as another pose.  Needs the MI355X."""
import numpy as np
import pytest

from test_map_update_device import LABELS, _frames

pytestmark = pytest.mark.gpu

REFUSAL = "Update: a coordinate or label is not finite (NaN / Inf); the map is unchanged"


class _Walk:
    def __init__(self, sage, scan_form, caps, seed, oracle_map=None):
        self.sage, self.compact = sage, int(scan_form == "compact")
        kw = dict(basic_points_per_voxel=caps[0], critical_points_per_voxel=caps[1])
        self.m, self.twin = sage.VoxelHashMap(1.0, 12.0, **kw), sage.VoxelHashMap(1.0, 12.0, **kw)
        self.om = oracle_map                    # a map in reference-order mode: the oracle follows every step too
        if oracle_map is not None:
            for x in (self.m, self.twin):
                x.set_reference_order(True)
        # (a sensor that moves 6 m per frame through a map of 12 m: every update evicts, freed blocks are taken again)
        self.frames = _frames(seed, 6, 4000, 9.0, 6.0)
        self.query = _frames(seed + 1, 1, 2000, 9.0, 6.0)[0][0]
        self.rng = np.random.default_rng(seed + 2)
        self.pose = sage.IDENTITY               # the sensor's at the last update: the query frame is registered from near it

    def check(self, step, resident, m=None, twin=None):
        """the map answers like its twin; `resident`: the HBM copy is expected to be the authority"""
        sage, m, twin = self.sage, m or self.m, twin or self.twin
        assert m.resident() == resident and not twin.resident(), step
        counts = lambda x: (x.size(), x.num_voxels(), x.Empty())            # noqa: E731
        print(step, "map", counts(m), m.point_slots(), m.table_stats(), "twin", counts(twin), twin.point_slots(),
              twin.table_stats())
        assert counts(m) == counts(twin), step
        assert m.point_slots() >= m.size(), step
        cap, used, voxels = m.table_stats()
        assert voxels == m.num_voxels() == twin.table_stats()[2], step
        assert used >= voxels if resident else used == voxels, step          # (a device pass leaves tombstones)
        assert used <= cap, step
        cloud = m.Pointcloud()
        assert m.resident() == resident, "%s: Pointcloud() moved the authority" % step
        assert np.array_equal(cloud, twin.Pointcloud()), step
        guess, q = np.array(self.pose, dtype=np.float64), self.query
        guess[4:] += [0.3, -0.2, 0.05]
        Ta, sa = sage.register_frame(q, m, guess, 3.0, 0.5, 0.4, return_stats=True)
        Tb, sb = sage.register_frame(q, twin, guess, 3.0, 0.5, 0.4, return_stats=True)
        print(step, "iterations", sa.iterations, sb.iterations, "pairs", sa.n_corr_last, sb.n_corr_last,
              "compact", sa.compact_scan, sb.compact_scan)
        assert m.resident() == resident, "%s: RegisterFrame moved the authority" % step
        if m.Empty():
            assert np.array_equal(Ta, guess) and np.array_equal(Tb, guess) and sa.iterations == 0, step
            return
        assert sa.compact_scan == sb.compact_scan == self.compact, step
        assert sa.iterations == sb.iterations > 0 and sa.n_corr_last == sb.n_corr_last > 0, step
        assert np.array_equal(Ta, Tb), "%s: another pose than on the twin" % step

    def follow(self, p, pose):
        """the oracle takes the update as well (the points moved by the product's own transform, as the other map tests
        do); the query frame is registered from this pose from now on"""
        if self.om is not None:
            self.om.add_points(self.sage.transform_points(pose, p))
            self.om.remove_far(pose[4:])
        self.pose = pose

    def update(self, k, m=None, twin=None, part=slice(None)):
        p, pose = self.frames[k]
        (m or self.m).UpdateOnDevice(p[part], pose)
        (twin or self.twin).Update(p[part], pose)
        self.follow(p[part], pose)

    def run(self):
        sage, m, twin = self.sage, self.m, self.twin
        p, pose = self.frames[0]
        for x in (m, twin):                                                  # 1: host-built
            x.Update(p, pose)
        self.follow(p, pose)
        self.check("1 host-built", False)                                    # (its search mirrors the map)
        m.sync()                                                             # 2: mirrored, and searched as it stands
        self.check("2 mirrored", False)
        self.update(1)                                                       # 3: the HBM copy becomes the authority
        self.check("3 device update", True)
        self.check("4 RegisterFrame on the resident map", True)              # 4, 5: neither it nor Pointcloud() hands back
        before = m.table_stats()
        assert np.array_equal(m.Pointcloud(), twin.Pointcloud()) and m.resident() and m.table_stats() == before, "5"
        q = sage.transform_points(self.pose, self.query)                     # 6: GetCorrespondences hands the map back
        got, want = m.GetCorrespondences(q, 3.0, 0.4, with_index=True), twin.GetCorrespondences(q, 3.0, 0.4, with_index=True)
        assert len(got[2]) > 0 and all(np.array_equal(a, b) for a, b in zip(got, want))
        self.check("6 handed back", False)
        extra = self.rng.uniform(-8, 8, size=(700, 4)) + np.append(self.pose[4:], 0.0)
        extra[:, 3] = self.rng.choice(LABELS, size=len(extra))
        for x in (m, twin):                                                  # 7: a host entry on the downloaded copy
            x.AddPoints(extra)
        if self.om is not None:
            self.om.add_points(extra)
        self.check("7 AddPoints", False)
        self.update(2)                                                       # 8: and back to the device
        self.check("8 device update again", True)
        clone = clone_twin = None
        if self.om is None:
            clone, clone_twin = m.clone(), twin.clone()                      # 9: a copy of the resident map, updated alone
            assert clone.resident() and m.resident()
            pose = self.pose
            self.update(3, clone, clone_twin, slice(0, 1000))
            self.check("9 clone", True, clone, clone_twin)
            assert clone.size() != m.size()
            self.pose = pose
            self.check("9 original", True)
            bad = self.frames[4][0].copy()                                   # 10: a refused update changes nothing
            bad[1234, 1] = np.nan
            with pytest.raises(sage.SageIcpError) as e:
                m.UpdateOnDevice(bad, self.frames[4][1])
            assert e.value.code == sage.ERR_INVALID and str(e.value).endswith(REFUSAL)
            self.check("10 refused update", True)
        for x in (m, twin):                                                  # 11: Clear
            x.Clear()
        if self.om is not None:
            self.om.clear()
        self.check("11 Clear", False)
        self.update(5)                                                       # 12: refill of the emptied handle on the device
        self.check("12 refill", True)
        if clone is not None:                                                # (the copy did not follow any of this)
            self.pose = self.frames[3][1]
            self.check("12 clone", True, clone, clone_twin)
            assert clone.size() != m.size()


def test_walk_through_every_residency_transition(gpu_sage, scan_form):
    _Walk(gpu_sage, scan_form, (4, 3), 5).run()


def test_walk_at_the_reference_capacities(gpu_sage):
    _Walk(gpu_sage, "full", (20, 20), 6).run()          # (2,000 queries: the library's own choice is the full records)


def test_walk_of_a_reference_order_map(gpu_sage, oracle, scan_form):
    """steps 1-8, 11 and 12 on a map in reference-order mode; the oracle's emulation of the bucket array (mode 3)
    follows the same entries and lists the same Pointcloud() at the end"""
    oracle.set_robin_order(3)
    try:
        w = _Walk(gpu_sage, scan_form, (4, 3), 7, oracle_map=oracle.Map(1.0, 12.0, 4, 3))
        w.run()
        assert w.m.reference_order() == 1 and w.twin.reference_order() == 1
        assert np.array_equal(w.m.Pointcloud(), w.om.pointcloud())
    finally:
        oracle.set_robin_order(False)
