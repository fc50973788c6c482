"""Recall on the GPU (include/sageicp.h "recall"): a place of the session's map put back into a map, compared
as bytes against the restatement (tests/recallref.py) applied to the SESSION export, and against the only route the library
offered before — ArchivedPointcloud("session"), AddPoints into a twin of max_distance = radius, RemovePointsFarFromLocation."""
import math
import os

import numpy as np
import pytest

import archiveref as ar
import recallref
from test_recall_host import CENTRES, CHECKPOINTS, RADII, _map

pytestmark = pytest.mark.gpu

VS = ar.PARAMS["voxel_size"]


def _twin(sage, session, centre, radius, **over):
    """the existing route"""
    t = _map(sage, **dict(over, max_distance=radius))
    t.AddPoints(session)
    t.RemovePointsFarFromLocation(np.asarray(centre, dtype=np.float64))
    return t


def _recall_and_check(sage, src, centre, radius, into=None, what="", **over):
    """one recall of src, everything the definition says about it asserted; returns (dst, twin, info).  The recall is made
    before the SESSION export, so it meets src's archive as the scene left it (a pending host tail included)."""
    was_resident = src.resident()
    dst, info = src.Recall(centre, radius, into=into)
    assert src.resident() == was_resident, what
    session = src.ArchivedPointcloud("session")
    n_arc = len(src.ArchivedPointcloud("latest"))
    want, voxels = recallref.recall(session, VS, centre, radius)
    assert info == recallref.info(session, n_arc, VS, centre, radius), what
    cloud = dst.Pointcloud()
    assert cloud.tobytes() == want.tobytes(), what
    assert dst.size() == len(want) and dst.num_voxels() == voxels and dst.resident(), what
    assert dst.Empty() == (voxels == 0)
    cap, used, live = dst.table_stats()
    assert used == live == voxels and (voxels + 1) * 4 <= cap and cap & (cap - 1) == 0, (what, cap, used, live)
    twin = _twin(sage, session, centre, radius, **over)
    assert twin.Pointcloud().tobytes() == cloud.tobytes(), what
    assert (twin.size(), twin.num_voxels()) == (dst.size(), dst.num_voxels()), what
    assert dst.point_slots() <= twin.point_slots() or voxels == 0, what         # each region in its final class
    return dst, twin, info


def _voxel_groups(cloud):
    """{key: the voxel's rows as bytes}: what two maps must share when their block numbering may differ"""
    return {k: np.array(rows).tobytes() for k, rows in recallref.groups(cloud, VS)}


# ---- 1. the walk -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reference_order", [False, True], ids=["default", "reference_order"])
@pytest.mark.parametrize("entry", ["remove_far", "update", "update_pose", "device"])
def test_the_walk_through_every_update_entry(gpu_sage, entry, reference_order):
    sage = gpu_sage
    src = _map(sage)
    if reference_order:
        src.set_reference_order(True)
    src.set_archive(True)
    ref = None if reference_order else ar.ArchiveRef(**ar.PARAMS)
    seen = set()
    for k, (pts, origin) in enumerate(ar.walk()):
        ar.apply_step(src, entry, pts, origin)
        if ref is not None:
            ar.ref_step(ref, pts, origin)
        if k + 1 not in CHECKPOINTS:
            continue
        if ref is not None:       # the session the recalls are held to is the restatement's
            live = ar.keys_of(ref.pointcloud(), VS)
            assert src.ArchivedPointcloud("session").tobytes() == ar.session(ref.log, live, ref.pointcloud()).tobytes()
        for centre in CENTRES:
            for radius in RADII:
                _, _, info = _recall_and_check(sage, src, centre, radius, what="%s step %d %r %r" % (entry, k, centre, radius))
                if k + 1 == 11:
                    assert info["map_voxels"] == info["map_rows"] == 0 and src.num_voxels() == 0
                if radius == math.inf:
                    assert info["rows"] == info["session_rows"] and info["voxels"] == info["session_voxels"] > 0
                seen.add("some" if 0 < info["voxels"] < info["session_voxels"] else "all" if info["voxels"] else "none")
                if info["archive_voxels"] and info["map_voxels"]:
                    seen.add("both parts")
        assert src.resident() == (entry == "device")
    assert seen == {"some", "all", "none", "both parts"}, seen
    counts = {len(rows) for _, rows in recallref.groups(src.ArchivedPointcloud("session"), VS)}
    assert counts >= {1, 4, 5, 8, 9, 16, 17, 40}, sorted(counts)          # both sides of every size class's edge


# ---- 2. the rule at the edge -------------------------------------------------------------------------------------------
# Coordinates are multiples of 1/64: every difference and square below is exact.  Centre (10.5, 10.5, 0.5), radius 5.
EDGE_CENTRE = (10.5, 10.5, 0.5)
EDGE_VOXELS = {
    "at the radius": [(13.5, 14.5, 0.5), (13.25, 14.25, 0.25), (13.75, 14.75, 0.75)],     # d = (3, 4, 0): d2 == r2, kept
    "1/64 beyond": [(7.5, 6.5 - 1 / 64, 0.5)],                                           # d = (-3, -4 - 1/64, 0): dropped
    "first row out, later rows in": [(15.75, 10.5, 0.5), (15.25, 10.5, 0.5), (15.0, 10.5, 0.5)],
    "first row in, later rows out": [(5.75, 10.5, 0.5), (5.25, 10.5, 0.5), (5.0, 10.5, 0.5)],
    "single row inside": [(10.5, 8.5, 0.5)],
    "single row at the radius on an axis": [(10.5, 10.5, 5.5)],
    "far away": [(40.5, 40.5, 0.5), (40.25, 40.5, 0.5)],
}
EDGE_KEPT = ["at the radius", "first row in, later rows out", "single row inside", "single row at the radius on an axis"]


def _edge_rows():
    return np.array([p + (71.0,) for rows in EDGE_VOXELS.values() for p in rows], dtype=np.float64)


def _rows_of(names):
    return np.array([p + (71.0,) for n in names for p in EDGE_VOXELS[n]], dtype=np.float64).reshape(-1, 4)


@pytest.mark.parametrize("state", ["live on the host", "live and resident", "archived"])
def test_the_rule_at_the_edge(gpu_sage, state):
    sage = gpu_sage
    src = _map(sage, max_distance=100.0).set_archive(True)
    if state == "live on the host":
        src.AddPoints(_edge_rows())
    else:
        src.UpdateOnDevice(_edge_rows(), ar.pose_of((0.0, 0.0, 0.0)))
    if state == "archived":
        src.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of((5000.0, 0.0, 0.0)))
        assert src.num_voxels() == 0 and src.archive_info()["voxels"] == len(EDGE_VOXELS)
    assert src.ArchivedPointcloud("session").tobytes() == _edge_rows().tobytes()
    dst, _, info = _recall_and_check(sage, src, EDGE_CENTRE, 5.0, what=state, max_distance=100.0)
    assert dst.Pointcloud().tobytes() == _rows_of(EDGE_KEPT).tobytes()
    part = "archive" if state == "archived" else "map"
    assert info[part + "_voxels"] == info["voxels"] == len(EDGE_KEPT)
    # a centre that is a first row, radius 0: exactly that voxel, whole
    first = EDGE_VOXELS["at the radius"][0]
    dst, _, _ = _recall_and_check(sage, src, first, 0.0, into=dst, what=state)
    assert dst.Pointcloud().tobytes() == _rows_of(["at the radius"]).tobytes()
    # a later row as the centre finds nothing: the first row alone decides
    dst, _, _ = _recall_and_check(sage, src, EDGE_VOXELS["at the radius"][1], 0.0, into=dst, what=state)
    assert dst.Empty()
    # nothing kept: empty, resident, and a map like any other
    dst, twin, info = _recall_and_check(sage, src, (1000.0, 1000.0, 1000.0), 3.0, what=state)
    assert info["voxels"] == 0 and dst.Empty() and dst.resident()
    # (the twin is empty too, but its evicted blocks are free and handed out first: a fresh map is what numbers its blocks alike)
    fresh = _map(sage, max_distance=3.0)
    pts, origin = ar.walk()[0]
    for m in (dst, twin, fresh):
        ar.apply_step(m, "device", pts, origin)
    assert dst.Pointcloud().tobytes() == fresh.Pointcloud().tobytes() and dst.size() > 0
    assert _voxel_groups(dst.Pointcloud()) == _voxel_groups(twin.Pointcloud())


# ---- 3. more than one wave and workgroup -------------------------------------------------------------------------------
SHEET_MAX_DISTANCE = 22.0
SHEET_CENTRE, SHEET_RADIUS = (13.5, 15.0, 0.5), 13.5


def _sheet(seed=5):
    """30 x 30 voxels of 1 m, counts cycling through archiveref.COUNTS, the rows shuffled"""
    rng = np.random.default_rng(seed)
    parts = [ar._voxel_points(rng, ix, iy, ar.COUNTS[(30 * ix + iy) % len(ar.COUNTS)]) for ix in range(30) for iy in range(30)]
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))]


def _sheet_source(sage, entry):
    """A few rows and a voxel born out of range first (the log gets its first, small allocation), then the sheet (the
    update's bound re-allocates the log), then one update that evicts about half of the sheet."""
    src = _map(sage, max_distance=SHEET_MAX_DISTANCE).set_archive(True)
    first = np.concatenate([ar._voxel_points(np.random.default_rng(1), 15, 15, 3), [[3000.5, 0.5, 0.5, 71.0]]])
    sizes = []
    for pts, origin in ((first, (15.0, 15.0, 0.5)), (_sheet(), (15.0, 15.0, 0.5)), (np.zeros((0, 4)), (-7.0, 15.0, 0.5))):
        ar.apply_step(src, entry, pts, origin)
        sizes.append(src.archive_info()["device_bytes"])
    return src, sizes


@pytest.mark.parametrize("form", ["device", "log re-allocated", "pending host tail"])
def test_a_sheet_of_many_voxels(gpu_sage, form):
    sage = gpu_sage
    if form == "log re-allocated":
        os.environ["SAGEICP_ARCHIVE_INITIAL_ROWS"] = "64"
    try:
        src, sizes = _sheet_source(sage, "update_pose" if form == "pending host tail" else "device")
    finally:
        if form == "log re-allocated":
            del os.environ["SAGEICP_ARCHIVE_INITIAL_ROWS"]
    before = src.archive_info()
    if form == "pending host tail":
        assert before["host_rows"] == before["rows"] > 0 and before["device_rows"] == 0 and not src.resident()
    else:
        assert before["device_rows"] == before["rows"] > 0 and src.resident()
    if form == "log re-allocated":
        assert 0 < sizes[0] < sizes[1], sizes
    dst, _, info = _recall_and_check(sage, src, SHEET_CENTRE, SHEET_RADIUS, what=form, max_distance=SHEET_MAX_DISTANCE)
    after = src.archive_info()
    assert after["host_rows"] == 0 and after["device_rows"] == after["rows"] == before["rows"]    # flushed, as by an export
    assert info["archive_voxels"] > 256 and info["map_voxels"] > 256, info
    assert info["archive_voxels"] % 64 and info["map_voxels"] % 64 and info["rows"] % 64, info    # the last wave ends mid-way
    assert 0.4 < info["archive_voxels"] / after["voxels"] < 0.7 and 0.4 < info["map_voxels"] / src.num_voxels() < 0.8, info
    assert info["session_voxels"] == 901


# ---- 4. dst as a map afterwards ----------------------------------------------------------------------------------------
def _walked_source(sage, steps=9):
    src = _map(sage).set_archive(True)
    for pts, origin in ar.walk()[:steps]:
        ar.apply_step(src, "device", pts, origin)
    return src


def _frame(rng, x0, n=400):
    """rows over voxels the walk filled and voxels it never saw (new voxels on both sides)"""
    p = np.empty((n, 4))
    p[:, 0] = x0 + rng.integers(0, 6 * 64, size=n) / 64.0
    p[:, 1] = rng.integers(0, 5 * 64, size=n) / 64.0
    p[:, 2] = rng.integers(4, 60, size=n) / 64.0
    p[:, 3] = rng.choice([71.0, 40.0, 0.0], size=n)
    return p


def test_a_recalled_map_is_searched_like_the_twin(gpu_sage):
    sage = gpu_sage
    src = _walked_source(sage)
    dst, twin, info = _recall_and_check(sage, src, (12.5, 1.0, 0.5), 6.5)
    assert info["archive_voxels"] and info["map_voxels"] and info["voxels"] < info["session_voxels"]
    frame = _frame(np.random.default_rng(4), 8.0)
    got, want = dst.GetCorrespondences(frame, 1.0, 0.5, with_index=True), twin.GetCorrespondences(frame, 1.0, 0.5, with_index=True)
    assert len(got[2]) > 50          # (rows from the host are answered by the host's path: the recalled map was downloaded)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()


def test_updates_after_a_recall_of_the_whole_session(gpu_sage):
    """radius inf into a map of max_distance 6.5: the existing route evicts nothing (its remove_far at max_distance = inf is
    the identity), so the twin is the SESSION rows added to a map of that max_distance, both maps hold the same blocks and
    every later update hands out the same ones: Pointcloud() stays equal byte for byte through an update on the device
    (which evicts), the download, and an insertion on the host"""
    sage = gpu_sage
    src = _walked_source(sage)
    dst, info = src.Recall((0.0, 0.0, 0.0), math.inf, into=_map(sage, max_distance=6.5))
    session = src.ArchivedPointcloud("session")
    twin = _map(sage, max_distance=6.5)
    twin.AddPoints(session)
    assert info["rows"] == len(session) and dst.Pointcloud().tobytes() == twin.Pointcloud().tobytes() == session.tobytes()
    rng = np.random.default_rng(6)
    frame, more = _frame(rng, 9.0), _frame(rng, 2.0)
    for m in (dst, twin):
        m.UpdateOnDevice(ar.sensor_rows(frame, (11.5, 1.0, 0.5)), ar.pose_of((11.5, 1.0, 0.5)))
    assert dst.resident() and session[:, 0].min() < 1.0 and dst.Pointcloud()[:, 0].min() > 4.0      # voxels were evicted
    assert dst.Pointcloud().tobytes() == twin.Pointcloud().tobytes()
    for m in (dst, twin):
        m.AddPoints(more)
    assert not dst.resident()
    assert dst.Pointcloud().tobytes() == twin.Pointcloud().tobytes()
    assert (dst.size(), dst.num_voxels()) == (twin.size(), twin.num_voxels())


def test_updates_after_a_recall_of_a_place(gpu_sage):
    """A recall that dropped voxels: the twin's evicted blocks are free and a later update hands them out first, while the
    recalled map's blocks below num_voxels are all taken — a new voxel may get another block, so Pointcloud() may list
    the voxels in another order.  Every voxel's rows (bit for bit, in stored order), the set of voxels and the counters
    stay equal through an update on the device that evicts, the download and an insertion on the host."""
    sage = gpu_sage
    src = _walked_source(sage)
    dst, twin, info = _recall_and_check(sage, src, (12.5, 1.0, 0.5), 6.5)
    assert info["archive_voxels"] and info["map_voxels"] and info["voxels"] < info["session_voxels"]
    rng = np.random.default_rng(6)
    frame, more = _frame(rng, 9.0), _frame(rng, 5.0)
    for m in (dst, twin):
        m.UpdateOnDevice(ar.sensor_rows(frame, (11.5, 1.0, 0.5)), ar.pose_of((11.5, 1.0, 0.5)))
    assert dst.resident() and dst.num_voxels() < info["voxels"] + 30         # max_distance 6.5 at x = 11.5: voxels left
    assert _voxel_groups(dst.Pointcloud()) == _voxel_groups(twin.Pointcloud())
    for m in (dst, twin):
        m.AddPoints(more)
    assert not dst.resident()
    assert _voxel_groups(dst.Pointcloud()) == _voxel_groups(twin.Pointcloud())
    assert (dst.size(), dst.num_voxels()) == (twin.size(), twin.num_voxels())
    frame2 = _frame(rng, 6.0)
    got, want = dst.GetCorrespondences(frame2, 1.0, 0.5), twin.GetCorrespondences(frame2, 1.0, 0.5)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and len(got[0]) > 50


def test_a_second_recall_replaces_the_first_and_the_destinations_archive_is_its_own(gpu_sage):
    sage = gpu_sage
    src = _walked_source(sage)
    dst = _map(sage, max_distance=3.0).set_archive(True)
    dst.UpdateOnDevice(ar.walk()[0][0], ar.pose_of((0.0, 0.0, 0.0)))
    dst.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of((900.0, 0.0, 0.0)))      # its own log: every voxel of that frame
    own = dst.archive_info()
    own_rows = dst.ArchivedPointcloud("all")
    assert own["voxels"] > 0 and dst.num_voxels() == 0
    _recall_and_check(sage, src, (0.5, 1.0, 0.5), 6.5, into=dst)
    first = dst.Pointcloud()
    assert dst.archive_info() == own and dst.ArchivedPointcloud("all").tobytes() == own_rows.tobytes()    # nothing logged
    _recall_and_check(sage, src, (16.5, 1.0, 0.5), 3.0, into=dst)
    assert dst.Pointcloud().tobytes() != first.tobytes()
    assert dst.archive_info() == own
    # ... and from now on it logs what it evicts, like any map
    held = dst.Pointcloud()
    dst.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of((900.0, 0.0, 0.0)))
    now = dst.archive_info()
    assert dst.num_voxels() == 0 and now["rows"] == own["rows"] + len(held) and now["updates"] == own["updates"] + 1
    assert dst.ArchivedPointcloud("all")[own["rows"]:].tobytes() == held.tobytes()


def test_the_pipelines_entry_recalls_from_its_local_map(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    p = sage.SageICP(voxel_size_map=1.0, max_range=60.0, min_range=1.0, local_map_range=30.0)
    p.set_archive(True)
    rng = np.random.default_rng(9)
    for i in range(3):
        T = syn.pose_from_rpy_t([0, 0, 0], [0.5 * i, 0.0, 0.0])
        p.RegisterFrame(syn.make_scan(rng, 3000, 60.0, T))
    session = p.SessionMap("session")
    centre, radius = (0.0, 0.0, 0.0), 10.0
    dst, info = p.Recall(centre, radius)
    c = p.config
    want, voxels = recallref.recall(session, c.voxel_size_map, centre, radius)
    assert 0 < voxels < info["session_voxels"] and info["voxels"] == voxels
    assert dst.Pointcloud().tobytes() == want.tobytes() and dst.resident()
    into = sage.VoxelHashMap(c.voxel_size_map, radius, c.basic_points_per_voxel, c.critical_points_per_voxel,
                             [c.basic_parts_labels[i] for i in range(c.n_basic_parts_labels)])
    again, info2 = p.Recall(centre, radius, into=into)
    assert again is into and info2 == info and into.Pointcloud().tobytes() == want.tobytes()


# ---- 5. run to run -----------------------------------------------------------------------------------------------------
def test_the_same_recall_twice_gives_the_same_bytes(gpu_sage):
    sage = gpu_sage
    src, _ = _sheet_source(sage, "device")
    a, ia = src.Recall(SHEET_CENTRE, SHEET_RADIUS)
    b, ib = src.Recall(SHEET_CENTRE, SHEET_RADIUS)
    c, ic = src.Recall(SHEET_CENTRE, SHEET_RADIUS, into=a)
    assert c is a and ia == ib == ic and ia["voxels"] > 512
    assert a.Pointcloud().tobytes() == b.Pointcloud().tobytes()
    assert (a.size(), a.num_voxels(), a.point_slots(), a.table_stats()) == (b.size(), b.num_voxels(), b.point_slots(), b.table_stats())


# ---- 5b. parts beyond one stride of the fill ---------------------------------------------------------------------------
# k_rc_fill launches at most 2048 x 256 lanes per part, a lane per row, and strides over the rest (as archive.hip's
# gathers do).  The sheet of archiveref.big_sheet holds 538,240 rows: 13,952 of a part are written on a second trip.
def test_an_archive_part_beyond_one_stride_of_the_fill(gpu_sage):
    sage = gpu_sage
    src = _map(sage, max_distance=ar.BIG_MAX_DISTANCE).set_archive(True)
    for pts, origin in ar.big_sheet_steps():                    # archived whole, 300 voxels in a second generation
        ar.apply_step(src, "device", pts, origin)
    assert src.num_voxels() == 0 and src.archive_info()["voxels"] == ar.BIG_SIDE ** 2 + ar.BIG_AGAIN
    dst, _, info = _recall_and_check(sage, src, ar.BIG_ORIGIN, math.inf, what="archive part")
    assert info["archive_rows"] == ar.BIG_SIDE ** 2 * ar.BIG_COUNT == 538240 and info["archive_rows"] > 524288 == ar.GATHER_STRIDE
    assert info["archive_voxels"] == ar.BIG_SIDE ** 2 and info["map_rows"] == 0
    # per voxel the rows offered last: the born-again voxels hold their second generation
    rows, again = ar.big_sheet()
    cloud = dst.Pointcloud()
    assert ar.by_voxel(cloud[-len(again):]).tobytes() == ar.by_voxel(again).tobytes()


def test_a_map_part_beyond_one_stride_of_the_fill(gpu_sage):
    sage = gpu_sage
    rows, _ = ar.big_sheet()
    token = np.array([[3000.5, 58.5, 0.5, 71.0], [3000.25, 58.5, 0.5, 71.0]])          # born out of range: archived at once
    src = _map(sage, max_distance=ar.BIG_MAX_DISTANCE).set_archive(True)
    ar.apply_step(src, "device", np.concatenate([token, rows]), ar.BIG_ORIGIN)
    assert src.resident() and src.num_voxels() == ar.BIG_SIDE ** 2 and src.archive_info()["rows"] == len(token)
    dst, _, info = _recall_and_check(sage, src, ar.BIG_ORIGIN, math.inf, what="map part")
    assert info["map_rows"] == len(rows) == 538240 and info["map_rows"] > 524288 == ar.GATHER_STRIDE
    assert info["archive_rows"] == len(token) and info["archive_voxels"] == 1
    assert ar.by_voxel(dst.Pointcloud()[len(token):]).tobytes() == ar.by_voxel(rows).tobytes()


# ---- 6. the loop closed ------------------------------------------------------------------------------------------------
# The street scene of tests/test_place_gpu.py driven through a map that forgets: 17 scans of 8000 points at their poses,
# 8 m apart, into a map of 1 m voxels and max_distance LOOP_MAX_DISTANCE with the archive on.  Place 9 lies 56 m behind
# place 16, so nothing of it is live when the revisit is recognised; the recall around it brings it back.
# The values needed: the scene as it is (8000 points per scan) with max_distance 30 and radius 25 — 25 + 30 < 56, so no
# first row can be within the radius of place 9 and still in the window at place 16.  Measured with them: the recall holds
# 3321 voxels / 10 912 rows of a session of 47 487 voxels / 75 327 rows, and Relocalize goes from 0.36 m / 1.00 deg at the
# prior to 0.127 m / 0.025 deg against the recalled map and against the twin alike (the scene needed no change to meet the
# bounds of test_closing_the_loop_through_relocalize).
LOOP_MAX_DISTANCE = 30.0
LOOP_RADIUS = 25.0


def test_the_loop_closed_through_recall(gpu_sage):
    from test_place_gpu import Street, _errors
    sage = gpu_sage
    s = Street(sage)
    vmap = sage.VoxelHashMap(1.0, LOOP_MAX_DISTANCE).set_archive(True)
    for scan, T in zip(s.scans, s.poses):
        vmap.UpdateOnDevice(scan, T)
    db = sage.PlaceDB(s.p)
    for i, e in enumerate(s.entries):
        db.add(e, tag=i, pose=s.poses[i])
    truth = s.q_poses[1]
    m = db.match(s.queries[1], top_k=1, h_tol=s.H_TOL)[0]
    assert m["index"] == 9
    centre = np.asarray(s.poses[9][4:7], dtype=np.float64)
    dst, info = vmap.Recall(centre, LOOP_RADIUS)
    print("recall around place 9:", info)
    assert info["map_voxels"] == 0 and info["archive_voxels"] > 0          # the local map has forgotten the place
    session = vmap.ArchivedPointcloud("session")
    twin = sage.VoxelHashMap(1.0, LOOP_RADIUS)
    twin.AddPoints(session)
    twin.RemovePointsFarFromLocation(centre)
    assert twin.Pointcloud().tobytes() == dst.Pointcloud().tobytes()
    ring_width = (s.p.max_range - s.p.min_range) / s.p.rings
    sector = 2.0 * math.pi / s.p.sectors
    args = dict(xy=(ring_width, ring_width / 2), yaw=(sector, sector / 2), refine_top=3)
    pose, _, _ = dst.Relocalize(s.q_scans[1], m["prior"], 2.0, 0.5, 0.05, **args)
    pose_twin, _, _ = twin.Relocalize(s.q_scans[1], m["prior"], 2.0, 0.5, 0.05, **args)
    before, after, after_twin = _errors(m["prior"], truth), _errors(pose, truth), _errors(pose_twin, truth)
    print("prior off by %.2f m %.2f deg; against the recalled map %.3f m %.3f deg; against the twin %.3f m %.3f deg"
          % (before + after + after_twin))
    assert pose.tobytes() == pose_twin.tobytes()
    assert after[0] < before[0] and after[1] < before[1]
    assert after[0] < 0.5 and after[1] < 3.0             # the bounds of test_closing_the_loop_through_relocalize
