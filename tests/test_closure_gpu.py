"""The device side of a loop closure on the GPU (include/sageicp.h "loop closure"): the pose every voxel of a
session's map is tied to (its stay), compared as integers, and the session's map re-posed, compared as bytes — against the
restatement (tests/closureref.py: the session enumerated from archive_voxels(), the plain exports and Pointcloud(); the
far test and the move in the library's operation order) and against sageicp_transform_points applied voxel by voxel.

Maps are tiny (voxels of 1 m, max_distance 5, a few points per frame, a few dozen poses), built with the update entries and
the archive on, without ICP; the one large map is the sheet that takes the walk beyond one grid stride of its launch and
the move beyond one of its own.  The street scene of the end-to-end case is sage_icp_amd.synthetic's (the one the place
tests recognise places in)."""
import ctypes

import numpy as np
import pytest
import torch

import archiveref as ar
import closureref as cr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
VS = 1.0
PARAMS = dict(ar.PARAMS, max_distance=5.0)
COUNTS = (1, 4, 5, 45, 9, 2, 17, 3)                    # 45 offered: the voxel keeps its maximum, 40
STAY_STRIDE = 512 * 256                                # closure.hip: voxels of one trip of the walk's launch
MOVE_STRIDE = 1024 * 256                               # ... rows of one trip of the move's


def _map(sage, **over):
    p = dict(PARAMS, **over)
    return sage.VoxelHashMap(p["voxel_size"], p["max_distance"], p["basic"], p["critical"], list(p["basic_labels"]))


def _corrections(sage, positions):
    """corrections that differ from pose to pose in rotation and translation: a closure over the positions themselves"""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    if n < 2:
        return np.array([[0.01, -0.02, 0.03, 0.9993, 0.25, -0.5, 0.125]])
    poses = np.concatenate([np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)), pos], axis=1)
    h = 0.5 * np.radians(6.0)
    closed = cr.se3_mul(np.array([0.0, 0.0, np.sin(h), np.cos(h), 0.75, -1.25, 0.125]), poses[n - 1])
    return sage.closure_corrections(poses, 0, n - 1, closed)[0]


def _by_transform_points(sage, rows, counts, stay, corrections):
    """sageicp_transform_points applied voxel by voxel"""
    out, at = [], 0
    for c, s in zip(counts, stay):
        out.append(sage.transform_points(corrections[int(s)], rows[at:at + c]))
        at += c
    return np.concatenate(out) if out else np.zeros((0, 4))


def _held(sage, m, positions, which, corrections=None, by_voxel=True, what=""):
    """stays as integers, corrected rows as bytes, for one selection; returns (rows, counts, updates, stays)"""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    was_resident = m.resident()
    got = m.SessionStays(pos, which)
    rows, counts, updates = cr.session_voxels(m, which, VS)
    want = cr.stays(cr.first_rows(rows, counts), updates, pos, m.max_distance_)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist(), what
    corr = _corrections(sage, pos) if corrections is None else corrections
    moved = m.CorrectedPointcloud(which, pos, corr)
    assert m.resident() == was_resident, what
    assert moved.tobytes() == cr.move(rows, counts, want, corr).tobytes(), what
    if by_voxel:
        assert moved.tobytes() == _by_transform_points(sage, rows, counts, want, corr).tobytes(), what
    assert moved[:, 3].tobytes() == rows[:, 3].tobytes(), what
    return rows, counts, updates, want


# ---- (a) out and back -------------------------------------------------------------------------------------------------
def _drive():
    """[(rows in the map frame, origin)]: out along x to 12, back to 0, out again to 8, each pass on its own lateral
    line (y = 1.0, 1.5, 2.0).  Every step inserts three voxels at the sensor's x, in y = 0, 1, 2; coordinates are multiples
    of 1/64.  The voxels at the start are evicted on the first pass, born again on the second and evicted again on the
    third; those at the far end are evicted on the second."""
    rng = np.random.default_rng(11)
    xs = list(range(0, 13)) + list(range(11, -1, -1)) + list(range(1, 9))
    lines = [1.0] * 13 + [1.5] * 12 + [2.0] * 8
    steps, k = [], 0
    for x, y in zip(xs, lines):
        parts = []
        for iy in (0, 1, 2):
            parts.append(ar._voxel_points(rng, x, iy, COUNTS[k % len(COUNTS)]))
            k += 1
        steps.append((np.concatenate(parts), (x + 0.5, y, 0.5)))
    return steps


_SCENES = {}


def _driven(sage, entry, reference_order=False):
    """the drive through one update entry, made once per module: (map, positions)"""
    key = (entry, reference_order)
    if key not in _SCENES:
        m = _map(sage)
        if reference_order:
            m.set_reference_order(True)
        m.set_archive(True)
        steps = _drive()
        for pts, origin in steps:
            ar.apply_step(m, entry, pts, origin)
        _SCENES[key] = (m, np.array([o for _, o in steps]))
    return _SCENES[key]


@pytest.fixture(scope="module", autouse=True)
def _scenes_go_with_the_module():
    yield
    _SCENES.clear()


@pytest.mark.parametrize("which", ["all", "latest", "session"])
@pytest.mark.parametrize("entry", ["device", "update_pose"])
def test_out_and_back(gpu_sage, entry, which):
    m, pos = _driven(gpu_sage, entry)
    assert m.archive_info()["updates"] == len(pos) and m.resident() == (entry == "device")
    rec = m.archive_voxels()
    keys = [(int(r.x), int(r.y), int(r.z)) for r in rec]
    assert max(keys.count(k) for k in set(keys)) >= 2                      # keys evicted twice
    rows, counts, updates, stay = _held(gpu_sage, m, pos, which, what="%s %s" % (entry, which))
    assert {1, 40} <= set(counts.tolist())                                 # a voxel of one row, one of the map's maximum
    if which == "session":
        assert (updates >= 0).any() and (updates < 0).any()
    # a record's stay ends before its eviction; nothing is tied to a pose at which its first row was far
    first = cr.first_rows(rows, counts)
    arc = updates >= 0
    assert (stay[arc] < updates[arc]).all()
    d2 = ((first[:, :3] - pos[stay]) ** 2).sum(axis=1)                      # (multiples of 1/64: exact)
    assert (d2 <= PARAMS["max_distance"] ** 2).all()


# ---- (b) the decider --------------------------------------------------------------------------------------------------
def test_the_stay_is_not_the_nearest_pose(gpu_sage):
    """live voxels born again on the third pass (y = 2.0) whose first row lies nearer to a pose of the first pass
    (y = 1.0): the nearest pose over all poses is not their stay, and its correction is the old pass's"""
    m, pos = _driven(gpu_sage, "device")
    rows, counts, updates = cr.session_voxels(m, "session", VS)
    first = cr.first_rows(rows, counts)
    live = updates < 0
    want = cr.stays(first, updates, pos, PARAMS["max_distance"])
    nearest = cr.nearest_pose(first, pos)
    differ = live & (nearest != want)
    assert differ.any()
    assert (nearest[differ] < 13).any()                                    # ... a pose of the first pass
    got = m.SessionStays(pos, "session")
    assert got.tolist() == want.tolist() and (got[differ] != nearest[differ]).all()
    # and the rows move with the stay's correction, not with the nearest pose's
    corr = _corrections(gpu_sage, pos)
    moved = m.CorrectedPointcloud("session", pos, corr)
    assert moved.tobytes() == cr.move(rows, counts, want, corr).tobytes()
    assert moved.tobytes() != cr.move(rows, counts, nearest, corr).tobytes()


# ---- (c) ties and the radius ------------------------------------------------------------------------------------------
def _one_voxel(sage, first_row, more=()):
    m = _map(sage)
    m.AddPoints(np.array([tuple(first_row) + (71.0,)] + [tuple(p) + (71.0,) for p in more]))
    assert m.num_voxels() == 1
    return m


def test_a_tie_goes_to_the_later_pose(gpu_sage):
    m = _one_voxel(gpu_sage, (10.5, 0.5, 0.5), more=[(10.25, 0.25, 0.25)])
    two = [(8.5, 0.5, 0.5), (12.5, 0.5, 0.5)]                               # both at 2 m
    assert m.SessionStays(two).tolist() == [1]
    assert m.SessionStays(two[::-1]).tolist() == [1]
    three = [(8.5, 0.5, 0.5), (12.5, 0.5, 0.5), (13.5, 0.5, 0.5)]           # 2, 2, 3 m: the walk meets 12.5 first
    assert m.SessionStays(three).tolist() == [1]
    assert m.SessionStays([(8.5, 0.5, 0.5), (8.5, 0.5, 0.5), (8.5, 0.5, 0.5)]).tolist() == [2]
    _held(gpu_sage, m, three, "session")


def test_exactly_at_max_distance_is_not_far(gpu_sage):
    # d = (3, 4, 0): d2 == 25 == max_distance^2 exactly.  The walk goes 2 (4 m), 1 (5 m: not far, goes on), 0 (1 m: nearest)
    pos = [(13.5, 13.5, 0.5), (10.5, 10.5, 0.5), (13.5, 18.5, 0.5)]
    at = _one_voxel(gpu_sage, (13.5, 14.5, 0.5))
    assert at.SessionStays(pos).tolist() == [0]
    # the next double above: far — the walk stops after position 2
    beyond = _one_voxel(gpu_sage, (13.5, float(np.nextafter(14.5, 15.0)), 0.5))
    assert beyond.SessionStays(pos).tolist() == [2]
    for m in (at, beyond):
        _held(gpu_sage, m, pos, "session")


# ---- (d) clamps -------------------------------------------------------------------------------------------------------
def test_clamps(gpu_sage):
    sage = gpu_sage
    # a record with update == 0: a voxel born out of range is evicted by the first call
    m = _map(sage).set_archive(True)
    m.AddPoints(np.array([[40.5, 0.5, 0.5, 71.0]]))
    steps = _drive()[:6]
    for pts, origin in steps:
        ar.apply_step(m, "device", pts, origin)
    pos = np.array([o for _, o in steps])
    rec = m.archive_voxels()
    assert rec[0].update == 0
    rows, counts, updates, stay = _held(sage, m, pos, "session", what="update == 0")
    assert stay[0] == 0
    # a stay that reaches k = 0: the first voxels are still live, never far from any of the six positions
    lengths = cr.stay_lengths(cr.first_rows(rows, counts), updates, pos, PARAMS["max_distance"])
    assert (lengths[updates < 0] == len(pos)).any()
    # n smaller than the archive's updates, and n == 1
    m2, pos2 = _driven(sage, "device")
    for n in (20, 7, 1):
        assert n < m2.archive_info()["updates"]
        _, _, updates, stay = _held(sage, m2, pos2[:n], "session", what="n = %d" % n)
        assert (stay < n).all() and (updates >= n).any()
    assert set(m2.SessionStays(pos2[:1], "session").tolist()) == {0}


# ---- (e) empty inputs -------------------------------------------------------------------------------------------------
def test_empty_inputs(gpu_sage):
    sage = gpu_sage
    pos = np.array([o for _, o in _drive()[:3]])
    off = _map(sage)                                                       # archive off: live voxels only
    on = _map(sage).set_archive(True)                                      # archive on and empty
    for m in (off, on):
        for pts, origin in _drive()[:3]:
            ar.apply_step(m, "device", pts, origin)
        assert m.archive_info()["voxels"] == 0
        for which in ("all", "latest"):
            assert len(m.SessionStays(pos, which)) == 0 and len(m.CorrectedPointcloud(which, pos, _corrections(sage, pos))) == 0
        rows, counts, updates, _ = _held(sage, m, pos, "session")
        assert len(counts) == m.num_voxels() > 0 and (updates < 0).all()
    empty = _map(sage)
    lib, dp = sage.lib(), ctypes.POINTER(ctypes.c_double)
    n_out = ctypes.c_uint64(99)
    corr = np.ascontiguousarray(_corrections(sage, pos))
    for which in (0, 1, 2):
        assert lib.sageicp_map_session_stays(empty._h, which, 0, pos.ctypes.data_as(dp), len(pos), None, 0, ctypes.byref(n_out)) == 0
        assert n_out.value == 0
        n_out.value = 99
        assert lib.sageicp_map_session_corrected(empty._h, which, 0, pos.ctypes.data_as(dp), corr.ctypes.data_as(dp), len(pos), None, 0,
                                                 ctypes.byref(n_out)) == 0
        assert n_out.value == 0
        n_out.value = 99


# ---- (f) sizes --------------------------------------------------------------------------------------------------------
def test_beyond_one_grid_stride(gpu_sage):
    """a sheet of 364 x 364 voxels of two rows: 132,496 voxels (one trip of the walk's launch takes 131,072) and 264,992
    rows (one trip of the move's takes 262,144) — live first, then evicted whole by one update far away"""
    sage = gpu_sage
    side = 364
    rng = np.random.default_rng(23)
    ix, iy = (a.reshape(-1) for a in np.meshgrid(np.arange(side), np.arange(side), indexing="ij"))
    n = 2 * side * side
    rows = np.empty((n, 4))
    rows[:, 0] = np.repeat(ix, 2) + rng.integers(4, 60, size=n) / 64.0
    rows[:, 1] = np.repeat(iy, 2) + rng.integers(4, 60, size=n) / 64.0
    rows[:, 2] = rng.integers(4, 60, size=n) / 64.0
    rows[:, 3] = 71.0
    rows = rows[rng.permutation(n)]
    m = _map(sage, max_distance=600.0).set_archive(True)                   # (holds the sheet from every position)
    near = [(40.5 + 12.0 * k, 300.5 - 9.0 * k, 0.5) for k in range(24)]    # a diagonal across the sheet
    m.UpdateOnDevice(ar.sensor_rows(rows, near[0]), ar.pose_of(near[0]))
    for o in near[1:]:
        m.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of(o))
    assert m.num_voxels() == side * side > STAY_STRIDE and m.size() == n > MOVE_STRIDE
    pos = np.array(near)
    corr = _corrections(sage, pos)
    _, counts, _, stay = _held(sage, m, pos, "session", corrections=corr, by_voxel=False, what="live")
    assert len(counts) > 256 and len(set(stay.tolist())) > 8
    away = (5000.5, 0.5, 0.5)
    m.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of(away))
    assert m.num_voxels() == 0 and m.archive_info()["voxels"] == side * side
    pos = np.array(near + [away])
    corr = _corrections(sage, pos)
    _, counts, updates, stay = _held(sage, m, pos, "all", corrections=corr, by_voxel=False, what="archived")
    assert (updates == len(near)).all() and (stay < len(near)).all()
    assert m.SessionStays(pos, "session").tolist() == stay.tolist()
    # one transform per correction is the same bytes as one per voxel: held once, at this size
    rows_, counts, updates = cr.session_voxels(m, "all", VS)
    per_row = np.repeat(stay, counts)
    want = np.empty_like(rows_)
    for s in np.unique(stay):
        pick = per_row == s
        want[pick] = sage.transform_points(corr[int(s)], rows_[pick])
    assert m.CorrectedPointcloud("all", pos, corr).tobytes() == want.tobytes()


# ---- (g) where the map lives ------------------------------------------------------------------------------------------
def test_a_log_partly_in_the_pending_host_tail(gpu_sage):
    sage = gpu_sage
    m = _map(sage).set_archive(True)
    steps = _drive()
    for pts, origin in steps[:20]:
        ar.apply_step(m, "device", pts, origin)
    for pts, origin in steps[20:]:                                         # the host copy evicts: its records wait on the host
        ar.apply_step(m, "remove_far", pts, origin)
    info = m.archive_info()
    assert info["device_rows"] > 0 and info["host_rows"] > 0 and info["updates"] == len(steps)
    pos = np.array([o for _, o in steps])
    stay = m.SessionStays(pos, "session")                                  # meets the pending tail
    assert m.archive_info()["host_rows"] == 0
    m2, _ = _driven(sage, "device")
    assert stay.tolist() == m2.SessionStays(pos, "session").tolist()
    _held(sage, m, pos, "session")


@pytest.mark.parametrize("which", ["latest", "session"])
def test_a_reference_order_source(gpu_sage, which):
    m, pos = _driven(gpu_sage, "update_pose", reference_order=True)
    _held(gpu_sage, m, pos, which)
    r, pos = _driven(gpu_sage, "device", reference_order=True)
    assert r.resident()
    _held(gpu_sage, r, pos, which)
    assert r.resident()


# ---- (h) export mechanics ---------------------------------------------------------------------------------------------
def test_export_mechanics(gpu_sage):
    sage = gpu_sage
    m, pos = _driven(sage, "device")
    corr = _corrections(sage, pos)
    whole = m.CorrectedPointcloud("session", pos, corr)
    total = len(whole)
    n_arc = len(m.ArchivedPointcloud("latest"))
    assert 0 < n_arc < total
    # in pieces through first and cap (a piece across the seam of the two parts among them); nothing beyond cap
    cuts = [0, 7, n_arc - 3, n_arc + 5, total]
    for a, b in zip(cuts[:-1], cuts[1:]):
        buf = torch.full((b - a + 4, 4), -7.0, dtype=torch.float64, device=DEV)
        got = m.CorrectedPointcloud("session", pos, corr, first=a, out=buf[:b - a])
        assert got.shape[0] == b - a and got.cpu().numpy().tobytes() == whole[a:b].tobytes()
        assert (buf[b - a:] == -7.0).all()
    assert len(m.CorrectedPointcloud("session", pos, corr, first=total)) == 0
    stays = m.SessionStays(pos, "session")
    assert m.SessionStays(pos, "session", first=5).tolist() == stays[5:].tolist()
    few = np.full(9, 77, dtype=np.uint32)
    k = ctypes.c_uint64(0)
    dp = ctypes.POINTER(ctypes.c_double)
    assert sage.lib().sageicp_map_session_stays(m._h, 2, 3, pos.ctypes.data_as(dp), len(pos),
                                                few.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 6, ctypes.byref(k)) == 0
    assert k.value == len(stays) and few[:6].tolist() == stays[3:9].tolist() and few[6:].tolist() == [77] * 3
    # float32 rows with the labels apart
    o, l = m.CorrectedPointcloud("session", pos, corr, out=torch.empty((total, 3), dtype=torch.float32, device=DEV),
                                 labels_out=torch.empty(total, dtype=torch.uint8, device=DEV))
    assert np.array_equal(o.cpu().numpy().view(np.uint32), whole[:, :3].astype(np.float32).view(np.uint32))
    assert np.array_equal(l.cpu().numpy(), whole[:, 3].astype(np.uint8))
    # a destination on a caller's stream, behind work the caller enqueued on it
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        dst = torch.zeros((total, 4), dtype=torch.float64, device=DEV)
        dst.fill_(3.0)
        got = m.CorrectedPointcloud("session", pos, corr, out=dst)
        doubled = got * 2.0
    s.synchronize()
    assert got.cpu().numpy().tobytes() == whole.tobytes() and np.array_equal(doubled.cpu().numpy(), whole * 2.0)
    with pytest.raises(sage.SageIcpError) as e:
        m.CorrectedPointcloud("session", pos, np.full_like(corr, np.nan))
    assert e.value.code == sage.ERR_INVALID


# ---- (i) identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "latest", "session"])
def test_identity_corrections_give_the_plain_export(gpu_sage, which):
    m, pos = _driven(gpu_sage, "device")
    identity = np.tile([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], (len(pos), 1))
    plain = m.ArchivedPointcloud(which, device=True)                       # sageicp_map_archive_rows_device
    got = m.CorrectedPointcloud(which, pos, identity, device=True)
    assert len(plain) > 0 and got.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    assert m.CorrectedPointcloud(which, pos, identity).tobytes() == m.ArchivedPointcloud(which).tobytes()


# ---- (j) end to end ---------------------------------------------------------------------------------------------------
def test_a_closed_loop_puts_the_street_back_together(gpu_sage):
    """A square of 20 m a side driven once round the street scene, back to its start, with a window (max_distance 4) that
    evicted the start long before.  The true frames are inserted at poses that drift sideways by DRIFT metres per metre
    driven; the closure says where the last pose really is."""
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    DRIFT, SIDE, RADIUS = 0.05, 20, 4.0
    u = np.array([0.6, 0.8, 0.0])                                          # the drift's direction
    corners = [(0.0, 0.0), (SIDE, 0.0), (SIDE, SIDE), (0.0, SIDE), (0.0, 0.0)]
    true_t = [np.array([8.0, 3.0, 0.0])]
    for (x0, y0), (x1, y1) in zip(corners[:-1], corners[1:]):
        for s in range(1, SIDE + 1):
            true_t.append(true_t[0] + np.array([x0 + (x1 - x0) * s / SIDE, y0 + (y1 - y0) * s / SIDE, 0.0]))
    true_t = np.array(true_t)
    n = len(true_t)
    # the drift is linear in the path length of the trajectory the session knows, the drifted one: step by step,
    # dL = |dt + DRIFT dL u|, solved for dL
    path = np.zeros(n)
    for k in range(1, n):
        dt = true_t[k] - true_t[k - 1]
        s2, b = dt @ dt, DRIFT * (dt @ u)
        path[k] = path[k - 1] + (b + np.sqrt(b * b + (1.0 - DRIFT * DRIFT) * s2)) / (1.0 - DRIFT * DRIFT)
    drift_t = true_t + DRIFT * path[:, None] * u
    assert np.allclose(np.linalg.norm(np.diff(drift_t, axis=0), axis=1), np.diff(path), rtol=1e-12, atol=0.0)
    rot = [0.0, 0.0, 0.0, 1.0]
    rng = np.random.default_rng(2024)
    m = sage.VoxelHashMap(1.0, RADIUS, 20, 20, [40, 44, 48]).set_archive(True)
    truth = {}
    for k in range(n):
        T = np.array(rot + list(true_t[k]))
        scan = syn.make_scan(rng, 160, 40.0, T, max_range=3.5, min_range=0.5, label_max_range=50.0)
        m.UpdateOnDevice(scan, np.array(rot + list(drift_t[k])))
        for w, t in zip(scan[:, :3] + drift_t[k], scan[:, :3] + true_t[k]):  # (identity rotation: the library's own sum)
            truth[w.tobytes()] = (t, k)
    assert m.archive_info()["updates"] == n
    poses = np.concatenate([np.tile(rot, (n, 1)), drift_t], axis=1)
    closed = np.array(rot + list(true_t[n - 1]))                            # the true pose of the last frame
    corr, fixed, info = sage.closure_corrections(poses, 0, n - 1, closed, return_info=True)
    whole_drift = DRIFT * path[-1]
    assert info["shift"] == pytest.approx(whole_drift, rel=1e-12) and info["path"] == pytest.approx(path[-1], rel=1e-12)
    plain = m.ArchivedPointcloud("session")
    true_rows = np.array([truth[p.tobytes()][0] for p in plain[:, :3]])    # every row of the session is a row some frame inserted
    frame_of = np.array([truth[p.tobytes()][1] for p in plain[:, :3]])
    # before: at the seam the first frames' rows are where they belong, the last frames' rows off by the whole drift
    before = np.linalg.norm(plain[:, :3] - true_rows, axis=1)
    at_seam = np.linalg.norm(true_rows[:, :2] - true_t[0, :2], axis=1) < 3.5
    old, new = at_seam & (frame_of <= 3), at_seam & (frame_of >= n - 3)
    assert old.any() and new.any()
    seam_error = before[new].max() - before[old].min()
    assert seam_error >= 0.95 * whole_drift
    # the bound, from this trajectory: a row was inserted inside its voxel's stay and is corrected by a pose of that stay
    rows, counts, updates = cr.session_voxels(m, "session", 1.0)
    first = cr.first_rows(rows, counts)
    lengths = cr.stay_lengths(first, updates, drift_t, RADIUS)
    hi = np.where(updates < 0, n, np.minimum(updates, n)) - 1
    assert (lengths > 0).all()
    longest = (path[hi] - path[hi - lengths + 1]).max()
    bound = DRIFT * longest + 1e-9
    print("whole drift %.3f m, seam error %.3f m, longest stay %.2f m of path, bound %.3f m" % (whole_drift, seam_error, longest, bound))
    assert bound < 0.25 * seam_error
    stay = m.SessionStays(drift_t, "session")
    assert stay.tolist() == cr.stays(first, updates, drift_t, RADIUS).tolist()
    per_row = np.repeat(stay, counts)
    assert (np.abs(frame_of - per_row) < lengths.max()).all()
    fixed_rows = m.CorrectedPointcloud("session", drift_t, corr)
    assert fixed_rows.tobytes() == cr.move(rows, counts, stay, corr).tobytes()
    after = np.linalg.norm(fixed_rows[:, :3] - true_rows, axis=1)
    print("corrected rows: worst %.4f m, at the seam %.4f m (before: %.3f m)" % (after.max(), after[at_seam].max(), before[at_seam].max()))
    assert (after <= bound).all()
    assert np.abs(fixed[n - 1] - closed).max() < 1e-12


# ---- (k) the pipeline -------------------------------------------------------------------------------------------------
def _stream():
    from sage_icp_amd import synthetic as syn
    return syn.make_stream(21, 14, points_per_frame=3000, step=(2.5, 0.0, 0.0), max_range=30.0)[0]


def test_the_pipeline_entries(gpu_sage):
    sage = gpu_sage
    frames = _stream()
    cfg = sage.make_pipeline_config(max_range=30.0, local_map_range=30.0, map_update_on_device=True)
    p = sage.SageICP(cfg).set_archive(True)
    late = sage.SageICP(cfg)
    for k, f in enumerate(frames):
        p.RegisterFrame(f)
        late.RegisterFrame(f)
        if k == 2:
            late.set_archive(True)
    poses = p.poses()
    n = len(poses)
    assert p.archive_info()["updates"] == n == len(frames) and p.archive_info()["voxels"] > 0
    h = 0.5 * np.radians(1.5)
    closed = cr.se3_mul(np.array([0.0, 0.0, np.sin(h), np.cos(h), 0.4, -0.3, 0.05]), poses[n - 1])
    corr, fixed, info = p.Closure(2, closed)
    want = sage.closure_corrections(poses, 2, n - 1, closed, return_info=True)
    assert corr.tobytes() == want[0].tobytes() and fixed.tobytes() == want[1].tobytes()
    assert info["delta"].tobytes() == want[2]["delta"].tobytes() and (info["i"], info["j"]) == (2, n - 1)
    assert p.poses().tobytes() == poses.tobytes()                          # the pipeline's own state is not touched
    # the re-posed session against the map entry fed the pipeline's poses
    lib, dp = sage.lib(), ctypes.POINTER(ctypes.c_double)
    handle = lib.sageicp_pipeline_local_map(p._h)
    pos = np.ascontiguousarray(poses[:, 4:])
    for which, name in ((0, "all"), (1, "latest"), (2, "session")):
        k = ctypes.c_uint64(0)
        assert lib.sageicp_map_session_corrected(handle, which, 0, pos.ctypes.data_as(dp), corr.ctypes.data_as(dp), n, None, 0,
                                                 ctypes.byref(k)) == 0
        rows = np.empty((k.value, 4))
        assert lib.sageicp_map_session_corrected(handle, which, 0, pos.ctypes.data_as(dp), corr.ctypes.data_as(dp), n,
                                                 rows.ctypes.data_as(dp), k.value, ctypes.byref(k)) == 0
        got = p.CorrectedSessionMap(corr, which=name)
        assert len(got) == k.value > 0 and got.tobytes() == rows.tobytes()
        on_device = p.CorrectedSessionMap(corr, which=name, device=True)
        assert on_device.cpu().numpy().tobytes() == rows.tobytes()
        assert got.tobytes() != p.SessionMap(which=name).tobytes()
    # the archive switched on late: serial s is not pose s
    assert late.archive_info()["updates"] == n - 3
    for call in (lambda: late.Closure(2, closed), lambda: late.CorrectedSessionMap(corr), lambda: late.CorrectedSessionMap(corr, device=True),
                 lambda: p.CorrectedSessionMap(corr[:-1])):
        with pytest.raises(sage.SageIcpError) as e:
            call()
        assert e.value.code == sage.ERR_INVALID
