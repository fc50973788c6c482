"""The session rebuild on the GPU (include/sageicp.h "session rebuild"): the corrected session voxelised again
into a map, compared as bytes against the restatement (tests/rebuildref.py: closureref's selection, stays and move, then
mapref's sequential add_points and remove_far) and against the only route the library offered before —
CorrectedPointcloud() into host rows, AddPoints into a twin of max_distance = radius, RemovePointsFarFromLocation.

Maps are tiny (voxels of 1 m, a few dozen poses) except the two sheets of one-row voxels that take every strided kernel of
rebuild.hip beyond one trip of its launch.  Coordinates are multiples of 1/64 and the hand-built corrections whole
translations, so those cases are exact by construction; the seeded corrections are not, and need not be: both sides
evaluate the same expressions in the same order."""
import ctypes
import math
import os

import numpy as np
import pytest

import archiveref as ar
import closureref as cr
import rebuildref as rr

pytestmark = pytest.mark.gpu

VS = 1.0
PARAMS = dict(ar.PARAMS, max_distance=5.0)
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
# rebuild.hip's launches: rows of one trip of the move, runs of one trip of the resolve (16 lanes a run), positions of one
# trip of the fill
MOVE_STRIDE, RESOLVE_STRIDE, FILL_STRIDE = 1024 * 256, 2048 * 16, 2048 * 256


def _map(sage, **over):
    p = dict(PARAMS, **over)
    return sage.VoxelHashMap(p["voxel_size"], p["max_distance"], p["basic"], p["critical"], list(p["basic_labels"]))


def _policy(**over):
    p = dict(PARAMS, **over)
    return dict(voxel_size=p["voxel_size"], basic=p["basic"], critical=p["critical"], basic_labels=p["basic_labels"])


def _max_distance(centre, radius, over):
    """of the twin (the contract's) and of a destination the helper creates: the radius where there is a crop"""
    return radius if centre is not None else over.get("max_distance", PARAMS["max_distance"])


def _twin(sage, moved, centre, radius, **over):
    """the existing route, from the corrected export's rows"""
    t = _map(sage, **dict(over, max_distance=_max_distance(centre, radius, over)))
    t.AddPoints(moved)
    if centre is not None:
        t.RemovePointsFarFromLocation(np.asarray(centre, dtype=np.float64))
    return t


def _rebuild_and_check(sage, src, which, pos, corr, centre=None, radius=math.inf, into=None, what="", **over):
    """one rebuild of src, everything the contract says about it asserted; returns (dst, twin, info).  The rebuild is made
    before any export, so it meets src's archive as the scene left it (a pending host tail included)."""
    pos, corr = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(corr, dtype=np.float64).reshape(-1, 7)
    was_resident = src.resident()
    if into is None:
        into = _map(sage, **dict(over, max_distance=_max_distance(centre, radius, over)))
    dst, info = src.RebuildSession(pos, corr, which=which, center=centre, radius=radius, into=into)
    assert dst is into
    assert src.resident() == was_resident, what
    want, want_info = rr.rebuild(src, which, pos, corr, _policy(**over), centre, radius)
    assert info == want_info, (what, info, want_info)
    cloud = dst.Pointcloud()
    assert cloud.tobytes() == want.tobytes(), what
    assert dst.size() == len(want) == info["rows"] and dst.num_voxels() == info["voxels"] and dst.resident(), what
    assert dst.Empty() == (info["voxels"] == 0)
    cap, used, live = dst.table_stats()
    assert used == live == info["voxels"] and (live + 1) * 4 <= cap and cap & (cap - 1) == 0, (what, cap, used, live)
    moved = src.CorrectedPointcloud(which, pos, corr)
    assert len(moved) == info["session_rows"], what
    twin = _twin(sage, moved, centre, radius, **over)
    assert twin.Pointcloud().tobytes() == cloud.tobytes(), what
    assert (twin.size(), twin.num_voxels()) == (dst.size(), dst.num_voxels()), what
    assert dst.point_slots() <= twin.point_slots() or info["voxels"] == 0, what      # each region in its final class
    return dst, twin, info


def _voxel_groups(cloud):
    import recallref
    return {k: np.array(rows).tobytes() for k, rows in recallref.groups(cloud, VS)}


def _seeded_corrections(n, seed):
    """one per pose: a rotation of up to 0.3 rad about a seeded axis, a shift of up to two voxels along each axis"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    h = 0.5 * rng.uniform(-0.3, 0.3, size=n)
    return np.concatenate([axis * np.sin(h)[:, None], np.cos(h)[:, None], rng.uniform(-2.0 * VS, 2.0 * VS, size=(n, 3))], axis=1)


# ---- 1. identity corrections: recall's bytes ------------------------------------------------------------------------------
def test_identity_corrections_give_recalls_bytes(gpu_sage):
    """with identity corrections and SESSION every key of the selection is unique: the rebuild is the recall"""
    from test_recall_gpu import _map as recall_map, _walked_source
    sage = gpu_sage
    src = _walked_source(sage)
    steps = ar.walk()[:9]
    pos = np.array([o for _, o in steps])
    corr = np.tile(IDENTITY, (len(pos), 1))
    session = src.ArchivedPointcloud("session")
    assert not np.signbit(session[:, :3][session[:, :3] == 0.0]).any()       # (no -0.0 coordinate: the move would leave +0.0)
    for centre, radius in (((12.5, 1.0, 0.5), 6.5), ((0.5, 1.0, 0.5), 3.0), ((500.5, 1.0, 0.5), 3.0)):
        recalled, rinfo = src.Recall(centre, radius)
        dst, info = src.RebuildSession(pos, corr, center=centre, radius=radius, into=recall_map(sage, max_distance=radius))
        assert dst.Pointcloud().tobytes() == recalled.Pointcloud().tobytes()
        assert (dst.size(), dst.num_voxels()) == (recalled.size(), recalled.num_voxels())
        assert (info["voxels"], info["rows"], info["session_voxels"], info["session_rows"]) == \
               (rinfo["voxels"], rinfo["rows"], rinfo["session_voxels"], rinfo["session_rows"])
        assert info["built_rows"] == info["session_rows"] and info["built_voxels"] == info["session_voxels"]
    dst, info = src.RebuildSession(pos, corr, into=recall_map(sage))
    fresh = recall_map(sage)
    fresh.AddPoints(session)
    assert dst.Pointcloud().tobytes() == fresh.Pointcloud().tobytes() == session.tobytes()
    assert info["cropped_voxels"] == info["cropped_rows"] == 0 and info["rows"] == len(session)


# ---- 2. the restatement and the host twin -----------------------------------------------------------------------------------
DRIVE_COUNTS = (1, 4, 5, 45, 9, 2, 17, 3)              # 45 offered: the voxel keeps its maximum, 40


def _drive():
    """The out-and-back drive of tests/test_closure_gpu.py: [(rows in the map frame, origin)], out along x to 12, back to 0,
    out again to 8, each pass on its own lateral line (y = 1.0, 1.5, 2.0); every step inserts three voxels at the sensor's
    x, in y = 0, 1, 2.  Coordinates are multiples of 1/64."""
    rng = np.random.default_rng(11)
    xs = list(range(0, 13)) + list(range(11, -1, -1)) + list(range(1, 9))
    lines = [1.0] * 13 + [1.5] * 12 + [2.0] * 8
    steps, k = [], 0
    for x, y in zip(xs, lines):
        parts = []
        for iy in (0, 1, 2):
            parts.append(ar._voxel_points(rng, x, iy, DRIVE_COUNTS[k % len(DRIVE_COUNTS)]))
            k += 1
        steps.append((np.concatenate(parts), (x + 0.5, y, 0.5)))
    return steps


def _source(sage, state):
    """the out-and-back drive of tests/test_closure_gpu.py in one of four states: (map, positions)"""
    steps = _drive()
    pos = [o for _, o in steps]
    if state == "live on the host":
        m = _map(sage, max_distance=100.0)
        for pts, origin in steps:
            m.AddPoints(pts)
    elif state == "live and resident":
        m = _map(sage, max_distance=100.0).set_archive(True)
        for pts, origin in steps:
            ar.apply_step(m, "device", pts, origin)
        assert m.resident() and m.archive_info()["voxels"] == 0
    elif state == "archived":
        m = _map(sage).set_archive(True)
        for pts, origin in steps:
            ar.apply_step(m, "device", pts, origin)
        away = (900.5, 1.0, 0.5)
        ar.apply_step(m, "device", np.zeros((0, 4)), away)
        pos = pos + [away]
        assert m.num_voxels() == 0 and m.archive_info()["voxels"] > 0
    elif state == "pending host tail":
        m = _map(sage).set_archive(True)
        for pts, origin in steps:
            ar.apply_step(m, "update_pose", pts, origin)
        info = m.archive_info()
        assert info["host_rows"] == info["rows"] > 0 and not m.resident() and m.num_voxels() > 0
    else:
        raise ValueError(state)
    return m, np.array(pos)


@pytest.mark.parametrize("state", ["live on the host", "live and resident", "archived", "pending host tail"])
def test_against_the_restatement_and_the_twin(gpu_sage, state):
    sage = gpu_sage
    seen = set()
    for which in ("all", "latest", "session"):
        # (a fresh source for every selection of the pending tail: the first rebuild flushes it)
        src, pos = _source(sage, state)
        corr = _seeded_corrections(len(pos), seed=7)
        centre = tuple(pos[len(pos) // 3])
        for ctr, radius in ((None, math.inf), (centre, 6.0)):
            what = "%s %s %r" % (state, which, ctr)
            dst, _, info = _rebuild_and_check(sage, src, which, pos, corr, ctr, radius, what=what)
            if state == "pending host tail":
                after = src.archive_info()
                assert after["host_rows"] == 0 and after["device_rows"] == after["rows"]          # flushed, as by an export
            if info["session_rows"] == 0:
                seen.add("empty selection")
                continue
            if info["built_rows"] < info["session_rows"]:
                seen.add("turned away")
            if 0 < info["voxels"] < info["built_voxels"]:
                seen.add("cropped")
            # rows of one source voxel in several destination voxels, rows of several source voxels in one
            rows, counts, updates = cr.session_voxels(src, which, VS)
            stay = cr.stays(cr.first_rows(rows, counts), updates, pos, src.max_distance_)
            moved = cr.move(rows, counts, stay, corr)
            keys = [tuple(k) for k in np.trunc(moved[:, :3] / VS).astype(np.int64).tolist()]
            sources, at = {}, 0
            for j, c in enumerate(counts):
                if len(set(keys[at:at + c])) > 1:
                    seen.add("scattered")
                for k in keys[at:at + c]:
                    sources.setdefault(k, set()).add(j)
                at += c
            if max(len(v) for v in sources.values()) > 1:
                seen.add("merged")
            if len({stay[j] for v in sources.values() for j in v if len(v) > 1}) > 1:
                seen.add("passes merged")
    print(state, sorted(seen))
    want = {"merged", "passes merged", "cropped", "scattered"}
    if state.startswith("live"):
        want.add("empty selection")       # "all" and "latest" of a source without an archive
    assert want <= seen, (state, seen)


def test_all_merges_the_generations_of_one_key(gpu_sage):
    """identity corrections, SAGEICP_ARCHIVE_ALL: every generation of a key lands in the key's one destination voxel"""
    sage = gpu_sage
    src, pos = _source(sage, "archived")
    corr = np.tile(IDENTITY, (len(pos), 1))
    rec = src.archive_voxels()
    keys = [(int(r.x), int(r.y), int(r.z)) for r in rec]
    assert max(keys.count(k) for k in set(keys)) >= 2
    dst, _, info = _rebuild_and_check(sage, src, "all", pos, corr, what="all")
    assert info["session_voxels"] == len(keys) and info["built_voxels"] == len(set(keys)) < len(keys)
    latest, _, linfo = _rebuild_and_check(sage, src, "latest", pos, corr, what="latest")
    assert linfo["built_voxels"] == linfo["session_voxels"] == len(set(keys))


# ---- 3. merges that decide --------------------------------------------------------------------------------------------------
FAR = 1000.0                 # a max_distance under which nothing is far: a live voxel's stay is its nearest pose
STRIDE_X = 10                # source voxels of pose i stand at x = 10 i; correction i takes them back to x = 0


def _poses_and_corrections(n):
    pos = np.array([(STRIDE_X * i + 0.5, 0.5, 0.5) for i in range(n)])
    corr = np.array([IDENTITY[:4] + (-float(STRIDE_X * i), 0.0, 0.0) for i in range(n)])
    return pos, corr


def _offered(rng, ix, iy, count, labels=(0.0, 44.0, 71.0, 72.0)):
    """`count` <= 40 rows of one source voxel that the policy (20, 20) keeps all of: the first 20 of any label, the rest critical"""
    p = ar._voxel_points(rng, ix, iy, count)
    p[:min(count, 20), 3] = rng.choice(labels, size=min(count, 20))
    return p


def _merged_runs_source(sage, lengths, seed):
    """for every length L a destination voxel (0, 2 r, 0) whose run of L arrivals comes from source voxels of 40 rows (the
    last one the rest) at x = 10 i, one per pose"""
    rng = np.random.default_rng(seed)
    parts = []
    for r, L in enumerate(lengths):
        left, i = L, 0
        while left > 0:
            parts.append(_offered(rng, STRIDE_X * i, 2 * r, min(left, 40)))
            left -= min(left, 40)
            i += 1
    src = _map(sage, max_distance=FAR)
    rows = np.concatenate(parts)
    src.AddPoints(rows)
    assert src.size() == len(rows) == sum(lengths)           # the source kept every offered row
    return src


def test_runs_around_a_group_a_wave_and_a_workgroup(gpu_sage):
    """runs of 15 .. 17, 63 .. 65, 255 .. 257 and 320 arrivals, each merged from up to eight source voxels of eight stays
    by pure translations: one run beyond a wave, beyond one workgroup's 256 positions"""
    sage = gpu_sage
    lengths = [15, 16, 17, 63, 64, 65, 255, 256, 257, 320]
    src = _merged_runs_source(sage, lengths, seed=23)
    pos, corr = _poses_and_corrections(8)
    assert src.SessionStays(pos).tolist() == [i for L in lengths for i in range((L + 39) // 40)]
    dst, _, info = _rebuild_and_check(sage, src, "session", pos, corr, what="runs", max_distance=FAR)
    assert info["built_voxels"] == len(lengths) and info["session_rows"] == sum(lengths)
    groups = {k: np.array(v) for k, v in __import__("recallref").groups(dst.Pointcloud(), VS)}
    assert sorted(groups) == [(0, 2 * r, 0) for r in range(len(lengths))]
    assert len(groups[(0, 18, 0)]) == 40 and len(groups[(0, 0, 0)]) == 15
    # the test decides: in the longest run unlabelled first rows were replaced by rows of later stays
    run320 = groups[(0, 18, 0)]
    offered320 = src.CorrectedPointcloud("session", pos, corr)[-320:]
    assert (offered320[:20, 3] == 0.0).any() and (run320[:20, 3] != 0.0).all()
    assert run320[20:].tobytes() == offered320[20:40].tobytes()


def test_size_classes_of_merged_counts(gpu_sage):
    """merged counts on both sides of every size class's edge, each from two source voxels of two stays"""
    sage = gpu_sage
    counts = [1, 4, 5, 8, 9, 16, 17, 40]
    rng = np.random.default_rng(31)
    parts = []
    for r, c in enumerate(counts):
        a = (c + 1) // 2
        parts.append(ar._voxel_points(rng, 0, 2 * r, a))
        if c - a:
            parts.append(ar._voxel_points(rng, STRIDE_X, 2 * r, c - a))
    src = _map(sage, max_distance=FAR)
    src.AddPoints(np.concatenate(parts))
    pos, corr = _poses_and_corrections(2)
    dst, twin, info = _rebuild_and_check(sage, src, "session", pos, corr, what="classes", max_distance=FAR)
    got = [len(v) for _, v in __import__("recallref").groups(dst.Pointcloud(), VS)]
    assert got == counts and info["built_voxels"] == len(counts) and info["session_voxels"] == 2 * len(counts) - 1
    if os.environ.get("SAGEICP_SIZE_CLASSES", "1") != "0":
        assert dst.point_slots() == 4 + 4 + 8 + 8 + 16 + 16 + 40 + 40        # each region in the class of its final count


P32 = dict(basic=3, critical=2)
# source voxel A (pose 0, at x = 0): an unlabelled first row and two critical ones; source voxel B (pose 1, at x = 10): a row
# of a basic-part label.  Merged at policy (3, 2): slot 0 is unlabelled, B's row is the first replacer and takes it.
A_ROWS = [(0.25, 0.5, 0.5, 0.0), (0.5, 0.5, 0.5, 71.0), (0.5, 0.25, 0.5, 71.0)]
B_ROW = (10.75, 0.5, 0.5, 44.0)


@pytest.mark.parametrize("centre, radius, kept", [
    ((0.0, 0.5, 0.5), 0.5, False),        # the original first row 0.25 away, inside; the replacer 0.75 away, outside: dropped
    ((1.0, 0.5, 0.5), 0.5, True),         # the other way round: kept
    ((0.0, 0.5, 0.5), 0.75, True),        # the replacer exactly on the radius: kept
    ((0.0, 0.5, 0.5), float(np.nextafter(0.75, 0.0)), False),
])
def test_the_crop_is_decided_by_the_final_first_row(gpu_sage, centre, radius, kept):
    sage = gpu_sage
    src = _map(sage, max_distance=FAR, **P32)
    src.AddPoints(np.array(A_ROWS + [B_ROW]))
    assert src.num_voxels() == 2
    pos, corr = _poses_and_corrections(2)
    dst, _, info = _rebuild_and_check(sage, src, "session", pos, corr, centre, radius, what="crop", max_distance=FAR, **P32)
    moved_b = (0.75, 0.5, 0.5, 44.0)
    assert info["built_voxels"] == 1 and info["built_rows"] == 3 and info["voxels"] == (1 if kept else 0)
    if kept:
        assert dst.Pointcloud().tobytes() == np.array([moved_b] + A_ROWS[1:]).tobytes()
    else:
        assert dst.Empty() and info["cropped_rows"] == 3


# ---- 4. beyond one stride of every strided launch --------------------------------------------------------------------------
SHEET_SIDE = 726             # 527 076 one-row voxels: beyond one trip of the move, of the resolve and of the fill
SHEET_ORIGIN, SHEET_AWAY = (363.0, 363.0, 0.5), (9000.0, 363.0, 0.5)
SHEET_SHIFT = (2.0, 3.0, 1.0)          # (away from zero: truncation merges the voxels on either side of it)


def _one_row_sheet():
    rng = np.random.default_rng(41)
    ix, iy = (a.reshape(-1) for a in np.meshgrid(np.arange(SHEET_SIDE), np.arange(SHEET_SIDE), indexing="ij"))
    n = len(ix)
    p = np.empty((n, 4))
    p[:, 0] = ix + rng.integers(4, 60, size=n) / 64.0
    p[:, 1] = iy + rng.integers(4, 60, size=n) / 64.0
    p[:, 2] = rng.integers(4, 60, size=n) / 64.0
    p[:, 3] = rng.choice([0.0, 44.0, 71.0], size=n)
    return p[rng.permutation(n)]


@pytest.mark.parametrize("part", ["archive", "live"])
def test_a_part_beyond_one_stride(gpu_sage, part):
    """one-row voxels, one pose, one whole translation: every key stays unique, so the rebuilt map is the shifted session
    in session order — known without the sequential restatement"""
    sage = gpu_sage
    rows = _one_row_sheet()
    assert len(rows) > max(MOVE_STRIDE, RESOLVE_STRIDE, FILL_STRIDE)
    src = _map(sage, max_distance=600.0).set_archive(True)
    src.UpdateOnDevice(ar.sensor_rows(rows, SHEET_ORIGIN), ar.pose_of(SHEET_ORIGIN))
    pos = [SHEET_ORIGIN]
    if part == "archive":
        src.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of(SHEET_AWAY))
        pos.append(SHEET_AWAY)
        assert src.num_voxels() == 0 and src.archive_info()["rows"] == len(rows)
    else:
        assert src.num_voxels() == len(rows) and src.archive_info()["rows"] == 0
    corr = np.tile(IDENTITY[:4] + SHEET_SHIFT, (len(pos), 1))
    dst, info = src.RebuildSession(np.array(pos), corr, into=_map(sage, max_distance=600.0))
    session = src.ArchivedPointcloud("session")
    want = session.copy()
    want[:, :3] += np.array(SHEET_SHIFT)
    assert info == dict(voxels=len(rows), rows=len(rows), session_voxels=len(rows), session_rows=len(rows), built_voxels=len(rows),
                        built_rows=len(rows), cropped_voxels=0, cropped_rows=0)
    assert dst.Pointcloud().tobytes() == want.tobytes()
    assert want.tobytes() == src.CorrectedPointcloud("session", np.array(pos), corr).tobytes()
    cap, used, live = dst.table_stats()
    assert used == live == len(rows)


# ---- 5. determinism and lifecycle ----------------------------------------------------------------------------------------
def test_the_same_rebuild_twice_gives_the_same_bytes(gpu_sage):
    sage = gpu_sage
    src, pos = _source(sage, "archived")
    corr = _seeded_corrections(len(pos), seed=9)
    centre = tuple(pos[5])
    a, ia = src.RebuildSession(pos, corr, which="all", center=centre, radius=7.0)
    b, ib = src.RebuildSession(pos, corr, which="all", center=centre, radius=7.0)
    c, ic = src.RebuildSession(pos, corr, which="all", center=centre, radius=7.0, into=a)
    assert c is a and ia == ib == ic and 0 < ia["voxels"] < ia["built_voxels"] and ia["built_rows"] < ia["session_rows"]
    assert a.Pointcloud().tobytes() == b.Pointcloud().tobytes()
    assert (a.size(), a.num_voxels(), a.point_slots(), a.table_stats()) == (b.size(), b.num_voxels(), b.point_slots(), b.table_stats())


def test_a_second_rebuild_replaces_the_first_and_the_destinations_archive_is_its_own(gpu_sage):
    sage = gpu_sage
    src, pos = _source(sage, "archived")
    corr = _seeded_corrections(len(pos), seed=9)
    dst = _map(sage, max_distance=3.0).set_archive(True)
    dst.UpdateOnDevice(ar.walk()[0][0], ar.pose_of((0.0, 0.0, 0.0)))
    dst.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of((900.0, 0.0, 0.0)))      # its own log: every voxel of that frame
    own, own_rows = dst.archive_info(), dst.ArchivedPointcloud("all")
    assert own["voxels"] > 0 and dst.num_voxels() == 0
    _rebuild_and_check(sage, src, "session", pos, corr, tuple(pos[3]), 5.0, into=dst)
    first = dst.Pointcloud()
    assert dst.archive_info() == own and dst.ArchivedPointcloud("all").tobytes() == own_rows.tobytes()    # nothing logged
    assert dst.max_distance_ == 3.0
    _rebuild_and_check(sage, src, "latest", pos, corr, into=dst)
    assert dst.Pointcloud().tobytes() != first.tobytes() and dst.archive_info() == own
    # ... and from now on it logs what it evicts, like any map (its own max_distance, 3, is what evicts)
    held = dst.Pointcloud()
    dst.UpdateOnDevice(np.zeros((0, 4)), ar.pose_of((900.0, 0.0, 0.0)))
    now = dst.archive_info()
    assert dst.num_voxels() == 0 and now["rows"] == own["rows"] + len(held) and now["updates"] == own["updates"] + 1
    assert dst.ArchivedPointcloud("all")[own["rows"]:].tobytes() == held.tobytes()


def _frame(rng, x0, n=400):
    p = np.empty((n, 4))
    p[:, 0] = x0 + rng.integers(0, 6 * 64, size=n) / 64.0
    p[:, 1] = rng.integers(0, 5 * 64, size=n) / 64.0
    p[:, 2] = rng.integers(4, 60, size=n) / 64.0
    p[:, 3] = rng.choice([71.0, 40.0, 0.0], size=n)
    return p


def test_updates_after_a_rebuild(gpu_sage):
    """without a crop the twin holds the same blocks, so every later update hands out the same ones: Pointcloud() stays
    equal byte for byte through an update on the device (which evicts), the download and an insertion on the host; after a
    crop the twin's evicted blocks are free and handed out first (recall's caveat): every voxel's rows and the counters"""
    sage = gpu_sage
    src, pos = _source(sage, "archived")
    corr = _seeded_corrections(len(pos), seed=9)
    rng = np.random.default_rng(6)
    frame, more = _frame(rng, 3.0), _frame(rng, 6.0)
    for centre, radius in ((None, math.inf), (tuple(pos[4]), 6.0)):
        dst, twin, info = _rebuild_and_check(sage, src, "session", pos, corr, centre, radius)
        same = (lambda a, b: a.tobytes() == b.tobytes()) if centre is None else (lambda a, b: _voxel_groups(a) == _voxel_groups(b))
        assert info["voxels"] > 20
        for m in (dst, twin):
            m.UpdateOnDevice(ar.sensor_rows(frame, (5.5, 1.0, 0.5)), ar.pose_of((5.5, 1.0, 0.5)))
        assert dst.resident() and same(dst.Pointcloud(), twin.Pointcloud())
        assert (dst.size(), dst.num_voxels()) == (twin.size(), twin.num_voxels())
        for m in (dst, twin):
            m.Update(more, np.array((8.5, 1.0, 0.5)))
        assert not dst.resident() and same(dst.Pointcloud(), twin.Pointcloud())
        assert (dst.size(), dst.num_voxels()) == (twin.size(), twin.num_voxels())
        got, want = dst.GetCorrespondences(frame, 1.0, 0.5), twin.GetCorrespondences(frame, 1.0, 0.5)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and len(got[0]) > 50


def test_an_empty_selection_gives_an_empty_usable_map(gpu_sage):
    sage = gpu_sage
    pos, corr = np.array([(0.5, 1.0, 0.5)]), np.array([IDENTITY])
    zero = dict.fromkeys(rr.INFO_FIELDS, 0)
    dst = _map(sage)
    dst.AddPoints(ar.walk()[0][0])
    for src, which in ((_map(sage), "session"), (_map(sage).set_archive(True), "latest")):
        out, info = src.RebuildSession(pos, corr, which=which, into=dst)
        assert out is dst and info == zero and dst.Empty() and dst.resident() and dst.size() == 0
    fresh = _map(sage)
    pts, origin = ar.walk()[0]
    for m in (dst, fresh):
        ar.apply_step(m, "device", pts, origin)
    assert dst.Pointcloud().tobytes() == fresh.Pointcloud().tobytes() and dst.size() > 0


# ---- 6. refusals found on the device -------------------------------------------------------------------------------------
def test_refusals_found_by_the_keying_kernel(gpu_sage):
    sage = gpu_sage
    src = _map(sage, max_distance=FAR)
    src.AddPoints(np.concatenate([ar._voxel_points(np.random.default_rng(1), 0, 0, 5), ar._voxel_points(np.random.default_rng(2), STRIDE_X, 0, 1)]))
    pos, good = _poses_and_corrections(2)
    dst = _map(sage, max_distance=FAR)
    dst.AddPoints(ar.walk()[0][0])
    beyond = good.copy()
    beyond[1, 4] = float(1 << 20)                      # pose 1's one row: voxel index 2^20 + 10
    overflow = good.copy()
    overflow[1, :4] = (1e155, 0.0, 0.0, 0.0)           # finite, but quat_to_mat squares it
    for corr, code in ((beyond, sage.ERR_CAPACITY), (overflow, sage.ERR_INVALID)):
        with pytest.raises(sage.SageIcpError) as e:
            src.RebuildSession(pos, corr, into=dst)
        assert e.value.code == code, str(e.value)
        assert dst.Empty() and dst.size() == 0 and dst.num_voxels() == 0
        # cleared, and it accepts the next call
        _rebuild_and_check(sage, src, "session", pos, good, into=dst, what="after a refusal", max_distance=FAR)
        assert dst.num_voxels() == 1 and dst.size() == 6
    # one row short of the limit is a voxel like any other
    edge = good.copy()
    edge[1, 4] = float((1 << 20) - 1 - STRIDE_X)
    _rebuild_and_check(sage, src, "session", pos, edge, into=dst, what="at the limit", max_distance=FAR)
    assert dst.num_voxels() == 2


# ---- 7. end to end: two laps of a street -----------------------------------------------------------------------------------
def test_two_laps_of_a_street_rebuilt_into_one_map(gpu_sage):
    """the scene of test_posegraph_gpu.test_two_laps_of_a_street_put_back_together: 81 poses, 160-point scans, a window of
    4 m; the session rebuilt under the graph's corrections merges the two laps, and a scan of lap two registers against
    it exactly as against the host twin"""
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    import graphscenes as gs
    DRIFT, SIDE, RADIUS = 0.05, 10, 4.0
    u = np.array([0.6, 0.8, 0.0])
    corners = [(0.0, 0.0), (SIDE, 0.0), (SIDE, SIDE), (0.0, SIDE), (0.0, 0.0)]
    lap = [np.array([x0 + (x1 - x0) * k / SIDE, y0 + (y1 - y0) * k / SIDE, 0.0])
           for (x0, y0), (x1, y1) in zip(corners[:-1], corners[1:]) for k in range(1, SIDE + 1)]
    true_t = np.array([np.zeros(3)] + lap + lap) + np.array([8.0, 3.0, 0.0])
    n = len(true_t)
    assert n == 81
    path = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(true_t, axis=0), axis=1))])
    drift_t = np.round((true_t + DRIFT * path[:, None] * u) * 1024.0) / 1024.0
    rot = [0.0, 0.0, 0.0, 1.0]
    poses = np.concatenate([np.tile(rot, (n, 1)), drift_t], axis=1)
    truth = np.concatenate([np.tile(rot, (n, 1)), true_t], axis=1)
    rng = np.random.default_rng(2025)
    m = sage.VoxelHashMap(1.0, RADIUS, 20, 20, [40, 44, 48]).set_archive(True)
    scans = []
    for k in range(n):
        scans.append(syn.make_scan(rng, 160, 40.0, truth[k], max_range=3.5, min_range=0.5, label_max_range=50.0))
        m.UpdateOnDevice(scans[-1], poses[k])
    s = dict(poses=poses, truth=truth, odom_info=gs.ODOM_INFO,
             closures=[(a, b, gs.rel(truth, a, b), 4.0 * gs.ODOM_INFO) for a, b in ((0, 4 * SIDE), (0, 8 * SIDE), (SIDE, 5 * SIDE))])
    corr, out, _ = gs.optimize(sage, s, where="device")
    dst, info = m.RebuildSession(drift_t, corr)
    export = m.CorrectedPointcloud("session", drift_t, corr)
    print("the corrected export: %d rows in %d voxels; rebuilt: %r" % (len(export), info["session_voxels"], info))
    assert info["session_rows"] == len(export)
    assert info["rows"] < len(export) and dst.num_voxels() == info["voxels"] < info["session_voxels"]       # the laps were merged
    have = {r.tobytes() for r in export}
    cloud = dst.Pointcloud()
    assert all(r.tobytes() in have for r in cloud)
    twin = sage.VoxelHashMap(1.0, RADIUS, 20, 20, [40, 44, 48])
    twin.AddPoints(export)
    assert twin.Pointcloud().tobytes() == cloud.tobytes()
    # a scan of lap two, registered from a prior 0.3 m off its corrected pose
    k = 6 * SIDE + 3
    prior = out[k].copy()
    prior[4:] += np.array([0.18, -0.24, 0.0])
    got = sage.register_frame(scans[k], dst, prior, 1.0, 0.5, 0.5, return_stats=True)
    want = sage.register_frame(scans[k], twin, prior, 1.0, 0.5, 0.5, return_stats=True)
    assert got[0].tobytes() == want[0].tobytes()
    for f in ("iterations", "converged", "n_queries", "n_corr_first", "n_corr_last", "last_step_norm"):
        assert getattr(got[1], f) == getattr(want[1], f), f
    assert list(got[1].n_corr_hist) == list(want[1].n_corr_hist)
    print("registered %d iterations, %d correspondences; %.3f m from the truth (the prior: %.3f m)"
          % (got[1].iterations, got[1].n_corr_last, np.linalg.norm(got[0][4:] - true_t[k]), np.linalg.norm(prior[4:] - true_t[k])))


# ---- 8. the pipeline's entry -------------------------------------------------------------------------------------------------
def test_the_pipeline_entry(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    frames = syn.make_stream(21, 14, points_per_frame=3000, step=(2.5, 0.0, 0.0), max_range=30.0)[0]
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
    h = 0.5 * np.radians(1.5)
    closed = cr.se3_mul(np.array([0.0, 0.0, np.sin(h), np.cos(h), 0.4, -0.3, 0.05]), poses[n - 1])
    corr, _, _ = p.Closure(2, closed)
    lib, dp = sage.lib(), ctypes.POINTER(ctypes.c_double)
    handle = lib.sageicp_pipeline_local_map(p._h)
    pos = np.ascontiguousarray(poses[:, 4:])
    c = p.config
    labels = [c.basic_parts_labels[i] for i in range(c.n_basic_parts_labels)]
    centre = np.ascontiguousarray(pos[n // 2])
    for which, name in ((0, "all"), (1, "latest"), (2, "session")):
        for ctr, radius in ((None, math.inf), (centre, 12.0)):
            by_map = sage.VoxelHashMap(c.voxel_size_map, c.local_map_range, c.basic_points_per_voxel, c.critical_points_per_voxel, labels)
            minfo = sage.RebuildInfo()
            assert lib.sageicp_map_session_rebuild(handle, which, pos.ctypes.data_as(dp), corr.ctypes.data_as(dp), n,
                                                   None if ctr is None else ctr.ctypes.data_as(dp), radius, by_map._h,
                                                   ctypes.byref(minfo)) == 0
            got, info = p.RebuildSessionMap(corr, which=name, center=ctr, radius=radius)
            assert info == minfo.as_dict() and info["built_rows"] > 0 and got.resident()
            assert got.Pointcloud().tobytes() == by_map.Pointcloud().tobytes()
            if ctr is None:
                assert info["rows"] == info["built_rows"] and info["cropped_voxels"] == 0
            elif name == "session":           # (what the archive alone holds lies 30 m behind: all of it is cropped)
                assert 0 < info["voxels"] < info["built_voxels"]
    assert p.poses().tobytes() == poses.tobytes()                          # the pipeline's own state is not touched
    # the archive switched on late: serial s is not pose s
    for call in (lambda: late.RebuildSessionMap(corr), lambda: p.RebuildSessionMap(corr[:-1])):
        with pytest.raises(sage.SageIcpError) as e:
            call()
        assert e.value.code == sage.ERR_INVALID
