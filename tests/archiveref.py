"""Plain Python restatement of a map's archive (include/sageicp.h "the archive of a map"), for the tests only.

ArchiveRef is tests/mapref.py's MapRef whose remove_far logs what it evicts — key, rows, serial — under the rules the
header states: calls in the order they were made, voxels in ascending block index (the order MapRef frees them), rows in
their stored order; a voxel is archived only while all its rows still fit under max_rows, the first that does not makes the
archive full for good and everything after it is only counted.  latest() and session() are the two selections written
from their definitions.  The walk below is the scene both test files drive through the library's entries."""
import numpy as np

import mapref

VOXEL_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("count", "<u4"), ("first_row", "<u8"), ("update", "<u8")])


class ArchiveRef(mapref.MapRef):
    def __init__(self, *a, max_rows=0, **kw):
        super().__init__(*a, **kw)
        self.max_rows = int(max_rows)
        self.archive_clear()

    def archive_clear(self):
        self.log = []               # (key, rows, serial) per archived voxel
        self.full = False
        self.dropped_rows = self.dropped_voxels = 0
        self.updates = 0
        self.evicted_by_call = []   # voxels each eviction-capable call evicted (archived or not)

    def rows_held(self):
        return sum(len(r) for _, r, _ in self.log)

    def remove_far(self, origin):
        live_before = [(b, self.keys[b], list(blk)) for b, blk in enumerate(self.blocks) if blk is not None]
        super().remove_far(origin)
        n = 0
        for b, key, rows in live_before:        # ascending block index
            if self.blocks[b] is not None and self.index.get(key) == b:
                continue
            n += 1
            if self.full or (self.max_rows and self.rows_held() + len(rows) > self.max_rows):
                self.full = True
                self.dropped_rows += len(rows)
                self.dropped_voxels += 1
                continue
            self.log.append((key, rows, self.updates))
        self.evicted_by_call.append(n)
        self.updates += 1

    def info(self):
        return {"full": int(self.full), "rows": self.rows_held(), "voxels": len(self.log), "dropped_rows": self.dropped_rows,
                "dropped_voxels": self.dropped_voxels, "max_rows": self.max_rows, "updates": self.updates}


def rows_of(log):
    return np.array([p for _, rows, _ in log for p in rows], dtype=np.float64).reshape(-1, 4)


def records_of(log):
    out = np.zeros(len(log), dtype=VOXEL_DTYPE)
    at = 0
    for i, (key, rows, serial) in enumerate(log):
        out[i] = (key[0], key[1], key[2], len(rows), at, serial)
        at += len(rows)
    return out


def limited(log, max_rows):
    """the prefix rule: the longest prefix of whole voxels that fits max_rows (0: all of it)"""
    if not max_rows:
        return list(log)
    out, held = [], 0
    for e in log:
        if held + len(e[1]) > max_rows:
            break
        out.append(e)
        held += len(e[1])
    return out


def latest(log, live_keys):
    """record i is kept iff no later record has the same key and the live map holds no voxel with that key; log order"""
    live = set(map(tuple, live_keys))
    return [e for i, e in enumerate(log) if tuple(e[0]) not in live and all(tuple(l[0]) != tuple(e[0]) for l in log[i + 1:])]


def session(log, live_keys, pointcloud):
    """the LATEST rows followed by the map's rows in Pointcloud()'s order"""
    return np.concatenate([rows_of(latest(log, live_keys)), np.asarray(pointcloud, dtype=np.float64).reshape(-1, 4)])


def keys_of(cloud, voxel_size):
    c = np.asarray(cloud).reshape(-1, 4)
    return [tuple(int(v / voxel_size) for v in p[:3]) for p in c.tolist()]


def evicted_groups(before, after, voxel_size):
    """For reference-order mode, from the oracle alone: the voxels of `before` (Pointcloud() after add_points) that are
    absent from `after` (Pointcloud() after remove_far), in the order of `before`, as (key, rows).  The sweep erases in
    iteration order, and a backward shift keeps the relative order of what is still to be visited."""
    kb = keys_of(before, voxel_size)
    gone = set(kb) - set(keys_of(after, voxel_size))
    out = []
    for k, p in zip(kb, np.asarray(before).reshape(-1, 4).tolist()):
        if k not in gone:
            continue
        if out and out[-1][0] == k:
            out[-1][1].append(tuple(p))
        else:
            out.append((k, [tuple(p)]))
    return out


# ---- the walk ---------------------------------------------------------------------------------------------------------
# A sensor along x over voxels of 1.0 m, max_distance 3.0, basic = critical = 20 (cap 40: the size classes 4 / 8 / 16 /
# 40).  Every coordinate is a multiple of 1/64, so the pose transform (rows given in the sensor frame, translation added
# back) is exact and all entries see the same rows.  Label 71 is a critical one: a voxel fills to 40.
PARAMS = dict(voxel_size=1.0, max_distance=3.0, basic=20, critical=20, basic_labels=(40, 44, 48))
COUNTS = (1, 4, 5, 8, 9, 16, 17, 40, 45, 2, 3, 20, 21)


def _voxel_points(rng, ix, iy, n, label=71.0):
    p = np.empty((n, 4))
    p[:, 0] = ix + rng.integers(4, 60, size=n) / 64.0
    p[:, 1] = iy + rng.integers(4, 60, size=n) / 64.0
    p[:, 2] = rng.integers(4, 60, size=n) / 64.0
    p[:, 3] = label
    return p


def walk(seed=3):
    """[(rows in the map frame, origin)]: steps of 2 m with six new voxels each (counts cycling through COUNTS), a step
    with no rows, a jump far away with no rows (every voxel goes), a return to the start (keys archived before are live
    again, then leave again: a second generation), two steps that stand still (nothing goes)"""
    rng = np.random.default_rng(seed)
    steps, k = [], 0

    def frame(cx):
        nonlocal k
        parts = []
        for dx in (0, 1):
            for dy in (0, 1, 2):
                parts.append(_voxel_points(rng, cx + dx, dy, COUNTS[k % len(COUNTS)]))
                k += 1
        pts = np.concatenate(parts)
        return pts[rng.permutation(len(pts))]

    for f in range(7):
        steps.append((frame(2 * f), (2.0 * f + 0.5, 1.0, 0.5)))
    steps.append((np.zeros((0, 4)), (15.5, 1.0, 0.5)))              # n == 0, evicts
    steps.append((frame(16), (16.5, 1.0, 0.5)))
    steps.append((frame(16)[:5], (16.5, 1.0, 0.5)))                 # stands still: nothing goes
    steps.append((np.zeros((0, 4)), (500.5, 1.0, 0.5)))             # every voxel of the map
    for f in (0, 1, 2, 3):                                          # back at the start: the same keys again
        steps.append((frame(2 * f), (2.0 * f + 0.5, 1.0, 0.5)))
    steps.append((_voxel_points(rng, 9, 1, 1), (9.75, 1.0, 0.5)))
    steps.append((_voxel_points(rng, 13, 1, 3), (9.75, 1.0, 0.5)))  # a voxel born out of range: exactly one goes
    return steps


# ---- a sheet beyond one stride of the row gathers ---------------------------------------------------------------------------
# archive.hip's gathers and recall.hip's fill launch at most 2048 workgroups of 256 lanes, a lane per row, and stride
# over what lies beyond.  116 x 116 voxels of 40 rows are 538,240 rows: 13,952 of them are written on a second trip.
GATHER_STRIDE = 2048 * 256
BIG_SIDE, BIG_COUNT, BIG_AGAIN = 116, 40, 300
BIG_MAX_DISTANCE = 100.0                                            # holds the sheet from BIG_ORIGIN (its corners: 82 m)
BIG_ORIGIN, BIG_AWAY = (58.0, 58.0, 0.5), (5000.0, 58.0, 0.5)


def big_sheet(seed=17):
    """(rows, again): BIG_SIDE^2 voxels of 1 m, each offered BIG_COUNT rows of label 71 (a critical one: all 40 are kept,
    in the order offered) at multiples of 1/64, shuffled; and BIG_COUNT other rows for BIG_AGAIN of the voxels, spread
    over the sheet, shuffled"""
    rng = np.random.default_rng(seed)

    def rows_of_voxels(ix, iy):
        n = len(ix) * BIG_COUNT
        p = np.empty((n, 4))
        p[:, 0] = np.repeat(ix, BIG_COUNT) + rng.integers(4, 60, size=n) / 64.0
        p[:, 1] = np.repeat(iy, BIG_COUNT) + rng.integers(4, 60, size=n) / 64.0
        p[:, 2] = rng.integers(4, 60, size=n) / 64.0
        p[:, 3] = 71.0
        return p[rng.permutation(n)]

    ix, iy = (a.reshape(-1) for a in np.meshgrid(np.arange(BIG_SIDE), np.arange(BIG_SIDE), indexing="ij"))
    rows = rows_of_voxels(ix, iy)
    pick = np.sort(rng.choice(BIG_SIDE * BIG_SIDE, size=BIG_AGAIN, replace=False))
    return rows, rows_of_voxels(ix[pick], iy[pick])


def big_sheet_steps():
    """the sheet inserted and evicted whole by one empty update far away, then BIG_AGAIN of its voxels born again with
    other rows and evicted again: a second generation, so LATEST is not the log"""
    rows, again = big_sheet()
    none = np.zeros((0, 4))
    return [(rows, BIG_ORIGIN), (none, BIG_AWAY), (again, BIG_ORIGIN), (none, BIG_AWAY)]


def by_voxel(rows, voxel_size=1.0):
    """the rows in ascending voxel key, each voxel's rows in the order they had (a stable sort)"""
    k = np.trunc(np.asarray(rows)[:, :3] / voxel_size).astype(np.int64)
    return rows[np.lexsort((k[:, 2], k[:, 1], k[:, 0]))]


IDENTITY_ROT = (0.0, 0.0, 0.0, 1.0)


def pose_of(origin):
    return np.array(IDENTITY_ROT + tuple(origin), dtype=np.float64)


def sensor_rows(pts, origin):
    q = np.array(pts, dtype=np.float64).reshape(-1, 4)
    q[:, :3] -= np.asarray(origin, dtype=np.float64)
    return q


def apply_step(m, entry, pts, origin):
    """one step through a library entry: "remove_far" (AddPoints + RemovePointsFarFromLocation), "update" (origin),
    "update_pose" (host), "device" (sageicp_map_update_pose_device)"""
    if entry == "remove_far":
        m.AddPoints(pts)
        m.RemovePointsFarFromLocation(origin)
    elif entry == "update":
        m.Update(pts, np.asarray(origin, dtype=np.float64))
    elif entry == "update_pose":
        m.Update(sensor_rows(pts, origin), pose_of(origin))
    elif entry == "device":
        m.UpdateOnDevice(sensor_rows(pts, origin), pose_of(origin))
    else:
        raise ValueError(entry)


def ref_step(ref, pts, origin):
    ref.update(sensor_rows(pts, origin), pose_of(origin))


def assert_equal_to_ref(m, ref, what=""):
    """info, records and the ALL rows of a library map against the restatement, on bytes"""
    info = m.archive_info()
    want = ref.info()
    got = {k: info[k] for k in want}
    assert got == want, "%s: info %r, the restatement %r" % (what, got, want)
    assert info["device_rows"] + info["host_rows"] == info["rows"]
    rec = m.archive_voxels()
    assert np.asarray(rec).tobytes() == records_of(ref.log).tobytes(), "%s: the records differ" % what
    rows = m.ArchivedPointcloud("all")
    assert rows.tobytes() == rows_of(ref.log).tobytes(), "%s: the rows differ" % what
