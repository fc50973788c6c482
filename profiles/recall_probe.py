"""What recall costs on the MI355X beside the only other route to the same map (results: profiles/r37/README.md).

  python profiles/recall_probe.py route [REPS]   a session of ~10 M archived rows (the log of archive_probe.py's exports: ten
                                                 grounds of a million points, every second one over the same ground), a radius
                                                 that holds ~2 M rows; in turns (the call after a route timed apart):
                                                   recall   Recall(centre, radius, into=dst), dst reused
                                                   route    the SESSION rows exported, inserted into a cleared twin of
                                                            max_distance = radius and swept in one device-side update at the
                                                            centre (insert + remove_far in one pass: the cheapest complete
                                                            form), the twin's buffers reused; its pieces timed one by one,
                                                            the export into device rows beside them
                                                 and the two maps compared on bytes
  python profiles/recall_probe.py fill [REPS]    the direct fill against the existing insert pass on the same selected rows: a
                                                 recall of everything from a resident map that holds exactly those rows (the
                                                 selection is one flag per block) against UpdateOnDevice of the rows into a
                                                 cleared map
  python profiles/recall_probe.py trace          recalls after recalls and after a route, each timed, to be run under a trace
                                                 (rocprofv3 --kernel-trace --stats, with --hip-trace for the runtime's calls)
                                                 for the split selection / fill / copies / allocations

Times are host clock around synchronous calls (every entry timed here ends in a stream synchronise), in microseconds."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                      # noqa: E402,F401  (before the library: one HIP runtime in the process)
import sage_icp_amd as sage                       # noqa: E402

GROUND = 3000.0            # metres between the grounds
RADIUS = 600.0             # holds one ground (800 m x 800 m around its centre) and nothing of its neighbours


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e6


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"n": int(len(v)), "min": round(float(v.min()), 1), "median": round(float(np.median(v)), 1),
            "max": round(float(v.max()), 1)}


def pose_at(x):
    return np.array([0.0, 0.0, 0.0, 1.0, x, 0.0, 0.0])


def big_session(grounds=10):
    """~10 M archived rows, half of them an older generation of their voxel; a live window over the last ground"""
    rng = np.random.default_rng(1)
    big = sage.VoxelHashMap(1.0, 1000.0, device=0).set_archive(True)
    pts = None
    for r in range(grounds):
        pts = np.zeros((1_000_000, 4))
        pts[:, :3] = rng.uniform(-400, 400, size=(1_000_000, 3)) * [1.0, 1.0, 0.02]
        pts[:, 3] = 40.0
        big.UpdateOnDevice(pts, pose_at(GROUND * (r // 2)))
        big.UpdateOnDevice(np.zeros((0, 4)), pose_at(-1e5))
    big.UpdateOnDevice(pts[:200000], pose_at(GROUND * ((grounds - 1) // 2)))
    return big


def route(src, twin, t=None):
    """the existing route around the origin (an identity pose moves no row: the twin takes the exported bytes), its pieces
    timed into t"""
    rows = [None]

    def export():
        rows[0] = src.ArchivedPointcloud("session")

    def insert_and_sweep():
        twin.Clear()
        twin.UpdateOnDevice(rows[0], pose_at(0.0))

    a, b = timed(export), timed(insert_and_sweep)
    if t is not None:
        t["route_export_host_rows"].append(a)
        t["route_insert_and_sweep"].append(b)
        t["route"].append(a + b)


def cmd_route(reps=30):
    src = big_session()
    centre = (0.0, 0.0, 0.0)
    dst = sage.VoxelHashMap(1.0, RADIUS, device=0)
    twin = sage.VoxelHashMap(1.0, RADIUS, device=0)
    info = src.Recall(centre, RADIUS, into=dst)[1]
    route(src, twin)                                  # warm, and the comparison
    same = dst.Pointcloud().tobytes() == twin.Pointcloud().tobytes()
    room = torch.empty((info["session_rows"], 4), dtype=torch.float64, device="cuda:0")
    # The call that follows a route is timed apart: whatever the route leaves to be paid later (its 300 MB of pageable host
    # rows going away, its buffers) lands there, whichever entry that call is — the SESSION export into device rows, which
    # this change does not touch, stands beside the recall in both positions.
    t = {k: [] for k in ("recall", "recall_after_route", "route", "route_export_host_rows", "route_insert_and_sweep",
                         "export_device_rows", "export_device_rows_after_route", "recall_fresh_dst")}
    for i in range(reps):
        t["recall_after_route"].append(timed(lambda: src.Recall(centre, RADIUS, into=dst)))
        t["recall"].append(timed(lambda: src.Recall(centre, RADIUS, into=dst)))
        t["export_device_rows"].append(timed(lambda: src.ArchivedPointcloud("session", out=room)))
        route(src, twin, t)
        t["export_device_rows_after_route"].append(timed(lambda: src.ArchivedPointcloud("session", out=room)))
        t["recall_fresh_dst"].append(timed(lambda: src.Recall(centre, RADIUS)))
        route(src, twin, t)
    print(json.dumps({"archive": src.archive_info(), "recall_info": info, "same_bytes_as_the_route": bool(same),
                      "point_slots": {"recall": dst.point_slots(), "route": twin.point_slots()},
                      "us": {k: stats(v) for k, v in t.items()},
                      "first_ten_us": {k: [round(x) for x in v[:10]] for k, v in t.items()}}), flush=True)


def cmd_fill(reps=30):
    src = big_session(grounds=2)
    centre = (0.0, 0.0, 0.0)
    held = src.Recall(centre, RADIUS)[0]                              # ~1 M rows, resident: the selected rows as a map
    rows = held.Pointcloud()
    dst = sage.VoxelHashMap(1.0, RADIUS, device=0)
    twin = sage.VoxelHashMap(1.0, RADIUS, device=0)
    t = {"direct_fill_recall_of_everything": [], "insert_pass_update_on_device": []}

    def insert():
        twin.Clear()
        twin.UpdateOnDevice(rows, pose_at(0.0))

    held.Recall(centre, float("inf"), into=dst)
    insert()
    same = dst.Pointcloud().tobytes() == twin.Pointcloud().tobytes()
    for i in range(reps):
        for what in (("a", "b") if i % 2 == 0 else ("b", "a")):
            if what == "a":
                t["direct_fill_recall_of_everything"].append(timed(lambda: held.Recall(centre, float("inf"), into=dst)))
            else:
                t["insert_pass_update_on_device"].append(timed(insert))
    print(json.dumps({"rows": int(len(rows)), "voxels": held.num_voxels(), "same_bytes": bool(same),
                      "us": {k: stats(v) for k, v in t.items()}}), flush=True)


def cmd_trace(reps=4):
    src = big_session()
    centre = (0.0, 0.0, 0.0)
    dst = sage.VoxelHashMap(1.0, RADIUS, device=0)
    twin = sage.VoxelHashMap(1.0, RADIUS, device=0)
    t = {"recall_after_recall": [], "recall_after_route": [], "route": []}
    src.Recall(centre, RADIUS, into=dst)
    for _ in range(reps):
        t["recall_after_recall"].append(timed(lambda: src.Recall(centre, RADIUS, into=dst)))
        t["recall_after_recall"].append(timed(lambda: src.Recall(centre, RADIUS, into=dst)))
        t["route"].append(timed(lambda: route(src, twin)))
        t["recall_after_route"].append(timed(lambda: src.Recall(centre, RADIUS, into=dst)))
    print(json.dumps({"us": t, "recall_info": src.Recall(centre, RADIUS, into=dst)[1]}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "route"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    if what == "route":
        cmd_route(reps)
    elif what == "fill":
        cmd_fill(reps)
    elif what == "trace":
        cmd_trace()
    else:
        raise SystemExit(__doc__)
