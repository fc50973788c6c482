"""What the archive of a map costs on the MI355X (results: profiles/r31/README.md).

  python profiles/archive_probe.py update      time of a device-side update per frame, archive off against on, alternating,
                                               beside one Pointcloud() into device memory of the same map in the same run
                                               (the cheapest piece of the only other route to the evicted rows: export
                                               the window before every update and diff it)
  python profiles/archive_probe.py exports     ALL / LATEST / SESSION at the end of the stream and on a log of ~10 M rows,
                                               into device rows and into host rows
  python profiles/archive_probe.py latest      LATEST over and over, to be run under a kernel trace for the shares of its kernels
  python profiles/archive_probe.py off [LABEL] the same two update streams with the archive off only (run on two trees,
                                               alternating, to compare them)

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
from sage_icp_amd import synthetic as syn         # noqa: E402


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e6


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"n": int(len(v)), "min": round(float(v.min()), 1), "median": round(float(np.median(v)), 1),
            "max": round(float(v.max()), 1)}


def c3_stream(frames=200, max_distance=50.0):
    """the c3-style stream: 30k-point frames, 1 m and 0.5 degrees per frame; a 50 m window, so that frames evict"""
    fr, poses = syn.make_stream(3, frames, max_range=max_distance)
    return [np.ascontiguousarray(f, dtype=np.float64) for f in fr], [np.asarray(p, dtype=np.float64) for p in poses], max_distance


def c2_moves(n=64):
    """the 1 M-point c2 map under a sensor that moves 3 m per update: an update evicts a few thousand voxels"""
    w = syn.make_workload("c2", lambda: sage.VoxelHashMap(1.0, 100.0, device=0))
    scan = np.ascontiguousarray(w["scan"], dtype=np.float64)
    poses = [np.array([0.0, 0.0, 0.0, 1.0, 3.0 * (k + 1), 0.0, 0.0]) for k in range(n)]
    return w["map"], scan, poses


def run_updates(maps, frames, poses, export_every=0):
    """the same updates through every map in turn (alternating per frame); per map the times, and the evicted voxels"""
    times = {k: [] for k in maps}
    export = []
    out = None
    for i, pose in enumerate(poses):
        pts = frames[i] if isinstance(frames, list) else frames
        for k in (sorted(maps) if i % 2 == 0 else sorted(maps, reverse=True)):
            times[k].append(timed(lambda: maps[k].UpdateOnDevice(pts, pose)))
        if export_every and i % export_every == 0:
            m = maps[sorted(maps)[0]]
            n = m.size()
            if out is None or out.shape[0] < n:
                out = torch.empty((n + n // 4, 4), dtype=torch.float64, device="cuda:0")
            export.append(timed(lambda: m.Pointcloud(out=out)))
    return times, export


def cmd_update(only_off=False, label=""):
    res = {"label": label}
    frames, poses, md = c3_stream()
    maps = {"off": sage.VoxelHashMap(0.8, md, device=0)}
    if not only_off:
        maps["on"] = sage.VoxelHashMap(0.8, md, device=0).set_archive(True)
    t, ex = run_updates(maps, frames, poses, export_every=0 if only_off else 5)
    warm = 20
    res["c3"] = {k: stats(v[warm:]) for k, v in t.items()}
    if not only_off:
        res["c3"]["added_per_update"] = stats(np.array(t["on"][warm:]) - np.array(t["off"][warm:]))
        res["c3"]["pointcloud_device"] = stats(ex[4:])
        res["c3"]["archive"] = maps["on"].archive_info()
        assert maps["on"].Pointcloud().tobytes() == maps["off"].Pointcloud().tobytes()
    base, scan, poses = c2_moves()
    maps = {"off": base}
    if not only_off:
        maps["on"] = base.clone().set_archive(True)
    t, ex = run_updates(maps, scan, poses, export_every=0 if only_off else 4)
    warm = 4
    res["c2"] = {k: stats(v[warm:]) for k, v in t.items()}
    if not only_off:
        res["c2"]["added_per_update"] = stats(np.array(t["on"][warm:]) - np.array(t["off"][warm:]))
        res["c2"]["pointcloud_device"] = stats(ex[1:])
        res["c2"]["archive"] = maps["on"].archive_info()
        res["c2"]["voxels_per_update"] = round(res["c2"]["archive"]["voxels"] / len(poses), 1)
    print(json.dumps(res), flush=True)


def time_exports(m, tag, reps=5):
    out = {}
    for which in ("all", "latest", "session"):
        dst = torch.empty((sage._archive_room(lambda: m._h, sage.ARCHIVE_WHICH[which], 0), 4), dtype=torch.float64, device="cuda:0")
        n = len(m.ArchivedPointcloud(which, out=dst))
        dev = [timed(lambda: m.ArchivedPointcloud(which, out=dst)) for _ in range(reps)]
        host = [timed(lambda: m.ArchivedPointcloud(which)) for _ in range(reps)]
        out[which] = {"rows": int(n), "device_rows_us": stats(dev[1:]), "host_rows_us": stats(host[1:])}
    print(json.dumps({tag: out, "archive": m.archive_info(), "map_rows": m.size()}), flush=True)


def cmd_exports():
    frames, poses, md = c3_stream()
    m = sage.VoxelHashMap(0.8, md, device=0).set_archive(True)
    for f, p in zip(frames, poses):
        m.UpdateOnDevice(f, p)
    time_exports(m, "c3_end")
    # a log of ~10 M rows: ten maps of a million points each, evicted whole; every second one over the same ground, so
    # that half the records have a later generation
    rng = np.random.default_rng(1)
    big = sage.VoxelHashMap(1.0, 1000.0, device=0).set_archive(True)
    here = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    away = here.copy()
    away[4] = -1e5
    for r in range(10):
        pts = np.zeros((1_000_000, 4))
        pts[:, :3] = rng.uniform(-400, 400, size=(1_000_000, 3)) * [1.0, 1.0, 0.02]
        pts[:, 3] = 40.0
        here[4] = 3000.0 * (r // 2)
        big.UpdateOnDevice(pts, here)
        big.UpdateOnDevice(np.zeros((0, 4)), away)
    big.UpdateOnDevice(pts[:200000], here)            # a live window over the last ground
    time_exports(big, "log_10M", reps=3)


def cmd_latest(reps=20):
    """LATEST at the end of the c3 stream into device rows, over and over: run under `rocprofv3 --kernel-trace --stats` for
    the shares of its kernels (sort, probe, selection, gather)"""
    frames, poses, md = c3_stream()
    m = sage.VoxelHashMap(0.8, md, device=0).set_archive(True)
    for f, p in zip(frames, poses):
        m.UpdateOnDevice(f, p)
    dst = torch.empty((m.archive_info()["rows"], 4), dtype=torch.float64, device="cuda:0")
    t = [timed(lambda: m.ArchivedPointcloud("latest", out=dst)) for _ in range(reps)]
    print(json.dumps({"latest_device_rows_us": stats(t[1:]), "archive": m.archive_info()}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "update"
    if what == "update":
        cmd_update()
    elif what == "off":
        cmd_update(only_off=True, label=sys.argv[2] if len(sys.argv) > 2 else "")
    elif what == "exports":
        cmd_exports()
    elif what == "latest":
        cmd_latest()
    else:
        raise SystemExit(__doc__)
