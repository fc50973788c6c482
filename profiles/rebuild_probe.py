"""What the session rebuild costs on the MI355X beside the only other route to the same map (results:
profiles/r43/rebuild_*.txt).

  python profiles/rebuild_probe.py route [REPS]   the log of recall_probe.py (10 M rows, 9.47 M records, a live window) and the
                                                  4 000 poses and corrections of closure_probe.py.  In turns, each with no
                                                  crop and with recall_probe's radius around the origin:
                                                    rebuild    RebuildSession(positions, corrections, "session", into=dst), dst reused
                                                    route      the parent commit's only way to the same map, timed piece by
                                                               piece: CorrectedPointcloud("session") into host rows, then
                                                               either AddPoints into a cleared twin (+ RemovePointsFarFromLocation
                                                               where cropped) or one UpdateOnDevice of the twin at the identity
                                                               pose (insert and sweep on the device; max_distance = radius)
                                                  and the results compared on bytes
  python profiles/rebuild_probe.py trace          a few calls of the rebuild, to be run under rocprofv3 --kernel-trace --stats

Times are host clock around synchronous calls, in microseconds; the first calls are warm-up and not counted."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch                                      # noqa: E402,F401  (before the library: one HIP runtime in the process)
import sage_icp_amd as sage                       # noqa: E402
from closure_probe import table                   # noqa: E402
from recall_probe import RADIUS, big_session, pose_at, stats, timed   # noqa: E402

CENTRE = (0.0, 0.0, 0.0)
NO_CROP_DISTANCE = 1e7                            # a twin that evicts nothing when it is updated at the origin


def cmd_route(reps=30, warm=3):
    src = big_session()
    pos, corr = table(src)
    forms = {"whole": (None, math.inf, NO_CROP_DISTANCE), "cropped": (CENTRE, RADIUS, RADIUS)}
    dst = {k: sage.VoxelHashMap(1.0, md, device=0) for k, (_, _, md) in forms.items()}
    twin_host = {k: sage.VoxelHashMap(1.0, md, device=0) for k, (_, _, md) in forms.items()}
    twin_dev = {k: sage.VoxelHashMap(1.0, md, device=0) for k, (_, _, md) in forms.items()}
    names = ["rebuild", "route_corrected_host_rows", "route_add_points", "route_remove_far", "route_host", "route_update_on_device",
             "route_device"]
    t = {k: {n: [] for n in names} for k in forms}
    info, same = {}, {}
    for i in range(warm + reps):
        keep = i >= warm
        for k, (centre, radius, _) in forms.items():
            got = {}
            us = {}
            us["rebuild"] = timed(lambda: got.__setitem__("info", src.RebuildSession(pos, corr, center=centre, radius=radius, into=dst[k])[1]))
            us["route_corrected_host_rows"] = timed(lambda: got.__setitem__("rows", src.CorrectedPointcloud("session", pos, corr)))
            rows = got["rows"]

            def add():
                twin_host[k].Clear()
                twin_host[k].AddPoints(rows)

            us["route_add_points"] = timed(add)
            us["route_remove_far"] = timed(lambda: twin_host[k].RemovePointsFarFromLocation(np.array(CENTRE))) if centre is not None else 0.0

            def update():
                twin_dev[k].Clear()
                twin_dev[k].UpdateOnDevice(rows, pose_at(0.0))

            us["route_update_on_device"] = timed(update)
            us["route_host"] = us["route_corrected_host_rows"] + us["route_add_points"] + us["route_remove_far"]
            us["route_device"] = us["route_corrected_host_rows"] + us["route_update_on_device"]
            if keep:
                for n in names:
                    t[k][n].append(us[n])
            info[k] = got["info"]
        print("call %d of %d" % (i + 1, warm + reps), file=sys.stderr, flush=True)
    for k in forms:
        cloud = dst[k].Pointcloud().tobytes()
        same[k] = {"host_route": cloud == twin_host[k].Pointcloud().tobytes(), "device_route": cloud == twin_dev[k].Pointcloud().tobytes(),
                   "point_slots": {"rebuild": dst[k].point_slots(), "host_route": twin_host[k].point_slots()}}
    out = {"archive": src.archive_info(), "poses": len(pos), "info": info, "same_bytes": same, "calls": reps, "warm_up": warm,
           "us": {k: {n: stats(v) for n, v in t[k].items()} for k in forms}}
    for k in forms:
        cheapest = min(np.median(t[k]["route_host"]), np.median(t[k]["route_device"]))
        out["rebuild_over_cheapest_route_" + k] = round(float(np.median(t[k]["rebuild"]) / cheapest), 4)
    print(json.dumps(out), flush=True)


def cmd_trace(reps=4):
    src = big_session()
    pos, corr = table(src)
    dst = sage.VoxelHashMap(1.0, RADIUS, device=0)
    t = {"whole": [], "cropped": []}
    for _ in range(reps):
        t["whole"].append(timed(lambda: src.RebuildSession(pos, corr, into=dst)))
        t["cropped"].append(timed(lambda: src.RebuildSession(pos, corr, center=CENTRE, radius=RADIUS, into=dst)))
    print(json.dumps({"us": t, "calls_of_each": reps}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "route"
    if what == "route":
        cmd_route(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
    elif what == "trace":
        cmd_trace()
    else:
        raise SystemExit(__doc__)
