"""What the loop-closure entries cost on the MI355X beside the only other route (results: profiles/r38/closure_*.txt).

  python profiles/closure_probe.py route [REPS]   the log of recall_probe.py (10 M rows, 9.47 M records, a live window) and a
                                                  table of 4 000 poses: the log's own 21 update positions first (serial s of a
                                                  record is one of them), then a drive of 1 m steps that ends over the live
                                                  window (the live voxels' walks run back along it until it is far).  In turns:
                                                    stays      SessionStays(positions, "session")
                                                    corrected  CorrectedPointcloud("session", ...) into device rows (reused)
                                                    export     the plain SESSION export into the same device rows
                                                    route      the only other way to the same rows on the parent commit: the
                                                               SESSION rows and the records to the host, the stay rule and the
                                                               move as a compiled host loop (the restatement's, C, -O2), the
                                                               rows back to the device; its pieces timed one by one
                                                  and the two results compared on bytes
  python profiles/closure_probe.py trace          a few calls of each entry, to be run under rocprofv3 --kernel-trace --stats

Times are host clock around synchronous calls, in microseconds; the first calls are warm-up and not counted."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch                                      # noqa: E402,F401  (before the library: one HIP runtime in the process)
import sage_icp_amd as sage                       # noqa: E402
from recall_probe import GROUND, big_session, stats, timed   # noqa: E402

N_POSES = 4000
MAX_DISTANCE = 1000.0                             # big_session's

HOST_C = r"""
#include <stdint.h>
#include <math.h>
typedef struct { int32_t x, y, z; uint32_t count; uint64_t first_row, update; } rec_t;
/* record i is LATEST iff no later record has its key and the live map does not hold it: the caller passes the verdicts
   (keep[i]); this loop is the stay rule and the move alone */
static uint32_t stay_of(const double *p, int64_t hi, const double *pos, double max2) {
    uint32_t best = hi > 0 ? (uint32_t)hi : 0u;
    double best_d = INFINITY;
    for (int64_t k = hi; k >= 0; --k) {
        const double dx = p[0] - pos[3 * k], dy = p[1] - pos[3 * k + 1], dz = p[2] - pos[3 * k + 2];
        const double d = (dx * dx + dy * dy) + dz * dz;
        if (d > max2) break;
        if (d < best_d) { best_d = d; best = (uint32_t)k; }
    }
    return best;
}
static void move_rows(double *rows, uint64_t n, const double *T) {
    const double x = T[0], y = T[1], z = T[2], w = T[3];
    const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    for (uint64_t r = 0; r < n; ++r) {
        double *p = rows + 4 * r;
        const double a = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + T[4];
        const double b = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + T[5];
        const double c = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + T[6];
        p[0] = a; p[1] = b; p[2] = c;
    }
}
/* rows: the SESSION rows (the kept records' rows in log order, then the live map's); returns the voxels seen */
uint64_t correct_session(double *rows, uint64_t n_rows, const rec_t *rec, const uint8_t *keep, uint64_t n_rec, double voxel,
                         const double *pos, uint64_t n, double max_distance, const double *corr) {
    const double max2 = max_distance * max_distance;
    uint64_t at = 0, voxels = 0;
    for (uint64_t i = 0; i < n_rec; ++i) {
        if (!keep[i]) continue;
        const int64_t hi = (int64_t)(rec[i].update < n ? rec[i].update : n) - 1;
        move_rows(rows + 4 * at, rec[i].count, corr + 7 * stay_of(rows + 4 * at, hi, pos, max2));
        at += rec[i].count;
        ++voxels;
    }
    while (at < n_rows) {                      /* the live voxels: consecutive rows of one key */
        const double *p = rows + 4 * at;
        const int32_t kx = (int32_t)(p[0] / voxel), ky = (int32_t)(p[1] / voxel), kz = (int32_t)(p[2] / voxel);
        uint64_t e = at + 1;
        while (e < n_rows && (int32_t)(rows[4 * e] / voxel) == kx && (int32_t)(rows[4 * e + 1] / voxel) == ky &&
               (int32_t)(rows[4 * e + 2] / voxel) == kz) ++e;
        move_rows(rows + 4 * at, e - at, corr + 7 * stay_of(p, (int64_t)n - 1, pos, max2));
        at = e;
        ++voxels;
    }
    return voxels;
}
"""


def host_loop():
    d = tempfile.mkdtemp(prefix="closure_probe_")
    src, so = os.path.join(d, "host.c"), os.path.join(d, "host.so")
    with open(src, "w") as f:
        f.write(HOST_C)
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so, "-lm"])
    lib = ctypes.CDLL(so)
    lib.correct_session.restype = ctypes.c_uint64
    lib.correct_session.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                    ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p]
    return lib


def latest_verdicts(rec, live_rows, voxel):
    """keep[i] of the records (numpy, outside the timed route: the route is charged only the stay rule and the move)"""
    def pack(x, y, z):                                             # (keys lie within +-2^20)
        return ((x.astype(np.int64) + (1 << 20)) << 42) | ((y.astype(np.int64) + (1 << 20)) << 21) | (z.astype(np.int64) + (1 << 20))

    key = pack(rec["x"], rec["y"], rec["z"])
    live = np.trunc(live_rows[:, :3] / voxel).astype(np.int64)
    live_key = np.unique(pack(live[:, 0], live[:, 1], live[:, 2]))
    _, last = np.unique(key[::-1], return_index=True)
    keep = np.zeros(len(rec), dtype=np.uint8)
    keep[len(rec) - 1 - last] = 1
    keep[np.isin(key, live_key)] = 0
    return keep


def table(src):
    """(positions (N_POSES, 3), corrections (N_POSES, 7))"""
    updates = src.archive_info()["updates"]
    own = []
    for r in range(10):
        own += [(GROUND * (r // 2), 0.0, 0.0), (-1e5, 0.0, 0.0)]
    own.append((GROUND * 4, 0.0, 0.0))
    assert len(own) == updates == 21
    end = GROUND * 4
    drive = [(end - (N_POSES - 1 - k) * 1.0, 0.0, 0.0) for k in range(len(own), N_POSES)]
    pos = np.array(own + drive, dtype=np.float64)
    poses = np.concatenate([np.tile([0.0, 0.0, 0.0, 1.0], (N_POSES, 1)), pos], axis=1)
    h = 0.5 * np.radians(2.0)
    closed = poses[-1] * 1.0
    closed[:4] = [0.0, 0.0, np.sin(h), np.cos(h)]
    closed[4:] += [3.0, -2.0, 0.2]
    return pos, sage.closure_corrections(poses, 0, N_POSES - 1, closed)[0]


def cmd_route(reps=30, warm=3):
    src = big_session()
    pos, corr = table(src)
    lib = host_loop()
    n_rows = len(src.ArchivedPointcloud("session"))
    room = torch.empty((n_rows, 4), dtype=torch.float64, device="cuda:0")
    t = {k: [] for k in ("stays", "corrected_device_rows", "export_device_rows", "route", "route_rows_and_records_to_host",
                         "route_stay_rule_and_move", "route_rows_to_device")}
    out = {}

    def route(keep_times):
        got = {}

        def down():
            got["rows"] = src.ArchivedPointcloud("session")
            got["rec"] = src.archive_voxels()

        a = timed(down)
        rows, rec = got["rows"], np.ascontiguousarray(got["rec"])
        keep = latest_verdicts(rec, src.Pointcloud(), 1.0)         # (not charged)

        def loop():
            got["voxels"] = lib.correct_session(rows.ctypes.data, len(rows), rec.ctypes.data, keep.ctypes.data, len(rec), 1.0,
                                                pos.ctypes.data, len(pos), MAX_DISTANCE, corr.ctypes.data)

        b = timed(loop)

        def up():
            got["dev"] = torch.from_numpy(rows).to("cuda:0")
            torch.cuda.synchronize()

        c = timed(up)
        if keep_times:
            t["route_rows_and_records_to_host"].append(a)
            t["route_stay_rule_and_move"].append(b)
            t["route_rows_to_device"].append(c)
            t["route"].append(a + b + c)
        return got

    for i in range(warm + reps):
        keep_times = i >= warm
        for name, f in (("stays", lambda: out.__setitem__("stays", src.SessionStays(pos, "session"))),
                        ("corrected_device_rows", lambda: src.CorrectedPointcloud("session", pos, corr, out=room)),
                        ("export_device_rows", lambda: src.ArchivedPointcloud("session", out=room))):
            us = timed(f)
            if keep_times:
                t[name].append(us)
        got = route(keep_times)
    src.CorrectedPointcloud("session", pos, corr, out=room)
    same = room.cpu().numpy().tobytes() == got["dev"].cpu().numpy().tobytes()
    stays = out["stays"]
    print(json.dumps({"archive": src.archive_info(), "session_rows": int(n_rows), "session_voxels": int(len(stays)),
                      "route_voxels": int(got["voxels"]), "poses": N_POSES, "same_bytes_as_the_route": bool(same),
                      "stay_histogram": {"min": int(stays.min()), "max": int(stays.max()), "distinct": int(len(np.unique(stays)))},
                      "us": {k: stats(v) for k, v in t.items()},
                      "device_over_route": round(float(np.median(t["corrected_device_rows"]) / np.median(t["route"])), 4),
                      "first_ten_us": {k: [round(x) for x in v[:10]] for k, v in t.items()}}), flush=True)


def cmd_trace(reps=4):
    src = big_session()
    pos, corr = table(src)
    n_rows = len(src.ArchivedPointcloud("session"))
    room = torch.empty((n_rows, 4), dtype=torch.float64, device="cuda:0")
    t = {"stays": [], "corrected_device_rows": []}
    for _ in range(reps):
        t["stays"].append(timed(lambda: src.SessionStays(pos, "session")))
        t["corrected_device_rows"].append(timed(lambda: src.CorrectedPointcloud("session", pos, corr, out=room)))
    print(json.dumps({"us": t, "calls_of_each": reps}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "route"
    if what == "route":
        cmd_route(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
    elif what == "trace":
        cmd_trace()
    else:
        raise SystemExit(__doc__)
