"""What the PointCloud2 entries cost (csrc/msg.hip) against the parent's way of producing the same bytes, written to
<out>/msg_probe.txt.  A host clock around each synchronous call; medians of --calls calls after --warmup.

  (a) LocalMapMsg of a c2-size map (synthetic.make_workload("c2"): 1M points, resident): the 21-byte records into a fresh
      numpy array and into a preallocated device tensor, against the parent's route — LocalMap() host rows, then the
      node's single-threaded fill loop with its std::map colour lookup (node_loops.cpp, g++ -O2) into a fresh buffer.
      The two host results are compared byte for byte first.
  (b) RegisterFrame of 120k-point frames as a message in host memory and as a message in device memory, against
      RegisterFrame(rows) with the node's host-side expansion of the message into double[n][4] (node_loops.cpp) inside
      the timed span.  A stream of --frames frames is run --calls / --frames times (reinitialize() between the passes),
      the same for every route; the first --warmup calls are dropped.  Poses are compared bit for bit across routes.
--quick: few calls (for a kernel-trace run)."""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import torch                                                    # noqa: E402  (before the library: one HIP runtime)
import sage_icp_amd as sage                                     # noqa: E402
from sage_icp_amd import synthetic as syn                       # noqa: E402

DEV = "cuda:0"
COLORS = {l: (l * 0x010305 + 7) & 0xFFFFFF for l in range(256)}


def node_loops():
    out = os.path.join(tempfile.mkdtemp(prefix="sageicp_r20_"), "libnode_loops.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "node_loops.cpp"), "-o", out])
    L = ctypes.CDLL(out)
    L.colors_new.restype = ctypes.c_void_p
    L.colors_new.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.fill_xyzlrgb.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.expand_xyzl.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_uint32] * 5 + [ctypes.c_int, ctypes.c_void_p]
    return L


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def part_a(L, calls, warmup, lines):
    w = syn.make_workload("c2", lambda: sage.VoxelHashMap(1.0, 1e6))
    m = w["map"]
    m.UpdateOnDevice(w["scan"][:5000], w["T_gt"])
    n = m.size()
    keys = np.array(sorted(COLORS), dtype=np.int32)
    vals = np.array([COLORS[k] for k in keys], dtype=np.int32)
    cl = L.colors_new(keys.ctypes.data, vals.ctypes.data, len(keys))

    def parent():
        rows = m.Pointcloud()
        data = np.zeros(len(rows) * 21, dtype=np.uint8)          # (data.resize of a fresh message)
        L.fill_xyzlrgb(rows.ctypes.data, len(rows), cl, data.ctypes.data)
        return data

    def fill_only(rows=m.Pointcloud()):
        data = np.zeros(len(rows) * 21, dtype=np.uint8)
        L.fill_xyzlrgb(rows.ctypes.data, len(rows), cl, data.ctypes.data)

    assert np.array_equal(parent().reshape(n, 21), m.PointcloudMsg(COLORS)), "the records differ from the node's loop"
    pre = torch.empty((n, 21), dtype=torch.uint8, device=DEV)
    lines.append("(a) LocalMapMsg, c2 map: %d points (%.1f MB of records, %.1f MB of float64 rows), resident=%s; median of %d "
                 "calls, ms" % (n, n * 21 / 1e6, n * 32 / 1e6, m.resident(), calls))
    for name, fn in (("parent: LocalMap() host rows + the node's fill loop", parent),
                     ("  of which the fill loop alone (rows given)", fill_only),
                     ("new: records into a fresh numpy array", lambda: m.PointcloudMsg(COLORS)),
                     ("new: records into a preallocated device tensor", lambda: m.PointcloudMsg(COLORS, out=pre)),
                     ("new: records into a fresh device tensor", lambda: m.PointcloudMsg(COLORS, device=True))):
        lines.append("  %-52s %8.3f" % (name, timed(fn, calls, warmup)))


def part_b(L, frames, calls, warmup, lines):
    fields = [sage.PointField("x", 0, 7), sage.PointField("y", 4, 7), sage.PointField("z", 8, 7),
              sage.PointField("label", 12, 2), sage.PointField("rgb", 13, 6)]
    blobs = []
    for f in frames:
        rec = np.zeros(len(f), dtype=np.dtype({"names": ["x", "y", "z", "label"], "formats": ["<f4", "<f4", "<f4", "u1"],
                                               "offsets": [0, 4, 8, 12], "itemsize": 21}))
        rec["x"], rec["y"], rec["z"], rec["label"] = f[:, 0], f[:, 1], f[:, 2], f[:, 3]
        blobs.append(rec.view(np.uint8))
    dev_blobs = [torch.from_numpy(b).to(DEV) for b in blobs]

    def rows_route(p, k):
        b = blobs[k]
        n = len(b) // 21
        rows = np.empty((n, 4))
        L.expand_xyzl(b.ctypes.data, n, 21, 0, 4, 8, 12, 1, rows.ctypes.data)
        return p.RegisterFrame(rows)

    def host_msg(p, k):
        return p.RegisterFrame(sage.PointCloud2(fields, 21, blobs[k], width=len(blobs[k]) // 21))

    def dev_msg(p, k):
        return p.RegisterFrame(sage.PointCloud2(fields, 21, dev_blobs[k], width=len(blobs[k]) // 21))

    passes = max(1, -(-(calls + warmup) // len(frames)))
    res, poses = {}, {}
    for name, route in (("parent: host expansion + RegisterFrame(rows)", rows_route),
                        ("new: RegisterFrame(msg), data in host memory", host_msg),
                        ("new: RegisterFrame(msg), data in device memory", dev_msg)):
        p = sage.SageICP()
        t = []
        for _ in range(passes):
            p.reinitialize()
            for k in range(len(frames)):
                t0 = time.perf_counter()
                route(p, k)
                t.append(time.perf_counter() - t0)
        res[name] = float(np.median(t[warmup:warmup + calls])) * 1e3
        poses[name] = p.poses().copy()
    ref = poses["parent: host expansion + RegisterFrame(rows)"]
    assert all(np.array_equal(ref.view(np.uint64), v.view(np.uint64)) for v in poses.values()), "poses differ across routes"
    lines.append("(b) RegisterFrame, %d frames of %d points run %d times; median of calls %d..%d, ms per frame (poses bit-equal "
                 "across the routes)" % (len(frames), len(frames[0]), passes, warmup + 1, warmup + calls))
    for name, v in res.items():
        lines.append("  %-52s %8.3f" % (name, v))
    n = len(frames[0])
    rows = np.empty((n, 4))
    lines.append("  %-52s %8.3f" % ("  of which the host expansion alone",
                                    timed(lambda: L.expand_xyzl(blobs[0].ctypes.data, n, 21, 0, 4, 8, 12, 1, rows.ctypes.data),
                                          calls, warmup)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=22)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    if sage.device_count() < 1:
        raise SystemExit("no HIP device: this probe measures the GPU path only")
    if a.quick:
        a.calls, a.warmup, a.frames = 6, 2, 4
    L = node_loops()
    lines = []
    part_a(L, a.calls, a.warmup, lines)
    frames, _ = syn.make_stream(0xD1, a.frames, points_per_frame=120000)
    frames = [np.ascontiguousarray(f, dtype=np.float64) for f in frames]
    part_b(L, frames, a.calls, a.warmup, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(a.out, "msg_probe_quick.txt" if a.quick else "msg_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
