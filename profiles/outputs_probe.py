"""What the outputs in device memory cost (csrc/egress.hip, sageicp_map_pointcloud_device, sageicp_pipeline_source_device),
against the host rows they replace.  Three parts, written to <out>/outputs_probe.txt:

  single   LocalMap of a c2-size map (synthetic.make_workload("c2"): 1M points, made resident by one device update):
           host rows into a fresh numpy array, and device rows in float64 and float32, into a preallocated tensor and into
           a fresh torch.empty.  A host clock around each synchronous call; the median of --calls calls after --warmup.
  ab       the same device call with the gather writing the caller's layout itself (fused, the default) against packing
           into the library's buffer and converting from there (SAGEICP_EGRESS_TWO_PASS=1), in alternating blocks.
  stream   a stream of 120k-point frames (synthetic.make_stream) with LocalMap after every frame, as the ROS node calls it:
           none / host rows / device float64 into a fresh tensor / device float64 into a preallocated one.  Wall time per
           frame (RegisterFrame + LocalMap), the median over the frames after the warm-up, median over --repeats streams.
--quick: few calls and one short stream (for a kernel-trace run)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                    # noqa: E402  (before the library: one HIP runtime)
import sage_icp_amd as sage                                     # noqa: E402
if os.environ.get("LOOP_LIB"):           # a variant build of the library (A/B runs)
    sage.LIB_PATH = os.path.abspath(os.environ["LOOP_LIB"])
from sage_icp_amd import synthetic as syn                       # noqa: E402

DEV = "cuda:0"


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def single(m, calls, warmup, lines):
    n = m.size()
    pre64 = torch.empty((n, 4), dtype=torch.float64, device=DEV)
    pre32 = torch.empty((n, 4), dtype=torch.float32, device=DEV)
    rows = [("host LocalMap() into a fresh numpy array", lambda: m.Pointcloud()),
            ("device float64 into a preallocated tensor", lambda: m.Pointcloud(out=pre64)),
            ("device float32 into a preallocated tensor", lambda: m.Pointcloud(out=pre32)),
            ("device float64 into a fresh torch.empty", lambda: m.Pointcloud(device=True)),
            ("device float32 into a fresh torch.empty", lambda: m.Pointcloud(device=True, dtype=torch.float32))]
    lines.append("single calls, c2 map: %d points (%.1f MB of float64 rows), resident=%s; median of %d calls, ms"
                 % (n, n * 32 / 1e6, m.resident(), calls))
    for name, fn in rows:
        lines.append("  %-46s %8.3f" % (name, timed(fn, calls, warmup)))
    return pre64, pre32


def ab(m, pre64, pre32, calls, warmup, lines, blocks=5):
    res = {}
    for b in range(blocks):
        for mode in ("fused", "two_pass"):
            if mode == "two_pass":
                os.environ["SAGEICP_EGRESS_TWO_PASS"] = "1"
            try:
                for dt, out in (("float64", pre64), ("float32", pre32)):
                    res.setdefault((mode, dt), []).append(timed(lambda: m.Pointcloud(out=out), calls // blocks + 1,
                                                                warmup if b == 0 else 2))
            finally:
                os.environ.pop("SAGEICP_EGRESS_TWO_PASS", None)
    lines.append("A/B: the gather writing the caller's layout (fused) against pack + k_egress (two_pass); %d alternating "
                 "blocks, median of the block medians, ms (min..max over blocks)" % blocks)
    for dt in ("float64", "float32"):
        for mode in ("fused", "two_pass"):
            v = res[(mode, dt)]
            lines.append("  %-8s %-9s %8.3f  (%.3f .. %.3f)" % (dt, mode, np.median(v), min(v), max(v)))


def stream(frames, warmup, repeats, lines):
    n = None
    modes = ("none", "host", "device_fresh", "device_prealloc")
    med = {k: [] for k in modes}
    for r in range(repeats):
        for mode in modes:
            p = sage.SageICP()
            buf = [None]

            def local_map():
                if mode == "host":
                    return p.LocalMap()
                if mode == "device_fresh":
                    return p.LocalMap(device=True)
                if mode == "device_prealloc":
                    k = int(sage.lib().sageicp_map_size(sage.lib().sageicp_pipeline_local_map(p._h)))
                    if buf[0] is None or buf[0].shape[0] < k:
                        buf[0] = torch.empty((k + k // 4, 4), dtype=torch.float64, device=DEV)
                    return p.LocalMap(out=buf[0])
                return None
            t = []
            for f in frames:
                t0 = time.perf_counter()
                p.RegisterFrame(f)
                lm = local_map()
                t.append(time.perf_counter() - t0)
                if lm is not None:
                    n = len(lm)
            med[mode].append(float(np.median(t[warmup:])) * 1e3)
            del p
    lines.append("stream: %d frames of %d points, LocalMap after every frame (last map: %s points); wall ms per frame "
                 "(RegisterFrame + LocalMap), median over frames %d.., median (min..max) over %d streams"
                 % (len(frames), len(frames[0]), n, warmup + 1, repeats))
    for mode in modes:
        v = med[mode]
        lines.append("  %-16s %8.3f  (%.3f .. %.3f)" % (mode, np.median(v), min(v), max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--frame-warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11"))
    a = ap.parse_args()
    if sage.device_count() < 1:
        raise SystemExit("no HIP device: this probe measures the GPU path only")
    if a.quick:
        a.calls, a.warmup, a.frames, a.frame_warmup, a.repeats = 10, 2, 8, 2, 1
    w = syn.make_workload("c2", lambda: sage.VoxelHashMap(1.0, 1e6))
    m = w["map"]
    m.UpdateOnDevice(w["scan"][:5000], w["T_gt"])
    lines = []
    pre64, pre32 = single(m, a.calls, a.warmup, lines)
    ab(m, pre64, pre32, a.calls, a.warmup, lines)
    frames, _ = syn.make_stream(0xD1, a.frames, points_per_frame=120000)
    frames = [np.ascontiguousarray(f, dtype=np.float64) for f in frames]
    stream(frames, a.frame_warmup, a.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if not a.quick:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "outputs_probe.txt"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
