"""What key-frame selection costs per frame (csrc/keyframe.hip, sageicp_pipeline_set_key_frames), against the host path
it replaces.  Written to <out>/keyframe_probe.txt:

  pipeline  a stream of 120k-point frames (synthetic.make_stream, the c2 size) registered with selection off and on
            (the launch files' 128 x 128 grid over +-51.2 m, overlap 0.5), in alternating streams.  Per frame: the wall
            time of RegisterFrame, and the wall time outside the span the call reports (wall - total_seconds), where
            the key-frame pass runs.  Medians over the frames after the warm-up, median over --repeats streams each.
  host      profiles/r12/keyframe_host.cpp (g++ -O3) on one of the same frames: the node's transform + grid + overlap on
            the CPU with its nested-vector grids, median of 50 calls.
--quick: one short stream (for a kernel-trace run)."""
import argparse
import os
import struct
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import torch                                                    # noqa: E402,F401  (before the library: one HIP runtime)
import sage_icp_amd as sage                                     # noqa: E402
from sage_icp_amd import synthetic as syn                       # noqa: E402


def stream(frames, select):
    p = sage.SageICP()
    if select:
        p.set_key_frames(True)
    wall, outside, keys = [], [], 0
    for f in frames:
        t0 = time.perf_counter()
        _, _, tot, _, _ = p.RegisterFrame(f)
        dt = time.perf_counter() - t0
        wall.append(dt)
        outside.append(dt - tot)
        if select:
            keys += p.key_frame_info()["is_key_frame"]
    return np.array(wall), np.array(outside), keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.frames, a.warmup, a.repeats = 6, 2, 1
    os.makedirs(a.out, exist_ok=True)
    frames, _ = syn.make_stream(7, a.frames, points_per_frame=120000)
    frames = [np.ascontiguousarray(f, dtype=np.float64) for f in frames]
    lines = ["frames of %d points, %d frames per stream, the first %d not counted, %d streams each"
             % (len(frames[0]), a.frames, a.warmup, a.repeats)]
    res = {False: [], True: []}
    for r in range(a.repeats):
        for select in ((False, True) if r % 2 == 0 else (True, False)):
            w, o, keys = stream(frames, select)
            res[select].append((np.median(w[a.warmup:]) * 1e3, np.median(o[a.warmup:]) * 1e6, keys))
    for select in (False, True):
        w = np.median([x[0] for x in res[select]])
        o = np.median([x[1] for x in res[select]])
        lines.append("selection %-3s  wall %.3f ms per frame, outside the reported span %.1f us, key frames %s"
                     % ("on" if select else "off", w, o, [x[2] for x in res[select]]))
    dw = np.median([x[0] for x in res[True]]) - np.median([x[0] for x in res[False]])
    do = np.median([x[1] for x in res[True]]) - np.median([x[1] for x in res[False]])
    lines.append("added by selection: %.1f us wall per frame, %.1f us of it outside the reported span" % (dw * 1e3, do))
    # the host path on the CPU
    exe = os.path.join(a.out, "keyframe_host")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-o", exe, os.path.join(HERE, "keyframe_host.cpp")])
    binf = os.path.join(a.out, "keyframe_frame.bin")
    f = frames[a.frames // 2]
    pose = np.array([0.0, 0.0, np.sin(0.01), np.cos(0.01), 1.0, 0.2, 0.0])
    with open(binf, "wb") as fh:
        fh.write(struct.pack("<Q", len(f)))
        fh.write(f.tobytes())
        fh.write(pose.tobytes())
    lines.append(subprocess.check_output([exe, binf, "50"], text=True).strip())
    os.remove(binf)
    os.remove(exe)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(a.out, "keyframe_probe.txt"), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
