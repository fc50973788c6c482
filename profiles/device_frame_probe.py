"""Per-frame cost of registering a frame that is already on the GPU (csrc/ingest.hip, sageicp_pipeline_register_frame_device)
against the same frame as host rows.  One seeded stream of 120k-point frames (synthetic.make_stream) goes through three
pipelines in one process, frame by frame alternately:
    host     (n,4) float64 rows in host memory (staged into pinned memory and uploaded by the library)
    dev64    the same rows as a float64 [N,4] torch tensor on the GPU
    dev32    a float32 [N,4] tensor (column 3: intensity) plus int64 labels on the GPU
The tensors are made before the timed loop (a segmentation network hands them over).  The whole stream is run `repeats`
times with fresh pipelines; each repeat gives the median of `total_seconds` (what the pipeline times from Preprocess to
the end of the ICP loop) over the frames after the warm-up.  Prints a table of the medians over the repeats and their
spread (min..max of the repeat medians), and writes it to <out>/device_frame_probe.txt.
The poses of host and dev64 are checked to be the same to the bit; dev32 registers the float32-rounded values."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                    # noqa: E402  (before the library: one HIP runtime)
import sage_icp_amd as sage                                     # noqa: E402
from sage_icp_amd import synthetic as syn                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10"))
    a = ap.parse_args()
    if sage.device_count() < 1:
        raise SystemExit("no HIP device: this probe measures the GPU path only")
    frames, _ = syn.make_stream(0xD1, a.frames, points_per_frame=a.points)
    frames = [np.ascontiguousarray(f, dtype=np.float64) for f in frames]
    rng = np.random.default_rng(7)
    dev64 = [torch.from_numpy(f).to("cuda:0") for f in frames]
    dev32 = []
    for f in frames:
        t = np.empty((len(f), 4), dtype=np.float32)
        t[:, :3] = f[:, :3]
        t[:, 3] = rng.uniform(0.0, 1.0, len(f))
        dev32.append((torch.from_numpy(t).to("cuda:0"), torch.from_numpy(f[:, 3].astype(np.int64)).to("cuda:0")))
    torch.cuda.synchronize()
    paths = ("host", "dev64", "dev32")
    med = {p: [] for p in paths}
    for r in range(a.repeats):
        pipes = {p: sage.SageICP() for p in paths}
        tot = {p: [] for p in paths}
        for k in range(a.frames):
            order = paths if (k + r) % 2 == 0 else paths[::-1]
            res = {}
            for p in order:
                if p == "host":
                    res[p] = pipes[p].RegisterFrame(frames[k])
                elif p == "dev64":
                    res[p] = pipes[p].RegisterFrame(dev64[k])
                else:
                    res[p] = pipes[p].RegisterFrame(dev32[k][0], labels=dev32[k][1])
                if k >= a.warmup:
                    tot[p].append(res[p][2])
            assert np.array_equal(res["host"][0].view(np.uint64), res["dev64"][0].view(np.uint64)), "frame %d" % k
        for p in paths:
            med[p].append(1e3 * float(np.median(tot[p])))
    lines = ["device_frame_probe: %d frames of %d..%d points, warm-up %d, %d repeats (fresh pipelines); total_seconds "
             "per frame, ms" % (a.frames, min(map(len, frames)), max(map(len, frames)), a.warmup, a.repeats),
             "%-8s %10s %20s" % ("path", "median", "spread (repeats)")]
    for p in paths:
        v = med[p]
        lines.append("%-8s %10.3f %9.3f .. %-9.3f" % (p, float(np.median(v)), min(v), max(v)))
    base = float(np.median(med["host"]))
    for p in paths[1:]:
        lines.append("%s - host: %+.3f ms" % (p, float(np.median(med[p])) - base))
    text = "\n".join(lines)
    print(text)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "device_frame_probe.txt"), "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
