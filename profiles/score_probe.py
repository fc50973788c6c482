"""What scoring a batch of candidate poses costs (csrc/score.hip).  Written to <out>/score_probe.txt; a
host clock around each synchronous call, the median of --calls calls after --warmup and their range.

  the batch      a 10 000-row frame (c1's size: the first rows of c2's scan), the 1 M-point c2 map made resident by one
                 device update, K poses scattered around T_gt: one sageicp_score_poses_device call against the only
                 route to the same numbers without it, K calls of sageicp_registration_quality_device — alternating in
                 one process, each ending in a synchronise (both entries are synchronous).  K = 256 and a sweep over
                 smaller K, to say from which K the batch pays.  The bytes of the shared fields are asserted equal.
  Relocalize     the street scene of tests/scoreref.py (35 000 map points at 0.8 m, a 2 000-row scan 4 m / 25 degrees
                 from the prior), the 637-candidate grid, refine_top = 3: the wall time, split into us_score / us_refine.
"""
import argparse
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch                                                    # noqa: E402  (before the library: one HIP runtime)
import sage_icp_amd as sage                                     # noqa: E402
from sage_icp_amd import synthetic as syn                       # noqa: E402

SHARED = ("fitness", "rmse", "step_norm", "sum_r2", "sum_w", "sum_w_r2", "step", "JTr", "JTJ", "n_queries", "n_pairs",
          "pairs_same_label", "pairs_unlabelled", "pairs_cross_label", "valid")


def line(name, t):
    t = np.asarray(t)
    return "  %-58s %9.3f  (min %.3f, p10 %.3f, p90 %.3f, max %.3f)" % (
        name, np.median(t), t.min(), np.percentile(t, 10), np.percentile(t, 90), t.max())


def batch(a):
    w = syn.make_workload("c2", lambda: sage.VoxelHashMap(1.0, 1e6))
    p = syn.PARAMS["cold"]
    md, kernel, th = p["max_dist"], p["kernel"], p["sem_th"]
    m = w["map"]
    m.UpdateOnDevice(w["scan"][:5000], w["T_gt"])
    assert m.resident()
    q = np.ascontiguousarray(w["scan"][:10000], dtype=np.float64)
    qt = torch.from_numpy(q).cuda()
    rng = np.random.default_rng(29)
    poses = np.tile(np.asarray(w["T_gt"], dtype=np.float64), (256, 1))
    poses[:, :4] += rng.uniform(-0.02, 0.02, size=(256, 4))
    poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1)[:, None]
    poses[:, 4:] += rng.uniform(-1.0, 1.0, size=(256, 3))
    torch.cuda.synchronize()
    lines = ["%d-row frame, map of %d points, resident; max_dist %g, kernel %g, sem_th %g; median of %d alternating "
             "repetitions after %d, ms" % (len(q), m.size(), md, kernel, th, a.calls, a.warmup)]
    for k in (256, 64, 16, 4, 1):
        got = {}

        def one():
            got["batch"] = m.ScorePoses(qt, poses[:k], md, kernel, th)

        def route():
            got["single"] = [m.RegistrationQuality(qt, md, kernel, th, pose=poses[c]) for c in range(k)]
        tb, tr = [], []
        for i in range(a.warmup + a.calls):
            for fn, acc in ((one, tb), (route, tr)) if i % 2 == 0 else ((route, tr), (one, tb)):
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    acc.append(dt)
        assert m.resident()
        for c in range(k):
            for f in SHARED:
                v = getattr(got["single"][c], f)
                v = np.array(v[:], dtype=np.float64).reshape(got["batch"][f][c].shape) if hasattr(v, "_length_") else v
                assert np.asarray(got["batch"][f][c]).tobytes() == np.asarray(v, dtype=got["batch"][f].dtype).tobytes(), (c, f)
        lines.append("K = %d (pairs of candidate 0: %d)" % (k, got["batch"]["n_pairs"][0]))
        lines.append(line("sageicp_score_poses_device, one call", tb))
        lines.append(line("sageicp_registration_quality_device, %d calls" % k, tr))
        lines.append("  ratio of the medians: %.2f" % (np.median(tr) / np.median(tb)))
    return lines


def relocalize(a):
    m = sage.VoxelHashMap(0.8, 100.0)
    m.AddPoints(syn.sample_surfaces(np.random.default_rng(0xC1), 35000, 60.0))
    T = syn.pose_from_rpy_t([0.0, 0.0, 25.0], [4.0, -3.0, 0.0])
    rows = syn.make_scan(np.random.default_rng(5), 2000, 60.0, T)
    grid = dict(xy=(6.0, 2.0), z=(0.0, 0.0), yaw=(math.radians(30.0), math.radians(5.0)))
    prior = sage.IDENTITY
    rt = torch.from_numpy(rows).cuda()
    wall, score, refine = [], [], []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        pose, q, info = m.Relocalize(rt, prior, 6.0, 2.0 / 3.0, 0.4, refine_top=3, **grid)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(dt)
            score.append(info["us_score"] / 1e3)
            refine.append(info["us_refine"] / 1e3)
    d = float(np.linalg.norm(pose[4:] - T[4:]))
    return ["Relocalize: %d-row scan, map of %d points at 0.8 m, %d candidates, refine_top 3; ends %.4f m from T_gt "
            "(candidate %d, rank %d, %d iterations); ms" % (len(rows), m.size(), info["candidates"], d, info["best_candidate"],
                                                             info["winner_rank"], info["iterations"]),
            line("Relocalize, wall (Python)", wall), line("us_score", score), line("us_refine", refine)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29"))
    a = ap.parse_args()
    if sage.device_count() < 1:
        raise SystemExit("no HIP device: this probe measures the GPU path only")
    text = "\n".join(batch(a) + relocalize(a)) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "score_probe.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
