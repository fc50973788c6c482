"""What the registration quality report costs (csrc/quality.hip).  Written to <out>/quality_probe_<what>.txt; a host clock
around each synchronous call, the median of --calls calls after --warmup and their range.

  --what entry     c2's shape (synthetic.make_workload("c2"): 120 k queries, a 1 M-point map made resident by one device
                   update), the frame a float64 (n, 4) tensor on the GPU.  One sageicp_registration_quality_device call
                   against the only route to the same numbers without it: sageicp_get_correspondences_device, the
                   download of both sides, sageicp_align_clouds on the pairs (JTJ and JTr; the histograms, fitness and
                   rmse would still be the caller's to build from the downloaded rows: not counted).
  --what pipeline  a c3-style stream (synthetic.make_stream, 30 k points per frame): per frame, the pipeline's icp_s and
                   the wall time of RegisterFrame with the report off and on, alternating frame by frame between two
                   pipelines fed the same frames (poses asserted equal); the difference is the report's cost per frame.

SAGE_TREE=<a checkout> measures that checkout's package and library instead of this tree's (the route only: an older
tree has no quality entry)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(os.environ.get("SAGE_TREE", ROOT))
sys.path.insert(0, TREE)
import torch                                                    # noqa: E402  (before the library: one HIP runtime)
import sage_icp_amd as sage                                     # noqa: E402
from sage_icp_amd import synthetic as syn                       # noqa: E402


def timed(fn, calls, warmup):
    t = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i >= warmup:
            t.append(dt * 1e3)
    return np.array(t)


def line(name, t):
    return "  %-66s %8.3f  (min %.3f, p10 %.3f, p90 %.3f, max %.3f)" % (
        name, np.median(t), t.min(), np.percentile(t, 10), np.percentile(t, 90), t.max())


def entry(a):
    w = syn.make_workload("c2", lambda: sage.VoxelHashMap(1.0, 1e6))
    p = syn.PARAMS["cold"]
    md, kernel, th = p["max_dist"], p["kernel"], p["sem_th"]
    m = w["map"]
    m.UpdateOnDevice(w["scan"][:5000], w["T_gt"])
    assert m.resident()
    q = np.ascontiguousarray(w["scan"], dtype=np.float64)
    qt = torch.from_numpy(q).cuda()
    pose = np.ascontiguousarray(w["T_gt"], dtype=np.float64)
    torch.cuda.synchronize()
    lines = ["tree %s; c2: %d queries, map of %d points, resident; max_dist %g, kernel %g, sem_th %g; median of %d calls "
             "after %d, ms" % ("this" if TREE == ROOT else "SAGE_TREE", len(q), m.size(), md, kernel, th, a.calls, a.warmup)]
    got = {}

    def route():
        src, tgt = m.GetCorrespondences(qt, md, th, pose=pose)
        s, g = src.cpu().numpy(), tgt.cpu().numpy()
        _, got["JTJ"], got["JTr"] = sage.align_clouds(s, g, kernel)
        got["pairs"] = len(s)
    t = timed(route, a.calls, a.warmup)
    lines.append(line("GetCorrespondences (device) + download + align_clouds (%d pairs)" % got["pairs"], t))
    if hasattr(m, "RegistrationQuality"):
        def one():
            got["q"] = m.RegistrationQuality(qt, md, kernel, th, pose=pose)
        t = timed(one, a.calls, a.warmup)
        assert m.resident()
        r = got["q"]
        d = r.as_dict()
        assert r.n_pairs == got["pairs"]
        rel = np.abs(d["JTJ"] - got["JTJ"]).max() / np.abs(got["JTJ"]).max()
        lines.append(line("RegistrationQuality (device) (%d pairs)" % r.n_pairs, t))
        lines.append("  fitness %.4f rmse %.4f step_norm %.3e covariance_valid %d; JTJ against the route's: %.1e of its largest entry"
                     % (r.fitness, r.rmse, r.step_norm, r.covariance_valid, rel))
    return lines


def pipeline(a):
    frames, _ = syn.make_stream(11, a.calls + a.warmup, points_per_frame=30000)
    cfg = sage.make_pipeline_config()
    off, on = sage.SageICP(cfg), sage.SageICP(cfg)
    on.set_quality(True)
    rows = []
    for k, f in enumerate(frames):
        t = {}
        for name, p in ((("off", off), ("on", on)) if k % 2 == 0 else (("on", on), ("off", off))):
            t0 = time.perf_counter()
            out = p.RegisterFrame(f)
            t[name] = ((time.perf_counter() - t0) * 1e3, out[1] * 1e3, out[0])
        assert np.array_equal(t["off"][2], t["on"][2]), "frame %d" % k
        if k >= a.warmup:
            rows.append((t["off"][0], t["on"][0], t["off"][1], t["on"][1], on.quality().n_queries))
    r = np.array(rows)
    lines = ["tree this; c3-style stream, 30000 points per frame, %d frames after %d; ms per frame (source cloud: %d..%d rows)"
             % (len(r), a.warmup, r[:, 4].min(), r[:, 4].max()),
             line("RegisterFrame wall, report off", r[:, 0]), line("RegisterFrame wall, report on", r[:, 1]),
             line("the report's cost per frame (on - off, frame by frame)", r[:, 1] - r[:, 0]),
             line("icp_s, report off", r[:, 2]), line("icp_s, report on (the report runs outside it)", r[:, 3])]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=["entry", "pipeline"])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28"))
    a = ap.parse_args()
    if sage.device_count() < 1:
        raise SystemExit("no HIP device: this probe measures the GPU path only")
    lines = entry(a) if a.what == "entry" else pipeline(a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "quality_probe_%s%s.txt" % (a.what, "" if TREE == ROOT else "_parent")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
