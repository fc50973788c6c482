"""What GetCorrespondences costs a caller whose frame is on the GPU and whose map is resident (csrc/correspond.hip,
sageicp_get_correspondences_device), against the host entry it had to use before.  Scene: c2's
(synthetic.make_workload("c2"): 120 k queries, a 1 M-point map), the map made resident by one device update.  Written
to <out>/correspond_probe_<entry>.txt; a host clock around each synchronous call, the median of --calls calls after
--warmup and their spread.

  --entry device   VoxelHashMap.GetCorrespondences(tensor, ..., with_index=True): the frame a float64 (n, 4) tensor, the
                   answers fresh tensors.  The map is resident before and after every call.
  --entry host     VoxelHashMap.GetCorrespondences(numpy rows, ..., with_index=True) on a RESIDENT map — every call gets
                   a fresh device-to-device clone of the same resident map, made outside the clock — plus what the call
                   leaves to be paid: it downloads the map and makes the host copy the authority, so the next search has
                   to mirror it again (sync(), inside the clock).  Host rows in and out: the tensor's trip through numpy
                   is not counted (it is shown on a line of its own).  Also: the same call on a map that is only
                   mirrored, where nothing is downloaded.

SAGE_TREE=<a checkout> measures that checkout's package and library instead of this tree's: the host entry on the
parent commit is `SAGE_TREE=<parent checkout> python profiles/correspond_probe.py --entry host`."""
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


def timed(fn, calls, warmup, before=lambda: None):
    """ms per call of fn(before()): `before` runs outside the clock"""
    t = []
    for i in range(warmup + calls):
        arg = before()
        t0 = time.perf_counter()
        fn(arg)
        dt = time.perf_counter() - t0
        if i >= warmup:
            t.append(dt * 1e3)
    return np.array(t)


def line(name, t):
    return "  %-62s %8.3f  (min %.3f, p10 %.3f, p90 %.3f, max %.3f)" % (
        name, np.median(t), t.min(), np.percentile(t, 10), np.percentile(t, 90), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", required=True, choices=["device", "host"])
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27"))
    a = ap.parse_args()
    if sage.device_count() < 1:
        raise SystemExit("no HIP device: this probe measures the GPU path only")
    w = syn.make_workload("c2", lambda: sage.VoxelHashMap(1.0, 1e6))
    p = syn.PARAMS["cold"]
    md, th = p["max_dist"], p["sem_th"]
    m = w["map"]
    m.UpdateOnDevice(w["scan"][:5000], w["T_gt"])
    assert m.resident()
    q = np.ascontiguousarray(w["scan"], dtype=np.float64)
    qt = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    lines = ["%s entry, tree %s; c2: %d queries, map of %d points, resident; max_dist %g, sem_th %g; median of %d calls "
             "after %d, ms" % (a.entry, "this" if TREE == ROOT else "SAGE_TREE", len(q), m.size(), md, th, a.calls, a.warmup)]
    if a.entry == "device":
        k = [0]

        def dev(_):
            k[0] = len(m.GetCorrespondences(qt, md, th, with_index=True)[2])
        t = timed(dev, a.calls, a.warmup)
        assert m.resident()
        lines.append(line("device entry, tensors in and out (%d pairs)" % k[0], t))
        t = timed(lambda _: m.GetCorrespondences(qt, md, th, with_index=True, dtype=torch.float32), a.calls, a.warmup)
        lines.append(line("device entry, float32 answers", t))
    else:
        k = [0]

        def host(c):
            k[0] = len(c.GetCorrespondences(q, md, th, with_index=True)[2])
            c.sync()

        def fresh():
            c = m.clone()
            assert c.resident()
            return c
        t = timed(host, a.calls, a.warmup, before=fresh)
        lines.append(line("host entry on a resident map + the re-mirror it leaves (%d pairs)" % k[0], t))

        def through_numpy(c):
            src, tgt, idx = c.GetCorrespondences(qt.cpu().numpy(), md, th, with_index=True)
            c.sync()
            return torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(idx).cuda()
        t = timed(through_numpy, a.calls, a.warmup, before=fresh)
        lines.append(line("... with the tensor's trip through numpy and back", t))
        c = m.clone()
        c.GetCorrespondences(q, md, th)                 # handed back: from here on a host map with a mirror
        assert not c.resident()
        t = timed(lambda _: c.GetCorrespondences(q, md, th, with_index=True), a.calls, a.warmup)
        lines.append(line("host entry on a map that is only mirrored (no download)", t))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "correspond_probe_%s%s.txt" % (a.entry, "" if TREE == ROOT else "_parent")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
