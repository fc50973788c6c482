"""Per-frame cost of the pipeline's deskew (csrc/deskew.hip): a stream of skewed ring frames (synthetic_skew, ~131k
points) registered by two pipelines in one process, deskew on (timestamped entry) and off (plain entry), frame by frame
alternately, and once more with the deskew-off pipeline using prefetch (what a deskewed stream gives up).  Prints the
median per-frame wall time of each.  Run under rocprofv3 --kernel-trace --stats (program after --) for k_deskew's
device time."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sage_icp_amd as sage                                     # noqa: E402
from sage_icp_amd import synthetic_skew as sk                   # noqa: E402


def main(n_frames=40, warm=5):
    S = sk.make_skewed_stream(n_frames=n_frames, az_steps=3072)
    F = [np.ascontiguousarray(f) for f in S["frames"]]
    T = [np.ascontiguousarray(t) for t in S["timestamps"]]
    print("points per frame: %d..%d" % (min(map(len, F)), max(map(len, F))))
    on = sage.SageICP(sage.make_pipeline_config(deskew=True))
    off = sage.SageICP(sage.make_pipeline_config())
    pf = sage.SageICP(sage.make_pipeline_config())
    t_on, t_off, t_pf, tot_on, tot_off = [], [], [], [], []
    for k in range(n_frames):
        a = time.perf_counter()
        r_on = on.RegisterFrame(F[k], T[k])
        b = time.perf_counter()
        r_off = off.RegisterFrame(F[k])
        c = time.perf_counter()
        if k + 1 < n_frames:
            pf.prefetch(F[k + 1])
        pf.RegisterFrame(F[k])
        d = time.perf_counter()
        if k >= warm:
            t_on.append(b - a); t_off.append(c - b); t_pf.append(d - c)
            tot_on.append(r_on[2]); tot_off.append(r_off[2])
    assert on.deskew_info()[0]
    ms = lambda v: 1e3 * float(np.median(v))                     # noqa: E731
    print("frames measured: %d (after %d warm-up)" % (len(t_on), warm))
    print("deskew on  (timestamped entry): wall %.3f ms  total_seconds %.3f ms" % (ms(t_on), ms(tot_on)))
    print("deskew off (plain entry)      : wall %.3f ms  total_seconds %.3f ms" % (ms(t_off), ms(tot_off)))
    print("deskew off with prefetch      : wall %.3f ms" % ms(t_pf))
    print("extra per frame for deskew    : %.3f ms (wall), %.3f ms (total_seconds)" % (ms(t_on) - ms(t_off),
                                                                                      ms(tot_on) - ms(tot_off)))


if __name__ == "__main__":
    main()
