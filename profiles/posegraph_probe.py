"""The pose-graph optimiser, device against host (results in profiles/r39/).

  python profiles/posegraph_probe.py sizes [calls]   n in {4 000, 36 000, 360 000} x c in {1, 8, 64}: where = 2 against where = 1
                                                     in the same run, host clock around synchronous calls, 3 warm-up calls,
                                                     medians and ranges of `calls` (30) calls; one JSON line per size
  python profiles/posegraph_probe.py trace           a few device calls of two sizes, to be run under
                                                     rocprofv3 --kernel-trace --stats (a run of its own)
  python profiles/posegraph_probe.py --robust [calls] [plain]   DESIGN.md D20 (results in profiles/r41/): 4 000 poses with c = 1
                                                     and 36 000 with c = 64, device, ITER iterations per call, 3 warm-up calls,
                                                     medians and ranges of `calls` (30): the plain entry, Cauchy without
                                                     anneal, and a Geman-McClure call with anneal run to its end (its total;
                                                     more iterations by design).  `plain`: the plain entry alone — what the
                                                     parent commit can run, for the comparison across commits

The scene: two laps of a ring driven in steps of 1 m, odometry that wanders (1 cm, 0.2 mrad per step), c closures that
join a place of lap one to the same place of lap two, spread over the lap.  At 360 000 poses the steps are 1 cm (and the
wander a hundredth): with steps of 1 m the chain's normal matrix is not positive definite to fp64 in the host path's order of
elimination and it refuses the call; what a call costs does not depend on the values.  A timed call runs exactly ITER Gauss-Newton
iterations on both paths (max_iterations = ITER, step_tol = 0), so that the two do the same work; one more call per size
runs to the end and is reported as it ends (status, iterations, F).  The host path is the yardstick: the parent commit has
no route to these numbers.  The host is given fewer calls where one takes long (at least 3; the count is in the output)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch                                      # noqa: E402,F401  (before the library: one HIP runtime in the process)
import sage_icp_amd as sage                       # noqa: E402
import graphscenes as gs                          # noqa: E402

ITER = 3


def drive(n, c, seed=11):
    lap = (n - 1) // 2
    step = 1.0 if n <= 100000 else 0.01
    truth = gs.circle_truth(n, step * lap / (2.0 * np.pi), per_lap=lap)
    poses = gs.wander(truth, seed, trans=0.01 * step, rot=2e-4 * step)
    starts = np.unique(np.linspace(0, lap, c + 2).astype(int)[1:-1]) if c > 1 else np.array([lap // 2])
    closures = [(int(a), int(a) + lap, gs.rel(truth, int(a), int(a) + lap), 4.0 * gs.ODOM_INFO) for a in starts[:c]]
    s = dict(poses=poses, truth=truth, odom_info=gs.ODOM_INFO, closures=closures)
    return s, gs.edges(sage, s)


def timed(fn, calls, warm):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(calls):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def stats(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), calls=len(ms))


def cmd_sizes(calls):
    for n in (4000, 36000, 360000):
        for c in (1, 8, 64):
            s, E = drive(n, c)
            run = lambda where, **kw: sage.graph_optimize(s["poses"], E, s["odom_info"], where=where, return_info=True, **kw)
            fixed = dict(max_iterations=ITER, step_tol=0.0)
            t = time.perf_counter()
            _, hout, hinfo = run("host", **fixed)
            one_host = (time.perf_counter() - t) * 1e3
            dev = timed(lambda: run("device", **fixed), calls, 3)
            if one_host > 1000.0:                            # a slow host call: three in all, the first among them
                host = [one_host] + timed(lambda: run("host", **fixed), 2, 0)
            else:
                host = timed(lambda: run("host", **fixed), int(max(3, min(calls, 20000.0 / one_host))), 3)
            _, dout, dinfo = run("device", **fixed)
            try:
                finfo = run("device")[2]
            except sage.SageIcpError as e:
                finfo = str(e)
            line = dict(n=n, c=len(E), iterations_timed=ITER, device=stats(dev), host=stats(host),
                        ratio=round(float(np.median(dev) / np.median(host)), 4),
                        device_vs_host_after_timed=float(np.abs(dout - hout).max()), timed_info_device=dinfo, timed_info_host=hinfo,
                        to_the_end_device=finfo)
            print(json.dumps(line), flush=True)


def cmd_trace():
    for n, c in ((36000, 8), (360000, 64)):
        s, E = drive(n, c)
        for _ in range(3):
            sage.graph_optimize(s["poses"], E, s["odom_info"], where="device", max_iterations=ITER, step_tol=0.0)
    print(json.dumps(dict(traced=[[36000, 8], [360000, 64]], calls_of_each=3, iterations=ITER)))


def cmd_robust(calls, plain_only):
    for n, c in ((4000, 1), (36000, 64)):
        s, E = drive(n, c)
        fixed = dict(max_iterations=ITER, step_tol=0.0)
        run = lambda **kw: sage.graph_optimize(s["poses"], E, s["odom_info"], where="device", return_info=True, **kw)
        plain = timed(lambda: run(**fixed), calls, 3)
        line = dict(n=n, c=len(E), iterations_timed=ITER, plain=stats(plain), plain_per_iteration_ms=round(float(np.median(plain)) / ITER, 3))
        if not plain_only:
            cauchy = timed(lambda: run(robust=dict(kernel="cauchy"), **fixed), calls, 3)
            again = timed(lambda: run(**fixed), calls, 0)        # the plain entry once more, after: the run's own drift
            anneal = timed(lambda: run(robust=dict(kernel="gm", anneal=1)), calls, 3)
            info = run(robust=dict(kernel="gm", anneal=1))[2]
            line.update(cauchy=stats(cauchy), cauchy_per_iteration_ms=round(float(np.median(cauchy)) / ITER, 3), plain_again=stats(again),
                        cauchy_info=run(robust=dict(kernel="cauchy"), **fixed)[2]["iterations"],
                        gm_anneal_to_the_end=stats(anneal), gm_anneal_iterations=info["iterations"], gm_anneal_stages=info["stages"],
                        gm_anneal_status=info["status"], gm_anneal_outliers=info["outliers"])
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "sizes"
    if what == "--robust":
        rest = sys.argv[2:]
        cmd_robust(int(next((a for a in rest if a.isdigit()), 30)), "plain" in rest)
    elif what == "sizes":
        cmd_sizes(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
    elif what == "trace":
        cmd_trace()
    else:
        sys.exit(__doc__)
