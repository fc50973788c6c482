"""The cases of tests/test_loop_deal.py's GPU half, and the child process that runs them.

    python tests/loopdeal_cases.py        one JSON line per case on stdout, in the order of CASES, flushed as it is done

Which unit a wave of the one-launch loop takes first (csrc/loop_deal.h) must not reach a bit of the result.  The table's
rows are those of a CU's fifth to seventh workgroup: they run only when the grid has more than 1,024 workgroups (256 CUs x
4).  The smallest frames that get there: 16 lanes per query forced (SAGEICP_LW=4: a unit is four queries, a workgroup of
four waves sixteen), 20 k to 27 k points.  One map of 4,000 points, one frame of 27,000, every case a prefix of it.  A
case registers its prefix with SAGEICP_LOOP_DEAL = 1 (table), 2 (formula), 0 (no deal) in the one-launch loop and with the
launch-per-iteration loop at the same lanes per query; SAGEICP_LOOP_DEBUG=1 gives the plan of the first."""
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

import loopinv_cases as base

ROOT = base.ROOT
MAX_DIST, KERNEL, SEM_TH = base.MAX_DIST, base.KERNEL, base.SEM_TH
N_FRAME = 27000


def _case(name, n, wgs, nw, gpw, **knobs):
    return dict(id=name, n=n, plan=[16, wgs, nw, gpw], knobs=knobs)


# (plan_loop, capi_run.hip: one unit per wave while round32(units / 4) workgroups fit 1,680 slots, else 1,664 workgroups
# with up to five units)
CASES = [
    # 1,024 workgroups, four per CU: slots 0-3 only, the parent's deal by construction
    _case("four-per-cu", 16384, 1024, 4, 4),
    # 1,280 workgroups: every CU holds a fifth workgroup — row 4
    _case("five-per-cu", 20480, 1280, 4, 4),
    # 5,125 units on 1,312 workgroups: 123 of them own three units — a wave dealt rank 3 there finds no unit
    _case("fewer-units-than-waves", 20500, 1312, 4, 4),
    # 1,664 workgroups, six or seven per CU: rows 4-6, every wave one unit
    _case("seven-per-cu", 26624, 1664, 4, 4),
    # ... and the frame's last unit holds two queries
    _case("partial-last-unit", 26622, 1664, 4, 4),
    # 6,750 units on 1,664 workgroups: 94 own a fifth unit, which goes by the counter
    _case("fifth-units", 27000, 1664, 4, 5),
    # eight waves per workgroup: the formula deals
    _case("eight-waves", 20480, 640, 8, 8, SAGEICP_LOOP_WAVES=8),
]
IDS = [c["id"] for c in CASES]
SETTINGS = [dict(SAGEICP_LOOP=2, SAGEICP_LOOP_DEAL=1), dict(SAGEICP_LOOP=2, SAGEICP_LOOP_DEAL=2), dict(SAGEICP_LOOP=2, SAGEICP_LOOP_DEAL=0),
            dict(SAGEICP_LOOP=0)]


def make_scene(oracle, syn):
    """-> map points, the frame of N_FRAME points, initial guess: the "plain" scene of loopinv_cases at this size"""
    rng = np.random.default_rng(30000)
    mp = rng.uniform(-7.0, 7.0, size=(base.N_MAP, 4))
    mp[:, 2] *= 0.25
    mp[:, 3] = rng.choice(base.LABELS, size=base.N_MAP)
    frame = mp[rng.integers(0, base.N_MAP, size=N_FRAME)].copy()
    frame[:, :3] += rng.normal(size=(N_FRAME, 3)) * 0.03
    true = syn.pose_from_rpy_t([0.01, -0.005, 0.02], [0.25, -0.15, 0.05])
    frame = np.ascontiguousarray(oracle.transform_points(oracle.se3_inv(true), frame))
    return mp, frame, np.array(oracle.IDENTITY, dtype=np.float64)


class Stderr:
    """the library's own lines on file descriptor 2 while inside"""
    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def main():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import oracle
    import sage_icp_amd as sage
    from sage_icp_amd import synthetic as syn
    mp, frame, init = make_scene(oracle, syn)
    gm = sage.VoxelHashMap(1.0, 100.0, device=0)
    gm.AddPoints(mp)
    for c in CASES:
        t0 = time.time()
        f = np.ascontiguousarray(frame[:c["n"]])
        runs, plan = [], None
        for i, s in enumerate(SETTINGS):
            with base.Env(SAGEICP_LW=4, SAGEICP_LOOP_DEBUG=1 if i == 0 else 0, **s, **c["knobs"]):
                with Stderr() as err:
                    pose, st = sage.register_frame(f, gm, init, MAX_DIST, KERNEL, SEM_TH, return_stats=True)
            status = gm.loop_status()
            if i == 0:
                m = re.search(r"(\d+) lanes/query, (\d+) workgroups of (\d+) waves, <= (\d+) units of (\d+) queries", err.text)
                plan = [int(m.group(k)) for k in (1, 2, 3, 4)] if m else err.text[-300:]
            runs.append(dict(pose=[float(x).hex() for x in np.asarray(pose).ravel()], single_launch=int(st.single_launch),
                             lanes=int(st.lanes_per_query), iterations=int(st.iterations), converged=int(st.converged),
                             hist=list(map(int, st.n_corr_hist)), n_corr=[int(st.n_corr_first), int(st.n_corr_last)],
                             step=float(st.last_step_norm).hex(), candidates=int(st.sum_candidates),
                             timeouts=int(status.timeouts), last_fallback=int(status.last_fallback)))
        print(json.dumps(dict(id=c["id"], plan=plan, runs=runs, seconds=round(time.time() - t0, 3))), flush=True)


if __name__ == "__main__":
    main()
