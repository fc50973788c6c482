"""The cases of tests/test_loop_staging.py, and the child process that runs them.

    python tests/loopstage_cases.py        one JSON line per case on stdout, in the order of CASES, flushed as it is done

As tests/loopinv_cases.py (whose scenes, environment switch and crossing count are used here): a case registers one small
frame with the one-launch loop shaped by the case's knobs, with the launch-per-iteration loop at the same lanes per query
and scan form, and with the oracle.  The shapes are chosen for the control flow of the staged first pass (loop_kernel.h):
a launch has 32 workgroups at least, a unit is 64 >> lw queries."""
import json
import os
import sys
import time

import numpy as np

import loopinv_cases as base

ROOT = base.ROOT
MAX_DIST, KERNEL, SEM_TH = base.MAX_DIST, base.KERNEL, base.SEM_TH


def _case(name, n, lw, filt, scene="plain", guess="identity", **knobs):
    return dict(id=name, n=n, lw=lw, filt=filt, scene=scene, guess=guess, knobs=knobs)


W4 = dict(SAGEICP_LOOP_WAVES=4)
CASES = []
# waves that outnumber their workgroup's units stage nothing and go to the counter behind the barrier; most workgroups
# own no unit at all (17 queries: 2 units at four lanes per query, 63: 4) — at every lanes per query
for _n in (17, 63):
    for _lw in (1, 2, 3, 4):
        CASES.append(_case("few-units-n%d-lw%d" % (_n, _lw), _n, _lw, 1, SAGEICP_LOOP_GPW=2, **W4))
# exactly one unit per wave: 32 workgroups x waves x 16 queries — every pass is a staged one, the counter hands out nothing
CASES.append(_case("one-unit-per-wave-4", 32 * 4 * 16, 2, 1, SAGEICP_LOOP_GPW=4, **W4))
CASES.append(_case("one-unit-per-wave-8", 32 * 8 * 16, 2, 0, SAGEICP_LOOP_WAVES=8, SAGEICP_LOOP_GPW=8))
# units beyond one per wave are staged behind a run: 80 queries (5 units) per workgroup of four waves, at 2, 4, 8 and 16
# lanes per query and both scan forms (fewer, larger units at two lanes; more at eight and sixteen) ...
for _lw in (1, 2, 3, 4):
    for _f in (0, 1):
        CASES.append(_case("second-units-lw%d-filt%d" % (_lw, _f), 32 * 80, _lw, _f, SAGEICP_LOOP_GPW=5 << max(_lw - 2, 0), **W4))
# ... and one wave per workgroup with three units: one staged in front of the wait, two behind a run
CASES.append(_case("one-wave-three-units", 32 * 3 * 16, 2, 1, SAGEICP_LOOP_WAVES=1, SAGEICP_LOOP_GPW=3))
CASES.append(_case("one-wave-three-units-8-lanes", 32 * 3 * 8, 3, 0, SAGEICP_LOOP_WAVES=1, SAGEICP_LOOP_GPW=3))
# no dealt first unit at all: nobody stages in front of the wait, every unit comes from the counter
CASES.append(_case("no-deal", 32 * 80, 2, 1, SAGEICP_LOOP_GPW=5, SAGEICP_LOOP_DEAL=0, **W4))
CASES.append(_case("no-priorities", 32 * 80, 2, 1, SAGEICP_LOOP_GPW=5, SAGEICP_LOOP_PRIO=0, **W4))
# the loop ends right after a stage: nothing in reach (one iteration), a frame of map points a tenth of a millimetre off
# their places (two)
for _scene in ("far", "near"):
    for _lw in (2, 3):
        CASES.append(_case("short-%s-lw%d" % (_scene, _lw), 257, _lw, 1, scene=_scene, SAGEICP_LOOP_GPW=2, **W4))
# a guess 1.5 voxels off on every axis: the first passes rebuild rows from staged keys through faces, edges and corners —
# in staged first passes and in passes staged behind a run
for _lw in (2, 3):
    for _f in (0, 1):
        CASES.append(_case("guess-off-lw%d-filt%d" % (_lw, _f), 1000, _lw, _f, guess="off"))
# (96 queries, 6 units, per workgroup: at this size the oracle's first iterations hold a corner crossing; at 80 they do not)
CASES.append(_case("guess-off-second-units", 32 * 96, 2, 1, guess="off", SAGEICP_LOOP_GPW=6, **W4))
IDS = [c["id"] for c in CASES]
assert len(set(IDS)) == len(IDS)


def make_scene(oracle, syn, scene, n, guess):
    """base.make_scene, and a scene of its own: "near" — the frame is a subset of the map moved by a tenth of a millimetre"""
    if scene != "near":
        return base.make_scene(oracle, syn, scene, n, guess)
    vs, mp, _, init = base.make_scene(oracle, syn, "plain", n, "identity")
    rng = np.random.default_rng(22000 + n)
    frame = mp[rng.choice(base.N_MAP, size=n, replace=False)].copy()
    frame = oracle.transform_points(oracle.se3_inv(syn.pose_from_rpy_t([0.0, 0.0, 0.0], [1e-4, -1e-4, 5e-5])), frame)
    return vs, mp, np.ascontiguousarray(frame), init


def main():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import oracle
    import sage_icp_amd as sage
    from sage_icp_amd import synthetic as syn
    oracle.lib()
    shared = {}
    for c in CASES:
        t0 = time.time()
        key = (c["scene"], c["n"], c["guess"])
        if key not in shared:
            vs, mp, frame, init = make_scene(oracle, syn, *key)
            om = oracle.Map(vs, 100.0)
            om.add_points(mp)
            gm = sage.VoxelHashMap(vs, 100.0, device=0)
            gm.AddPoints(mp)
            opose, ost = om.register_frame(frame, init, MAX_DIST, KERNEL, SEM_TH)
            cross = base.crossings(oracle, om, frame, init, vs, min(ost.iterations, 10)) if c["guess"] == "off" else None
            shared[key] = (frame, init, gm, opose, ost, cross, om.size() == gm.size())
        frame, init, gm, opose, ost, cross, same_map = shared[key]
        with base.Env(SAGEICP_LOOP=2, SAGEICP_LW=c["lw"], SAGEICP_FILTER=c["filt"], **c["knobs"]):
            b, sb = sage.register_frame(frame, gm, init, MAX_DIST, KERNEL, SEM_TH, return_stats=True)
        status = gm.loop_status()
        with base.Env(SAGEICP_LOOP=0, SAGEICP_LW=c["lw"], SAGEICP_FILTER=c["filt"]):
            a, sa = sage.register_frame(frame, gm, init, MAX_DIST, KERNEL, SEM_TH, return_stats=True)
        e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(opose), b))
        print(json.dumps(dict(
            id=c["id"], same_map=bool(same_map),
            single_launch=[int(sb.single_launch), int(sa.single_launch)], lanes=[int(sb.lanes_per_query), int(sa.lanes_per_query)],
            compact=[int(sb.compact_scan), int(sa.compact_scan)], timeouts=int(status.timeouts), last_fallback=int(status.last_fallback),
            same_pose=bool(np.array_equal(a, b)),
            iterations=[int(sb.iterations), int(sa.iterations), int(ost.iterations)],
            converged=[int(sb.converged), int(sa.converged), int(ost.converged)],
            hist=[list(map(int, sb.n_corr_hist)), list(map(int, sa.n_corr_hist))],
            n_corr=[[int(sb.n_corr_first), int(sb.n_corr_last)], [int(sa.n_corr_first), int(sa.n_corr_last)],
                    [int(ost.n_corr_first), int(ost.n_corr_last)]],
            step=[float(sb.last_step_norm).hex(), float(sa.last_step_norm).hex()],
            candidates=[int(sb.sum_candidates), int(sa.sum_candidates), int(ost.sum_candidates_total)],
            dt=float(np.linalg.norm(e[:3])), dr=float(np.linalg.norm(e[3:])), crossings=cross,
            seconds=round(time.time() - t0, 3))), flush=True)


if __name__ == "__main__":
    main()
