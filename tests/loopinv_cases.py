"""The cases of tests/test_loop_invariants.py, and the child process that runs them.

    python tests/loopinv_cases.py          one JSON line per case on stdout, in the order of CASES, flushed as it is done

A case registers one small frame three ways — the one-launch loop shaped by the case's knobs, the launch-per-iteration
loop at the same lanes per query and scan form, the oracle — and reports what the test asserts on.  The scenes and the
oracle's registrations are made once per (scene, frame size, initial guess) and shared by the cases that use them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAX_DIST, KERNEL, SEM_TH = 3.0, 1.0 / 3.0, 0.4
N_MAP = 4000
FRAMES = (17, 64, 65, 257, 1000, 4100)
LABELS = (0, 10, 40, 44, 70, 80)


def _case(name, n, lw, filt, scene="plain", guess="identity", **knobs):
    return dict(id=name, n=n, lw=lw, filt=filt, scene=scene, guess=guess, knobs=knobs)


CASES = []
# every frame size at every lanes per query, both scan forms: 1, 2 and 5 units at 16 queries per wave, one short
for _n in FRAMES:
    for _lw in (1, 2, 3, 4):
        for _f in (0, 1):
            CASES.append(_case("n%d-lw%d-filt%d" % (_n, _lw, _f), _n, _lw, _f))
# the units of a workgroup (16 queries per unit at four lanes per query; a launch has 32 workgroups at least):
#   17 units, 2 per workgroup at most: 15 workgroups own none — their waves' dealt first unit is past the end
CASES.append(_case("workgroups-without-units", 257, 2, 1, SAGEICP_LOOP_WAVES=4, SAGEICP_LOOP_GPW=2))
#   63 units over 32 workgroups of up to 3: 31 own two, the last one a single unit — nobody has gpw of them
CASES.append(_case("fewer-units-than-gpw", 1000, 2, 1, SAGEICP_LOOP_WAVES=4, SAGEICP_LOOP_GPW=3))
#   one unit per workgroup: nblk <= BPW, the blocks keep the frame's order
CASES.append(_case("no-reordering", 257, 2, 0, SAGEICP_LOOP_WAVES=1, SAGEICP_LOOP_GPW=1))
#   257 units, 8 or 9 per workgroup: 32 / 36 blocks, the closing wave's rank sort
CASES.append(_case("rank-sort", 4100, 2, 1, SAGEICP_LOOP_WAVES=4, SAGEICP_LOOP_GPW=9))
CASES.append(_case("rank-sort-8-lanes", 4100, 3, 0, SAGEICP_LOOP_WAVES=4, SAGEICP_LOOP_GPW=5))
#   more than 64 blocks per workgroup needs 65 x 32 units of four queries: 2,100 units, 65 or 66 per workgroup, no sort
CASES.append(_case("more-than-64-blocks", 8400, 4, 1, SAGEICP_LOOP_WAVES=4, SAGEICP_LOOP_GPW=66))
for _w in (1, 4, 8):
    for _lw in (2, 3):
        CASES.append(_case("waves%d-lw%d" % (_w, _lw), 1000, _lw, 1, SAGEICP_LOOP_WAVES=_w, SAGEICP_LOOP_GPW=2))
# a guess 1.5 voxels off on every axis: the first iterations rebuild rows after face, edge and corner crossings
for _lw in (2, 3):
    for _f in (0, 1):
        CASES.append(_case("guess-off-lw%d-filt%d" % (_lw, _f), 1000, _lw, _f, guess="off"))
# coordinates of kilometres, queries within and just outside the slack of a voxel face (1e-9 vs + 1e-13 |x|)
for _lw in (2, 3):
    for _f in (0, 1):
        CASES.append(_case("face-slack-lw%d-filt%d" % (_lw, _f), 1000, _lw, _f, scene="faces"))
# nothing in reach: every accumulator word is cleared and sent with zeros
for _lw in (2, 3):
    CASES.append(_case("no-correspondence-lw%d" % _lw, 257, _lw, 1, scene="far"))
IDS = [c["id"] for c in CASES]
assert len(set(IDS)) == len(IDS)


def make_scene(oracle, syn, scene, n, guess):
    """-> voxel size, map points, frame, initial guess"""
    rng = np.random.default_rng(21000 + n)
    vs = 0.8 if scene == "faces" else 1.0
    centre = np.array([4321.0, -2750.0, 12.0]) if scene == "faces" else np.zeros(3)
    mp = rng.uniform(-7.0, 7.0, size=(N_MAP, 4))
    mp[:, 2] *= 0.25
    mp[:, :3] += centre
    mp[:, 3] = rng.choice(LABELS, size=N_MAP)
    pick = rng.integers(0, N_MAP, size=n)
    frame = mp[pick].copy()
    frame[:, :3] += rng.normal(size=(n, 3)) * 0.03
    init = np.array(oracle.IDENTITY, dtype=np.float64)
    if scene == "faces":
        # the first iteration runs at the identity: the queries ARE the frame.  Every query sits on a face of its voxel
        # on one axis at least — exactly, 5e-10 inside or outside it (the slack there is 0.8e-9 + 1e-13 x 4321 = 1.2e-9
        # on x: the slack decides), or 3e-9 away (it does not)
        k = np.round(frame[:, :3] / vs)
        on = rng.integers(0, 8, size=n)
        delta = rng.choice([0.0, 5e-10, -5e-10, 3e-9, -3e-9], size=(n, 3))
        for a in range(3):
            sel = (on >> a) & 1 == 1
            frame[sel, a] = k[sel, a] * vs + delta[sel, a]
    elif scene == "far":
        frame[:, :3] += 5000.0
    else:
        true = syn.pose_from_rpy_t([0.01, -0.005, 0.02], [0.25, -0.15, 0.05])
        frame = np.ascontiguousarray(oracle.transform_points(oracle.se3_inv(true), frame))
        if guess == "off":
            init = syn.pose_from_rpy_t([0.01, -0.005, 0.02], [0.25 + 1.5 * vs, -0.15 - 1.5 * vs, 0.05 + 1.5 * vs])
    return vs, mp, np.ascontiguousarray(frame), np.asarray(init, dtype=np.float64)


def crossings(oracle, om, frame, init, vs, iterations):
    """queries whose home voxel moved to a neighbour through a face / an edge / a corner between two consecutive
    iterations of the oracle (summed over the first iterations), and those that jumped further"""
    def index(pose):
        return np.trunc(oracle.transform_points(pose, frame)[:, :3] / vs).astype(np.int64)
    out = {"face": 0, "edge": 0, "corner": 0, "jump": 0}
    prev = index(init)
    for it in range(1, iterations + 1):
        pose, _ = om.register_frame(frame, init, MAX_DIST, KERNEL, SEM_TH, max_iter=it)
        cur = index(pose)
        d = np.abs(cur - prev)
        near = d.max(axis=1) == 1
        axes = (d != 0).sum(axis=1)
        out["face"] += int((near & (axes == 1)).sum())
        out["edge"] += int((near & (axes == 2)).sum())
        out["corner"] += int((near & (axes == 3)).sum())
        out["jump"] += int((d.max(axis=1) > 1).sum())
        prev = cur
    return out


class Env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


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
            cross = crossings(oracle, om, frame, init, vs, min(ost.iterations, 10)) if c["guess"] == "off" else None
            shared[key] = (vs, frame, init, om, gm, opose, ost, cross, om.size() == gm.size())
        vs, frame, init, om, gm, opose, ost, cross, same_map = shared[key]
        with Env(SAGEICP_LOOP=2, SAGEICP_LW=c["lw"], SAGEICP_FILTER=c["filt"], **c["knobs"]):
            b, sb = sage.register_frame(frame, gm, init, MAX_DIST, KERNEL, SEM_TH, return_stats=True)
        status = gm.loop_status()
        with Env(SAGEICP_LOOP=0, SAGEICP_LW=c["lw"], SAGEICP_FILTER=c["filt"]):
            a, sa = sage.register_frame(frame, gm, init, MAX_DIST, KERNEL, SEM_TH, return_stats=True)
        e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(opose), b))
        print(json.dumps(dict(
            id=c["id"], same_map=bool(same_map),
            single_launch=[int(sb.single_launch), int(sa.single_launch)], lanes=[int(sb.lanes_per_query), int(sa.lanes_per_query)],
            compact=[int(sb.compact_scan), int(sa.compact_scan)], timeouts=int(status.timeouts), last_fallback=int(status.last_fallback),
            same_pose=bool(np.array_equal(a, b)), pose_is_guess=bool(np.array_equal(b, init)),
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
