"""A neighbourhood row that follows its query into a NEIGHBOURING voxel (icp_body.h, SAGE_ROW_SHIFT_LAYER; the index
arithmetic is csrc/row_shift.h, checked on the CPU by tests/test_row_shift_host.py): in the one-launch loop at four lanes
per query the kept words move inside the row, only the new layer is probed, the occupancy mask is the old one shifted
and C_q is re-summed.  What can go wrong: a word moved from or to the wrong place, a new voxel probed twice or not at
all, a mask bit or a count carried across a layer, a seed kept whose voxel left the block, truncated indices around 0.

Every registration is run as the one-launch loop and the launch-per-iteration loop (whose k_icp at four lanes probes all
27 voxels anew and so builds the row independently), at four and eight lanes per query, full records and the compact
scan: ONE pose, n_corr_hist and sum_candidates, to the bit; and the oracle's iterations, converged flag, first and last
correspondence counts and sum_candidates_total, pose within 1e-7.  Before that, on the CPU and by the oracle alone: the
queries do change their home voxel by exactly the shift the case is about between two consecutive iterations
(`_crossings`), so a case that does not produce its crossings fails.

The scene is a lattice of separate neighbourhoods, voxel size 1.  A neighbourhood's queries sit within 0.02 voxel of the
face, edge or corner of their home voxel they are about to cross; their true counterparts in the map lie 0.2 voxel
further on every crossing axis, so the first Gauss-Newton step carries them across.  Kinds of neighbourhood (each in every registration):
  full          the 5 x 5 x 5 voxels around the home hold 0, 1, 4, 5, 8, 9, 16, 17 or 40 points in rotation (every
                storage class; empty voxels in the new layer too), and the queries' true counterparts
  nolayer       only the old 3 x 3 x 3 block is occupied: the whole new layer is empty
  behind        the ONLY occupied voxel lies on the side the query moves away from (case d): the seed's voxel leaves the
                block, the neighbourhood is fully empty after the move and the answer vanishes
  behind_ahead  as `behind`, plus one voxel two steps ahead, which enters with the new layer: the answer changes
`origin` registrations put the homes at index 1, 0 and -1 on one axis each, and at (0, 0, 0): the cell of index 0 is two
voxels wide under truncation, and the crossings go 1 -> 0, 0 -> -1 (negative directions) and back (positive ones).

Two registrations of their own:
  jumps and near moves   the frame is turned by 0.03 rad about z: in ONE iteration the neighbourhoods at radius 10 step
                         0.3 voxel into the next voxel and those at radius 90 jump 2.7 voxels; the frame alternates
                         between them query by query, so every wave runs the new-layer path and the walk side by side
  tombstones, chains     the chain scene of tests/mapscenes.py after three device-side updates (tombstones in a probe
                         chain that wraps from the last slot to slot 0); queries step into the voxel NEXT to a chain
                         voxel, which enters with the new layer and is found through the chain

Needs a real MI355X:  python -m pytest tests -m gpu"""
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 4, 5, 8, 9, 16, 17, 40)
VS, MAX_POINTS = 1.0, 40
MAX_DIST, KERNEL, SEM_TH = 3.0, 1.0 / 3.0, 0.4
LABELS = (40, 70, 0)
PITCH = 6                                   # voxels between two homes: 5 x 5 x 5 blocks do not touch
STEP = 0.2                                  # the frame's offset per crossing axis, voxels
NQ = 8                                      # queries per neighbourhood
FORMS = [(loop, lw, filt) for loop in (1, 0) for lw in (2, 3) for filt in (0, 1)]
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
ORIGIN_DIRECTIONS = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1), (-1, -1, -1), (1, 1, 1)]
KINDS = ["full"] * 18 + ["nolayer"] * 4 + ["behind"] * 4 + ["behind_ahead"] * 4


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


def _index(x):
    """home voxel index of a coordinate: truncation toward zero"""
    return np.trunc(np.asarray(x) / VS).astype(np.int64)


def _lo(k):
    """a unit interval inside the cell of index k: [k, k + 1) for k > 0, (k - 1, k] for k < 0, [0, 1) of (-1, 1) for k = 0"""
    return float(k) if k >= 0 else float(k - 1)


def _upper(k):
    return float(k + 1) if k >= 0 else float(k)      # where index k ends and k + 1 begins


def _lower(k):
    return float(k) if k > 0 else float(k - 1)       # where index k ends and k - 1 begins


def _homes(origin):
    if origin:
        hs = [(0, 0, 0)]
        for axis in range(3):
            for h in (1, 0, -1):
                v = [8 + PITCH * (h + 1)] * 3
                v[(axis + 2) % 3] += 3 * PITCH * axis
                v[axis] = h
                hs.append(tuple(v))
        return hs
    return [(2 + PITCH * (c % 5), 2 + PITCH * ((c // 5) % 5), 2 + PITCH * (c // 25)) for c in range(len(KINDS))]


def _case(d, origin=False):
    """-> map points (insertion order), the frame, the kind of every query"""
    rng = np.random.default_rng(2000 + 27 * (9 * d[0] + 3 * d[1] + d[2]) + (1000 if origin else 0))
    d = np.array(d)
    pts, qs, kinds = [], [], []
    rot = 0
    for c, home in enumerate(_homes(origin)):
        home = np.array(home)
        kind = KINDS[c % len(KINDS)] if not origin else ("full", "full", "nolayer", "behind_ahead")[c % 4]
        # the queries: within 0.02 of the faces they cross, about the middle of the cell on the other axes
        q = np.empty((NQ, 4))
        for a in range(3):
            if d[a] > 0:
                q[:, a] = _upper(home[a]) - rng.uniform(0.005, 0.02, size=NQ)
            elif d[a] < 0:
                q[:, a] = _lower(home[a]) + rng.uniform(0.005, 0.02, size=NQ)
            else:
                q[:, a] = _lo(home[a]) + 0.5 + rng.uniform(-0.05, 0.05, size=NQ)
        q[:, 3] = rng.choice((40, 70, 0, 10), size=NQ)
        assert (_index(q[:, :3]) == home).all()
        qs.append(q)
        kinds += [kind] * NQ
        for off in itertools.product(range(-2, 3), repeat=3):
            off = np.array(off)
            inner = np.abs(off).max() <= 1
            if kind == "full":
                n = COUNTS[(rot + 25 * (off[0] + 2) + 5 * (off[1] + 2) + off[2] + 2) % len(COUNTS)]
            elif kind == "nolayer":
                n = COUNTS[1 + (rot + 9 * off[0] + 3 * off[1] + off[2]) % (len(COUNTS) - 1)] if inner else 0
            elif kind == "behind":
                n = COUNTS[1 + rot % (len(COUNTS) - 1)] if (off == -d).all() else 0
            else:
                n = COUNTS[1 + rot % (len(COUNTS) - 1)] if ((off == -d).all() or (off == 2 * d).all()) else 0
            counterparts = kind in ("full", "nolayer") and (off == d).all()
            if counterparts:
                n = min(n, MAX_POINTS - NQ)
            if n:
                k = home + off
                p = np.empty((n, 4))
                p[:, :3] = np.array([_lo(k[0]), _lo(k[1]), _lo(k[2])]) + rng.uniform(0.35, 0.65, size=(n, 3))
                p[:, 3] = LABELS[(c + off.sum()) % 3]
                assert (_index(p[:, :3]) == k).all()
                pts.append(p)
            if counterparts:
                p = q.copy()
                p[:, :3] += STEP * d
                assert (_index(p[:, :3]) == home + d).all()
                pts.append(p)
        rot += 2
    # (the frame is the queries where they start: the registration has to find the translation STEP * d)
    return np.concatenate(pts), np.concatenate(qs), kinds


def _crossings(oracle, om, frame, d, iterations):
    """the most queries that change their home voxel by exactly d between two consecutive iterations of the oracle"""
    best, prev = 0, _index(frame[:, :3])
    for it in range(1, iterations + 1):
        pose, _ = om.register_frame(frame, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH, max_iter=it)
        cur = _index(oracle.transform_points(pose, frame)[:, :3])
        best = max(best, int(((cur - prev) == np.array(d)).all(axis=1).sum()))
        prev = cur
    return best


def _compare(gpu_sage, oracle, om, gm, frame, opose, ost):
    """every forced form gives ONE pose, n_corr_hist and sum_candidates, to the bit, and the oracle's registration"""
    runs = []
    for loop, lw, filt in FORMS:
        with Env(SAGEICP_LOOP=loop, SAGEICP_LW=lw, SAGEICP_FILTER=filt):
            pose, st = gpu_sage.register_frame(frame, gm, gpu_sage.IDENTITY, MAX_DIST, KERNEL, SEM_TH, return_stats=True)
        assert st.lanes_per_query == 1 << lw and st.compact_scan == filt and st.single_launch == loop
        runs.append(((loop, lw, filt), pose, st))
    _, pose0, st0 = runs[0]
    for f, pose, st in runs[1:]:
        assert np.array_equal(pose, pose0), f
        assert st.iterations == st0.iterations and st.converged == st0.converged, f
        assert list(st.n_corr_hist) == list(st0.n_corr_hist), f
        assert st.sum_candidates == st0.sum_candidates, f
    e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(opose), pose0))
    assert np.linalg.norm(e[:3]) < 1e-7 and np.linalg.norm(e[3:]) < 1e-7
    assert st0.iterations == ost.iterations and st0.converged == ost.converged
    assert st0.n_corr_first == ost.n_corr_first and st0.n_corr_last == ost.n_corr_last
    assert st0.sum_candidates == ost.sum_candidates_total


def _check(gpu_sage, oracle, d, origin):
    mp, frame, kinds = _case(d, origin)
    om = oracle.Map(VS, 100.0, basic=MAX_POINTS, critical=MAX_POINTS)
    om.add_points(mp)
    gm = gpu_sage.VoxelHashMap(VS, 100.0, MAX_POINTS, MAX_POINTS)
    gm.AddPoints(mp)
    assert om.size() == len(mp) == gm.size()                 # every point kept: the voxels hold what the scene says
    opose, ost = om.register_frame(frame, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH)
    assert ost.iterations >= 2
    # the precondition, by the oracle alone: three quarters of the queries cross by exactly d in ONE iteration
    crossed = _crossings(oracle, om, frame, d, min(ost.iterations, 6))
    print("shift %s origin %d: %d of %d queries cross together, %d iterations" % (d, origin, crossed, len(frame), ost.iterations))
    assert crossed >= 3 * len(frame) // 4
    _compare(gpu_sage, oracle, om, gm, frame, opose, ost)


@pytest.mark.parametrize("d", DIRECTIONS, ids=lambda d: "%+d%+d%+d" % d)
def test_every_direction(gpu_sage, oracle, d):
    """(a), (d), (e): all 26 shifts, every storage class, empty new layers, seeds left behind"""
    _check(gpu_sage, oracle, d, origin=False)


@pytest.mark.parametrize("d", ORIGIN_DIRECTIONS, ids=lambda d: "%+d%+d%+d" % d)
def test_cell_zero_and_negative_indices(gpu_sage, oracle, d):
    """(b): homes at index 1, 0 and -1; crossings 1 -> 0, 0 -> -1 and back"""
    _check(gpu_sage, oracle, d, origin=True)


# ---- (c) jumps and near moves in one wave ----------------------------------------------------------------------------
YAW = 0.03                                  # the frame is turned by this about the z axis: a point at radius r moves r * YAW
R_NEAR, R_JUMP = 10, 90                     # home index on x of the two groups: 0.3 voxel and 2.7 voxels in +y


def _turn_case(oracle):
    """-> map points, the frame, which queries are of the jump group.  Two stacks of neighbourhoods along z, at x index 10
    and 90, homes at y index 1, the queries just under the upper y face of their home voxel.  The map holds the queries
    turned by YAW about z: the first Gauss-Newton step finds the turn, which carries the near group 0.3 voxel (shift
    (0, +1, 0)) and the jump group 2.7 voxels (y index 1 -> 4) in the SAME iteration.  The frame alternates between the
    groups query by query, so every wave of the loop holds both."""
    rng = np.random.default_rng(3003)
    turn = oracle.se3_exp(np.array([0.0, 0.0, 0.0, 0.0, 0.0, YAW]))
    pts, near, jump = [], [], []
    for i in range(12):
        for group, hx in ((near, R_NEAR), (jump, R_JUMP)):
            home = np.array([hx, 1, 2 + PITCH * i])
            q = np.empty((NQ, 4))
            q[:, 0] = home[0] + 0.5 + rng.uniform(-0.05, 0.05, size=NQ)
            q[:, 1] = home[1] + 1 - rng.uniform(0.005, 0.02, size=NQ)
            q[:, 2] = home[2] + 0.5 + rng.uniform(-0.05, 0.05, size=NQ)
            q[:, 3] = rng.choice((40, 70, 0, 10), size=NQ)
            assert (_index(q[:, :3]) == home).all()
            group.append(q)
            pts.append(oracle.transform_points(turn, q))                     # the true counterparts
            dest = _index(pts[-1][:, :3])
            assert (dest == home + (np.array([0, 1, 0]) if hx == R_NEAR else np.array([0, 3, 0]))).all()
            # filler: the 5 x 5 x 5 voxels around a near home; around a jump's destination the rows at and beyond it
            for off in itertools.product(range(-2, 3), repeat=3):
                off = np.array(off)
                if hx == R_JUMP and off[1] < 0:
                    continue
                k = (home if hx == R_NEAR else dest[0]) + off
                n = COUNTS[(i + 25 * (off[0] + 2) + 5 * (off[1] + 2) + off[2] + 2) % len(COUNTS)]
                n = min(n, MAX_POINTS - NQ)
                if n:
                    p = np.empty((n, 4))
                    p[:, :3] = k + rng.uniform(0.35, 0.65, size=(n, 3))
                    p[:, 3] = LABELS[(i + off.sum()) % 3]
                    pts.append(p)
    near, jump = np.concatenate(near), np.concatenate(jump)
    frame = np.empty((2 * len(near), 4))
    frame[0::2], frame[1::2] = near, jump
    is_jump = np.arange(len(frame)) % 2 == 1
    return np.concatenate(pts), frame, is_jump


def _mixed_moves(oracle, om, frame, is_jump, iterations):
    """per iteration of the oracle: (near-group queries that moved by exactly (0, +1, 0), jump-group queries that moved
    two voxels or more on an axis) -> the pair of the iteration with the most of both"""
    best, prev = (0, 0), _index(frame[:, :3])
    for it in range(1, iterations + 1):
        pose, _ = om.register_frame(frame, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH, max_iter=it)
        cur = _index(oracle.transform_points(pose, frame)[:, :3])
        step = cur - prev
        n_near = int(((step == np.array([0, 1, 0])).all(axis=1) & ~is_jump).sum())
        n_jump = int(((np.abs(step).max(axis=1) >= 2) & is_jump).sum())
        if min(n_near, n_jump) > min(best):
            best = (n_near, n_jump)
        prev = cur
    return best


def test_jumps_and_near_moves_in_one_wave(gpu_sage, oracle):
    """(c): the not-near walk and the new-layer path as two divergent regions of the same pass, each writing its rows"""
    mp, frame, is_jump = _turn_case(oracle)
    om = oracle.Map(VS, 200.0, basic=MAX_POINTS, critical=MAX_POINTS)
    om.add_points(mp)
    gm = gpu_sage.VoxelHashMap(VS, 200.0, MAX_POINTS, MAX_POINTS)
    gm.AddPoints(mp)
    assert om.size() == len(mp) == gm.size()
    opose, ost = om.register_frame(frame, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH)
    assert ost.iterations >= 2
    n_near, n_jump = _mixed_moves(oracle, om, frame, is_jump, min(ost.iterations, 6))
    print("jumps and near moves: %d near, %d jumps of %d + %d in one iteration, %d iterations"
          % (n_near, n_jump, (~is_jump).sum(), is_jump.sum(), ost.iterations))
    # both kinds in ONE iteration, three quarters of each group; the groups alternate in the frame: in every wave
    assert n_near >= 3 * (~is_jump).sum() // 4 and n_jump >= 3 * is_jump.sum() // 4
    _compare(gpu_sage, oracle, om, gm, frame, opose, ost)


# ---- (f) tombstones and wrapping hash chains -------------------------------------------------------------------------
def _chain_frame(live):
    """queries around the live chain voxels (points at the voxel's centre in x and y, mapscenes.frame_from_runs): every
    third voxel gets queries 1.01 voxel below its lower x face — home two voxels below it, the chain voxel is NOT in
    their neighbourhood — the others queries 0.3 voxel below its centre.  The first step moves the frame by a fraction
    of a voxel in +x: the former step into the voxel next to the chain voxel, which enters with the new layer and is
    found through the chain."""
    rng = np.random.default_rng(4004)
    q, crosser = [], []
    for i, k in enumerate(live):
        far = i % 3 == 0
        for j in range(4):
            x = k[0] - 1.01 - 0.002 * j if far else k[0] + 0.2 + 0.002 * j
            q.append((x, k[1] + 0.5 + rng.uniform(-0.02, 0.02), k[2] + 0.5 + rng.uniform(-0.02, 0.02), (0.0, 71.0, 40.0, 80.0)[j]))
            crosser.append(far)
    return np.array(q), np.array(crosser)


def test_new_layer_found_through_tombstones_and_a_wrapped_chain(gpu_sage, oracle):
    """(f): the map of tests/mapscenes.py's chain scene after three device-side updates, the second of which evicts
    every second link of a probe chain that wraps from the last slot to slot 0"""
    import mapref
    import mapscenes
    sage = gpu_sage
    s = mapscenes.scene("c_ffff", sage)
    p = s["params"]
    dev = mapscenes.make_map(sage, s)
    om = oracle.Map(p["voxel_size"], p["max_distance"], p["basic"], p["critical"])
    for k, (pts, pose, _) in enumerate(s["passes"][:3]):
        dev.UpdateOnDevice(pts, pose)
        om.add_points(np.array(mapref.transform(pose, pts)).reshape(-1, 4))
        om.remove_far(pose[4:])
    cap, used, live_slots = dev.table_stats()
    assert dev.resident() and used > live_slots, "no tombstone in the table"
    assert dev.size() == om.size()
    box1, box2, held = s["chain"]
    live = box1 + held
    assert len({sage.voxel_hash(*k) & (cap - 1) for k in live}) == 1       # one chain, whatever the table's size here
    frame, crosser = _chain_frame(live)
    opose, ost = om.register_frame(frame, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH)
    assert ost.iterations >= 2
    prev, best = _index(frame[:, :3]), 0
    for it in range(1, min(ost.iterations, 6) + 1):
        pose, _ = om.register_frame(frame, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH, max_iter=it)
        cur = _index(oracle.transform_points(pose, frame)[:, :3])
        best = max(best, int(((cur - prev) == np.array([1, 0, 0])).all(axis=1)[crosser].sum()))
        prev = cur
    print("chain: %d of %d queries step to the voxel next to a chain voxel in one iteration, %d iterations, table %d / %d / %d"
          % (best, crosser.sum(), ost.iterations, cap, used, live_slots))
    assert best >= 3 * crosser.sum() // 4
    _compare(gpu_sage, oracle, om, dev, frame, opose, ost)
