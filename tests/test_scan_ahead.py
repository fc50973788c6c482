"""The per-voxel restart scan opens a lane's next voxel one step ahead (icp_body.h, SAGE_SCAN_AHEAD): the row word of
the voxel after the open one is read while the loads of the step are in flight, and the step that finds the open voxel
exhausted takes it.  What can go wrong is the cursor: a voxel opened twice or not at all, a partial last step, a lane
without a point in a voxel (fewer points than its lane index), a descriptor read ahead from a row that was rebuilt.

The scene is a lattice of separate 3 x 3 x 3 neighbourhoods, voxel size 1, whose voxels hold 1, 3, 4, 5, 7, 8, 9, 12, 13,
16, 17 and 40 points (every size class of the map's storage; full, partial and empty second halves of a step at 1, 2 and
4 lanes per query):
  mixed     all 27 voxels occupied, the counts above in rotation
  tiny      all 27 voxels occupied by 1..3 points: every step of a lane opens a voxel, lanes 1..3 often find nothing
  lonely    the home voxel empty, exactly ONE neighbour occupied
  hollow    the home voxel empty, all 26 neighbours occupied: nothing bounds the search, every voxel is scanned
  foreign   the home voxel holds points of another label far from the query: its scaled bound (sem_th 0.4) prunes
            nothing, all 27 voxels are scanned
  last      the true neighbour is the LAST point of the LAST voxel in enumeration order (voxel 26, added last)
Every query has an accepted correspondence by the oracle alone (asserted on the CPU, nothing is skipped).

Needs a real MI355X:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 40)
VS, MAX_POINTS = 1.0, 40
MAX_DIST, KERNEL, SEM_TH = 3.0, 1.0 / 3.0, 0.4
LABEL_A, LABEL_B = 40, 70
PITCH = 6                                   # voxels between the homes of two neighbourhoods: they do not see each other
FORMS = [(loop, lw, filt) for loop in (1, 0) for lw in (1, 2, 3) for filt in (0, 1)]   # 2, 4, 8 lanes per query


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


def _voxel_points(rng, corner, count, label, lo=0.2, hi=0.8):
    p = np.empty((count, 4))
    p[:, :3] = corner + rng.uniform(lo, hi, size=(count, 3)) * VS
    p[:, 3] = label
    return p


def _scene():
    """-> map points (in insertion order), queries, the kind of every query"""
    rng = np.random.default_rng(1906)
    pts, qs, kinds = [], [], []
    kinds_cycle = ["mixed"] * 10 + ["tiny"] * 8 + ["lonely"] * 8 + ["hollow"] * 4 + ["foreign"] * 4 + ["last"] * 6
    rot = 0
    for c, kind in enumerate(kinds_cycle):
        # positive coordinates only (the cell of index 0 is two voxels wide); homes on a lattice
        home = np.array([2 + PITCH * (c % 5), 2 + PITCH * ((c // 5) % 5), 2 + PITCH * (c // 25)], dtype=float)
        lonely_v = (0, 26, 14, 4, 22, 12, 9, 17)[c % 8]
        for v in range(27):
            corner = home + np.array([v // 9 - 1, (v // 3) % 3 - 1, v % 3 - 1], dtype=float)
            label = (LABEL_A, LABEL_B, 0)[(c + v) % 3]
            if kind == "mixed" or kind == "last":
                n = COUNTS[(rot + v) % len(COUNTS)]
            elif kind == "tiny":
                n = 1 + (rot + v) % 3
            elif kind == "lonely":
                n = COUNTS[(rot + c) % len(COUNTS)] if v == lonely_v else 0
            elif kind == "hollow":
                n = 0 if v == 13 else COUNTS[(rot + v) % len(COUNTS)]
            else:                            # foreign: the home voxel's points sit in its corners, label B
                n = COUNTS[(rot + v) % len(COUNTS)]
            if n == 0:
                continue
            if kind == "foreign" and v == 13:
                p = np.empty((8, 4))
                p[:, :3] = corner + np.array([[a, b, d] for a in (0.06, 0.94) for b in (0.06, 0.94) for d in (0.06, 0.94)])
                p[:, 3] = LABEL_B
            elif kind == "last" and v == 26:
                p = _voxel_points(rng, corner, n, label)
                p[-1, :3] = corner + 0.03   # the last point of the last voxel: next to the home voxel's far corner
            else:
                p = _voxel_points(rng, corner, n, label)
            pts.append(p)
        rot += 5
        # queries of this neighbourhood, all inside its home voxel
        if kind == "last":
            q = np.empty((4, 4))
            q[:, :3] = home + 0.97 - rng.uniform(0.0, 0.01, size=(4, 3))
            q[:, 3] = (LABEL_A, LABEL_B, 0, 10)
        elif kind == "foreign":
            q = np.empty((6, 4))
            q[:, :3] = home + 0.5 + rng.uniform(-0.05, 0.05, size=(6, 3))
            q[:, 3] = LABEL_A
        else:
            q = np.empty((8, 4))
            q[:, :3] = home + rng.uniform(0.02, 0.98, size=(8, 3))
            q[:, 3] = rng.choice((LABEL_A, LABEL_B, 0, 10), size=8)
        qs.append(q)
        kinds += [kind] * len(q)
    return np.concatenate(pts), np.concatenate(qs), kinds


def _voxel_counts(cloud):
    keys = np.floor(cloud[:, :3] / VS).astype(np.int64)
    _, counts = np.unique(keys, axis=0, return_counts=True)
    return counts


@pytest.fixture(scope="module")
def scene(gpu_sage, oracle):
    mp, q, kinds = _scene()
    om = oracle.Map(VS, 100.0, basic=MAX_POINTS, critical=MAX_POINTS)
    om.add_points(mp)
    gm = gpu_sage.VoxelHashMap(VS, 100.0, MAX_POINTS, MAX_POINTS)
    gm.AddPoints(mp)
    # the map holds what the scene says: every point kept, every voxel count of the list present
    assert om.size() == len(mp) == gm.size()
    counts = _voxel_counts(om.pointcloud())
    assert set(COUNTS) <= set(counts.tolist()) and counts.max() == MAX_POINTS
    # the oracle alone accepts a correspondence for every query (no case is skipped)
    _, otgt, oidx = om.get_correspondences(q, MAX_DIST, SEM_TH, with_index=True)
    assert np.array_equal(oidx, np.arange(len(q)))
    # ... and the `last` queries' answer is the point the scene put last into voxel 26
    last = [i for i, k in enumerate(kinds) if k == "last"]
    assert len(last) == 24
    for i in last:
        home = np.floor(q[i, :3])
        assert np.allclose(otgt[i, :3], home + 1.03)
    opose, ost = om.register_frame(q, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH)
    return dict(map=gm, omap=om, q=q, kinds=kinds, otgt=otgt, oidx=oidx, opose=opose, ost=ost)


@pytest.mark.parametrize("lw", [0, 1, 2, 3])
@pytest.mark.parametrize("filt", [0, 1])
def test_correspondences_are_index_exact(gpu_sage, scene, lw, filt):
    """the search alone (k_icp), 1, 2, 4 and 8 lanes per query, full records and the compact scan"""
    with Env(SAGEICP_LW=lw, SAGEICP_FILTER=filt):
        _, tgt, idx = scene["map"].GetCorrespondences(scene["q"], MAX_DIST, SEM_TH, with_index=True)
    assert np.array_equal(idx, scene["oidx"])
    assert np.array_equal(tgt, scene["otgt"])


def _register(gpu_sage, scene, q, init, loop, lw, filt):
    with Env(SAGEICP_LOOP=loop, SAGEICP_LW=lw, SAGEICP_FILTER=filt):
        pose, st = gpu_sage.register_frame(q, scene["map"], init, MAX_DIST, KERNEL, SEM_TH, return_stats=True)
    assert st.lanes_per_query == 1 << lw and st.compact_scan == filt
    assert st.single_launch == (1 if loop else 0)
    return pose, st


def test_pose_is_one_in_every_forced_form(gpu_sage, oracle, scene):
    """both loops x 2, 4, 8 lanes per query x both scan forms: ONE pose, to the bit, and the oracle's correspondences"""
    runs = [(f, _register(gpu_sage, scene, scene["q"], gpu_sage.IDENTITY, *f)) for f in FORMS]
    pose0, st0 = runs[0][1]
    for f, (pose, st) in runs[1:]:
        assert np.array_equal(pose, pose0), f
        assert st.iterations == st0.iterations and st.converged == st0.converged, f
        assert list(st.n_corr_hist) == list(st0.n_corr_hist), f
        assert st.sum_candidates == st0.sum_candidates, f
    ost = scene["ost"]
    e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(scene["opose"]), pose0))
    assert np.linalg.norm(e[:3]) < 1e-7 and np.linalg.norm(e[3:]) < 1e-7
    assert st0.iterations == ost.iterations and st0.converged == ost.converged
    assert st0.n_corr_first == ost.n_corr_first == len(scene["q"]) and st0.n_corr_last == ost.n_corr_last
    assert st0.sum_candidates == ost.sum_candidates_total


def test_face_crossings_rebuild_the_row_under_the_cursor(gpu_sage, oracle, scene):
    """The queries start 0.45 voxels and 40 mrad off: the registration takes three iterations or more, its first
    steps move the queries by a good part of a voxel, so rows are shifted or rebuilt between iterations and the
    descriptor read ahead in the iteration before must not be used after."""
    off = oracle.se3_exp(np.array([0.45, -0.3, 0.2, 0.0, 0.0, 0.04]))
    # (without the `lonely` neighbourhoods: moved this far, some of their queries lose sight of their one voxel)
    q = scene["q"][[k != "lonely" for k in scene["kinds"]]].copy()
    q[:, :3] = oracle.transform_points(oracle.se3_inv(off), q)[:, :3]
    om = scene["omap"]
    opose, ost = om.register_frame(q, oracle.IDENTITY, MAX_DIST, KERNEL, SEM_TH)
    assert ost.iterations >= 3
    # queries do cross faces between the first and the last pose of the oracle's run
    k0 = np.floor(q[:, :3] / VS)
    k1 = np.floor(oracle.transform_points(opose, q)[:, :3] / VS)
    assert (k0 != k1).any(axis=1).sum() >= len(q) // 4
    # (an accepted correspondence for every query at the start, by the oracle alone)
    _, _, oidx = om.get_correspondences(q, MAX_DIST, SEM_TH, with_index=True)
    assert np.array_equal(oidx, np.arange(len(q)))
    runs = [(f, _register(gpu_sage, scene, q, gpu_sage.IDENTITY, *f)) for f in FORMS]
    pose0, st0 = runs[0][1]
    for f, (pose, st) in runs[1:]:
        assert np.array_equal(pose, pose0), f
        assert st.iterations == st0.iterations and list(st.n_corr_hist) == list(st0.n_corr_hist), f
        assert st.sum_candidates == st0.sum_candidates, f
    e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(opose), pose0))
    assert np.linalg.norm(e[:3]) < 1e-7 and np.linalg.norm(e[3:]) < 1e-7
    assert st0.iterations == ost.iterations and st0.converged == ost.converged
    assert st0.n_corr_first == ost.n_corr_first and st0.n_corr_last == ost.n_corr_last
    assert st0.sum_candidates == ost.sum_candidates_total
