"""End to end: test_posegraph_gpu.py's two laps of a street, with one ALIASED closure among the true ones.

The drive, the drift, the window and the three true closures are that test's.  The fourth closure is made the way a false
place match makes one: the scan of the end of lap one is relocalised (public entries: Recall, Relocalize) against the old
map around the start, which is where it really is; the place matcher is then taken to have answered with the look-alike
place one period (3 m) down the street, where the same registration lands 3 m further along x.  Its information is
graph_edge_info of the quality report at the relocalised pose (the right tangent's information does not change under the
common shift), with the gain that makes its translation part 4 ODOM_INFO's, the true closures' own.
Asserted: Geman-McClure with anneal gives the aliased closure a weight below 0.5 and the true ones above, and its
corrections, fed to CorrectedPointcloud, leave the session's rows closer to the truth than the plain optimiser's do."""
import numpy as np
import pytest

import closureref as cr
import graphscenes as gs
import posegraphref as pg

pytestmark = pytest.mark.gpu


def test_an_aliased_closure_among_true_ones(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    DRIFT, SIDE, RADIUS, PERIOD = 0.05, 10, 4.0, 3.0
    u = np.array([0.6, 0.8, 0.0])
    corners = [(0.0, 0.0), (SIDE, 0.0), (SIDE, SIDE), (0.0, SIDE), (0.0, 0.0)]
    lap = [np.array([x0 + (x1 - x0) * k / SIDE, y0 + (y1 - y0) * k / SIDE, 0.0])
           for (x0, y0), (x1, y1) in zip(corners[:-1], corners[1:]) for k in range(1, SIDE + 1)]
    true_t = np.array([np.zeros(3)] + lap + lap) + np.array([8.0, 3.0, 0.0])
    n = len(true_t)
    path = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(true_t, axis=0), axis=1))])
    drift_t = np.round((true_t + DRIFT * path[:, None] * u) * 1024.0) / 1024.0
    rot = [0.0, 0.0, 0.0, 1.0]
    poses = np.concatenate([np.tile(rot, (n, 1)), drift_t], axis=1)
    truth = np.concatenate([np.tile(rot, (n, 1)), true_t], axis=1)
    rng = np.random.default_rng(2025)
    m = sage.VoxelHashMap(1.0, RADIUS, 20, 20, [40, 44, 48]).set_archive(True)
    old = sage.VoxelHashMap(1.0, RADIUS, 20, 20, [40, 44, 48]).set_archive(True)      # the drive up to three sides of lap one
    true_of, scans = {}, []
    for k in range(n):
        scan = syn.make_scan(rng, 160, 40.0, truth[k], max_range=3.5, min_range=0.5, label_max_range=50.0)
        scans.append(scan)
        m.UpdateOnDevice(scan, poses[k])
        if k <= 3 * SIDE:
            old.UpdateOnDevice(scan, poses[k])
        for w, t in zip(scan[:, :3] + drift_t[k], scan[:, :3] + true_t[k]):
            true_of[w.tobytes()] = t
    # the end of lap one seen again at the start: recall the old map there, relocalise the scan from a prior half a metre off
    b = 4 * SIDE
    recalled, rinfo = old.Recall(drift_t[0], 6.0)
    prior = poses[0].copy()
    prior[4:] += [0.4, -0.3, 0.0]
    closed, q, info = recalled.Relocalize(scans[b], prior, 1.0, 0.5, 0.05, xy=(1.0, 0.5), refine_top=3)
    off = float(np.linalg.norm(closed[4:] - drift_t[0]))
    print("recalled %s; relocalised %.3f m from the old pose of the place, fitness %.3f, rmse %.3f, covariance_valid %d"
          % (rinfo, off, q.fitness, q.rmse, q.covariance_valid))
    assert q.valid == 1 and q.covariance_valid == 1 and off < 0.5
    raw = sage.graph_edge_info(q, closed)
    gain = 4.0 * gs.ODOM_INFO[0, 0] / raw[0, 0]
    info_q = sage.graph_edge_info(q, closed, gain)
    print("the report's information: diagonal %s at gain 1; gain %.3g" % (np.diag(raw), gain))
    alias = closed.copy()
    alias[4] += PERIOD
    s = dict(poses=poses, truth=truth, odom_info=gs.ODOM_INFO,
             closures=[(a, c, gs.rel(truth, a, c), 4.0 * gs.ODOM_INFO) for a, c in ((0, 4 * SIDE), (0, 8 * SIDE), (SIDE, 5 * SIDE))])
    E = gs.edges(sage, s) + [sage.graph_edge(poses, 0, b, alias, info_q)]
    plain = sage.graph_optimize(poses, E, gs.ODOM_INFO, where="device", return_info=True)
    robust = sage.graph_optimize(poses, E, gs.ODOM_INFO, where="device", return_info=True, robust=dict(kernel="gm", anneal=1))
    w = robust[2]["closure_weight"]
    print("weights %s, chi2 %s, %d stages, %d iterations" % (w, robust[2]["closure_chi2"], robust[2]["stages"], robust[2]["iterations"]))
    assert (w[:3] > 0.5).all() and w[3] < 0.5 and robust[2]["outliers"] == 1
    rows = m.ArchivedPointcloud("session")
    true_rows = np.array([true_of[p.tobytes()] for p in rows[:, :3]])
    worst, pose_err = {}, {}
    for name, (C, out, _) in (("plain", plain), ("robust", robust)):
        fixed = m.CorrectedPointcloud("session", drift_t, C)
        worst[name] = float(np.linalg.norm(fixed[:, :3] - true_rows, axis=1).max())
        pose_err[name] = float(np.linalg.norm(out[:, 4:] - true_t, axis=1).max())
    before = float(np.linalg.norm(rows[:, :3] - true_rows, axis=1).max())
    print("rows off the truth by at most %.3f m before, %.3f m under the plain optimiser, %.3f m under Geman-McClure with anneal; "
          "poses %.3f / %.3f m" % (before, worst["plain"], worst["robust"], pose_err["plain"], pose_err["robust"]))
    assert worst["robust"] < worst["plain"] and pose_err["robust"] < pose_err["plain"]
    assert worst["robust"] < before
    # dropping the match the weights name gives the optimum of the true closures alone
    kept = [e for e, wk in zip(E, w) if wk >= 0.5]
    clean = sage.graph_optimize(poses, kept, gs.ODOM_INFO, where="device", return_info=True)
    assert len(kept) == 3 and pg.distance(robust[1], clean[1]) < 0.01
    assert cr.se3_mul(robust[1][5], cr.se3_inv(poses[5])) == pytest.approx(robust[0][5], abs=1e-12)
