"""The pose-graph optimiser on the device (where = 2; csrc/posegraph.hip), held to the restatement
(tests/posegraphref.py), to the host path (where = 1) and to itself (the same bytes on every run).

Bounds.  Scenes and shapes of n <= 129 poses: 4 * max(d_ref, step_tol) from the restatement's np.longdouble optimum, d_ref the
restatement's own fp64-against-longdouble distance for that very graph, step_tol = 1e-9 — the host tests' bound; host and
device are then within twice that of each other.  n = 1000 and the large case have no dense restatement; there the device
is held to
  * the restatement's vectorised gradient (at every vertex; in the large case at every 37th, around the closures' ends and
    around the stride's end; fp64, fourth-order differences: relative truncation h^4 = 1.6e-11 and rounding
    2^-53 / h = 5.5e-14 of the terms' scale S = max sum |J^T| |w|; allowed 64 times that, 1e-9 S) — grad_max is what the
    restatement finds at the device's poses, and it is at most 2 |H|_inf d, |H|_inf the largest row sum of |sum J^T J| from the
    restatement's Jacobians and d the distance from the minimiser that the next point allows (to first order dF = 2 H dx);
  * F <= F(initial);
  * the host path, within 4 * max(step_tol / (1 - 0.8), sqrt(2^-52 F / lambda)): a path stops within step_tol / (1 - ratio)
    of the minimiser (ratio <= 0.8 is what the restatement asserts of the scenes) unless it meets the floating-point floor
    first, where F's rounding (2^-52 F) hides a displacement d along the chain's softest mode with lambda d^2 below it;
    lambda = 100 (pi / (2 n))^2 is the smallest eigenvalue of a chain of n poses of translation information 100 fixed at one
    end (closures only stiffen it).

THE LARGE CASE: n = 300 001, c = 3.  Every kernel of posegraph.hip is launched with at most kPgBlocks = 1024 workgroups of
256 lanes = 262 144 items, so with 300 000 free vertices and 300 003 edges each of k_pg_lin, k_pg_cost, k_pg_asm,
k_pg_update, k_pg_rhs_final, the first levels of k_pg_inv / k_pg_red / k_pg_fwd / k_pg_bwd, k_pg_rhs_cols (19 columns) and
k_pg_red1 takes a second stride; the cyclic reduction goes 19 levels deep (10 at n = 1000) and k_pg_red2 sums 1024 slabs,
four per lane, where the other tests give it at most one."""
import math

import numpy as np
import pytest

import closureref as cr
import graphscenes as gs
import posegraphref as pg

pytestmark = pytest.mark.gpu
STEP_TOL, SCENES, scene, measured, _bits, _opt, _sequential = (gs.STEP_TOL, gs.SCENES, gs.scene, gs.measured, gs.bits, gs.optimize,
                                                                  gs.sequential)


def _both(sage, s, **kw):
    dev = _opt(sage, s, where="device", **kw)
    host = _opt(sage, s, where="host", **kw)
    assert dev[2]["where"] == 2 and host[2]["where"] == 1
    return dev, host


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_against_the_restatement_and_the_host(gpu_sage, name):
    s, m = scene(name), measured(name)
    (corr, out, info), (_, hout, hinfo) = _both(gpu_sage, s)
    bound = 4.0 * max(m["d_ref"], STEP_TOL)
    d, dh = pg.distance(out, m["opt"]), pg.distance(out, hout)
    print("%s: device %.3g from the longdouble optimum (allowed %.3g), %.3g from the host; %s" % (name, d, bound, dh, info))
    assert d <= bound and dh <= 2.0 * bound
    assert pg.distance(m["fixed_identity"], m["opt"]) > 10.0 * bound
    assert info["status"] in (0, 1) and info["cost_final"] == pytest.approx(m["F"], rel=1e-9)
    # F as the device sums it (a tree, the device's sin / cos / atan2) against the host's sequential sum of the same terms:
    # E terms re-associated, each a few ulps apart
    E = len(out) - 1 + len(s["closures"])
    host_F = gpu_sage.graph_cost(s["poses"], gs.edges(gpu_sage, s), s["odom_info"], at=out)
    assert info["cost_final"] == pytest.approx(host_F, rel=(E + 64) * 2.0 ** -52)
    assert _bits(out[0]) == _bits(s["poses"][0]) and _bits(corr[0]) == _bits([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    for k in range(1, len(out)):
        assert _bits(corr[k]) == _bits(cr.se3_mul(out[k], cr.se3_inv(s["poses"][k])))


def _soft_bound(n, F):
    lam = 100.0 * (math.pi / (2.0 * n)) ** 2
    return 4.0 * max(STEP_TOL / (1.0 - 0.8), math.sqrt(2.0 ** -52 * max(F, 0.0) / lam))


def _gradient_check(s, out, info, anchor, sample=None):
    """the restatement's gradient at `out` (at the vertices of `sample` only, from their incident edges, if given)"""
    G = pg.Graph(s["poses"], s["odom_info"], s["closures"], np.float64, anchor)
    if sample is not None:
        keep = np.zeros(G.n, dtype=bool)
        keep[sample] = True
        sel = np.nonzero(keep[G.a] | keep[G.b])[0]
        G.a, G.b, G.zinv, G.L, G.E = G.a[sel], G.b[sel], G.zinv[sel], G.L[sel], len(sel)
    w, Ja, Jb = G.jacobians(out)
    scale, g = np.zeros((G.n, 6)), np.zeros((G.n, 6))
    np.add.at(scale, G.a, np.einsum("eki,ek->ei", np.abs(Ja), np.abs(w)))
    np.add.at(scale, G.b, np.einsum("eki,ek->ei", np.abs(Jb), np.abs(w)))
    np.add.at(g, G.a, np.einsum("eki,ek->ei", Ja, w))
    np.add.at(g, G.b, np.einsum("eki,ek->ei", Jb, w))
    g *= 2.0
    g[anchor] = 0.0
    if sample is not None:
        g, scale = g[sample], scale[sample]
    rows = np.zeros((G.n, 6))                                    # row sums of |H|, H = sum J^T J over the whitened Jacobians
    both = np.abs(Ja) + np.abs(Jb)
    np.add.at(rows, G.a, np.einsum("eki,ekj->ei", np.abs(Ja), both))
    np.add.at(rows, G.b, np.einsum("eki,ekj->ei", np.abs(Jb), both))
    if sample is not None:
        rows = rows[sample]
    S, got, Hn = 2.0 * float(scale.max()), float(np.abs(g).max()), float(rows.max())
    small = 2.0 * Hn * _soft_bound(G.n, info["cost_final"])
    print("  grad_max %.4g, the restatement's %.4g (scale of its terms %.3g; |H|_inf %.3g: allowed %.3g)" % (info["grad_max"], got, S, Hn, small))
    assert got <= small
    if sample is None:
        assert abs(info["grad_max"] - got) <= 1e-9 * S
    else:
        assert info["grad_max"] >= got - 1e-9 * S


@pytest.mark.parametrize("c", [0, 1, 2, 7])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 17, 64, 65, 66, 129, 1000])
def test_shapes_that_cross_the_solvers_structure(gpu_sage, n, c):
    """closures at the anchor, at the last pose, on adjacent poses, twice on one pair and reversed (graphscenes.chain's
    "edges" menu); the anchor in the middle for every other size"""
    anchor = n // 2 if n in (3, 5, 64, 66, 1000) else 0
    s = gs.chain(n, c, seed=100 * n + c, how="edges", anchor=anchor)
    (corr, out, info), (_, hout, hinfo) = _both(gpu_sage, s, anchor=anchor)
    assert _bits(out[anchor]) == _bits(s["poses"][anchor]) and _bits(corr[anchor]) == _bits([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    assert info["cost_final"] <= info["cost_initial"] and info["status"] in (0, 1)
    if not s["closures"]:
        assert info["iterations"] <= 1 and pg.distance(out, s["poses"]) <= STEP_TOL
        return
    if n <= 129:
        m = pg.measured(("chain", n, c), s["poses"], s["odom_info"], s["closures"], anchor=anchor, identity=False)
        bound = 4.0 * max(m["d_ref"], STEP_TOL)
        d = pg.distance(out, m["opt"])
        print("n %d c %d anchor %d: device %.3g from the longdouble optimum (allowed %.3g), host %.3g; F %.4g -> %.4g in %d"
              % (n, len(s["closures"]), anchor, d, bound, pg.distance(hout, m["opt"]), info["cost_initial"], info["cost_final"], info["iterations"]))
        assert d <= bound and pg.distance(out, hout) <= 2.0 * bound
    else:
        bound = _soft_bound(n, info["cost_final"])
        print("n %d c %d: device %.3g from the host (allowed %.3g); F %.4g -> %.4g" % (n, c, pg.distance(out, hout), bound,
                                                                                         info["cost_initial"], info["cost_final"]))
        assert pg.distance(out, hout) <= bound
        _gradient_check(s, out, info, anchor)


def test_the_large_case(gpu_sage):
    n = 300001
    # two laps of a circle of 5 cm: a sensor that all but stands still, with jitter.  (A drive of 300 000 one-metre steps with
    # three closures has a normal matrix that fp64 cannot factor to any purpose — its condition grows like n^4, a beam's;
    # here the rotations are held by their own information, the chain is a string, n^2: DESIGN.md D19.)
    truth = gs.circle_truth(n, 0.05, per_lap=(n - 1) // 2)
    poses = gs.wander(truth, 77, trans=2e-5, rot=2e-6)
    closures = [(a, b, gs.rel(truth, a, b), gs.ODOM_INFO * 4.0) for a, b in ((0, 150000), (262200, 112200), (5, n - 1))]
    s = dict(poses=poses, truth=truth, odom_info=gs.ODOM_INFO, closures=closures)
    (corr, out, info), (_, hout, hinfo) = _both(gpu_sage, s)
    bound = _soft_bound(n, info["cost_final"])
    print("large: F %.6g -> %.6g (host %.6g), device %.3g from the host (allowed %.3g); %s" %
          (info["cost_initial"], info["cost_final"], hinfo["cost_final"], pg.distance(out, hout), bound, info))
    assert info["cost_final"] < info["cost_initial"] and info["status"] in (0, 1)
    assert pg.distance(out, hout) <= bound
    near = lambda k: np.arange(max(0, k - 2), min(n, k + 3))
    sample = np.unique(np.concatenate([np.arange(0, n, 37)] + [near(k) for k in (0, 5, 112200, 150000, 262143, 262144, 262200, n - 1)]))
    _gradient_check(s, out, info, 0, sample)
    assert _bits(out[0]) == _bits(poses[0])


def test_the_same_bytes_on_two_runs(gpu_sage):
    s = scene("two_laps")
    a, b = _opt(gpu_sage, s, where="device"), _opt(gpu_sage, s, where="device")
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and a[2] == b[2]
    s = gs.chain(1000, 7, seed=5, how="spread")
    a, b = _opt(gpu_sage, s, where="device"), _opt(gpu_sage, s, where="device")
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and a[2] == b[2]


def test_per_edge_information_equals_the_broadcast_form(gpu_sage):
    s = scene("full_info")
    n = len(s["poses"])
    per_edge = np.tile(np.asarray(s["odom_info"]).reshape(1, 6, 6), (n - 1, 1, 1))
    a = gpu_sage.graph_optimize(s["poses"], gs.edges(gpu_sage, s), s["odom_info"], where="device")
    b = gpu_sage.graph_optimize(s["poses"], gs.edges(gpu_sage, s), per_edge, where="device")
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])


def test_the_pipeline_entry(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    frames = syn.make_stream(21, 14, points_per_frame=3000, step=(2.5, 0.0, 0.0), max_range=30.0)[0]
    p = sage.SageICP(sage.make_pipeline_config(max_range=30.0, local_map_range=30.0, map_update_on_device=True))
    for f in frames:
        p.RegisterFrame(f)
    poses = p.poses()
    n = len(poses)
    h = 0.5 * np.radians(1.0)
    closed = [cr.se3_mul(np.array([0.0, 0.0, np.sin(h), np.cos(h), 0.3, -0.2, 0.02]), poses[n - 1]),
              cr.se3_mul(np.array([0.0, 0.0, 0.0, 1.0, -0.1, 0.2, 0.0]), poses[n - 3])]
    E = [sage.graph_edge(poses, 1, n - 1, closed[0], 4.0 * gs.ODOM_INFO), sage.graph_edge(poses, 0, n - 3, closed[1], gs.ODOM_INFO)]
    for where in ("device", "host"):
        corr, fixed, info = p.OptimizeGraph(E, gs.ODOM_INFO, where=where)
        want = sage.graph_optimize(poses, E, gs.ODOM_INFO, where=where, return_info=True)
        assert _bits(corr) == _bits(want[0]) and _bits(fixed) == _bits(want[1]) and info == want[2]
        assert info["cost_final"] < info["cost_initial"]
    assert _bits(p.poses()) == _bits(poses)                                  # the pipeline's own state is not touched


def test_two_laps_of_a_street_put_back_together(gpu_sage):
    """Two laps of a square of 10 m a side through the street scene, a window (max_distance 4) that evicts the start long
    before it is passed again; the true frames are inserted at poses that drift sideways by 5 cm per metre driven.  Three
    closures from the truth: the start seen again after one lap and after two, and a corner of lap one seen from lap two.
    All at once (the graph, on the device) against one after another (sageicp_closure_corrections): the same export, the
    rows against the truth."""
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    DRIFT, SIDE, RADIUS = 0.05, 10, 4.0
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
    true_of = {}
    for k in range(n):
        scan = syn.make_scan(rng, 160, 40.0, truth[k], max_range=3.5, min_range=0.5, label_max_range=50.0)
        m.UpdateOnDevice(scan, poses[k])
        for w, t in zip(scan[:, :3] + drift_t[k], scan[:, :3] + true_t[k]):
            true_of[w.tobytes()] = t
    s = dict(poses=poses, truth=truth, odom_info=gs.ODOM_INFO,
             closures=[(a, b, gs.rel(truth, a, b), 4.0 * gs.ODOM_INFO) for a, b in ((0, 4 * SIDE), (0, 8 * SIDE), (SIDE, 5 * SIDE))])
    ref = pg.measured("street", poses, gs.ODOM_INFO, s["closures"], identity=False)
    corr, out, info = _opt(sage, s, where="device")
    bound = 4.0 * max(ref["d_ref"], STEP_TOL)
    assert pg.distance(out, ref["opt"]) <= bound
    seq = _sequential(sage, s, (0, 1, 2))
    corr_seq = np.array([cr.se3_mul(seq[k], cr.se3_inv(poses[k])) for k in range(n)])
    plain = m.ArchivedPointcloud("session")
    true_rows = np.array([true_of[p.tobytes()] for p in plain[:, :3]])
    rows, counts, updates = cr.session_voxels(m, "session", 1.0)
    stay = m.SessionStays(drift_t, "session")
    worst = {}
    for name, C in (("graph", corr), ("sequential", corr_seq)):
        fixed = m.CorrectedPointcloud("session", drift_t, C)
        assert fixed.tobytes() == cr.move(rows, counts, stay, C).tobytes()
        worst[name] = float(np.linalg.norm(fixed[:, :3] - true_rows, axis=1).max())
    before = float(np.linalg.norm(plain[:, :3] - true_rows, axis=1).max())
    pose_err = {"graph": float(np.linalg.norm(out[:, 4:] - true_t, axis=1).max()),
                "sequential": float(np.linalg.norm(seq[:, 4:] - true_t, axis=1).max())}
    print("rows off the truth by at most %.3f m before, %.3f m under sequential closures, %.3f m under the graph; poses %.3f / %.3f m"
          % (before, worst["sequential"], worst["graph"], pose_err["sequential"], pose_err["graph"]))
    # the rows under the graph's corrections are where the restatement's optimum puts them (a row lies within 4 m + 3.5 m of
    # its pose: the bound on a pose times that lever for its rotation, plus the bound for its translation)
    corr_ref = np.array([cr.se3_mul(np.asarray(ref["opt"][k], dtype=np.float64), cr.se3_inv(poses[k])) for k in range(n)])
    expected = cr.move(rows, counts, stay, corr_ref)
    got = m.CorrectedPointcloud("session", drift_t, corr)
    assert np.abs(got[:, :3] - expected[:, :3]).max() <= bound * (1.0 + 2.0 * (RADIUS + 3.5 + np.abs(drift_t).max()))
    assert info["cost_final"] <= sage.graph_cost(poses, gs.edges(sage, s), gs.ODOM_INFO, at=seq)
    assert worst["graph"] < before and pose_err["graph"] <= pose_err["sequential"]


def test_a_chain_beyond_fp64_is_refused_or_solved_never_garbled(gpu_sage):
    """3 001 poses a kilometre apart with 0.2 mrad of wander per step and one closure: the chain's normal matrix, fixed at
    one end, is beyond fp64 (its condition grows like n^4 d^2).  The host's sequential block Thomas meets a
    diagonal block that is not positive definite and refuses the call.  The device's cyclic reduction eliminates in another
    order and need not meet one: it either refuses in the same words or returns finite poses with F not above where it
    started, the anchor's bytes and a status — never numbers that are not a trajectory."""
    sage = gpu_sage
    n, step = 3001, 1000.0
    lap = (n - 1) // 2
    truth = gs.circle_truth(n, step * lap / (2.0 * np.pi), per_lap=lap)
    poses = gs.wander(truth, 3, trans=0.01 * step, rot=2e-4)
    s = dict(poses=poses, truth=truth, odom_info=gs.ODOM_INFO,
             closures=[(100, 100 + lap, gs.rel(truth, 100, 100 + lap), 4.0 * gs.ODOM_INFO)])
    with pytest.raises(sage.SageIcpError) as e:
        _opt(sage, s, where="host")
    assert e.value.code == sage.ERR_INVALID and "not positive definite" in str(e.value)
    try:
        corr, out, info = _opt(sage, s, where="device")
    except sage.SageIcpError as e:
        print("the device refuses too: %s" % e)
        assert e.code == sage.ERR_INVALID and "not positive definite" in str(e)
        return
    print("the device solves it: %s" % info)
    assert np.isfinite(out).all() and np.isfinite(corr).all() and info["status"] in (0, 1, 2)
    assert info["cost_final"] <= info["cost_initial"] and _bits(out[0]) == _bits(poses[0])
    assert info["cost_final"] == pytest.approx(sage.graph_cost(poses, gs.edges(sage, s), gs.ODOM_INFO, at=out), rel=1e-9)
