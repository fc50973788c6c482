"""The robust pose-graph optimiser on the device (where = 2; k_pg_lin<true> / k_pg_cost<true> of csrc/posegraph.hip;
DESIGN.md D20), held to the restatement (tests/robustref.py), to the host path and to itself.

Bounds: test_posegraph_robust_host.py's rule — the device's poses within 4 max(d_ref, STEP_TOL) of themselves polished by
the longdouble restatement at the final scale, and on the named scenes of the restatement run from the start; host and
device within twice that of each other; weights within 1e-6.  Beyond n = 130 there is no dense restatement: there the
weights are the restatement's kernel evaluated (fp64) at the device's own poses, and host and device are held to
test_posegraph_gpu.py's soft bound."""
import math

import numpy as np
import pytest

import closureref as cr
import graphscenes as gs
import graphsteps as gst
import posegraphref as pg
import robustref as rr
import robustscenes as rs

pytestmark = pytest.mark.gpu
STEP_TOL, _bits = gs.STEP_TOL, gs.bits
IDENTITY = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def _both(sage, s, kernel, anneal=False, **kw):
    dev = rs.optimize(sage, s, kernel, anneal, where="device", **kw)
    host = rs.optimize(sage, s, kernel, anneal, where="host", **kw)
    assert dev[2]["where"] == 2 and host[2]["where"] == 1
    return dev, host


def _verdicts(w):
    return [bool(v < 0.5) for v in w]


@pytest.mark.parametrize("name,kernel,anneal", [(n, k, a) for n in rs.SCENES for k, a in (("cauchy", False), ("gm", True))])
def test_scenes_against_the_restatement_and_the_host(gpu_sage, name, kernel, anneal):
    s, m = rs.scene(name), rs.measured(name, kernel, anneal)
    (corr, out, info), (_, hout, hinfo) = _both(gpu_sage, s, kernel, anneal)
    bound, d = rs.held_to_the_rule(s, kernel, out, m, name)
    d_start, dh = pg.distance(out, m["opt"]), pg.distance(out, hout)
    print("  %.3g from the restatement run from the start, %.3g from the host; %s" % (d_start, dh, info))
    assert d <= bound and d_start <= bound and dh <= 2.0 * bound
    assert np.abs(info["closure_weight"] - m["weights"]).max() <= 1e-6
    assert _verdicts(info["closure_weight"]) == _verdicts(hinfo["closure_weight"]) == [k in s["false"] for k in range(len(s["closures"]))]
    assert info["outliers"] == hinfo["outliers"] == len(s["false"]) and info["stages"] == hinfo["stages"] == len(m["stages"])
    assert info["status"] in (0, 1) and info["cost_final"] == pytest.approx(m["F"], rel=1e-9)
    assert _bits(out[0]) == _bits(s["poses"][0]) and _bits(corr[0]) == _bits(IDENTITY)
    for k in range(1, len(out)):
        assert _bits(corr[k]) == _bits(cr.se3_mul(out[k], cr.se3_inv(s["poses"][k])))


def with_a_false_last_closure(s):
    """the scene with its last closure's measurement moved 5 m along x"""
    out = dict(s)
    a, b, z, info = s["closures"][-1]
    z = np.array(z, dtype=np.float64)
    z[4] += 5.0
    out["closures"] = list(s["closures"][:-1]) + [(a, b, z, info)]
    return out


@pytest.mark.parametrize("c", [1, 2, 7])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 17, 64, 65, 66, 129])
def test_shapes_that_cross_the_solvers_structure(gpu_sage, n, c):
    """graphscenes.chain's "edges" menu (closures at the anchor, at the last pose, adjacent, doubled, reversed), the last
    closure false; the anchor in the middle for every other size"""
    anchor = n // 2 if n in (3, 5, 64, 66) else 0
    s = with_a_false_last_closure(gs.chain(n, c, seed=100 * n + c, how="edges", anchor=anchor))
    (corr, out, info), (_, hout, hinfo) = _both(gpu_sage, s, "cauchy", anchor=anchor)
    assert _bits(out[anchor]) == _bits(s["poses"][anchor]) and _bits(corr[anchor]) == _bits(IDENTITY)
    m = rr.measured(("chain", n, c), s["poses"], s["odom_info"], s["closures"], "cauchy", anchor=anchor)
    m = dict(m, anchor=anchor)
    bound, d = rs.held_to_the_rule(s, "cauchy", out, m, "n %d c %d anchor %d" % (n, c, anchor))
    print("  host %.3g from the device; weights %s, the restatement's %s" % (pg.distance(out, hout), info["closure_weight"], m["weights"]))
    assert d <= bound and pg.distance(out, hout) <= 2.0 * bound
    assert np.abs(info["closure_weight"] - hinfo["closure_weight"]).max() <= 1e-6
    assert np.abs(info["closure_weight"] - m["weights"]).max() <= 1e-6
    assert _verdicts(info["closure_weight"]) == _verdicts(m["weights"])
    assert info["cost_final"] <= info["cost_initial"] and info["status"] in (0, 1)


def _soft_bound(n, F):
    lam = 100.0 * (math.pi / (2.0 * n)) ** 2
    return 4.0 * max(STEP_TOL / (1.0 - 0.8), math.sqrt(2.0 ** -52 * max(F, 0.0) / lam))


def test_256_closures_every_fourth_false(gpu_sage):
    """four iterations on either path (the 1536 x 1536 capacitance system is factored on the host in both: half a second
    each); the two paths take the same steps to rounding, far inside the soft bound of converged runs"""
    n, c = 300, 256
    s = gs.chain(n, c, seed=41, how="spread")
    closures = []
    for k, (a, b, z, info) in enumerate(s["closures"]):
        z = np.array(z, dtype=np.float64)
        if k % 4 == 3:
            z[4] += 5.0
        closures.append((a, b, z, info))
    s = dict(s, closures=closures)
    (corr, out, info), (_, hout, hinfo) = _both(gpu_sage, s, "cauchy", max_iterations=4)
    G = rr.RobustGraph(s["poses"], s["odom_info"], s["closures"], np.float64, 0, "cauchy")
    want = G.weights(out)
    print("c = 256: device %.3g from the host; %d outliers; weights of the false %.3g .. %.3g, of the true %.3g .. %.3g; %s" %
          (pg.distance(out, hout), info["outliers"], info["closure_weight"][3::4].min(), info["closure_weight"][3::4].max(),
           np.delete(info["closure_weight"], np.s_[3::4]).min(), np.delete(info["closure_weight"], np.s_[3::4]).max(), info))
    assert np.abs(info["closure_weight"] - want).max() <= 1e-6
    assert np.abs(info["closure_weight"] - hinfo["closure_weight"]).max() <= 1e-6
    assert _verdicts(info["closure_weight"]) == _verdicts(want) == _verdicts(hinfo["closure_weight"])
    assert info["outliers"] == hinfo["outliers"] == int((want < 0.5).sum())
    assert pg.distance(out, hout) <= _soft_bound(n, info["cost_final"])
    assert info["iterations"] == hinfo["iterations"] == 4 and info["cost_final"] < info["cost_initial"]
    assert int((want[3::4] < 0.5).sum()) >= 48                  # (most of the 64 false ones are out after four iterations)


def test_beyond_a_grid_stride(gpu_sage):
    """graphsteps.large_scene(): n = 262 146, one edge and one vertex beyond 1024 x 256 items; two iterations under Cauchy"""
    sage, s = gpu_sage, gst.large_scene()
    E = gs.edges(sage, s)
    kw = dict(initial=s["initial"], max_iterations=2, max_halvings=gst.MAX_HALVINGS, return_info=True, robust=dict(kernel="cauchy"))
    a = sage.graph_optimize(s["poses"], E, s["odom_info"], where="device", **kw)
    b = sage.graph_optimize(s["poses"], E, s["odom_info"], where="device", **kw)
    h = sage.graph_optimize(s["poses"], E, s["odom_info"], where="host", **kw)
    print("large: device %s; host %s" % (a[2], h[2]))
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])
    assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    assert a[2]["iterations"] == h[2]["iterations"] >= 1
    assert np.abs(a[2]["closure_weight"] - h[2]["closure_weight"]).max() <= 1e-6
    assert a[2]["cost_final"] < a[2]["cost_initial"] and a[2]["cost_final"] == pytest.approx(h[2]["cost_final"], rel=1e-9)
    assert _bits(a[1][0]) == _bits(s["initial"][0])


def test_kernel_none_is_the_plain_device_path(gpu_sage):
    for s in (gs.scene("two_laps"), gs.chain(65, 7, seed=5, how="edges")):
        plain = gs.optimize(gpu_sage, s, where="device")
        none = rs.optimize(gpu_sage, s, "none", where="device")
        assert _bits(plain[0]) == _bits(none[0]) and _bits(plain[1]) == _bits(none[1])
        assert all(none[2][k] == v for k, v in plain[2].items())
        assert (none[2]["closure_weight"] == 1.0).all() and none[2]["stages"] == 1 and none[2]["outliers"] == 0


def test_the_verdict_at_a_weight_of_exactly_a_half(gpu_sage):
    """the decision is the host's on either path, from the same numbers (test_posegraph_robust_host.py)"""
    rs.check_the_verdict_at_a_weight_of_a_half(gpu_sage, "device")


def test_the_schedule_at_a_power_of_the_factor(gpu_sage):
    rs.check_the_schedule_at_a_power_of_the_factor(gpu_sage, "device")


def test_the_same_bytes_on_two_runs(gpu_sage):
    s = rs.scene("hard")
    a, b = rs.optimize(gpu_sage, s, "gm", True, where="device"), rs.optimize(gpu_sage, s, "gm", True, where="device")
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])
    assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2]) and a[2]["stages"] > 1


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
              cr.se3_mul(np.array([0.0, 0.0, 0.0, 1.0, -0.1, 0.2, 0.0]), poses[n - 3]),
              cr.se3_mul(np.array([0.0, 0.0, 0.0, 1.0, 6.0, 0.0, 0.0]), poses[n - 2])]          # a false one, 6 m off
    E = [sage.graph_edge(poses, 1, n - 1, closed[0], 4.0 * gs.ODOM_INFO), sage.graph_edge(poses, 0, n - 3, closed[1], gs.ODOM_INFO),
         sage.graph_edge(poses, 2, n - 2, closed[2], 4.0 * gs.ODOM_INFO)]
    robust = dict(kernel="gm", anneal=1)
    for where in ("device", "host"):
        corr, fixed, info = p.OptimizeGraph(E, gs.ODOM_INFO, where=where, robust=robust)
        want = sage.graph_optimize(poses, E, gs.ODOM_INFO, where=where, return_info=True, robust=robust)
        assert _bits(corr) == _bits(want[0]) and _bits(fixed) == _bits(want[1])
        assert all(np.array_equal(info[k], want[2][k]) for k in want[2]) and set(info) == set(want[2])
        assert _verdicts(info["closure_weight"]) == [False, False, True] and info["outliers"] == 1
    assert _bits(p.poses()) == _bits(poses)                                  # the pipeline's own state is not touched
