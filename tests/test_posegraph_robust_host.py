"""The robust pose-graph optimiser on the CPU (include/sageicp.h "robust pose graph"): where = 1 everywhere,
no test here needs a GPU.  The scenes are tests/robustscenes.py's (true closures plus aliased ones), the reference is
tests/robustref.py (IRLS Gauss-Newton in np.longdouble and np.float64).

Bounds: the pose-graph tests' rule, no new number.  The library's poses x are polished by the longdouble restatement at
the final scale; x lies within 4 max(d_ref, STEP_TOL) of the polished point, d_ref the distance of the fp64 and the
longdouble restatement on that scene, STEP_TOL = 1e-9; on these scenes x also lies within the same bound of the restatement
run from the start (the same basin).  Weights within 1e-6 of the restatement's.

MEASURED (recomputed and printed by every run): distance to the optimum of the scene WITHOUT its false closures
    scene      plain    Huber    Cauchy    GM        GM + anneal
    two_laps   10.5 m   4.0 m    0.044 m   3.3e-5    3.3e-5   (15 stages)
    ring       17.7 m   10.3 m   0.036 m   2.5e-3    2.5e-3   (17 stages)
    hard       12.1 m   -        0.075 m   3.8 m, all five weights 0    1.1e-3, weights 0.98 / 0.99 / 0.996 / 0 / 0
Huber's IRLS contracts at 0.91 per iteration on the ring (192 iterations to a step of 1e-9, which then leaves 1e-8): the
tolerance test asks it for a step of 1e-11 under 2000 iterations; the bound is the rule's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import graphscenes as gs
import posegraphref as pg
import robustref as rr
import robustscenes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TOL, _bits = gs.STEP_TOL, gs.bits
DP = ctypes.POINTER(ctypes.c_double)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(DP)


def _raw_call(sage, s, robust, where=1, fill=None, c_out=None, **prm):
    """sageicp_graph_optimize_robust itself: (rc, poses_out, corrections, GraphInfo, chi2, weight, GraphRobustInfo)"""
    lib = sage.lib()
    P = np.ascontiguousarray(s["poses"], dtype=np.float64)
    n = len(P)
    O = np.ascontiguousarray(s["odom_info"], dtype=np.float64).reshape(-1)
    E = gs.edges(sage, s)
    arr = (sage.GraphEdge * max(1, len(E)))(*E)
    params = sage.GraphParams()
    lib.sageicp_graph_params_default(ctypes.byref(params))
    params.where = where
    for k, v in prm.items():
        setattr(params, k, v)
    c = len(E)
    out, corr = np.full((n, 7), 7.25), np.full((n, 7), 7.25)
    chi2, weight = np.full(max(1, c), 7.25), np.full(max(1, c), 7.25)
    gi, ri = sage.GraphInfo(), sage.GraphRobustInfo()
    gi.cost_final, ri.scale2_first = 7.25, 7.25
    rc = lib.sageicp_graph_optimize_robust(_ptr(P), n, _ptr(O), 0 if O.size == 36 else 36, arr, c, None, ctypes.byref(params), _ptr(out),
                                           _ptr(corr), ctypes.byref(gi), None if robust is None else ctypes.byref(robust), _ptr(chi2),
                                           _ptr(weight), ctypes.byref(ri))
    return rc, out, corr, gi, chi2[:c], weight[:c], ri


def _robust(sage, **kw):
    r = sage.GraphRobust()
    sage.lib().sageicp_graph_robust_default(ctypes.byref(r))
    for k, v in kw.items():
        setattr(r, k, v)
    return r


# ---- the entries -----------------------------------------------------------------------------------------------------------
def test_symbols_structs_and_defaults(sage, tmp_path):
    lib = sage.lib()
    header = open(os.path.join(ROOT, "include", "sageicp.h")).read()
    for name in ("sageicp_graph_robust_default", "sageicp_graph_optimize_robust", "sageicp_pipeline_graph_optimize_robust",
                 "sageicp_graph_info_from_quality"):
        assert getattr(lib, name)
        assert name + "(" in header, name
    assert lib.sageicp_abi_version() == 4
    layout = {"sageicp_graph_robust": (sage.GraphRobust, ["kernel", "anneal", "scale", "anneal_factor", "stage_iterations", "reserved"]),
              "sageicp_graph_robust_info": (sage.GraphRobustInfo, ["scale2_first", "stages", "outliers"])}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){'
    want = []
    for cname, (cls, fields) in layout.items():
        src += 'printf(" %%zu", sizeof(%s));' % cname
        want.append(ctypes.sizeof(cls))
        for f in fields:
            src += 'printf(" %%zu", offsetof(%s, %s));' % (cname, f)
            want.append(getattr(cls, f).offset)
    src += 'printf(" %d %d %d %d", SAGEICP_GRAPH_KERNEL_NONE, SAGEICP_GRAPH_KERNEL_HUBER, SAGEICP_GRAPH_KERNEL_CAUCHY, SAGEICP_GRAPH_KERNEL_GM);'
    src += "return 0;}"
    exe = str(tmp_path / "robust_layout_probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want + [0, 1, 2, 3]
    assert (ctypes.sizeof(sage.GraphRobust), ctypes.sizeof(sage.GraphRobustInfo)) == (32, 16)
    r = _robust(sage)
    assert (r.kernel, r.anneal, r.scale, r.anneal_factor, r.stage_iterations, r.reserved) == (0, 0, np.sqrt(16.81), 2.0, 3, 0)
    assert sage.GRAPH_KERNEL == {"none": 0, "huber": 1, "cauchy": 2, "gm": 3}
    assert callable(sage.graph_edge_info)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_posegraph_robust_check(tmp_path, flags):
    """csrc/posegraph.h's kernels on their own: rho' against central differences of rho in long double, one robust host
    step against a dense solve"""
    exe = str(tmp_path / "posegraph_robust_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "sage-icp_amd", "csrc"), os.path.join(ROOT, "tests", "posegraph_robust_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "posegraph_robust_check: ok" in r.stdout


def test_shim_graph_robust_type_checks():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_stubs", "graph_robust_user.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the decisions ---------------------------------------------------------------------------------------------------------
def _verdicts(s, info):
    false = set(s["false"])
    w = info["closure_weight"]
    return all((w[k] < 0.5) == (k in false) for k in range(len(w)))


@pytest.mark.parametrize("name", list(rs.SCENES))
def test_false_closures_are_rejected_and_true_ones_kept(sage, name):
    s, clean = rs.scene(name), rs.clean_optimum(name)
    _, plain, _ = rs.optimize(sage, s, None)
    d_plain = pg.distance(plain, clean)
    for kernel, anneal in (("cauchy", False), ("gm", name == "hard")):
        _, out, info = rs.optimize(sage, s, kernel, anneal)
        d = pg.distance(out, clean)
        print("%s %s anneal %d: %.3g m from the clean optimum (plain %.3g m); weights %s; stages %d" %
              (name, kernel, anneal, d, d_plain, info["closure_weight"], info["stages"]))
        assert _verdicts(s, info), info["closure_weight"]
        assert info["outliers"] == len(s["false"])
        assert d < d_plain and d < 0.1 and d_plain > 10.0
        assert info["status"] in (0, 1) and np.isfinite(out).all()


def test_the_continuation_decides_the_hard_scene(sage):
    s, clean = rs.scene("hard"), rs.clean_optimum("hard")
    _, stuck, i0 = rs.optimize(sage, s, "gm", False)
    _, out, i1 = rs.optimize(sage, s, "gm", True)
    print("hard: GM alone %.3g m off, weights %s; annealed %.3g m off, weights %s, %d stages from c^2 = %.4g" %
          (pg.distance(stuck, clean), i0["closure_weight"], pg.distance(out, clean), i1["closure_weight"], i1["stages"], i1["scale2_first"]))
    assert i0["outliers"] == len(s["closures"]) and (i0["closure_weight"] < 0.5).all() and i0["stages"] == 1
    assert pg.distance(stuck, clean) > 1.0
    assert i1["outliers"] == len(s["false"]) and _verdicts(s, i1) and i1["stages"] > 1
    assert pg.distance(out, clean) < 0.01
    # the schedule is the restatement's: fixed by the largest closure term at the start
    G = rr.RobustGraph(s["poses"], s["odom_info"], s["closures"], np.float64)
    stages = rr.schedule(float(G.raw(s["poses"]).max()), rr.SCALE ** 2)
    assert i1["stages"] == len(stages) and i1["scale2_first"] == pytest.approx(stages[0], rel=1e-15)
    assert i0["scale2_first"] == pytest.approx(rr.SCALE ** 2, rel=1e-15)


@pytest.mark.parametrize("name", ["two_laps", "ring"])
def test_huber_bounds_it_does_not_reject(sage, name):
    s, clean = rs.scene(name), rs.clean_optimum(name)
    _, plain, _ = rs.optimize(sage, s, None)
    _, out, info = rs.optimize(sage, s, "huber", max_iterations=400)
    d = pg.distance(out, clean)
    print("%s: Huber %.3g m from the clean optimum (plain %.3g m), weights %s" % (name, d, pg.distance(plain, clean), info["closure_weight"]))
    assert 1.0 < d < pg.distance(plain, clean)
    # the false closure keeps pulling: metres off, and the true closures are bent with it
    assert info["closure_chi2"][s["false"][0]] > rr.SCALE ** 2


# ---- the tolerance rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel,anneal", [(n, k, a) for n in rs.CASES for k, a in rs.CASES[n]])
def test_host_against_the_restatement(sage, name, kernel, anneal):
    s, m = rs.scene(name), rs.measured(name, kernel, anneal)
    kw = dict(max_iterations=2000, step_tol=1e-11) if kernel == "huber" else {}
    _, out, info = rs.optimize(sage, s, kernel, anneal, **kw)
    bound, d = rs.held_to_the_rule(s, kernel, out, m, name)
    d_start = pg.distance(out, m["opt"])
    dw = float(np.abs(info["closure_weight"] - m["weights"]).max())
    print("  %.3g from the restatement run from the start; weights differ by %.3g; %s" % (d_start, dw, info))
    assert d <= bound and d_start <= bound
    assert dw <= 1e-6
    assert info["stages"] == len(m["stages"])
    assert info["status"] in (0, 1) and info["where"] == 1
    assert info["cost_final"] == pytest.approx(m["F"], rel=1e-9)
    if not anneal:
        assert info["cost_final"] <= info["cost_initial"]
    # the raw terms are sageicp_graph_cost's at poses_out
    E = gs.edges(sage, s)
    _, per = sage.graph_cost(s["poses"], E, s["odom_info"], at=out, per_edge=True)
    n = len(out)
    assert np.abs(info["closure_chi2"] - per[n - 1:]).max() <= (len(per) + 64) * 2.0 ** -52 * per[n - 1:].max()
    assert np.array_equal(info["closure_weight"], rr.weight(kernel, rr.SCALE ** 2, info["closure_chi2"])) or \
        np.abs(info["closure_weight"] - rr.weight(kernel, rr.SCALE ** 2, info["closure_chi2"])).max() <= 4 * 2.0 ** -52
    # cost_initial: the final kernel's F at the start
    G = rr.RobustGraph(s["poses"], s["odom_info"], s["closures"], np.longdouble, 0, kernel)
    assert info["cost_initial"] == pytest.approx(float(G.cost(s["poses"])), rel=1e-12)


# ---- the edges of the kernels --------------------------------------------------------------------------------------------------
def test_a_closure_met_exactly_under_huber(sage):
    s = dict(gs.chain(17, 0, seed=3))
    P = s["poses"]
    e = sage.graph_edge(P, 3, 12, P[12], gs.ODOM_INFO)
    corr, out, info = sage.graph_optimize(P, [e], s["odom_info"], where="host", return_info=True, robust=dict(kernel="huber"))
    print(info)
    assert np.isfinite(out).all() and np.isfinite(corr).all() and np.isfinite(info["cost_final"])
    assert info["closure_chi2"][0] < 1e-20 and info["closure_weight"][0] == 1.0 and info["outliers"] == 0
    assert pg.distance(out, P) <= STEP_TOL


def test_a_closure_exactly_at_the_scale_under_huber(sage):
    """max_iterations = 0: the call stops where it starts, and the closure's s there is made c^2 to the bit (an information
    scaled until sqrt(s)^2 == s in fp64)"""
    s, E, scale, _ = rs.exactly_at_a_scale(sage)
    _, out, info = sage.graph_optimize(s["poses"], E, s["odom_info"], where="host", return_info=True, max_iterations=0,
                                       robust=dict(kernel="huber", scale=scale))
    assert _bits(out) == _bits(s["poses"])
    assert info["closure_chi2"][0] == scale * scale and info["closure_weight"][0] == 1.0
    # one ulp above, Huber's other branch
    _, _, info = sage.graph_optimize(s["poses"], E, s["odom_info"], where="host", return_info=True, max_iterations=0,
                                     robust=dict(kernel="huber", scale=float(np.nextafter(scale, 0.0))))
    assert info["closure_weight"][0] < 1.0


def test_the_verdict_at_a_weight_of_exactly_a_half(sage):
    rs.check_the_verdict_at_a_weight_of_a_half(sage, "host")


def test_the_schedule_at_a_power_of_the_factor(sage):
    rs.check_the_schedule_at_a_power_of_the_factor(sage, "host")


def test_a_closure_of_1e12_under_gm(sage):
    base = gs.two_laps()
    truth = base["truth"]
    z = gs.rel(truth, 10, 70).copy()
    z[4] += 5.0e4                                                # 400 * (5e4)^2 = 1e12
    s = dict(base, closures=list(base["closures"]) + [(10, 70, z, 4.0 * gs.ODOM_INFO)])
    m = rr.measured("two_laps_without", base["poses"], base["odom_info"], base["closures"], "gm")
    _, out, info = rs.optimize(sage, s, "gm")
    bound = 4.0 * max(m["d_ref"], STEP_TOL)
    d = pg.distance(out, m["opt"])
    print("s = %.3g, weight %.3g: %.3g from the problem without it (allowed %.3g)" % (info["closure_chi2"][3], info["closure_weight"][3], d, bound))
    assert np.isfinite(out).all() and np.isfinite(info["cost_final"]) and info["closure_chi2"][3] > 9e11
    assert d <= bound and info["outliers"] == 1


# ---- equality with the existing entry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gs.SCENES))
def test_none_is_the_existing_entry_bit_for_bit(sage, name):
    s = gs.scene(name)
    corr, out, info = gs.optimize(sage, s)
    E = gs.edges(sage, s)
    _, per = sage.graph_cost(s["poses"], E, s["odom_info"], at=out, per_edge=True)
    n = len(out)
    for robust in (None, _robust(sage), _robust(sage, kernel=0, anneal=1, scale=0.5)):
        rc, o2, c2, gi, chi2, weight, ri = _raw_call(sage, s, robust)
        assert rc == 0
        assert _bits(o2) == _bits(out) and _bits(c2) == _bits(corr) and gi.as_dict() == info
        assert (weight == 1.0).all() and ri.stages == 1 and ri.outliers == 0
        assert np.abs(chi2 - per[n - 1:]).max() <= (len(per) + 64) * 2.0 ** -52 * per[n - 1:].max()


# ---- every refusal -----------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(sage):
    s = rs.scene("ring")
    bad = [dict(kernel=4), dict(kernel=2, anneal=2), dict(kernel=2, scale=float("nan")), dict(kernel=2, scale=float("inf")),
           dict(kernel=2, scale=0.0), dict(kernel=2, scale=-1.0), dict(kernel=3, anneal=1, anneal_factor=1.0),
           dict(kernel=3, anneal=1, anneal_factor=0.5), dict(kernel=3, anneal_factor=float("nan")),
           dict(kernel=3, anneal_factor=float("inf")), dict(kernel=1, stage_iterations=0), dict(kernel=0, stage_iterations=0),
           dict(kernel=0, scale=-2.0)]
    for kw in bad:
        rc, out, corr, gi, chi2, weight, ri = _raw_call(sage, s, _robust(sage, **kw))
        assert rc == sage.ERR_INVALID, kw
        assert (out == 7.25).all() and (corr == 7.25).all() and (chi2 == 7.25).all() and (weight == 7.25).all(), kw
        assert gi.cost_final == 7.25 and ri.scale2_first == 7.25, kw
    # the existing entry's refusals hold under a kernel too
    rc, out, corr, gi, chi2, weight, ri = _raw_call(sage, s, _robust(sage, kernel=2), anchor=len(s["poses"]))
    assert rc == sage.ERR_INVALID and (out == 7.25).all() and (weight == 7.25).all() and ri.scale2_first == 7.25
    with pytest.raises(ValueError):
        sage.graph_optimize(s["poses"], gs.edges(sage, s), s["odom_info"], robust=dict(kernel="tukey"))
    with pytest.raises(ValueError):
        sage.graph_optimize(s["poses"], gs.edges(sage, s), s["odom_info"], robust=dict(scale=2.0))
