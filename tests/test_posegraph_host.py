"""The pose-graph optimiser on the CPU (include/sageicp.h "pose graph"): symbols and struct layouts, the
stand-alone check of csrc/posegraph.h (plain and under AddressSanitizer / UBSan), the cost and the host optimum against the
restatement (tests/posegraphref.py) on the scenes of tests/graphscenes.py, the approximation Jr^-1 = I shown to lie outside
the bound, the anchor, c = 0, every refusal, translation equivariance, the comparison with sequential closures, the shim.
where = 1 everywhere: no test here needs a GPU.

Bounds.  The restatement runs Gauss-Newton to a stall in np.longdouble and in np.float64; d_ref is the distance of the two
optima (max abs over quaternion components and translations).  The library is allowed 4 * max(d_ref, step_tol) from the
longdouble optimum, step_tol = 1e-9 (the default).  MEASURED (recomputed and printed by every run; the bound is the run's):

    scene      F before -> after   d_ref      the library   Jr^-1 = I's fixed point   contraction   cond(H)
    ring       407.2 -> 3.372      6.7e-10    6.2e-10       3.7e-4                    0.080         4.6e5
    ring, UTM  407.2 -> 3.372      1.4e-09    1.4e-09       3.7e-4                    0.080         4.6e5
    full info  1417  -> 4.567      3.3e-10    1.2e-09       5.0e-3                    0.23          3.0e6
    two laps   2479  -> 2.522      6.9e-09    2.6e-09       1.2e-4                    0.061         3.6e6

Sequential closures on the two laps (sageicp_closure_corrections, each closure in turn): F = 409.7 against 2.522 at the
optimum, a factor of 162; the closures applied first are reopened to terms of 195 and 206, against 0.017 and 0.008 at the
optimum.  The closure applied LAST is met exactly by construction (its term is 1e-26): no minimiser of F can be below that
on that one term, so "each closure's own residual is smaller" is asserted for each closure against the orders in which it
is not the last one applied, and F(optimum) <= F(sequential) against all six orders."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import closureref as cr
import graphscenes as gs
import posegraphref as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TOL, SCENES, scene, measured, _bits, _opt = gs.STEP_TOL, gs.SCENES, gs.scene, gs.measured, gs.bits, gs.optimize


# ---- the entries -----------------------------------------------------------------------------------------------------------
def test_symbols_and_structs(sage, tmp_path):
    lib = sage.lib()
    names = ("sageicp_graph_params_default", "sageicp_graph_edge_from_closed", "sageicp_graph_cost", "sageicp_graph_optimize",
             "sageicp_pipeline_graph_optimize")
    header = open(os.path.join(ROOT, "include", "sageicp.h")).read()
    for name in names:
        assert getattr(lib, name)
        assert name + "(" in header, name
    assert lib.sageicp_abi_version() == 4
    layout = {"sageicp_graph_edge": (sage.GraphEdge, ["a", "b", "z", "info"]),
              "sageicp_graph_params": (sage.GraphParams, ["anchor", "max_iterations", "max_halvings", "step_tol", "where", "reserved"]),
              "sageicp_graph_info": (sage.GraphInfo, ["cost_initial", "cost_final", "grad_max", "step_last", "max_shift", "iterations",
                                                      "halvings", "status", "where"])}
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){'
    want = []
    for cname, (cls, fields) in layout.items():
        src += 'printf(" %%zu", sizeof(%s));' % cname
        want.append(ctypes.sizeof(cls))
        for f in fields:
            src += 'printf(" %%zu", offsetof(%s, %s));' % (cname, f)
            want.append(getattr(cls, f).offset)
    src += "return 0;}"
    exe = str(tmp_path / "graph_layout_probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert (ctypes.sizeof(sage.GraphEdge), ctypes.sizeof(sage.GraphParams), ctypes.sizeof(sage.GraphInfo)) == (360, 32, 56)
    prm = sage.GraphParams()
    lib.sageicp_graph_params_default(ctypes.byref(prm))
    assert (prm.anchor, prm.max_iterations, prm.max_halvings, prm.step_tol, prm.where, prm.reserved) == (0, 50, 10, STEP_TOL, 0, 0)
    for f in ("graph_edge", "graph_cost", "graph_optimize"):
        assert callable(getattr(sage, f))
    assert callable(sage.SageICP.OptimizeGraph)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_posegraph_check(tmp_path, flags):
    """csrc/posegraph.h on its own: the Jacobians against central differences, the structured solve against a dense one"""
    exe = str(tmp_path / "posegraph_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "sage-icp_amd", "csrc"), os.path.join(ROOT, "tests", "posegraph_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "posegraph_check: ok" in r.stdout


def test_shim_graph_type_checks():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_stubs", "graph_user.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the restatement against closureref's scalar SE(3) -----------------------------------------------------------------------
def test_the_restatements_rows_are_closurerefs_functions():
    rng = np.random.default_rng(4)
    a = np.concatenate([rng.normal(size=(20, 3)), 0.8 * rng.normal(size=(20, 3))], axis=1)
    a[0, 3:] = 0.0
    T = pg.vexp(a)
    U = pg.vexp(a[::-1].copy())
    # (numpy's sin, cos and arctan2 over an array and over a scalar may differ in the last place)
    close = lambda x, y: np.abs(x - y).max() <= 8 * 2.0 ** -52 * (1.0 + np.abs(y).max())
    for k in range(len(a)):
        assert close(T[k], cr.se3_exp(a[k]))
        assert close(pg.vmul(T, U)[k], cr.se3_mul(T[k], U[k]))
        assert close(pg.vinv(T)[k], cr.se3_inv(T[k]))
        assert close(pg.vlog(T)[k], cr.se3_log(T[k]))
        # between = inv * mul up to the rounding of the translation
        assert np.abs(pg.vbetween(T, U)[k] - cr.se3_mul(cr.se3_inv(T[k]), U[k])).max() < 1e-14


# ---- the cost ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_cost_against_the_restatement(sage, name):
    s = scene(name)
    rng = np.random.default_rng(8)
    at = pg.vmul(s["poses"], pg.vexp(0.01 * rng.normal(size=(len(s["poses"]), 6))))
    G64 = pg.Graph(s["poses"], s["odom_info"], s["closures"], np.float64)
    Gl = pg.Graph(s["poses"], s["odom_info"], s["closures"], np.longdouble)
    for x in (s["poses"], at):
        F, per = sage.graph_cost(s["poses"], gs.edges(sage, s), s["odom_info"], at=x, per_edge=True)
        ext = Gl.per_edge(x)
        own = np.abs(G64.per_edge(x).astype(np.longdouble) - ext)
        got = np.abs(per.astype(np.longdouble) - ext)
        # per edge: four times the fp64 restatement's own error on the scene, with one ulp of the largest term as the floor
        floor = float(ext.max()) * 2.0 ** -52
        allowed = 4.0 * max(float(own.max()), floor)
        print("%s: per-edge cost, fp64 restatement vs extended %.3g, the library %.3g (allowed %.3g); F %.9g" %
              (name, float(own.max()), float(got.max()), allowed, F))
        assert float(got.max()) <= allowed
        assert abs(F - float(ext.sum())) <= len(per) * allowed
        assert F == pytest.approx(float(per.sum()), rel=1e-14)
    # at the poses themselves the odometry edges cost nothing beyond rounding
    F, per = sage.graph_cost(s["poses"], gs.edges(sage, s), s["odom_info"], per_edge=True)
    assert per[:len(s["poses"]) - 1].max() < 1e-20


# ---- the optimum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_host_optimum_against_the_restatement(sage, name):
    s, m = scene(name), measured(name)
    corr, out, info = _opt(sage, s)
    bound = 4.0 * max(m["d_ref"], STEP_TOL)
    d = pg.distance(out, m["opt"])
    d_id = pg.distance(m["fixed_identity"], m["opt"])
    print("%s: F %.6g -> %.6g (restatement %.6g), d_ref %.3g, the library %.3g (allowed %.3g), Jr^-1 = I at %.3g, contraction %.3g, "
          "cond(H) %.3g, %s" % (name, info["cost_initial"], info["cost_final"], m["F"], m["d_ref"], d, bound, d_id, m["ratio"], m["cond"], info))
    assert m["d_ref"] > 0.0 and m["ratio"] <= 0.8
    assert d <= bound
    # the approximation Jr^-1 = I settles elsewhere: this test tells the two apart
    assert d_id > 10.0 * bound
    assert info["status"] in (0, 1) and info["where"] == 1 and info["iterations"] >= 3
    assert info["cost_initial"] == pytest.approx(m["F0"], rel=1e-12) and info["cost_final"] == pytest.approx(m["F"], rel=1e-9)
    assert info["cost_final"] == sage.graph_cost(s["poses"], gs.edges(sage, s), s["odom_info"], at=out)
    # grad_max as the restatement evaluates it at the library's optimum: four times the fp64 restatement's own error
    Gl = pg.Graph(s["poses"], s["odom_info"], s["closures"], np.longdouble)
    G64 = pg.Graph(s["poses"], s["odom_info"], s["closures"], np.float64)
    ext = Gl.gradient(out)
    own = float(np.abs(G64.gradient(out).astype(np.longdouble) - ext).max())
    print("  grad_max %.6g, the restatement's %.6g (fp64 restatement's own error %.3g)" % (info["grad_max"], float(np.abs(ext).max()), own))
    assert abs(info["grad_max"] - float(np.abs(ext).max())) <= 4.0 * own
    assert info["grad_max"] < 1e-5 * info["cost_initial"]
    # the corrections: poses_out * poses^-1, sageicp_closure_corrections' convention
    for k in range(len(out)):
        if k == 0:
            assert _bits(corr[k]) == _bits([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]) and _bits(out[k]) == _bits(s["poses"][k])
        else:
            assert _bits(corr[k]) == _bits(cr.se3_mul(out[k], cr.se3_inv(s["poses"][k])))
    assert info["max_shift"] == pytest.approx(np.linalg.norm(out[:, 4:] - s["poses"][:, 4:], axis=1).max(), rel=1e-12)


def test_translation_equivariance(sage):
    """the ring and its UTM twin: the same quaternions, the shifted translations — to four times what the fp64
    restatement's own pair of runs differs by (not below step_tol)"""
    a, b = measured("ring"), measured("ring_utm")
    pair = np.array(b["opt64"], dtype=np.float64)
    pair[:, 4:] -= gs.UTM
    d_pair = pg.distance(pair, a["opt64"])
    _, o0, _ = _opt(sage, scene("ring"))
    _, o1, _ = _opt(sage, scene("ring_utm"))
    o1 = o1.copy()
    o1[:, 4:] -= gs.UTM
    d = pg.distance(o1, o0)
    print("the restatement's pair differs by %.3g, the library's by %.3g (allowed %.3g)" % (d_pair, d, 4.0 * max(d_pair, STEP_TOL)))
    assert d <= 4.0 * max(d_pair, STEP_TOL)


def test_anchor_and_no_closures(sage):
    s = scene("ring")
    n = len(s["poses"])
    identity = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    for anchor in (0, 17, n - 1):
        corr, out, info = _opt(sage, s, anchor=anchor)
        assert _bits(out[anchor]) == _bits(s["poses"][anchor]) and _bits(corr[anchor]) == _bits(identity)
        m = pg.measured(("ring", anchor), s["poses"], s["odom_info"], s["closures"], anchor=anchor)
        assert pg.distance(out, m["opt"]) <= 4.0 * max(m["d_ref"], STEP_TOL)
        # the same minimum seen from another fixed pose: F does not depend on the anchor
        assert info["cost_final"] == pytest.approx(measured("ring")["F"], rel=1e-9)
    # c == 0: the odometry is met by the poses themselves
    for anchor in (0, 20):
        corr, out, info = sage.graph_optimize(s["poses"], [], s["odom_info"], anchor=anchor, where="host", return_info=True)
        assert info["iterations"] <= 1 and info["status"] in (0, 1)
        assert pg.distance(out, s["poses"]) <= STEP_TOL
        assert _bits(out[anchor]) == _bits(s["poses"][anchor]) and _bits(corr[anchor]) == _bits(identity)
    # an `initial` that is not the poses: the same optimum, the anchor at initial's
    rng = np.random.default_rng(2)
    x0 = pg.vmul(s["poses"], pg.vexp(0.02 * rng.normal(size=(n, 6))))
    x0[0] = s["poses"][0]
    _, out, info = _opt(sage, s, initial=x0)
    m = measured("ring")
    assert pg.distance(out, m["opt"]) <= 4.0 * max(m["d_ref"], STEP_TOL) and _bits(out[0]) == _bits(x0[0])
    # max_iterations is a cap: status 2, and F has gone down
    _, _, info = _opt(sage, s, max_iterations=2)
    assert info["status"] == 2 and info["iterations"] == 2 and info["cost_final"] < info["cost_initial"]


def test_per_edge_information_equals_the_broadcast_form(sage):
    s = scene("full_info")
    n = len(s["poses"])
    per_edge = np.tile(np.asarray(s["odom_info"]).reshape(1, 6, 6), (n - 1, 1, 1))
    a = sage.graph_optimize(s["poses"], gs.edges(sage, s), s["odom_info"], where="host")
    b = sage.graph_optimize(s["poses"], gs.edges(sage, s), per_edge, where="host")
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1])


_sequential = gs.sequential


def test_the_optimum_against_sequential_closures(sage):
    s = scene("two_laps")
    E, n = gs.edges(sage, s), len(s["poses"])
    _, out, info = _opt(sage, s)
    F_opt, per_opt = sage.graph_cost(s["poses"], E, s["odom_info"], at=out, per_edge=True)
    for order in itertools.permutations(range(3)):
        P = _sequential(sage, s, order)
        F_seq, per_seq = sage.graph_cost(s["poses"], E, s["odom_info"], at=P, per_edge=True)
        print("order %s: F sequential %.6g against %.6g at the optimum (factor %.1f); the closures' terms %s against %s" %
              (order, F_seq, F_opt, F_seq / F_opt, per_seq[n - 1:], per_opt[n - 1:]))
        assert F_opt <= F_seq
        assert per_seq[n - 1 + order[-1]] < 1e-18            # the closure applied last is met exactly, by construction
        for k in order[:-1]:                                  # the others are reopened: the optimum holds each of them closer
            assert per_opt[n - 1 + k] < per_seq[n - 1 + k]


# ---- every refusal ---------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(sage):
    lib, dp = sage.lib(), ctypes.POINTER(ctypes.c_double)
    s = scene("ring")
    poses, n, O = s["poses"], len(s["poses"]), np.ascontiguousarray(s["odom_info"]).reshape(36)
    good = gs.edges(sage, s)

    def ptr(a):
        return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)

    def refused(what, P=poses, n_=n, info=O, stride=0, edges=good, c=None, initial=None, want=sage.ERR_INVALID, out=True, **prm):
        arr = (sage.GraphEdge * max(1, len(edges)))(*edges) if edges is not None else None
        c_ = len(edges) if c is None else c
        params = sage.GraphParams()
        lib.sageicp_graph_params_default(ctypes.byref(params))
        params.where = 1
        for k, v in prm.items():
            setattr(params, k, v)
        Po, Co, gi = np.full((n, 7), 7.25), np.full((n, 7), 7.25), sage.GraphInfo()
        gi.cost_final = 7.25
        rc = lib.sageicp_graph_optimize(ptr(P), n_, ptr(info), stride, arr, c_, ptr(initial), ctypes.byref(params),
                                        Po.ctypes.data_as(dp) if out else None, Co.ctypes.data_as(dp), ctypes.byref(gi))
        assert rc == want, (what, rc)
        assert (Po == 7.25).all() and (Co == 7.25).all() and gi.cost_final == 7.25, what
        if out and want == sage.ERR_INVALID:
            cost, pe = ctypes.c_double(7.25), np.full(n - 1 + len(good) + 8, 7.25)
            if not prm and initial is None:
                rc = lib.sageicp_graph_cost(ptr(P), n_, ptr(info), stride, arr, c_, ptr(poses), ctypes.byref(cost), pe.ctypes.data_as(dp))
                assert rc == sage.ERR_INVALID and cost.value == 7.25 and (pe == 7.25).all(), what

    def edge(**kw):
        e = sage.GraphEdge.from_buffer_copy(good[0])
        for k, v in kw.items():
            if k in ("z", "info"):
                getattr(e, k)[:] = list(np.asarray(v, dtype=np.float64).reshape(-1))
            else:
                setattr(e, k, v)
        return [e, good[1]]

    refused("poses NULL", P=None)
    refused("odom_info NULL", info=None)
    refused("closures NULL with c > 0", edges=None, c=2)
    refused("poses_out NULL", out=False)
    refused("n == 1", n_=1, edges=[])
    refused("n == 0", n_=0, edges=[])
    refused("a == b", edges=edge(a=5, b=5))
    refused("a >= n", edges=edge(a=n))
    refused("b >= n", edges=edge(b=n + 3))
    refused("anchor >= n", anchor=n)
    refused("stride 6", stride=6)
    refused("stride 35", stride=35)
    refused("where 3", where=3)
    refused("step_tol NaN", step_tol=float("nan"))
    refused("step_tol < 0", step_tol=-1.0)
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 3, 6):
            P = poses.copy()
            P[n - 2, col] = bad
            refused("a non-finite pose", P=P)
            refused("a non-finite initial", initial=P)
            z = np.array(good[0].z[:])
            z[col] = bad
            refused("a non-finite z", edges=edge(z=z))
        M = np.array(s["odom_info"], dtype=np.float64)
        M[2, 2] = bad
        refused("a non-finite odom_info", info=M)
        refused("a non-finite closure info", edges=edge(info=M))
    P = poses.copy()
    P[3, :4] = 0.0
    refused("a pose's quaternion of norm 0", P=P)
    refused("initial's quaternion of norm 0", initial=P)
    refused("z's quaternion of norm 0", edges=edge(z=[0, 0, 0, 0, 1, 2, 3]))
    M = np.array(s["odom_info"], dtype=np.float64)
    M[1, 4] = 1e-300                                         # symmetric to 1e-300, not to the bit
    refused("an info not symmetric to the bit", info=M)
    refused("a closure info not symmetric to the bit", edges=edge(info=M))
    M = np.array(s["odom_info"], dtype=np.float64)
    M[0, 3] = M[3, 0] = 600.0                                # 100 * 2500 < 600^2: indefinite
    refused("an indefinite info", info=M)
    refused("an indefinite closure info", edges=edge(info=M))
    refused("a semidefinite info", info=np.zeros((6, 6)))
    per_edge = np.tile(np.asarray(s["odom_info"]).reshape(1, 36), (n - 1, 1))
    per_edge[n - 2, 0] = -1.0
    refused("the last per-edge info is not positive definite", info=per_edge, stride=36)
    refused("257 closures", edges=[good[0]] * 257, want=sage.ERR_CAPACITY)
    if lib.sageicp_device_count() == 0:
        refused("where = 2 without a device", where=2, want=sage.ERR_NO_DEVICE)
    # 256 closures are taken (two iterations are enough to see it run)
    _, _, info = sage.graph_optimize(poses[:12], [good[0].__class__.from_buffer_copy(e) for e in _many(sage, poses[:12], 256)],
                                     s["odom_info"], where="host", max_iterations=2, return_info=True)
    assert info["iterations"] >= 1
    # graph_edge: z = poses[i]^-1 * closed, and its refusals
    closed = cr.se3_mul(poses[0], np.array(good[0].z[:]))
    e = sage.graph_edge(poses, 0, 47, closed, 4.0 * gs.ODOM_INFO)
    assert (e.a, e.b) == (0, 47) and np.abs(np.array(e.z[:]) - np.array(good[0].z[:])).max() < 1e-14
    for args in ((poses, 0, 0, closed, gs.ODOM_INFO), (poses, 0, n, closed, gs.ODOM_INFO), (poses, 0, 5, closed * np.nan, gs.ODOM_INFO),
                 (poses, 0, 5, closed, -gs.ODOM_INFO)):
        with pytest.raises(Exception):
            sage.graph_edge(*args)
    with pytest.raises(ValueError):
        sage.graph_optimize(poses[:, :6], good, s["odom_info"])


def _many(sage, poses, c):
    rng = np.random.default_rng(31)
    out = []
    for k in range(c):
        a = int(rng.integers(0, len(poses)))
        b = int((a + 1 + rng.integers(0, len(poses) - 1)) % len(poses))
        z = pg.vmul(pg.vbetween(poses[a][None], poses[b][None]), pg.vexp(0.01 * rng.normal(size=(1, 6))))[0]
        e = sage.GraphEdge()
        e.a, e.b = a, b
        e.z[:] = list(z)
        e.info[:] = list(gs.ODOM_INFO.reshape(-1))
        out.append(e)
    return out
