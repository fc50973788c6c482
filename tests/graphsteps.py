"""ONE Gauss-Newton step of the pose-graph optimiser held to extended precision: the cases and the checks that
tests/test_posegraph_step_host.py (where = "host") and tests/test_posegraph_step_gpu.py (where = "device") share, so that
the two paths are asked the same questions.

The entry is run for one iteration (max_iterations = 1, max_halvings = 3) from graphscenes.stepped()'s start: no residual
is zero there, the odometry residuals lie on either side of kPgSeriesAngle, the closures' reach 3 rad, some quaternions
come with qw < 0.  After one accepted iteration the output is initial_k * exp(2^-halvings * delta_k), so the step itself
is held, vertex by vertex, to posegraphref.step_measured()'s np.longdouble step — not only where the iteration ends.

Bounds (none comes from the library's own numbers):
  * pose after the step: 4 * max(d_ref, u) from the longdouble x1.  d_ref is what the fp64 restatement (dense solve) is off
    by for this very graph; 4 is the project's margin over it (test_posegraph_host.py); u = 8 * 2^-53 * max(1, max |x1|) is
    the retraction's own rounding floor (a handful of fp64 operations per coordinate of x1).
  * halvings: the longdouble run's h, which step_measured() has shown not to hang on rounding.
  * step_last against 2^-h max |d|: a pose within `bound` in every coordinate has its tangent within 2 sqrt(3) bound to
    first order (quaternion components are half angles; three translation coordinates rotate into one).
  * cost_final against the longdouble F(x1): (E + 64) 2^-52 relative, the cost comparison of the scene tests (E terms
    re-associated, each a few ulps), plus 2 bound |grad F(x1)|_1 / F, what the allowed displacement can move F.
  * cost_initial (max_iterations = 0) against the longdouble F(x0): (E + 64) 2^-52.
  * grad_max against the longdouble gradient's largest entry at x0: (deg + 64) 2^-52 S, deg the most edges at one vertex
    and S = 2 max sum |J^T| |w| the size of the terms one entry is summed from.
  * rho, the relative residual of the library's step (recovered as log(x0_k^-1 out_k) / s in longdouble) under the
    longdouble graph: 4 * max(rho_ref, 2^-53) on the dense shapes, rho_ref the fp64 restatement's own; beyond them 4 * R,
    R the largest rho_ref the dense shapes of the run showed, floored at 2^-53.  Recovering the step divides the pose's
    rounding (2^-53 per coordinate of x1, relative to 1 for the quaternion) by s; that enters rho as 2^-53 |H| / S / s and
    is inside the margin of 4 at the sizes used (measured by rounding the longdouble x1 itself: 6e-17 ... 3e-16 of rho).

Under a robust kernel (ROBUST; tests/test_posegraph_robust_step_host.py and tests/test_posegraph_robust_step_gpu.py) the
same scenes go through sageicp_graph_optimize_robust, every function here takes the kernel and the scale, and the graph on
the reference's side is robustref.RobustGraph with c^2 = scale * scale formed in fp64 as the library forms it: F, its
gradient, d_ref, rho_ref, S and R are then those of the robust graph, and the rules above apply word for word.
"""
import math

import numpy as np

import graphscenes as gs
import posegraphref as pg
import robustref as rr

MAX_HALVINGS = 3
M_SIZES = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
ANCHORS = ("0", "1", "n//2", "n-2", "n-1")
COUNTS = (0, 1, 2, 7)


def _anchor(kind, n):
    return {"0": 0, "1": 1, "n//2": n // 2, "n-2": n - 2, "n-1": n - 1}[kind]


def _dense_cases():
    """(n, c, anchor, how): every free size with one (anchor, closure count) pair, the 20 pairs taken in turn (i mod 5 and
    i mod 4 run through all of them in 20 steps); then 43 spread closures at n = 130 (259 columns: one beyond a
    workgroup's 256 lanes), kPgMaxClosures = 256 at n = 9 and 66, and three closures of 3.0, 1.5 and 3.0 rad at n = 33, whose
    full step does not decrease F"""
    out = []
    for i, m in enumerate(M_SIZES):
        n = m + 1
        out.append((n, COUNTS[i % 4], _anchor(ANCHORS[i % 5], n), "edges"))
    out += [(130, 43, 1, "spread"), (9, 256, 0, "spread"), (66, 256, 33, "spread"), (33, 3, 0, "spread")]
    return out


# the closures' angles where they are not stepped()'s menu.  On the chains of 1 000 and 4 097 poses, up to a kilometre across,
# a closure of 0.25 rad moves poses by hundreds of metres and no step within three halvings decreases F: there the
# closures' angles are milliradians, and the odometry's menu alone crosses kPgSeriesAngle
BEYOND_ANGLES = (1e-3, 2.5e-4, 5e-4)
ANGLES = {(33, 3, 0, "spread"): (3.0, 1.5, 3.0)}


DENSE = _dense_cases()
SECOND = [(6, 7, 3, "edges"), (34, 7, 33, "edges"), (129, 7, 0, "edges")]          # m = 5, 33, 128
BEYOND = [(1000, 7, 0), (1000, 7, 500), (4097, 7, 0), (4097, 7, 2048)]
ANGLES.update({case: BEYOND_ANGLES for case in BEYOND})
LARGE_N = 262146

# The same scenes with a robust kernel on their closures: (case, kernel, the name of a scale for scale_of()).
# Every dense case with closures under each kernel at the library's scale; the small ones and the three closures of
# 3.0, 1.5, 3.0 rad also at a scale between their closures' terms
KERNELS = ("huber", "cauchy", "gm")
SCALES = ("default", "mid")
ROBUST = [(case, k, "default") for case in DENSE if case[1] > 0 for k in KERNELS] + \
         [(case, k, "mid") for case in DENSE if case[1] > 0 and (case[0] <= 17 or case == (33, 3, 0, "spread")) for k in KERNELS]
ROBUST_SECOND = [((34, 7, 33, "edges"), "gm", "default")]
ROBUST_BEYOND = [((1000, 7, 0), "cauchy", "default"), ((4097, 7, 2048), "cauchy", "default")]


def robust_id(rcase):
    return case_id(*rcase)


def case_id(case, kernel=None, scale=None):
    """scale: a number, or the name of one (SCALES)"""
    if kernel is None:
        return "n%d-c%d-a%d" % case[:3]
    return "n%d-c%d-a%d-%s-%s" % (case[:3] + (kernel, scale if isinstance(scale, str) else "%.6g" % scale))


_SCENES = {}


def scene_of(case):
    if case not in _SCENES:
        n, c, anchor = case[:3]
        how = case[3] if len(case) > 3 else "spread"
        _SCENES[case] = gs.stepped(n, c, seed=1000 * n + 10 * c + anchor, anchor=anchor, how=how, angles=ANGLES.get(case, gs.CLOSURE_ANGLES))
    return _SCENES[case]


def large_scene():
    """test_posegraph_gpu.py's large case — two laps of a circle of 5 cm, so that fp64 can factor the chain — at
    n = 262 146: m = 262 145 = 1024 * 256 + 1 free vertices leave every first-level kernel exactly one item for its second
    stride.  Three closures; the start disturbed as stepped() does, the translations by what the drive's own jitter is."""
    if "large" not in _SCENES:
        n = LARGE_N
        truth = gs.circle_truth(n, 0.05, per_lap=(n - 1) // 2)
        poses = gs.wander(truth, 77, trans=2e-5, rot=2e-6)
        closures = [(a, b, gs.rel(truth, a, b), gs.ODOM_INFO * 4.0) for a, b in ((0, 131000), (262145, 112200), (5, 262143))]
        base = dict(poses=poses, truth=truth, odom_info=gs.ODOM_INFO, closures=closures)
        _SCENES["large"] = gs.stepped(n, 3, seed=77, angles=(0.01, 0.2501, 1.5), trans=2e-5, base=base)
    return _SCENES["large"]


def scale_of(case, which):
    """the robust scale of a ROBUST case.  "default": the library's.  "mid": c^2 = sqrt(s_min s_max) of the closures' raw
    terms at the start under the fp64 restatement (one closure: c^2 = s), so closures lie on both sides of it"""
    if which == "default":
        return rr.SCALE
    s = scene_of(case)
    raw = pg.Graph(s["poses"], s["odom_info"], s["closures"], np.float64, case[2]).per_edge(s["initial"])[case[0] - 1:]
    return float(np.sqrt(np.sqrt(raw.min() * raw.max())))


def graph_of(s, dtype, anchor, kernel=None, scale=None):
    """the restatement of the scene's graph; under a kernel c^2 is scale * scale in fp64, as the library forms it"""
    if kernel is None:
        return pg.Graph(s["poses"], s["odom_info"], s["closures"], dtype, anchor)
    return rr.RobustGraph(s["poses"], s["odom_info"], s["closures"], dtype, anchor, kernel, float(scale) * float(scale))


def reference(case, x0=None, tag=None, kernel=None, scale=None):
    """step_measured of the case's scene from its own start (or from x0, under the key `tag`)"""
    s = scene_of(case)
    return pg.step_measured((case, tag), s["poses"], s["odom_info"], s["closures"], case[2], s["initial"] if x0 is None else x0, MAX_HALVINGS,
                            kernel=kernel, c2=None if kernel is None else float(scale) * float(scale))


def run(sage, s, anchor, where, x0=None, iterations=1, kernel=None, scale=None):
    robust = None if kernel is None else dict(kernel=kernel, scale=scale)
    return sage.graph_optimize(s["poses"], gs.edges(sage, s), s["odom_info"], initial=s["initial"] if x0 is None else x0, anchor=anchor,
                               max_iterations=iterations, max_halvings=MAX_HALVINGS, where=where, return_info=True, robust=robust)


def floor_of(x1):
    return 8.0 * 2.0 ** -53 * max(1.0, float(np.abs(np.asarray(x1, dtype=np.float64)).max()))


def recovered(x0, out, s, rows=None):
    """the step the library took, log(x0_k^-1 out_k) / s in longdouble, (n, 6); rows: only these (the others zero)"""
    x0, out = np.asarray(x0, dtype=np.longdouble), np.asarray(out, dtype=np.longdouble)
    d = np.zeros((len(x0), 6), dtype=np.longdouble)
    rows = slice(None) if rows is None else rows
    d[rows] = pg.vlog(pg.vbetween(x0[rows], out[rows])) / np.longdouble(s)
    return d


_RHO_REF = {}


def allowance(robust=False):
    """R: the largest rho_ref the fp64 restatement showed over the dense shapes (robust: over ROBUST, the dense shapes under
    their kernels), floored at 2^-53 — measured in the run"""
    if robust:
        return max(max(reference(case, kernel=k, scale=scale_of(case, which))["rho_ref"] for case, k, which in ROBUST), 2.0 ** -53)
    for case in DENSE:
        _RHO_REF[case] = reference(case)["rho_ref"]
    return max(max(_RHO_REF.values()), 2.0 ** -53)


def check_one_step(sage, where, case, x0=None, tag=None, kernel=None, scale=None):
    """the step from the scene's start (or from x0) against the longdouble step; returns the library's output.  kernel,
    scale: the robust entry under them, against the restatement of the same robust graph"""
    s, anchor = scene_of(case), case[2]
    m = reference(case, x0, tag, kernel, scale)
    start = s["initial"] if x0 is None else np.asarray(x0, dtype=np.float64)
    corr, out, info = run(sage, s, anchor, where, x0, kernel=kernel, scale=scale)
    E = len(out) - 1 + len(s["closures"])
    bound = 4.0 * max(m["d_ref"], floor_of(m["x1"]))
    dist = pg.distance(out, m["x1"])
    rho = graph_of(s, np.longdouble, anchor, kernel, scale).residual(start, recovered(start, out, 2.0 ** -info["halvings"]))
    dmax = float(np.abs(m["d"]).max())
    print("%s %s: h %d (reference %d), distance %.3g, d_ref %.3g, distance / d_ref %.3g (allowed %.3g), rho %.3g, rho_ref %.3g, "
          "the longdouble step's own rho %.3g, cond %.3g, max|d| %.3g, F %.6g -> %.6g"
          % (where, case_id(case, kernel, scale) + ("" if tag is None else "-" + str(tag)), info["halvings"], m["h"], dist, m["d_ref"], dist / m["d_ref"],
             bound, rho, m["rho_ref"], m["rho"], m["cond"], dmax, float(m["F0"]), info["cost_final"]))
    assert info["where"] == {"host": 1, "device": 2}[where]
    assert info["iterations"] == 1 and info["halvings"] == m["h"]
    assert gs.bits(out[anchor]) == gs.bits(start[anchor])
    assert dist <= bound
    assert abs(info["step_last"] - m["s"] * dmax) <= 2.0 * math.sqrt(3.0) * bound
    F1 = float(m["F1"])
    rel = (E + 64) * 2.0 ** -52 + 2.0 * bound * float(np.abs(m["grad1"]).sum()) / F1
    assert abs(info["cost_final"] - F1) <= rel * F1
    assert rho <= 4.0 * max(m["rho_ref"], 2.0 ** -53)
    return out


def check_the_start(sage, where, case, kernel=None, scale=None):
    """max_iterations = 0: cost_initial and grad_max at a point where neither is near zero; the poses come back as given.
    Under a kernel F is the robust F and grad_max its gradient's largest entry"""
    s, anchor = scene_of(case), case[2]
    m = reference(case, kernel=kernel, scale=scale)
    corr, out, info = run(sage, s, anchor, where, iterations=0, kernel=kernel, scale=scale)
    E = len(out) - 1 + len(s["closures"])
    F0 = float(m["F0"])
    G = graph_of(s, np.longdouble, anchor, kernel, scale)
    w, Ja, Jb = G.jacobians(s["initial"])
    size = np.zeros((G.n, 6), dtype=np.longdouble)
    np.add.at(size, G.a, np.einsum("eki,ek->ei", np.abs(Ja), np.abs(w)))
    np.add.at(size, G.b, np.einsum("eki,ek->ei", np.abs(Jb), np.abs(w)))
    S, want = 2.0 * float(size.max()), float(np.abs(m["grad0"]).max())
    print("%s %s: cost_initial off by %.3g of F0 = %.6g (allowed %.3g); grad_max %.17g, longdouble %.17g: off by %.3g of S = %.4g (allowed %.3g)"
          % (where, case_id(case, kernel, scale), abs(info["cost_initial"] - F0) / F0, F0, (E + 64) * 2.0 ** -52, info["grad_max"], want,
             abs(info["grad_max"] - want) / S, S, (m["deg"] + 64) * 2.0 ** -52))
    assert info["iterations"] == 0 and gs.bits(out) == gs.bits(s["initial"])
    assert abs(info["cost_initial"] - F0) <= (E + 64) * 2.0 ** -52 * F0 and info["cost_final"] == info["cost_initial"]
    assert abs(info["grad_max"] - want) <= (m["deg"] + 64) * 2.0 ** -52 * S


def check_the_robust_scenes_decide():
    """conditions on ROBUST alone (the restatement; no library): every reference accepts within MAX_HALVINGS on trials that
    rounding cannot turn (step_measured asserts both); at the starts Huber has closures of weight 1 and of weight below 1 in
    one case, and under each of the other two kernels there are weights below 1e-3 and weights above 0.9"""
    both, lo, hi, span = [], {k: 0 for k in KERNELS}, {k: 0 for k in KERNELS}, [1.0, 0.0]
    for case, kernel, which in ROBUST:
        scale = scale_of(case, which)
        m, s = reference(case, kernel=kernel, scale=scale), scene_of(case)
        w = graph_of(s, np.longdouble, case[2], kernel, scale).weights(s["initial"]).astype(np.float64)
        assert m["h"] <= MAX_HALVINGS and len(w) == case[1] and ((w > 0) & (w <= 1)).all()
        span = [min(span[0], float(w.min())), max(span[1], float(w.max()))]
        lo[kernel] += int((w < 1e-3).sum())
        hi[kernel] += int((w > 0.9).sum())
        if kernel == "huber" and (w == 1.0).any() and (w < 1.0).any():
            both.append(case_id(case, kernel, which))
    print("%d robust cases; weights at the starts %.3g ... %.3g; below 1e-3 %s; above 0.9 %s; Huber on both branches in %d cases: %s"
          % (len(ROBUST), span[0], span[1], lo, hi, len(both), " ".join(both)))
    assert both and all(lo[k] and hi[k] for k in ("cauchy", "gm"))


def check_the_scenes_decide(robust=False):
    """conditions on the scenes alone (the restatement; no library): every reference accepts within MAX_HALVINGS on trials
    that rounding cannot turn (step_measured asserts both); over the accepted cases there are closure residuals at 0.2501,
    1.5 and 3.0 rad, odometry residuals on both sides of kPgSeriesAngle with none zero, and quaternions with qw < 0 on
    both kinds of edge.  robust: check_the_robust_scenes_decide(), the conditions on ROBUST"""
    if robust:
        return check_the_robust_scenes_decide()
    seen, odo_lo, odo_hi, neg_odo, neg_clo, hs = set(), 0, 0, 0, 0, set()
    for case in DENSE:
        m, n = reference(case), case[0]
        th, qw = m["theta"], m["qw"]
        assert (th[:n - 1] > 5e-4).all()
        odo_lo += int((th[:n - 1] < 0.25).sum())
        odo_hi += int((th[:n - 1] >= 0.25).sum())
        neg_odo += int((qw[:n - 1] < 0).sum())
        neg_clo += int((qw[n - 1:] < 0).sum())
        hs.add(m["h"])
        for a in (0.2499, 0.2501, 1.5, 3.0):
            if (np.abs(th[n - 1:] - a) < 1e-9).any():
                seen.add(a)
    print("halvings taken %s; closure angles met %s; odometry residuals below / above 0.25 rad: %d / %d; qw < 0 on %d odometry and %d closure edges"
          % (sorted(hs), sorted(seen), odo_lo, odo_hi, neg_odo, neg_clo))
    assert seen == {0.2499, 0.2501, 1.5, 3.0} and odo_lo and odo_hi and neg_odo and neg_clo


def cond_bound(G, x, n):
    """|H|_inf / lambda: the largest row sum of |sum J^T J| over the chain's softest mode, lambda = 100 (pi / (2 n))^2
    (test_posegraph_gpu.py)"""
    w, Ja, Jb = G.jacobians(x)
    rows = np.zeros((G.n, 6))
    both = np.abs(Ja) + np.abs(Jb)
    np.add.at(rows, G.a, np.einsum("eki,ekj->ei", np.abs(Ja), both))
    np.add.at(rows, G.b, np.einsum("eki,ekj->ei", np.abs(Jb), both))
    return float(rows.max()) / (100.0 * (math.pi / (2.0 * n)) ** 2)


def check_beyond(sage, wheres, s, anchor, R, sample=None, name="", kernel=None, scale=None):
    """no dense restatement: the residual of each path's step under the longdouble graph (at `sample`), and the paths
    against each other within 4 R cond_bound max|d|.  kernel, scale: the robust entry and the robust graph (whole graphs
    only: RobustGraph tells its closures by their place among all the edges)"""
    assert kernel is None or sample is None
    x0, n = s["initial"], len(s["poses"])
    G = graph_of(s, np.longdouble, anchor, kernel, scale)
    outs = {}
    for where in wheres:
        corr, out, info = run(sage, s, anchor, where, kernel=kernel, scale=scale)
        assert info["iterations"] == 1 and info["halvings"] <= MAX_HALVINGS and gs.bits(out[anchor]) == gs.bits(x0[anchor])
        assert info["cost_final"] < info["cost_initial"]
        rows = None
        if sample is not None:                                   # the sample and the other ends of its edges
            keep = np.zeros(n, dtype=bool)
            keep[sample] = True
            sel = keep[G.a] | keep[G.b]
            rows = np.unique(np.concatenate([G.a[sel], G.b[sel]]))
        d = recovered(x0, out, 2.0 ** -info["halvings"], rows)
        rho = G.residual(x0, d, sample)
        print("%s %s n %d anchor %d: h %d, rho %.3g (R %.3g, allowed %.3g), step_last %.3g, F %.6g -> %.6g"
              % (where, name, n, anchor, info["halvings"], rho, R, 4.0 * R, info["step_last"], info["cost_initial"], info["cost_final"]))
        outs[where] = (out, info, d, rho)
    if len(outs) == 2:
        (oa, ia, da, _), (ob, ib, _, _) = outs["host"], outs["device"]
        G64 = graph_of(s, np.float64, anchor, kernel, scale)
        if sample is not None:
            G64.a, G64.b, G64.zinv, G64.L, G64.E = G64.a[sel], G64.b[sel], G64.zinv[sel], G64.L[sel], int(sel.sum())
        allowed = 4.0 * R * cond_bound(G64, x0, n) * float(np.abs(da).max())
        print("  host and device %.3g apart (allowed %.3g)" % (pg.distance(oa, ob), allowed))
        assert ia["halvings"] == ib["halvings"] and pg.distance(oa, ob) <= allowed
    for where in wheres:                                         # (last, so that every path's figures are printed first)
        assert outs[where][3] <= 4.0 * R, (where, outs[where][3])
    return outs


def check_a_second_step(sage, where, case, kernel=None, scale=None):
    """two iterations in one call reuse the first's buffers (under a kernel the `lin` buffer then holds scaled blocks):
    their output is, to the bit, one step (held to the reference computed at that point) from the output of a call of one
    iteration"""
    s, anchor = scene_of(case), case[2]
    first = check_one_step(sage, where, case, kernel=kernel, scale=scale)
    second = check_one_step(sage, where, case, x0=first, tag="second-" + where, kernel=kernel, scale=scale)
    corr, both, info = run(sage, s, anchor, where, iterations=2, kernel=kernel, scale=scale)
    assert info["iterations"] == 2 and gs.bits(both) == gs.bits(second)


HUBER_BEYOND = 1e9                                               # c^2 = 1e18: no closure term of these scenes is near it


def check_huber_beyond_every_term(sage, where, s, **kw):
    """Huber at a scale beyond every closure term is the identity on them: sqrt(rho') = 1 and rho = s, so the call is
    kernel "none" bit for bit — poses, corrections and every field of sageicp_graph_info"""
    E = gs.edges(sage, s)
    call = lambda kernel: sage.graph_optimize(s["poses"], E, s["odom_info"], where=where, return_info=True,
                                              robust=dict(kernel=kernel, scale=HUBER_BEYOND), **kw)
    (c0, o0, i0), (c1, o1, i1) = call("none"), call("huber")
    raw = graph_of(s, np.float64, kw.get("anchor", 0)).per_edge(s["poses"] if kw.get("initial") is None else kw["initial"])
    assert raw[len(o0) - 1:].max() < 1e-6 * HUBER_BEYOND ** 2 and i1["closure_chi2"].max() < 1e-6 * HUBER_BEYOND ** 2
    plain = [k for k in i0 if k not in ("closure_chi2", "closure_weight", "stages", "outliers", "scale2_first")]
    print("%s n %d: %d iterations, F %.17g -> %.17g" % (where, len(o0), i1["iterations"], i1["cost_initial"], i1["cost_final"]))
    assert len(plain) == 9 and i1["iterations"] >= 1 and i1["where"] == {"host": 1, "device": 2}[where]
    assert gs.bits(o1) == gs.bits(o0) and gs.bits(c1) == gs.bits(c0)
    for k in plain:
        assert gs.bits(np.float64(i1[k])) == gs.bits(np.float64(i0[k])), (k, i0[k], i1[k])
    assert gs.bits(i1["closure_chi2"]) == gs.bits(i0["closure_chi2"])
    assert (i1["closure_weight"] == 1.0).all() and i1["outliers"] == 0 and i1["stages"] == 1
