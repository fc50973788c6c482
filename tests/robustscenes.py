"""Scenes for the robust pose-graph tests (tests/test_posegraph_robust_host.py, tests/test_posegraph_robust_gpu.py), built
from tests/graphscenes.py: a drive with true closures plus aliased ones — a place matched to a neighbouring place of a
repetitive street, so the measurement is a good relative pose of the WRONG pair.  A scene is graphscenes' dict plus
false: the indices of the aliased closures, and clean: the same scene without them."""
import numpy as np

import graphscenes as gs
import posegraphref as pg
import robustref as rr

INFO = 4.0 * gs.ODOM_INFO


def _with_false(base, extra):
    s = dict(base)
    truth = base["truth"]
    s["closures"] = list(base["closures"]) + [(a, b, gs.rel(truth, ta, tb), INFO.copy()) for a, b, ta, tb in extra]
    s["false"] = list(range(len(base["closures"]), len(s["closures"])))
    s["clean"] = base
    return s


def two_laps():
    return _with_false(gs.two_laps(), [(10, 70, 22, 70)])


def ring():
    return _with_false(gs.ring(), [(10, 40, 10, 16)])


def hard():
    """two laps from a start that has drifted so far that the TRUE closures lie outside c^2 as well: what decides the
    scale continuation"""
    base = gs.two_laps()
    base["poses"] = gs.drift(base["truth"], 23, trans_frac=0.15, rot=1e-2)
    return _with_false(base, [(10, 70, 22, 70), (30, 90, 36, 84)])


SCENES = {"two_laps": two_laps, "ring": ring, "hard": hard}
# what each scene is solved under: (kernel, anneal)
CASES = {"two_laps": (("huber", False), ("cauchy", False), ("gm", False), ("gm", True)),
         "ring": (("huber", False), ("cauchy", False), ("gm", False), ("gm", True)),
         "hard": (("cauchy", False), ("gm", False), ("gm", True))}
_SCENE = {}


def scene(name):
    if name not in _SCENE:
        _SCENE[name] = SCENES[name]()
    return _SCENE[name]


def measured(name, kernel, anneal):
    s = scene(name)
    return rr.measured(name, s["poses"], s["odom_info"], s["closures"], kernel, anneal)


def clean_optimum(name):
    s = scene(name)["clean"]
    return pg.measured(("robust-clean", name), s["poses"], s["odom_info"], s["closures"], identity=False)["opt"]


def optimize(sage, s, kernel, anneal=False, where="host", **kw):
    robust = None if kernel is None else dict(kernel=kernel, anneal=int(anneal))
    return sage.graph_optimize(s["poses"], gs.edges(sage, s), s["odom_info"], where=where, return_info=True, robust=robust, **kw)


def held_to_the_rule(s, kernel, out, ref, what=""):
    """the tolerance rule: `out` within 4 max(d_ref, STEP_TOL) of itself polished in np.longdouble at the final scale.
    Returns (bound, distance to the polished point)"""
    bound = 4.0 * max(ref["d_ref"], gs.STEP_TOL)
    x = rr.polish(s["poses"], s["odom_info"], s["closures"], kernel, out, anchor=ref.get("anchor", 0))
    d = pg.distance(out, x)
    print("%s %s: d_ref %.3g, %.3g from its own polished point (allowed %.3g)" % (what, kernel, ref["d_ref"], d, bound))
    return bound, d


# ---- decisions on inputs that decide -----------------------------------------------------------------------------------------
def exactly_at_a_scale(sage, also=lambda scale, term: True):
    """(scene, edges, scale, term): a chain of 17 poses whose one closure has, at the poses as given, a raw term with
    sqrt(term)^2 == term in fp64 (an information scaled until it is so), so that scale = sqrt(term) puts c^2 on the term to
    the bit; also(scale, term): a further condition on the pair, decided by the restatement's own fp64 arithmetic"""
    base = gs.chain(17, 1, seed=11, how="spread")
    a, b, z, info0 = base["closures"][0]
    for j in range(64):
        s = dict(base, closures=[(a, b, z, info0 * (1.0 + j / 64.0))])
        E = gs.edges(sage, s)
        _, per = sage.graph_cost(s["poses"], E, s["odom_info"], per_edge=True)
        scale = float(np.sqrt(per[-1]))
        if scale * scale == per[-1] and per[-1] > 0.0 and also(scale, float(per[-1])):
            return s, E, scale, float(per[-1])
    raise AssertionError("no information among 64 gives sqrt(s)^2 == s")


def _stopped_at_the_start(sage, s, E, where, **robust):
    _, out, info = sage.graph_optimize(s["poses"], E, s["odom_info"], where=where, return_info=True, max_iterations=0, robust=robust)
    assert info["where"] == {"host": 1, "device": 2}[where]
    return out, info


def check_the_verdict_at_a_weight_of_a_half(sage, where):
    """Cauchy's weight is 1 / (1 + s / c^2): exactly 0.5 at c^2 == s, which is NOT an outlier (the verdict is weight < 0.5);
    one ulp of scale below, the weight is under 0.5 and the closure is one.  The scene is one where fp64 itself puts
    1 / (1 + s / c^2) under 0.5 at that scale (for half of all mantissas 1 + s / c^2 rounds back to 2)"""
    below = lambda scale: float(np.nextafter(scale, 0.0))
    decided = lambda scale, term: float(rr.weight("cauchy", below(scale) * below(scale), np.float64(term))) < 0.5
    s, E, scale, term = exactly_at_a_scale(sage, decided)
    out, info = _stopped_at_the_start(sage, s, E, where, kernel="cauchy", scale=scale)
    print("%s: s = c^2 = %.17g: weight %.17g, outliers %d" % (where, term, info["closure_weight"][0], info["outliers"]))
    assert gs.bits(out) == gs.bits(s["poses"]) and info["iterations"] == 0
    assert info["closure_chi2"][0] == term == scale * scale
    assert gs.bits(info["closure_weight"][0]) == gs.bits(0.5) and info["outliers"] == 0
    out, info = _stopped_at_the_start(sage, s, E, where, kernel="cauchy", scale=below(scale))
    print("%s: one ulp of scale below: weight %.17g, outliers %d" % (where, info["closure_weight"][0], info["outliers"]))
    assert gs.bits(out) == gs.bits(s["poses"]) and info["closure_chi2"][0] == term
    assert info["closure_weight"][0] < 0.5 and info["outliers"] == 1


def check_the_schedule_at_a_power_of_the_factor(sage, where):
    """the continuation's stages c^2 f^m, ..., c^2 with m the smallest count with c^2 f^m >= s0: at s0 == c^2 f^2 exactly
    (scale = sqrt(s0) / 2, f = 2) there are three, the first at s0 to the bit; one ulp of scale below there are four, the
    first at 8 c^2.  robustref.schedule counts the same, by itself"""
    s, E, scale, term = exactly_at_a_scale(sage)
    for sc, stages, first in ((0.5 * scale, 3, term), (float(np.nextafter(0.5 * scale, 0.0)), 4, None)):
        first = 8.0 * sc * sc if first is None else first
        want = rr.schedule(term, sc * sc, 2.0)
        assert len(want) == stages and gs.bits(want[0]) == gs.bits(first)
        _, _, info = sage.graph_optimize(s["poses"], E, s["odom_info"], where=where, return_info=True, max_iterations=0,
                                         robust=dict(kernel="gm", anneal=1, anneal_factor=2.0, scale=sc))
        print("%s: scale %.17g, s0 %.17g: %d stages from c^2 = %.17g" % (where, sc, term, info["stages"], info["scale2_first"]))
        assert info["where"] == {"host": 1, "device": 2}[where]
        assert info["stages"] == stages and gs.bits(info["scale2_first"]) == gs.bits(first)
    assert 0.25 * term == (0.5 * scale) ** 2
