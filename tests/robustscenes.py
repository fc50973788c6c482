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
