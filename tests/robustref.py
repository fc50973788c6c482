"""Plain numpy restatement of the robust pose-graph optimiser (include/sageicp.h "robust pose graph"), for the
tests only: posegraphref.Graph with a kernel rho on the closures' terms.

  * rho(), weight(): the table of the header, in any numpy float type;
  * RobustGraph: per_edge() puts rho on the closure edges (so cost() is the robust F), jacobians() scales a closure's w, Ja,
    Jb by sqrt(rho'(s)) — everything posegraphref builds from them (gradient, step, gauss_newton) is then IRLS Gauss-Newton
    on that F; raw() and weights() are the closures' s and rho'(s);
  * schedule(): the stages of the scale continuation, fixed by s0 alone;
  * solve(): the stages run one after another, each but the last for at most stage_iterations accepted steps, the last to
    a stall; polish(): Gauss-Newton to a stall at the final scale from a given point;
  * measured(): per (scene, kernel, anneal) the longdouble run, the fp64 run and d_ref, their distance — computed once."""
import numpy as np

import posegraphref as pg

KERNELS = ("none", "huber", "cauchy", "gm")
SCALE = float(np.sqrt(16.81))                                    # chi-square, 6 dof, 99 %
STEP_TOL = 1e-9


def rho(kernel, c2, s):
    s = np.asarray(s)
    f = s.dtype.type
    c2 = f(c2)
    if kernel == "huber":
        return np.where(s <= c2, s, f(2) * np.sqrt(c2 * s) - c2)
    if kernel == "cauchy":
        return c2 * np.log1p(s / c2)
    if kernel == "gm":
        return c2 * s / (c2 + s)
    return s.copy()


def weight(kernel, c2, s):
    s = np.asarray(s)
    f = s.dtype.type
    c2 = f(c2)
    if kernel == "huber":
        return np.where(s <= c2, f(1), np.sqrt(c2 / np.where(s > 0, s, f(1))))
    if kernel == "cauchy":
        return f(1) / (f(1) + s / c2)
    if kernel == "gm":
        return (c2 / (c2 + s)) ** 2
    return np.ones_like(s)


class RobustGraph(pg.Graph):
    def __init__(self, poses, odom_info, closures, dtype=np.float64, anchor=0, kernel="none", c2=SCALE * SCALE):
        super().__init__(poses, odom_info, closures, dtype, anchor)
        self.kernel, self.c2 = kernel, c2

    def raw(self, x):
        """the closures' s = r^T info r"""
        return pg.Graph.per_edge(self, x)[self.n - 1:]

    def weights(self, x):
        return weight(self.kernel, self.c2, self.raw(x))

    def per_edge(self, x):
        s = pg.Graph.per_edge(self, x)
        s[self.n - 1:] = rho(self.kernel, self.c2, s[self.n - 1:])
        return s

    def jacobians(self, x, mode="exact"):
        w, Ja, Jb = pg.Graph.jacobians(self, x, mode)
        sw = np.ones(self.E, dtype=self.dtype)
        sw[self.n - 1:] = np.sqrt(weight(self.kernel, self.c2, (w * w).sum(axis=1)[self.n - 1:]))
        return w * sw[:, None], Ja * sw[:, None, None], Jb * sw[:, None, None]


def schedule(s0, c2, factor=2.0, anneal=True):
    """the stages' c^2, first to last: c2 f^m, ..., c2 f, c2 with m the smallest count with c2 f^m >= s0"""
    out = [float(c2)]
    if anneal:
        while out[-1] < s0:
            out.append(out[-1] * float(factor))
    return out[::-1]


def _stage(G, x, max_iterations, to_stall, max_halvings=40):
    """Gauss-Newton with backtracking at G's scale: to a stall, or at most max_iterations accepted steps, ending on a step
    <= STEP_TOL as the library's status 0 does"""
    x = np.asarray(x).astype(G.dtype)
    F = G.cost(x)
    for _ in range(max_iterations):
        d, _H = G.step(x)
        s, ok = 1.0, False
        for _h in range(max_halvings + 1):
            xt = G.retract(x, s * d)
            Ft = G.cost(xt)
            if Ft < F:
                x, F, ok = xt, Ft, True
                break
            s *= 0.5
        if not ok or (not to_stall and float(np.abs(s * d).max()) <= STEP_TOL):
            break
    return x


def solve(G, x0, anneal=False, factor=2.0, stage_iterations=3, max_iterations=300):
    """(x, the stages' c^2).  G.c2 is the final scale, and is left at it"""
    c2 = G.c2
    s0 = float(G.raw(x0).max()) if G.E > G.n - 1 else 0.0
    stages = schedule(s0, c2, factor, anneal)
    x = np.asarray(x0).astype(G.dtype)
    for k, v in enumerate(stages):
        G.c2 = v
        last = k == len(stages) - 1
        x = _stage(G, x, max_iterations if last else stage_iterations, to_stall=last)
    G.c2 = c2
    return x, stages


def polish(poses, odom_info, closures, kernel, x, anchor=0, c2=SCALE * SCALE):
    """x run to a stall at the final scale, in np.longdouble"""
    G = RobustGraph(poses, odom_info, closures, np.longdouble, anchor, kernel, c2)
    return _stage(G, x, 300, to_stall=True)


_MEASURED = {}


def measured(key, poses, odom_info, closures, kernel, anneal=False, anchor=0, c2=SCALE * SCALE):
    """dict(opt: the longdouble run from the poses, opt64: the fp64 run, d_ref: their distance, weights and raw: the closures'
    at opt, stages) — computed once per key"""
    key = (key, kernel, anneal)
    if key not in _MEASURED:
        Gl = RobustGraph(poses, odom_info, closures, np.longdouble, anchor, kernel, c2)
        G64 = RobustGraph(poses, odom_info, closures, np.float64, anchor, kernel, c2)
        xl, stages = solve(Gl, poses, anneal)
        x64, _ = solve(G64, poses, anneal)
        _MEASURED[key] = dict(opt=xl, opt64=x64, d_ref=pg.distance(x64, xl), weights=Gl.weights(xl).astype(np.float64),
                              raw=Gl.raw(xl).astype(np.float64), stages=stages, F=float(Gl.cost(xl)))
    return _MEASURED[key]
