"""Plain numpy restatement of the pose-graph optimiser (include/sageicp.h "pose graph"), for the tests only,
written from the definitions:

  * vectorised SE(3) over rows (N, 7) in any numpy float type, in the operation order of csrc/se3_math.h and posegraph.h
    (closureref's scalar functions are what they are checked against in test_posegraph_host.py);
  * whitened(): every edge's L^T r, so F = sum |L^T r|^2; cost(); gradient(): dF/d delta per pose, with the edges'
    Jacobians by FOURTH-order central differences in the given type (np.longdouble: h = 1e-4, truncation ~ h^4 = 1e-16);
  * gauss_newton(): the dense Gauss-Newton with backtracking for n <= 130, the linear solve in fp64 (a step's accuracy
    does not move the fixed point, which is where the gradient of the chosen type vanishes); mode "identity" replaces
    Jr^-1 by I — the approximation the library must NOT be;
  * measured(): for a scene, the longdouble optimum, d_ref = the distance between the fp64 and the longdouble runs, both
    run to a stall, and the contraction ratio of the late steps — asserted <= 0.8 here, on the restatement's own;
  * step_exact(): ONE Gauss-Newton step to the precision of the graph's type (the dense system assembled from the edges'
    blocks in that type, an fp64 factorisation refined with residuals of that type); residual(): what a given step leaves
    of H d + g, edge by edge with no dense matrix, relative to the size of its terms; step_measured(): for a scene and a
    start, the longdouble step, the halvings the longdouble run takes, the pose after it, and how far the fp64
    restatement's own step is from all of that — what tests/graphsteps.py holds one step of the library to."""
import copy

import numpy as np

import closureref as cr


def _f(dtype):
    return np.dtype(dtype).type


# ---- SE(3) over rows -----------------------------------------------------------------------------------------------------
def vrot(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = np.empty((len(q), 3, 3), dtype=q.dtype)
    R[:, 0, 0] = one - two * (yy + zz); R[:, 0, 1] = two * (xy - wz); R[:, 0, 2] = two * (xz + wy)
    R[:, 1, 0] = two * (xy + wz); R[:, 1, 1] = one - two * (xx + zz); R[:, 1, 2] = two * (yz - wx)
    R[:, 2, 0] = two * (xz - wy); R[:, 2, 1] = two * (yz + wx); R[:, 2, 2] = one - two * (xx + yy)
    return R


def _apply(R, p):
    return np.stack([R[:, i, 0] * p[:, 0] + R[:, i, 1] * p[:, 1] + R[:, i, 2] * p[:, 2] for i in range(3)], axis=1)


def _qmul(a, b):
    ax, ay, az, aw = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=1)
    return q / np.sqrt((q * q).sum(axis=1))[:, None]


def vmul(A, B):
    return np.concatenate([_qmul(A[:, :4], B[:, :4]), _apply(vrot(A[:, :4]), B[:, 4:]) + A[:, 4:]], axis=1)


def vinv(A):
    qi = A[:, :4] * np.array([-1, -1, -1, 1], dtype=A.dtype)
    return np.concatenate([qi, -_apply(vrot(qi), A[:, 4:])], axis=1)


def vbetween(A, B):
    """A^-1 B, the translations subtracted first (posegraph.h pg_between)"""
    qi = A[:, :4] * np.array([-1, -1, -1, 1], dtype=A.dtype)
    return np.concatenate([_qmul(qi, B[:, :4]), _apply(vrot(qi), B[:, 4:] - A[:, 4:])], axis=1)


def _cross(w, u):
    return np.stack([w[:, 1] * u[:, 2] - w[:, 2] * u[:, 1], w[:, 2] * u[:, 0] - w[:, 0] * u[:, 2],
                     w[:, 0] * u[:, 1] - w[:, 1] * u[:, 0]], axis=1)


def vlog(T):
    f = T.dtype.type
    n2 = (T[:, :3] * T[:, :3]).sum(axis=1)
    qw = T[:, 3]
    small = n2 < 1e-20
    n = np.sqrt(np.where(small, f(1), n2))
    at = np.where(qw < 0, np.arctan2(-n, -qw), np.arctan2(n, qw))
    k = np.where(small, f(2) / qw - (f(2) / f(3)) * n2 / (qw * qw * qw), f(2) * at / n)
    th = np.where(small, f(2) * n2 / qw, k * n)
    w = k[:, None] * T[:, :3]
    tiny = np.abs(th) < 1e-10
    ths = np.where(tiny, f(1), th)
    half = f(0.5) * ths
    c = np.where(tiny, f(1) / f(12), (f(1) - ths * np.cos(half) / (f(2) * np.sin(half))) / (ths * ths))
    t = T[:, 4:]
    c1 = _cross(w, t)
    c2 = _cross(w, c1)
    return np.concatenate([t - f(0.5) * c1 + c[:, None] * c2, w], axis=1)


def vexp(a):
    f = a.dtype.type
    w, u = a[:, 3:], a[:, :3]
    th2 = (w * w).sum(axis=1)
    th = np.sqrt(th2)
    tiny = th < 1e-10
    ths = np.where(tiny, f(1), th)
    t2 = ths * ths
    th4 = th2 * th2
    half = f(0.5) * ths
    imag = np.where(tiny, f(0.5) - th2 / f(48) + th4 / f(3840), np.sin(half) / ths)
    real = np.where(tiny, f(1) - th2 / f(8) + th4 / f(384), np.cos(half))
    A = np.where(tiny, f(0.5) - th2 / f(24), (f(1) - np.cos(ths)) / t2)
    B = np.where(tiny, f(1) / f(6) - th2 / f(120), (ths - np.sin(ths)) / (t2 * ths))
    c1 = _cross(w, u)
    c2 = _cross(w, c1)
    return np.concatenate([imag[:, None] * w, real[:, None], u + A[:, None] * c1 + B[:, None] * c2], axis=1)


def _hat(t):
    H = np.zeros((len(t), 3, 3), dtype=t.dtype)
    H[:, 0, 1] = -t[:, 2]; H[:, 0, 2] = t[:, 1]
    H[:, 1, 0] = t[:, 2]; H[:, 1, 2] = -t[:, 0]
    H[:, 2, 0] = -t[:, 1]; H[:, 2, 1] = t[:, 0]
    return H


def vadjoint(T):
    """Ad(T) for the tangent (upsilon, omega): [[R, hat(t) R], [0, R]]"""
    R = vrot(T[:, :4])
    Ad = np.zeros((len(T), 6, 6), dtype=T.dtype)
    Ad[:, :3, :3] = R
    Ad[:, 3:, 3:] = R
    Ad[:, :3, 3:] = _hat(T[:, 4:]) @ R
    return Ad


# ---- the graph -----------------------------------------------------------------------------------------------------------
class Graph:
    """poses (n, 7) fp64; odom_info 6x6 or (n - 1, 6, 6); closures: list of (a, b, z[7], info 6x6); dtype of the arithmetic"""

    def __init__(self, poses, odom_info, closures, dtype=np.float64, anchor=0):
        self.dtype = np.dtype(dtype)
        P = np.asarray(poses, dtype=np.float64).astype(dtype)
        self.n, self.anchor = len(P), anchor
        c = len(closures)
        self.a = np.concatenate([np.arange(self.n - 1), np.array([e[0] for e in closures], dtype=np.int64)]).astype(np.int64)
        self.b = np.concatenate([np.arange(1, self.n), np.array([e[1] for e in closures], dtype=np.int64)]).astype(np.int64)
        Z = vbetween(P[:-1], P[1:])
        if c:
            Z = np.concatenate([Z, np.array([e[2] for e in closures], dtype=np.float64).astype(dtype)])
        self.zinv = vinv(Z)
        O = np.asarray(odom_info, dtype=np.float64)
        O = np.broadcast_to(O.reshape(-1, 6, 6), (self.n - 1, 6, 6)) if O.size == 36 else O.reshape(self.n - 1, 6, 6)
        infos = np.concatenate([O, np.array([e[3] for e in closures], dtype=np.float64).reshape(c, 6, 6)]) if c else O
        self.L = np.linalg.cholesky(infos).astype(dtype)              # (E, 6, 6), info = L L^T
        self.E = len(self.a)

    def whitened_of(self, xa, xb, sel=slice(None)):
        r = vlog(vmul(self.zinv[sel], vbetween(xa, xb)))
        return np.einsum("eki,ek->ei", self.L[sel], r)

    def whitened(self, x):
        x = np.asarray(x).astype(self.dtype)
        return self.whitened_of(x[self.a], x[self.b])

    def per_edge(self, x):
        w = self.whitened(x)
        return (w * w).sum(axis=1)

    def cost(self, x):
        return self.per_edge(x).sum()

    def jacobians(self, x, mode="exact"):
        """(w, Ja, Jb): d w / d delta_a, d w / d delta_b per edge, (E, 6, 6).  exact: fourth-order central differences;
        identity: Jr^-1 replaced by I (Jb = L^T, Ja = -L^T Ad((x_a^-1 x_b)^-1))"""
        x = np.asarray(x).astype(self.dtype)
        xa, xb = x[self.a], x[self.b]
        w = self.whitened_of(xa, xb)
        Lt = np.swapaxes(self.L, 1, 2)
        if mode == "identity":
            Ad = vadjoint(vinv(vbetween(xa, xb)))
            return w, -(Lt @ Ad), Lt.copy()
        f = self.dtype.type
        h = f(1e-4) if self.dtype == np.dtype(np.longdouble) else f(2e-3)
        Ja = np.empty((self.E, 6, 6), dtype=self.dtype)
        Jb = np.empty_like(Ja)
        for i in range(6):
            def at(side, s):
                d = np.zeros((self.E, 6), dtype=self.dtype)
                d[:, i] = s * h
                e = vexp(d)
                return self.whitened_of(vmul(xa, e), xb) if side == 0 else self.whitened_of(xa, vmul(xb, e))
            for side, J in ((0, Ja), (1, Jb)):
                J[:, :, i] = (f(8) * (at(side, 1) - at(side, -1)) - (at(side, 2) - at(side, -2))) / (f(12) * h)
        return w, Ja, Jb

    def gradient(self, x, mode="exact"):
        """dF/d delta, (n, 6), the anchor's row zero"""
        w, Ja, Jb = self.jacobians(x, mode)
        g = np.zeros((self.n, 6), dtype=self.dtype)
        np.add.at(g, self.a, np.einsum("eki,ek->ei", Ja, w))
        np.add.at(g, self.b, np.einsum("eki,ek->ei", Jb, w))
        g *= self.dtype.type(2)
        g[self.anchor] = 0
        return g

    def step(self, x, mode="exact"):
        """the Gauss-Newton step (n, 6), by a dense fp64 solve"""
        assert self.n <= 130
        w, Ja, Jb = self.jacobians(x, mode)
        J = np.zeros((6 * self.E, 6 * self.n))
        for e in range(self.E):
            J[6 * e:6 * e + 6, 6 * self.a[e]:6 * self.a[e] + 6] = Ja[e].astype(np.float64)
            J[6 * e:6 * e + 6, 6 * self.b[e]:6 * self.b[e] + 6] = Jb[e].astype(np.float64)
        keep = np.ones(6 * self.n, dtype=bool)
        keep[6 * self.anchor:6 * self.anchor + 6] = False
        Jk = J[:, keep]
        H, g = Jk.T @ Jk, Jk.T @ w.astype(np.float64).reshape(-1)
        d = np.zeros(6 * self.n)
        d[keep] = np.linalg.solve(H, -g)
        return d.reshape(self.n, 6), H

    def step_exact(self, x, rounds=4):
        """the Gauss-Newton step (n, 6) and H, both in the graph's type: H and g summed from the edges' 6x6 blocks in that
        type (the Jacobians are step()'s), the solve by an fp64 factorisation refined `rounds` times with residuals of the
        graph's type (each round gains cond(H) 2^-53: four reach 1e-19 at cond 5e8)"""
        assert self.n <= 130
        w, Ja, Jb = self.jacobians(x)
        N = self.n
        H = np.zeros((N, N, 6, 6), dtype=self.dtype)
        g = np.zeros((N, 6), dtype=self.dtype)
        np.add.at(H, (self.a, self.a), np.einsum("eki,ekj->eij", Ja, Ja))
        np.add.at(H, (self.b, self.b), np.einsum("eki,ekj->eij", Jb, Jb))
        np.add.at(H, (self.a, self.b), np.einsum("eki,ekj->eij", Ja, Jb))
        np.add.at(H, (self.b, self.a), np.einsum("eki,ekj->eij", Jb, Ja))
        np.add.at(g, self.a, np.einsum("eki,ek->ei", Ja, w))
        np.add.at(g, self.b, np.einsum("eki,ek->ei", Jb, w))
        keep = np.ones(6 * N, dtype=bool)
        keep[6 * self.anchor:6 * self.anchor + 6] = False
        H = H.transpose(0, 2, 1, 3).reshape(6 * N, 6 * N)[np.ix_(keep, keep)]
        rhs = -g.reshape(-1)[keep]
        H64 = H.astype(np.float64)
        dk = np.linalg.solve(H64, rhs.astype(np.float64)).astype(self.dtype)
        for _ in range(rounds):
            r = rhs - np.array([(row * dk).sum() for row in H])
            dk = dk + np.linalg.solve(H64, r.astype(np.float64)).astype(self.dtype)
        d = np.zeros(6 * N, dtype=self.dtype)
        d[keep] = dk
        return d.reshape(N, 6), H

    def residual(self, x, d, sample=None):
        """rho = max |r| / max S of the step d (n, 6) at x: per free vertex i, r_i = sum J_i^T (Ja d_a + Jb d_b + w) over its
        edges and S_i = sum |J_i^T| (|Ja| |d_a| + |Jb| |d_b| + |w|), the size of the terms r_i is summed from.  Edge by
        edge, no dense matrix.  sample: these vertices only, from their incident edges (rows of d beyond the sample and
        its neighbours are not read)"""
        G = self
        if sample is not None:
            keep = np.zeros(self.n, dtype=bool)
            keep[sample] = True
            sel = np.nonzero(keep[self.a] | keep[self.b])[0]
            G = copy.copy(self)
            G.a, G.b, G.zinv, G.L, G.E = self.a[sel], self.b[sel], self.zinv[sel], self.L[sel], len(sel)
        w, Ja, Jb = G.jacobians(x)
        d = np.array(d, dtype=self.dtype)
        d[self.anchor] = 0
        da, db = d[G.a], d[G.b]
        lin = np.einsum("eki,ei->ek", Ja, da) + np.einsum("eki,ei->ek", Jb, db) + w
        mag = np.einsum("eki,ei->ek", np.abs(Ja), np.abs(da)) + np.einsum("eki,ei->ek", np.abs(Jb), np.abs(db)) + np.abs(w)
        r = np.zeros((self.n, 6), dtype=self.dtype)
        S = np.zeros((self.n, 6), dtype=self.dtype)
        np.add.at(r, G.a, np.einsum("eki,ek->ei", Ja, lin))
        np.add.at(r, G.b, np.einsum("eki,ek->ei", Jb, lin))
        np.add.at(S, G.a, np.einsum("eki,ek->ei", np.abs(Ja), mag))
        np.add.at(S, G.b, np.einsum("eki,ek->ei", np.abs(Jb), mag))
        r[self.anchor] = 0
        S[self.anchor] = 0
        if sample is not None:
            r, S = r[sample], S[sample]
        return float(np.abs(r).max() / S.max())

    def retract(self, x, d):
        x = np.asarray(x).astype(self.dtype)
        out = vmul(x, vexp(np.asarray(d).astype(self.dtype)))
        out[self.anchor] = x[self.anchor]
        return out


def gauss_newton(G, x0, mode="exact", max_iterations=100, max_halvings=40):
    """run to a stall: until no halving decreases F.  Returns (x, F, list of the accepted steps' inf-norms, H of the last)"""
    x = np.asarray(x0).astype(G.dtype)
    F = G.cost(x)
    steps, H = [], None
    if mode == "identity":
        # its fixed point is where ITS gradient vanishes, not a minimum of F: plain steps, no test of F
        for _ in range(max_iterations):
            d, H = G.step(x, mode)
            x = G.retract(x, d)
            steps.append(float(np.abs(d).max()))
            if steps[-1] < 1e-14:
                break
        return x, G.cost(x), steps, H
    for _ in range(max_iterations):
        d, H = G.step(x, mode)
        s, ok = 1.0, False
        for _h in range(max_halvings + 1):
            xt = G.retract(x, s * d)
            Ft = G.cost(xt)
            if Ft < F:
                x, F, ok = xt, Ft, True
                steps.append(float(np.abs(s * d).max()))
                break
            s *= 0.5
        if not ok:
            break
    return x, F, steps, H


def distance(x, y):
    """max abs difference of two trajectories, quaternions up to sign"""
    x, y = np.asarray(x, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)
    sgn = np.where((x[:, :4] * y[:, :4]).sum(axis=1) < 0, -1, 1)[:, None]
    return float(max(np.abs(x[:, :4] - sgn * y[:, :4]).max(), np.abs(x[:, 4:] - y[:, 4:]).max()))


_MEASURED = {}


def measured(key, poses, odom_info, closures, anchor=0, initial=None, identity=True):
    """dict(opt: the longdouble optimum, opt64: the fp64 run's, F, d_ref, ratio, steps, fixed_identity: the fixed point with Jr^-1 = I (longdouble),
    cond: of the last H) — computed once per key"""
    if key not in _MEASURED:
        x0 = poses if initial is None else initial
        Gl = Graph(poses, odom_info, closures, np.longdouble, anchor)
        G64 = Graph(poses, odom_info, closures, np.float64, anchor)
        xl, Fl, steps, H = gauss_newton(Gl, x0)
        x64, _, _, _ = gauss_newton(G64, x0)
        # the contraction of successive accepted steps while they are above 1e-7: below it the fp64 linear solve's own
        # error (cond(H) 2^-53 of a step) and the halvings show, not the method's rate
        big = [s for s in steps if s > 1e-7]
        ratio = max([b / a for a, b in zip(big[:-1], big[1:])] + [0.0])
        assert ratio <= 0.8, (key, ratio, steps)
        xi = gauss_newton(Gl, x0, mode="identity")[0] if identity else None
        _MEASURED[key] = dict(opt=xl, opt64=x64, F=float(Fl), d_ref=distance(x64, xl), ratio=ratio, steps=steps, fixed_identity=xi,
                              cond=float(np.linalg.cond(H)), F0=float(Gl.cost(x0)))
    return _MEASURED[key]


def angles(G, x):
    """the rotation angle of every edge's residual at x, and the real part of the quaternion se3_log is handed"""
    x = np.asarray(x).astype(G.dtype)
    T = vmul(G.zinv, vbetween(x[G.a], x[G.b]))
    return np.linalg.norm(vlog(T)[:, 3:].astype(np.float64), axis=1), T[:, 3].astype(np.float64)


_STEPPED = {}


def step_measured(key, poses, odom_info, closures, anchor, initial, max_halvings, kernel=None, c2=None):
    """One Gauss-Newton iteration from `initial`, in np.longdouble, and the fp64 restatement's distance from it — computed
    once per key.  kernel, c2: the graph at both precisions is robustref.RobustGraph under that kernel at that c^2 (the key
    then holds both); everything below follows from its per_edge() and jacobians().  dict(d: the longdouble step (n, 6); h: the halvings the longdouble run takes, the first s = 2^-h with
    F(x0 exp(s d)) < F(x0); s; x1 = retract(x0, s d); F0, F1; d_ref = distance(x1, the fp64 graph's own x1 at the same h);
    rho_ref: the residual of the fp64 graph's step under the longdouble graph; rho: the longdouble step's own; cond of H;
    grad0, grad1: the longdouble gradients at x0 and x1; theta, qw: angles(); deg: the most edges at one vertex).
    Asserted here, on the restatement alone, as conditions on the scene: h <= max_halvings, and at every trial up to and
    including the accepted one |F_trial - F0| > 1e-6 F0, so that no path's rounding decides h."""
    make = Graph
    if kernel is not None:
        import robustref                                             # (it imports this module)
        key = (key, kernel, float(c2))
        make = lambda *a: robustref.RobustGraph(*a, kernel=kernel, c2=float(c2))
    if key not in _STEPPED:
        Gl = make(poses, odom_info, closures, np.longdouble, anchor)
        G64 = make(poses, odom_info, closures, np.float64, anchor)
        x0 = np.asarray(initial, dtype=np.float64)
        d, H = Gl.step_exact(x0)
        F0 = Gl.cost(x0)
        h, s, x1, F1 = None, np.longdouble(1), None, None
        for k in range(max_halvings + 1):
            xt = Gl.retract(x0, s * d)
            Ft = Gl.cost(xt)
            assert abs(Ft - F0) > 1e-6 * F0, (key, k, float(Ft), float(F0))
            if Ft < F0:
                h, x1, F1 = k, xt, Ft
                break
            s = s / 2
        assert h is not None, (key, "no trial up to max_halvings = %d decreases F" % max_halvings)
        d64, _ = G64.step(x0)
        x1_64 = G64.retract(x0, float(s) * d64)
        theta, qw = angles(Gl, x0)
        _STEPPED[key] = dict(d=d, h=h, s=float(s), x1=x1, F0=F0, F1=F1, d_ref=distance(x1_64, x1),
                             rho_ref=Gl.residual(x0, d64), rho=Gl.residual(x0, d), cond=float(np.linalg.cond(H.astype(np.float64))),
                             grad0=Gl.gradient(x0), grad1=Gl.gradient(x1), theta=theta, qw=qw,
                             deg=int(np.bincount(np.concatenate([Gl.a, Gl.b])).max()))
    return _STEPPED[key]
