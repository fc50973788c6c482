"""One Gauss-Newton step of the registration, pairs to pose, in extended precision: the truth the device step and the
fp64 oracle are both measured against (tests/test_gn_step_host.py, tests/test_gn_step_gpu.py).

A restatement of AlignClouds (core/Registration.cpp:59-94) and SE3::exp over Python integers as fixed point with FRAC
fractional bits and fractions.Fraction; the standard library and numpy only.  Inputs are fp64 numbers taken as the
exact rationals they are.  Sums and products are rounded at 2^-FRAC (absolute), the 6x6 inverse is exact over the
rounded sums, square roots are math.isqrt, sin and cos are Taylor series (summed as the series in theta^2 of
sin(t)/t, (1 - cos t)/t^2 and (t - sin t)/t^3, which do not cancel).

    J_i = [ I | -hat(s_i) ],  r_i = s_i - q_i,  w_i = k^2 / (k + |r_i|^2)^2
    A = sum m_i w_i J_i^T J_i,  b = sum m_i w_i J_i^T r_i,  x* = -A^-1 b,  pose = exp(x*)      (m_i: multiplicities)

The error budget of a computed pose at a point p, first order and worst case (u = 2^-53):

    budget(p, gamma) = || |J_p A^-1| (E_b gamma + extra_b + E_A |x*| gamma) || + 16 u |p| + e_exp + extra
    e_exp = (min(theta / 2, 8 u / theta) + 8 u) |x*_t|

E_A and E_b are the sums of the magnitudes of the terms of A and b; gamma counts the roundings of a term and the depth
of its summation (GAMMA_*); 16 u |p| is the quaternion, its rotation matrix and the action; e_exp is the cancellation
of (1 - cos t)/t^2 and (t - sin t)/t^3 evaluated in fp64 above t = 1e-10 (u / t^2 relative on terms of size t |x_t| / 2
and t^2 |x_t| / 6, capped by the terms themselves), plus the roundings of V x_t.

Where A is rank deficient (one pair, collinear pairs) x is not unique and the check is the residual of the normal
equations, |A x + b| <= (E_b + E_A |x|) gamma componentwise (Step.residual_ratio); for an x that is the logarithm of a
returned pose the pose's own two terms above are added through sum w |J|^T, and the check is made only where the
residuals cannot ask for a large turn (Step.turn)."""
import math
from fractions import Fraction

import numpy as np

FRAC = 512
ONE = 1 << FRAC
U = 2.0 ** -53

GAMMA_EPILOGUE = 16 * U                      # the fused epilogue: ~12 roundings of a term, 2 of (t0+t1)+(t2+t3), then integers


def gamma_partials(n):
    """k_gn followed by reduce_partials"""
    return (16 + -(-n // 32768) + 70) * U


def gamma_serial(n):
    """the oracle with one thread: a running sum of n terms"""
    return (16 + n) * U


def fx(v):
    """an fp64 number (or a Fraction) in fixed point"""
    if isinstance(v, Fraction):
        return (v.numerator << FRAC) // v.denominator
    n, d = float(v).as_integer_ratio()
    return (n << FRAC) // d


def fr(a):
    return Fraction(a, ONE)


def mul(a, b):
    return (a * b) >> FRAC


def div(a, b):
    return (a << FRAC) // b


def fsqrt(a):
    """square root of a fixed-point number"""
    return math.isqrt(a << FRAC)


def frac_sqrt(q):
    """square root of a non-negative Fraction, to 2^-FRAC"""
    return fr(fsqrt(fx(q)))


def _series(th2, first):
    """sum_k (-1)^k th2^k / (2k + first)!  — first = 1: sin(t)/t, 2: (1 - cos t)/t^2, 3: (t - sin t)/t^3; 0: cos t"""
    term = div(ONE, math.factorial(first) << FRAC)
    total, k = 0, 0
    while term:
        total += term if k % 2 == 0 else -term
        k += 1
        term = mul(term, th2) // ((2 * k + first - 1) * (2 * k + first))
    return total


def _hat(w):
    return [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]


def _matmul3(X, Y):
    return [[sum(X[i][k] * Y[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def exp_se3(x):
    """SE3::exp of a tangent x = (upsilon, omega) of Fractions -> (R, t) of Fractions, and theta as a float"""
    w = [Fraction(v) for v in x[3:]]
    th2 = fx(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    sinc, A, B = fr(_series(th2, 1)), fr(_series(th2, 2)), fr(_series(th2, 3))
    W = _hat(w)
    W2 = _matmul3(W, W)
    eye = [[Fraction(int(i == j)) for j in range(3)] for i in range(3)]
    R = [[eye[i][j] + sinc * W[i][j] + A * W2[i][j] for j in range(3)] for i in range(3)]
    V = [[eye[i][j] + A * W[i][j] + B * W2[i][j] for j in range(3)] for i in range(3)]
    u = [Fraction(v) for v in x[:3]]
    t = [sum(V[i][j] * u[j] for j in range(3)) for i in range(3)]
    return R, t, float(fr(fsqrt(th2)))


def _solve(M, rhs):
    """exact Gauss-Jordan over Fractions: M^-1 rhs, rhs a list of columns (a matrix given by rows)"""
    n = len(M)
    a = [list(M[i]) + list(rhs[i]) for i in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda i: abs(a[i][c]))
        if a[p][c] == 0:
            raise ZeroDivisionError("singular")
        a[c], a[p] = a[p], a[c]
        inv = 1 / a[c][c]
        a[c] = [v * inv for v in a[c]]
        for i in range(n):
            if i != c and a[i][c] != 0:
                f = a[i][c]
                a[i] = [vi - f * vc for vi, vc in zip(a[i], a[c])]
    return [row[n:] for row in a]


def pose_parts(T):
    """the exact action of a pose of seven fp64 numbers (qx, qy, qz, qw, t) as the product forms it: the rotation matrix
    of quat_to_mat without renormalising -> (R, t) of Fractions"""
    x, y, z, w = (Fraction(float(v)) for v in T[:4])
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    return R, [Fraction(float(v)) for v in T[4:7]]


def act(Rt, p):
    R, t = Rt
    p = [Fraction(float(v)) if not isinstance(v, Fraction) else v for v in p]
    return [R[i][0] * p[0] + R[i][1] * p[1] + R[i][2] * p[2] + t[i] for i in range(3)]


def compose(a, b):
    """a after b, both (R, t)"""
    return _matmul3(a[0], b[0]), act(a, b[1])


def distance(a, b):
    """|a - b| of two points of Fractions, as a float"""
    return float(frac_sqrt(sum((x - y) ** 2 for x, y in zip(a, b))))


def log_se3(T):
    """the logarithm of a pose of seven fp64 numbers (its quaternion normalised) with |omega| in [0, 2 pi): the x whose
    exponential is the pose, which is the solver's own x as long as that turns by less than 2 pi.  The half angle is
    found from fp64's atan2 by Newton steps on its sine and cosine (Taylor series) -> x of six Fractions"""
    q = [Fraction(float(v)) for v in T[:4]]
    vn = frac_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2])
    if vn == 0:
        w = [Fraction(0)] * 3
    else:
        qn = frac_sqrt(sum(v * v for v in q))
        c, s = fx(q[3] / qn), fx(vn / qn)                 # cos and sin of the half angle, in [0, pi]
        phi = fx(math.atan2(float(vn), float(q[3])))
        for _ in range(6):                                 # the error is cubed every step: 1e-16 -> below 2^-FRAC in four
            p2 = mul(phi, phi)
            sp, cp = mul(phi, _series(p2, 1)), _series(p2, 0)
            phi += mul(s, cp) - mul(c, sp)                 # sin(true - phi)
        scale = 2 * fr(phi) / vn
        w = [scale * v for v in q[:3]]
    th2 = fx(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    A, B = fr(_series(th2, 2)), fr(_series(th2, 3))
    W = _hat(w)
    W2 = _matmul3(W, W)
    V = [[int(i == j) + A * W[i][j] + B * W2[i][j] for j in range(3)] for i in range(3)]
    t = [Fraction(float(v)) for v in T[4:7]]
    u = _solve(V, [[v] for v in t])
    return [u[0][0], u[1][0], u[2][0]] + w


def _collinear(s):
    """whether the points (exact) lie on one line (one point does)"""
    P = [[Fraction(float(v)) for v in p[:3]] for p in s]
    base = P[0]
    d = None
    for p in P[1:]:
        e = [p[i] - base[i] for i in range(3)]
        if all(v == 0 for v in e):
            continue
        if d is None:
            d = e
            continue
        c = (d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0])
        if any(v != 0 for v in c):
            return False
    return True


class Step:
    """the truth of one step: A, b, E_A, E_b (Fractions), n; and for full rank Ainv, x, (R, t), theta"""

    def __init__(self, s, q, k, mult=None, variant=None):
        s = np.asarray(s, dtype=np.float64)
        s = s.reshape(len(s), -1)[:, :3] if s.size else np.zeros((0, 3))
        q = np.asarray(q, dtype=np.float64)
        q = q.reshape(len(s), -1)[:, :3] if q.size else np.zeros((0, 3))
        mult = [1] * len(s) if mult is None else [int(m) for m in mult]
        self.n = sum(mult)
        kf = fx(k)
        k2 = mul(kf, kf)
        A = [[0] * 6 for _ in range(6)]
        EA = [[0] * 6 for _ in range(6)]
        b, Eb = [0] * 6, [0] * 6
        pert = [0] * 6                                # see perturbation()
        slack1, slack_s = [0] * 6, [0] * 6            # see residual_ratio()
        for si, qi, m in zip(s, q, mult):
            if m == 0:
                continue
            x, y, z = (fx(v) for v in si)
            r = [x - fx(qi[0]), y - fx(qi[1]), z - fx(qi[2])]
            den = kf + mul(r[0], r[0]) + mul(r[1], r[1]) + mul(r[2], r[2])
            w = div(k2, den) if variant == "weight" else div(k2, mul(den, den))
            w *= m
            rows = [[(0, ONE), (4, z), (5, -y)],
                    [(1, ONE), (3, -z), (5, x)],
                    [(2, ONE), (3, y), (4, -x)]]
            if variant == "sign":
                rows[1][2] = (5, -x)
            for kk in range(3):
                wj = [(a, mul(w, v)) for a, v in rows[kk]]
                for ia, (a, wa) in enumerate(wj):
                    for (c, vc) in rows[kk][ia:]:
                        term = mul(wa, vc)
                        A[a][c] += term
                        EA[a][c] += abs(term)
                    term = mul(wa, r[kk])
                    b[a] += term
                    Eb[a] += abs(term)
            ns = fsqrt(mul(x, x) + mul(y, y) + mul(z, z))
            nr = fsqrt(den - kf)
            for kk in range(3):
                for a, v in rows[kk]:
                    slack1[a] += mul(w, abs(v))
                    slack_s[a] += mul(mul(w, abs(v)), ns)
            for a in range(3):
                pert[a] += 5 * mul(w, ns)
                pert[3 + a] += mul(w, mul(ns, 5 * ns + nr))
        for a in range(6):
            for c in range(a):
                A[a][c], EA[a][c] = A[c][a], EA[c][a]
        self.A = [[fr(v) for v in row] for row in A]
        self.EA = [[fr(v) for v in row] for row in EA]
        self.b = [fr(v) for v in b]
        self.Eb = [fr(v) for v in Eb]
        self._pert = [float(fr(v)) for v in pert]
        self._slack1, self._slack_s = [fr(v) for v in slack1], [fr(v) for v in slack_s]
        self.full_rank = self.n > 0 and not _collinear(s[np.asarray(mult) > 0])
        # what a solver that is free to (rank-deficient sets) may turn by to explain the residuals: |r| / |s|.  From ~0.1
        # the pose is no longer the linear step's, and from 2 pi its logarithm no longer the solver's x
        self.turn = float(np.max(np.linalg.norm(s - q, axis=1)) / max(np.max(np.linalg.norm(s, axis=1)), 1e-300)) if len(s) else 0.0
        if self.full_rank:
            eye = [[Fraction(int(i == j)) for j in range(6)] for i in range(6)]
            Ainv = _solve(self.A, eye)
            # (both rounded at 2^-FRAC: the exact quotients carry thousands of bits)
            self.x = [fr(fx(-sum(Ainv[i][j] * self.b[j] for j in range(6)))) for i in range(6)]
            self.Ainv = [[fr(fx(v)) for v in row] for row in Ainv]
            self._budgets = {}
            self.R, self.t, self.theta = exp_se3(self.x)
            self.x_norm = float(frac_sqrt(sum(v * v for v in self.x)))
            self.xt_norm = float(frac_sqrt(sum(v * v for v in self.x[:3])))

    # -- the 6x6 system as fp64 arrays (each entry rounded once)
    def A64(self):
        return np.array([[float(v) for v in row] for row in self.A])

    def b64(self):
        return np.array([float(v) for v in self.b])

    def EA64(self):
        return np.array([[float(v) for v in row] for row in self.EA])

    def Eb64(self):
        return np.array([float(v) for v in self.Eb])

    def sums16(self):
        """the 16 closed-form sums of sageicp_types.h (Sum), each rounded once to fp64, and the pair count"""
        A, b = self.A, self.b
        S = np.zeros(20)
        S[0] = float(A[0][0])
        S[1:4] = [float(A[1][5]), float(A[2][3]), float(A[0][4])]
        # A_ww = W(|s|^2 I - s s^T): xx = (A44 + A55 - A33) / 2, ...
        S[4] = float((A[4][4] + A[5][5] - A[3][3]) / 2)
        S[5] = float(-A[3][4])
        S[6] = float(-A[3][5])
        S[7] = float((A[3][3] + A[5][5] - A[4][4]) / 2)
        S[8] = float(-A[4][5])
        S[9] = float((A[3][3] + A[4][4] - A[5][5]) / 2)
        S[10:16] = [float(v) for v in b]
        S[16] = self.n
        return S

    def perturbation(self, rel):
        """first-order bound on the change of b when every s moves by up to rel |s| (r = s - q moves with it): with
        d = rel |s|,  |dw| |r| <= 4 w d,  so  |db_t| <= 5 w d  and  |db_w| = |d(w s x r)| <= w d (|r| + |s|) + 4 w d |s|"""
        return np.array(self._pert) * rel

    def e_exp(self):
        th = self.theta
        c = 0.5 * th if th == 0.0 else min(0.5 * th, 8 * U / th)
        return (c + 8 * U) * self.xt_norm

    def _load(self, gamma, x_abs, extra_b):
        load = [float(self.Eb[i]) * gamma + sum(float(self.EA[i][j]) * x_abs[j] for j in range(6)) * gamma for i in range(6)]
        if extra_b is not None:
            load = [l + float(e) for l, e in zip(load, extra_b)]
        return load

    def budget_x(self, gamma, extra_b=None):
        """|| |A^-1| (E_b gamma + extra_b + E_A |x*| gamma) ||"""
        load = self._load(gamma, [abs(float(v)) for v in self.x], extra_b)
        e = [sum(abs(float(self.Ainv[i][j])) * load[j] for j in range(6)) for i in range(6)]
        return math.sqrt(sum(v * v for v in e))

    def budget(self, p, gamma, extra_b=None, extra=0.0):
        key = (tuple(float(v) for v in p[:3]), gamma, None if extra_b is None else tuple(float(v) for v in extra_b), extra)
        if key not in self._budgets:
            self._budgets[key] = self._budget(p, gamma, extra_b, extra)
        return self._budgets[key]

    def _budget(self, p, gamma, extra_b, extra):
        p = [Fraction(float(v)) for v in p[:3]]
        Jp = [[1, 0, 0, 0, p[2], -p[1]], [0, 1, 0, -p[2], 0, p[0]], [0, 0, 1, p[1], -p[0], 0]]
        JA = [[abs(float(sum(Jp[i][k] * self.Ainv[k][j] for k in range(6)))) for j in range(6)] for i in range(3)]
        load = self._load(gamma, [abs(float(v)) for v in self.x], extra_b)
        e = [sum(JA[i][j] * load[j] for j in range(6)) for i in range(3)]
        pn = math.sqrt(sum(float(v) ** 2 for v in p))
        return math.sqrt(sum(v * v for v in e)) + 16 * U * pn + self.e_exp() + extra

    def ratio(self, pose, points, gamma, guess=None, extra_b=None, extra=0.0):
        """the worst over `points` of |pose p - exp(x*) guess p| / budget(guess p): `pose` seven fp64 numbers or (R, t),
        `guess` likewise (the identity if None)"""
        got = pose if isinstance(pose, tuple) else pose_parts(pose)
        g = None if guess is None else (guess if isinstance(guess, tuple) else pose_parts(guess))
        worst = 0.0
        for p in points:
            at = act(g, p) if g is not None else [Fraction(float(v)) for v in p[:3]]
            want = act((self.R, self.t), at)
            worst = max(worst, distance(act(got, p), want) / self.budget([float(v) for v in at], gamma, extra_b, extra))
        return worst

    def sums_ratio(self, JTJ, JTr, gamma):
        """the worst of |JTJ - A| / (gamma E_A) and |JTr - b| / (gamma E_b), componentwise; an entry whose E is zero
        must be exactly zero (inf otherwise)"""
        worst = 0.0
        JTJ = np.asarray(JTJ, dtype=np.float64).reshape(6, 6)
        for i in range(6):
            for got, want, e in [(JTJ[i][j], self.A[i][j], self.EA[i][j]) for j in range(6)] + [(JTr[i], self.b[i], self.Eb[i])]:
                d = abs(Fraction(float(got)) - want)
                if d != 0:
                    worst = max(worst, float(d / (e * Fraction(gamma))) if e != 0 else math.inf)
        return worst

    def residual_ratio(self, x, gamma, of_pose=False):
        """the worst component of |A x + b| / ((E_b + E_A |x|) gamma): the check of a step where A is rank deficient and x
        is not unique.  of_pose: x is the logarithm of a pose that was rounded to seven fp64 numbers after an fp64
        exponential, not the solver's x itself; A x + b = sum w J^T (J x + r), and J_i dx is (to first order) what the
        pose moved s_i by: the two pose terms of budget(), 16 u |s_i| + e_exp, enter through sum w |J_i|^T"""
        x = [Fraction(v) for v in x]
        slack = [Fraction(0)] * 6
        if of_pose:
            th = float(frac_sqrt(sum(v * v for v in x[3:])))
            e = ((0.5 * th if th == 0.0 else min(0.5 * th, 8 * U / th)) + 8 * U) * float(frac_sqrt(sum(v * v for v in x[:3])))
            slack = [16 * Fraction(U) * self._slack_s[i] + Fraction(e) * self._slack1[i] for i in range(6)]
        worst = 0.0
        for i in range(6):
            res = abs(sum(self.A[i][j] * x[j] for j in range(6)) + self.b[i])
            bound = (self.Eb[i] + sum(self.EA[i][j] * abs(x[j]) for j in range(6))) * Fraction(gamma) + slack[i]
            if res != 0:
                worst = max(worst, float(res / bound) if bound != 0 else math.inf)
        return worst


def spread(centre, extent):
    """eight points through a frame: the corners of the box of half-size `extent` about `centre`"""
    c = np.asarray(centre, dtype=np.float64)[:3]
    e = np.asarray(extent, dtype=np.float64) * np.ones(3)
    return [c + e * np.array([sx, sy, sz]) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]


def tile(n, base):
    """multiplicities of `base` pairs tiled to n pairs (pair i of the tiling is pair i % base of the base)"""
    return [n // base + (1 if i < n % base else 0) for i in range(base)]
