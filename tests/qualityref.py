"""The registration quality report (sageicp_quality, include/sageicp.h) in extended precision: the truth
tests/test_quality_host.py and tests/test_quality_gpu.py measure the device pass against.

A restatement of the definitions over Python integers as fixed point with gnref's FRAC fractional bits and
fractions.Fraction.  The input is a set of accepted pairs — what the oracle's get_correspondences returns: the moved
query rows, the map rows — and the labels of ALL the queries (the class tables count every query).  fp64 inputs are taken
as the exact rationals they are.  For a pair with moved query s (label ls) and map point q (label lq):

    r = s - q,   e = |r|^2,   w = k^2 / (k + e)^2,   J = [ I | -hat(s) ]
    n_pairs;  sum_r2 = sum e;  sum_w = sum w;  sum_w_r2 = sum w e;  JTJ = sum w J^T J;  JTr = sum w J^T r;
    info = sum J^T J;  class_sum_r2[c] = sum e over the pairs whose query has class c  (c = int(ls) in 0 .. 255, else 256)
    pairs_same_label: int(lq) == int(ls);  pairs_unlabelled: not same and int(lq * ls) == 0;  pairs_cross_label: the rest

Every real sum comes with E = the sum of the magnitudes of its terms.  A term is one product as the definition writes
it: w y^2 and w z^2 are the two terms a pair adds to JTJ[3][3], w y r_z and -w z r_y the two it adds to JTr[3].  A
computed sum is held to |got - exact| <= gamma_serial(n_pairs) E: gamma_serial = (16 + n) u bounds the roundings of a
term plus ANY order of summation, so the bound is derived, not measured.

Derived from the exact sums, exactly (Fractions): step = -JTJ^-1 JTr, covariance = s2 JTJ^-1 with
s2 = sum_w_r2 / (3 n_pairs - 6), covariance_pose = G covariance G^T with G = [[I, -hat(t)], [0, I]]."""
import math
from fractions import Fraction

import numpy as np

from gnref import U, _solve, fr, fx, gamma_serial  # noqa: F401  (U and gamma_serial: for the tests that import them from here)
from gnref import FRAC, ONE, _collinear

N_CLASSES = 256


def _mul(a, b):
    return (a * b) >> FRAC


def class_of(label):
    """static_cast<int>(label) where that lies in 0 .. 255, else N_CLASSES (the others)"""
    c = int(label)
    return c if 0 <= c < N_CLASSES else N_CLASSES


def counts(query_labels, src, tgt):
    """the integer part of the report from the pairs, in plain Python: a dict"""
    cq = np.zeros(N_CLASSES + 1, dtype=np.int64)
    cp = np.zeros(N_CLASSES + 1, dtype=np.int64)
    for l in query_labels:
        cq[class_of(l)] += 1
    same = unl = cross = 0
    for s, q in zip(src, tgt):
        cp[class_of(s[3])] += 1
        if int(q[3]) == int(s[3]):
            same += 1
        elif int(q[3] * s[3]) == 0:
            unl += 1
        else:
            cross += 1
    return {"n_queries": len(query_labels), "n_pairs": len(src), "pairs_same_label": same, "pairs_unlabelled": unl,
            "pairs_cross_label": cross, "class_queries": cq[:N_CLASSES], "class_pairs": cp[:N_CLASSES],
            "other_queries": int(cq[N_CLASSES]), "other_pairs": int(cp[N_CLASSES])}


def hat(t):
    return [[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]


def pose_covariance(C, t):
    """G C G^T over Fractions, and the sum of the magnitudes of the terms of every entry (6 x 6 lists)"""
    C = [[Fraction(v) for v in row] for row in C]
    t = [Fraction(float(v)) for v in t]
    H = hat(t)
    G = [[Fraction(int(i == j)) for j in range(6)] for i in range(6)]
    for i in range(3):
        for j in range(3):
            G[i][3 + j] = -H[i][j]
    P = [[sum(G[a][i] * C[i][j] * G[b][j] for i in range(6) for j in range(6)) for b in range(6)] for a in range(6)]
    E = [[sum(abs(G[a][i] * C[i][j] * G[b][j]) for i in range(6) for j in range(6)) for b in range(6)] for a in range(6)]
    return P, E


class Quality:
    """the truth of one report.  Real sums: .real[name] = (exact, E) with Fractions, or lists / 6 x 6 lists of them, for
    name in sum_r2, sum_w, sum_w_r2, JTJ, JTr, info, class_sum_r2 (N_CLASSES + 1 entries: the last is other_sum_r2).
    .counts: the dict of counts().  With derive=True and a regular JTJ: .step, .covariance, .covariance_pose."""

    def __init__(self, query_labels, src, tgt, kernel, t=(0.0, 0.0, 0.0), derive=True):
        src = np.asarray(src, dtype=np.float64).reshape(-1, 4)
        tgt = np.asarray(tgt, dtype=np.float64).reshape(-1, 4)
        self.counts = counts(query_labels, src, tgt)
        n = self.n = len(src)
        kf = fx(kernel)
        k2 = _mul(kf, kf)
        A = [[0] * 6 for _ in range(6)]
        EA = [[0] * 6 for _ in range(6)]
        Iu = [[0] * 6 for _ in range(6)]
        EI = [[0] * 6 for _ in range(6)]
        b, Eb = [0] * 6, [0] * 6
        r2 = w_sum = wr2 = 0
        cls = [0] * (N_CLASSES + 1)
        for s, q in zip(src, tgt):
            x, y, z = (fx(v) for v in s[:3])
            r = [x - fx(q[0]), y - fx(q[1]), z - fx(q[2])]
            e = _mul(r[0], r[0]) + _mul(r[1], r[1]) + _mul(r[2], r[2])
            den = kf + e
            w = (k2 << FRAC) // _mul(den, den)
            r2 += e
            w_sum += w
            wr2 += _mul(w, e)
            cls[class_of(s[3])] += e
            # the rows of J = [ I | -hat(s) ]: (column, value)
            rows = [[(0, ONE), (4, z), (5, -y)],
                    [(1, ONE), (3, -z), (5, x)],
                    [(2, ONE), (3, y), (4, -x)]]
            for kk in range(3):
                for ia, (a, va) in enumerate(rows[kk]):
                    wa = _mul(w, va)
                    for (c, vc) in rows[kk][ia:]:
                        term = _mul(wa, vc)
                        A[a][c] += term
                        EA[a][c] += abs(term)
                        term = _mul(va, vc)
                        Iu[a][c] += term
                        EI[a][c] += abs(term)
                    term = _mul(wa, r[kk])
                    b[a] += term
                    Eb[a] += abs(term)
        for M in (A, EA, Iu, EI):
            for a in range(6):
                for c in range(a):
                    M[a][c] = M[c][a]

        def F(M):
            return [[fr(v) for v in row] for row in M]

        self.real = {
            "sum_r2": (fr(r2), fr(r2)), "sum_w": (fr(w_sum), fr(w_sum)), "sum_w_r2": (fr(wr2), fr(wr2)),
            "JTJ": (F(A), F(EA)), "JTr": ([fr(v) for v in b], [fr(v) for v in Eb]), "info": (F(Iu), F(EI)),
            "class_sum_r2": ([fr(v) for v in cls], [fr(v) for v in cls]),
        }
        self.fitness = Fraction(n, len(query_labels)) if len(query_labels) else Fraction(0)
        self.rmse2 = fr(r2) / n if n else Fraction(0)          # rmse squared
        self.step = self.covariance = self.covariance_pose = None
        # (collinear queries: JTJ is singular, which the sums rounded at 2^-FRAC no longer show)
        if derive and n >= 3 and not _collinear(src):
            eye = [[Fraction(int(i == j)) for j in range(6)] for i in range(6)]
            try:
                Ainv = _solve(self.real["JTJ"][0], eye)
            except ZeroDivisionError:
                return
            bb = self.real["JTr"][0]
            self.step = [-sum(Ainv[i][j] * bb[j] for j in range(6)) for i in range(6)]
            s2 = fr(wr2) / (3 * n - 6)
            self.covariance = [[s2 * v for v in row] for row in Ainv]
            self.covariance_pose, _ = pose_covariance(self.covariance, t)

    def flat(self):
        """every real sum as (name, exact, E), one scalar each"""
        for name, (v, e) in self.real.items():
            if isinstance(v, Fraction):
                yield name, v, e
            elif isinstance(v[0], list):
                for i in range(6):
                    for j in range(6):
                        yield "%s[%d][%d]" % (name, i, j), v[i][j], e[i][j]
            else:
                for i in range(len(v)):
                    yield "%s[%d]" % (name, i), v[i], e[i]

    def sums_ratio(self, got, gamma=None):
        """the worst of |got - exact| / (gamma E) over every real sum, and its name; a sum whose E is zero must be exactly
        zero (inf otherwise).  `got`: a dict with sum_r2, sum_w, sum_w_r2, JTJ (6 x 6), JTr, info (6 x 6), class_sum_r2
        (256) and other_sum_r2 — Quality.as_dict() of the binding, or a numpy evaluation"""
        gamma = Fraction(gamma_serial(self.n) if gamma is None else gamma)
        flat = {}
        for name in ("sum_r2", "sum_w", "sum_w_r2"):
            flat[name] = got[name]
        for name in ("JTJ", "info"):
            M = np.asarray(got[name], dtype=np.float64).reshape(6, 6)
            for i in range(6):
                for j in range(6):
                    flat["%s[%d][%d]" % (name, i, j)] = M[i][j]
        for i in range(6):
            flat["JTr[%d]" % i] = np.asarray(got["JTr"])[i]
        if "class_sum_r2" in got:
            for i in range(N_CLASSES):
                flat["class_sum_r2[%d]" % i] = np.asarray(got["class_sum_r2"])[i]
            flat["class_sum_r2[%d]" % N_CLASSES] = got["other_sum_r2"]
        worst, where = 0.0, None
        for name, want, e in self.flat():
            if name not in flat:
                continue
            d = abs(Fraction(float(flat[name])) - want)
            if d != 0:
                ratio = float(d / (e * gamma)) if e != 0 else math.inf
                if ratio > worst:
                    worst, where = ratio, name
        return worst, where


def numpy_quality(query_labels, src, tgt, kernel):
    """the same sums as a plain fp64 evaluation, pair after pair (a running sum: gamma_serial's case)"""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 4)
    tgt = np.asarray(tgt, dtype=np.float64).reshape(-1, 4)
    JTJ, info, JTr = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6)
    r2 = ws = wr2 = 0.0
    cls = np.zeros(N_CLASSES + 1)
    for s, q in zip(src, tgt):
        r = s[:3] - q[:3]
        e = float(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
        w = kernel * kernel / ((kernel + e) * (kernel + e))
        J = np.zeros((3, 6))
        J[:, :3] = np.eye(3)
        J[:, 3:] = -np.array(hat(s[:3]))
        for a in range(6):
            for c in range(6):
                for kk in range(3):
                    JTJ[a, c] += (w * J[kk, a]) * J[kk, c]
                    info[a, c] += J[kk, a] * J[kk, c]
            for kk in range(3):
                JTr[a] += (w * J[kk, a]) * r[kk]
        r2 += e
        ws += w
        wr2 += w * e
        cls[class_of(s[3])] += e
    return {"sum_r2": r2, "sum_w": ws, "sum_w_r2": wr2, "JTJ": JTJ, "JTr": JTr, "info": info,
            "class_sum_r2": cls[:N_CLASSES], "other_sum_r2": cls[N_CLASSES]}
