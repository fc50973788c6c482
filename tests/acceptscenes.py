"""Scenes whose pairs sit ON the acceptance radius of GetCorrespondences, (nn - p).norm() < max_correspondence_distance
(VoxelHashMap.cpp:111), for tests/test_accept_threshold_host.py and tests/test_accept_boundary_gpu.py.  Plain numpy, seeded.

The device takes no square root: it tests r2 <= T with T = accept_threshold(max_dist) (csrc/accept.h), r2 the three squares
added in the association SAGE_SQNORM3_ACCEPT names (csrc/sageicp_types.h; this module follows SAGE_SQNORM3_ORDER as
tests/mapref.py does).  `threshold()` below is T from exact arithmetic, not from the library.

A scene is a set of isolated clusters, at least 4 voxels apart: one map point g and one query s = g + d, |d| ~ max_dist.
The query's x is solved so that r2 ~ T, then walked over +-40 ulps with nextafter; every position whose r2 lies within
4 ulps of T becomes a row.  The rows of a scene are shuffled once (accepted and rejected rows then alternate irregularly
within blocks of four and within 64-row waves); frame(n) is the first n of them.  What each row's answer must be follows
from the arithmetic here alone (`accept`, `own`); the tests hold the oracle to it first, then the library to the oracle.

With pose=P the rows are built so that the rows MOVED by P (as k_tf moves them: scoreref.move) sit on the boundary."""
import math
import os
from fractions import Fraction

import numpy as np

import scoreref

SQNORM3_ORDER = 0 if os.environ.get("SAGE_SQNORM3_ORDER", "2") == "0" else 2
DBL_MAX = float(np.finfo(np.float64).max)
LABELS = np.array([0.0, 10.0, 40.0, 44.0, 50.0, 70.0, 71.0, 80.0, 251.0])
TH = 0.4
WALK, KEEP_ULPS = 40, 4
POSE = np.array([0.02, -0.05, 0.1, 0.99, 0.4, -0.3, 0.05])
POSE[:4] /= np.linalg.norm(POSE[:4])


# ---- the threshold from exact arithmetic ---------------------------------------------------------------------------------
def threshold(m):
    """The largest double x whose correctly rounded square root is below m.  With mid = (pred(m) + m) / 2 exactly,
    fl(sqrt(x)) < m iff sqrt(x) < mid iff x < mid^2; mid^2 needs more than 53 bits, so no double equals it: the answer is
    the largest double below mid^2 (DBL_MAX where mid^2 is beyond the doubles; 0 where it is below every positive one).
    -1 (nothing passes) for 0, a negative or a NaN."""
    m = float(m)
    if not m > 0.0:
        return -1.0
    if math.isinf(m):
        return DBL_MAX
    mid = (Fraction(math.nextafter(m, 0.0)) + Fraction(m)) / 2
    t = mid * mid
    if t > Fraction(DBL_MAX):
        return DBL_MAX
    x = float(t)                        # correctly rounded (fractions.Fraction.__float__ is)
    if Fraction(x) >= t:
        x = math.nextafter(x, -math.inf)
    assert Fraction(x) < t <= Fraction(math.nextafter(x, math.inf))
    return x


# ---- the arithmetic of the acceptance site, elementwise in fp64 -------------------------------------------------------------
def _sq3(xx, yy, zz, order):
    return xx + (yy + zz) if order == 0 else (xx + yy) + zz


def r2_both(s, g):
    """(r2 in this build's ACCEPT association, r2 in the other one) of queries s and map points g, (n, >=3) each"""
    d = g[:, :3] - s[:, :3]
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    return _sq3(xx, yy, zz, SQNORM3_ORDER), _sq3(xx, yy, zz, 2 - SQNORM3_ORDER)


def _ulps(a, b):
    """a - b in units in the last place (positive doubles)"""
    return np.asarray(a, dtype=np.float64).view(np.int64) - np.float64(b).view(np.int64)


def _inverse(pose):
    R = np.array(scoreref.quat_to_mat(pose[:4])).reshape(3, 3)
    t = -R.T @ np.asarray(pose[4:7], dtype=np.float64)
    return np.array([-pose[0], -pose[1], -pose[2], pose[3], t[0], t[1], t[2]])


def _voxel(p, voxel):
    return (p[:, :3] / voxel).astype(np.int64)             # truncation toward zero (VoxelHashMap.cpp:52-54)


# ---- configurations ---------------------------------------------------------------------------------------------------------
# name -> voxel, max_dist, sem_th, centre, clusters, spacing of the cluster grid in voxels, the cells per axis, what `d` is:
#   "fine":   dx is made so small that one ulp of the query's x moves r2 by about 3/4 ulp (exact hits of T in most clusters)
#   "wide":   any direction with every component below 2 voxels (max_dist beyond a voxel: some pairs the 27 voxels miss)
#   "any":    any direction
CONFIGS = {
    "v1.0_d0.7": dict(voxel=1.0, max_dist=0.7, sem_th=TH, centre=(0.0, 0.0, 0.0), clusters=1800, spacing=5, cells=19, d="fine"),
    "v1.0_d3.0": dict(voxel=1.0, max_dist=3.0, sem_th=TH, centre=(0.0, 0.0, 0.0), clusters=1600, spacing=6, cells=15, d="wide"),
    "v0.5_d0.9": dict(voxel=0.5, max_dist=0.9, sem_th=TH, centre=(0.0, 0.0, 0.0), clusters=1000, spacing=8, cells=23, d="fine"),
    "v1.0_d1e-3": dict(voxel=1.0, max_dist=1e-3, sem_th=TH, centre=(0.0, 0.0, 0.0), clusters=600, spacing=5, cells=19, d="fine"),
    "km": dict(voxel=1.0, max_dist=0.7, sem_th=TH, centre=(4321.0, -2750.0, 12.0), clusters=400, spacing=5, cells=19, d="any",
               bracket=True),
    "competitor": dict(voxel=1.0, max_dist=0.7, sem_th=0.05, centre=(0.0, 0.0, 0.0), clusters=600, spacing=5, cells=19, d="fine",
                       competitor=True),
}
NEAR_ORIGIN = ("v1.0_d0.7", "v1.0_d3.0", "v0.5_d0.9", "v1.0_d1e-3", "competitor")
SIZES = {"v1.0_d0.7": (1, 63, 257, 4097, 16500), "v1.0_d3.0": (1, 63, 257, 4097), "v0.5_d0.9": (1, 63, 257, 4097),
         "v1.0_d1e-3": (1, 63, 257, 4097), "km": (1, 63, 257, 800), "competitor": (1, 63, 257, 4097)}
POSED_SIZES = (257, 4097)           # (a walk in the RAW x moves all three moved coordinates: fewer rows stay within 4 ulps)


class AcceptScene:
    """.map (m, 4): the map points in insertion order.  Per row of the shuffled pool: .rows (the frame, raw), .moved (the
    rows as the search sees them: .rows, or .rows moved by .pose), .own (the map point that must answer), .r2 / .r2_other
    (this build's association / the other one), .accept / .accept_other (r2 <= T), .cluster."""

    def __init__(self, name, pose=None):
        cfg = CONFIGS[name]
        self.name, self.pose = name, None if pose is None else np.asarray(pose, dtype=np.float64)
        self.voxel, self.max_dist, self.sem_th = cfg["voxel"], cfg["max_dist"], cfg["sem_th"]
        self.bracket = bool(cfg.get("bracket"))
        self.sizes = SIZES[name] if pose is None else POSED_SIZES
        self.T = T = threshold(self.max_dist)
        rng = np.random.default_rng([sum(name.encode()), 0 if pose is None else 1])
        v, md, K = self.voxel, self.max_dist, cfg["clusters"]
        # the clusters' map points: distinct cells of a grid `spacing` voxels wide, anywhere in the middle of a cell's
        # first voxel — two clusters are at least spacing - 0.6 voxels apart along some axis
        c = cfg["cells"]
        cells = rng.choice(c ** 3, size=K, replace=False)
        ijk = np.stack([cells // (c * c), (cells // c) % c, cells % c], axis=1) - c // 2
        nominal = np.asarray(cfg["centre"]) + (ijk * cfg["spacing"] + 0.5) * v
        ql = rng.choice(LABELS[1:], size=K)
        # the nominal offset d, |d|^2 = T
        sx = np.where(rng.random(K) < 0.5, -1.0, 1.0)
        frac = rng.uniform(0.2, 0.8, size=(K, 3))
        if cfg["d"] == "fine":
            ulp_x = np.spacing(np.abs(nominal[:, 0]))
            dx = np.clip(0.75 * np.spacing(T) / (2.0 * ulp_x), None, 0.5 * md) * rng.uniform(0.8, 1.25, size=K)
            phi = rng.uniform(0.0, 2.0 * np.pi, size=K)
            rho = np.sqrt(T - dx * dx)
            d = np.stack([sx * dx, rho * np.cos(phi), rho * np.sin(phi)], axis=1)
        else:
            d = np.empty((K, 3))
            todo = np.ones(K, dtype=bool)
            while todo.any():
                u = rng.normal(size=(K, 3))
                u *= md / np.linalg.norm(u, axis=1)[:, None]
                ok = np.abs(u[:, 0]) > 0.2 * md
                if cfg["d"] == "wide":
                    ok &= (np.abs(u) < 1.9 * v).all(axis=1)
                d[todo & ok] = u[todo & ok]
                todo &= ~ok
            if cfg["d"] == "wide":
                # where in its voxel g sits so that s = g - d lands in the voxel beside it, not two away
                e = np.abs(d) / v
                f = rng.uniform(np.maximum(e - 1.0, 0.0) + 0.02, 0.98)
                frac = np.where(d > 0, f, 1.0 - f)
        g = np.empty((K, 4))
        g[:, :3] = np.asarray(cfg["centre"]) + (ijk * cfg["spacing"] + frac) * v
        g[:, 3] = np.where(rng.random(K) < 0.4, ql, rng.choice(LABELS, size=K))
        if self.pose is not None:
            assert np.allclose(scoreref.move(self.pose, scoreref.move(_inverse(self.pose), g)), g, atol=1e-9)
        # s: y and z first, as they round; then the x that makes r2 = T with them
        s = g.copy()
        s[:, 3] = ql
        s[:, 1:3] = g[:, 1:3] - d[:, 1:3]
        ry, rz = g[:, 1] - s[:, 1], g[:, 2] - s[:, 2]
        s[:, 0] = g[:, 0] - np.sign(d[:, 0]) * np.sqrt(T - (ry * ry + rz * rz))
        raw0 = s if self.pose is None else scoreref.move(_inverse(self.pose), s)
        # the walk: raw x over -WALK .. +WALK ulps
        steps = [raw0[:, 0].copy()]
        for _ in range(WALK):
            steps.append(np.nextafter(steps[-1], np.inf))
        down = raw0[:, 0].copy()
        for _ in range(WALK):
            down = np.nextafter(down, -np.inf)
            steps.insert(0, down)
        rows = np.repeat(raw0[None, :, :], 2 * WALK + 1, axis=0)              # (walk, K, 4)
        rows[:, :, 0] = np.stack(steps)
        rows = rows.reshape(-1, 4)
        own = np.tile(g, (2 * WALK + 1, 1))
        cluster = np.tile(np.arange(K), 2 * WALK + 1)
        moved = rows if self.pose is None else scoreref.move(self.pose, rows)
        r2, r2o = r2_both(moved, own)
        if self.bracket:
            # per cluster the two adjacent positions that bracket T (r2 moves by far more than an ulp per step there)
            acc = (r2 <= T).reshape(2 * WALK + 1, K)
            flip = acc[1:] != acc[:-1]
            assert (flip.sum(axis=0) == 1).all(), "every cluster's walk crosses T exactly once"
            first = flip.argmax(axis=0)
            keep = np.zeros_like(acc)
            keep[first, np.arange(K)] = True
            keep[first + 1, np.arange(K)] = True
            keep = keep.reshape(-1)
        else:
            keep = np.abs(_ulps(r2, T)) <= KEEP_ULPS
        # pairs the 27 voxels around the query do not reach are no pairs (max_dist beyond a voxel)
        keep &= (np.abs(_voxel(moved, v) - _voxel(own, v)) <= 1).all(axis=1)
        order = rng.permutation(int(keep.sum()))
        pick = np.flatnonzero(keep)[order]
        self.rows, self.moved, self.own, self.cluster = rows[pick], moved[pick], own[pick], cluster[pick]
        self.r2, self.r2_other = r2[pick], r2o[pick]
        self.accept, self.accept_other = self.r2 <= T, self.r2_other <= T
        self.map = g
        if cfg.get("competitor"):
            # the winner by SCALED distance is g (the query's label, r2 * sem_th ~ T / 20); a point of another label at
            # half the distance (r2 ~ T / 4, unscaled) loses the argmin and must not decide the acceptance either
            g[:, 3] = ql
            u = rng.normal(size=(K, 3))
            u *= 0.5 * md / np.linalg.norm(u, axis=1)[:, None]
            other = np.empty((K, 4))
            other[:, :3] = s[:, :3] + u
            other[:, 3] = np.where(ql == 40.0, 44.0, 40.0)
            self.map = np.concatenate([g, other])[rng.permutation(2 * K)]
            self.own[:, 3] = self.rows[:, 3]
            rival = other[self.cluster]
            rr, _ = r2_both(self.moved, rival)
            assert (rr < 0.3 * T).all() and (rr > self.r2 * self.sem_th).all() and (rr > 0.2 * T).all()
        self._check()

    # what must hold of the scene before anything is compared with it: from the scene alone
    def _check(self):
        n, T = len(self.rows), self.T
        lim = 50.0 if self.name in NEAR_ORIGIN else 5000.0
        assert np.abs(self.moved[:, :3]).max() < lim and np.abs(self.map[:, :3]).max() < lim
        assert n >= max(self.sizes), (self.name, n)
        share = self.accept.mean()
        assert 0.4 <= share <= 0.6, (self.name, share)
        if self.bracket:
            # per cluster: one accepted, one rejected, adjacent
            for flag in (self.accept, ~self.accept):
                assert np.array_equal(np.sort(self.cluster[flag]), np.arange(len(self.map)))
            return
        assert (self.r2 == T).any() and (self.r2 == np.nextafter(T, np.inf)).any(), self.name
        assert self.deciders().sum() >= 20, (self.name, int(self.deciders().sum()))
        # irregular order: blocks of four show most of the 16 patterns, every full wave both kinds of row
        m = (min(n, 4096) // 64) * 64
        a = self.accept[:m]
        assert len(set(map(tuple, a.reshape(-1, 4)))) >= 12
        waves = a.reshape(-1, 64).sum(axis=1)
        assert waves.min() >= 8 and waves.max() <= 56 and len(set(waves)) >= 4

    def deciders(self):
        """rows whose two associations land on different sides of T"""
        return self.accept != self.accept_other

    def frame(self, n):
        return np.ascontiguousarray(self.rows[:n])

    def expect(self, n):
        """(src, tgt, idx) of frame(n) as GetCorrespondences must answer: the moved rows, the own map points"""
        idx = np.flatnonzero(self.accept[:n])
        return self.moved[idx], self.own[idx], idx


_SCENES = {}


def scene(name, pose=None):
    key = (name, pose is not None)
    if key not in _SCENES:
        _SCENES[key] = AcceptScene(name, pose)
    return _SCENES[key]
