"""Seeded scenes for the pose-graph tests (tests/test_posegraph_host.py, tests/test_posegraph_gpu.py): a drive's truth, its
drifted odometry, and closures taken from the truth.  A scene is a dict: poses (n, 7), truth (n, 7), odom_info (6x6 or
(n - 1, 6, 6)), closures [(a, b, z[7], info 6x6)] with z = T_a_b.  Translations of `poses` lie on a grid of 2^-10 m, so the
UTM twin (shifted by (5e5, 5e6, 0)) is the same trajectory exactly."""
import math

import numpy as np

import posegraphref as pg

UTM = np.array([5.0e5, 5.0e6, 0.0])
ODOM_INFO = np.diag([100.0, 100.0, 100.0, 2500.0, 2500.0, 2500.0])
DISAGREE = np.array([0.3, -0.2, 0.1, 0.01, 0.0, 0.02])


def _yaw_pose(yaw, t):
    return np.array([0.0, 0.0, math.sin(yaw / 2.0), math.cos(yaw / 2.0), t[0], t[1], t[2]])


def circle_truth(n, radius, laps=1, per_lap=None):
    per_lap = per_lap or n
    out = []
    for k in range(n):
        th = 2.0 * math.pi * k / per_lap
        out.append(_yaw_pose(th + math.pi / 2.0, (radius * math.cos(th), radius * math.sin(th), 0.0)))
    return np.array(out)


def drift(truth, seed, trans_frac=0.05, rot=3e-3):
    """the truth's relative poses, each disturbed by exp(noise), integrated from truth[0]; translations snapped to 2^-10 m"""
    rng = np.random.default_rng(seed)
    Z = pg.vbetween(truth[:-1], truth[1:])
    step = np.linalg.norm(Z[:, 4:], axis=1)
    noise = np.concatenate([rng.normal(0.0, 1.0, (len(Z), 3)) * (trans_frac * step)[:, None], rng.normal(0.0, rot, (len(Z), 3))], axis=1)
    Z = pg.vmul(Z, pg.vexp(noise))
    poses = [truth[0].copy()]
    for k in range(len(Z)):
        poses.append(pg.vmul(poses[-1][None], Z[k][None])[0])
    poses = np.array(poses)
    poses[:, 4:] = np.round(poses[:, 4:] * 1024.0) / 1024.0
    return poses


def wander(truth, seed, trans=1e-4, rot=1e-6):
    """the truth with a random walk in the tangent laid over it (vectorised: for drives too long for drift()'s loop)"""
    rng = np.random.default_rng(seed)
    e = np.cumsum(rng.normal(0.0, 1.0, (len(truth), 6)) * np.array([trans] * 3 + [rot] * 3), axis=0)
    e[0] = 0.0
    poses = pg.vmul(truth, pg.vexp(e))
    poses[:, 4:] = np.round(poses[:, 4:] * 1024.0) / 1024.0
    return poses


def rel(truth, a, b, disturb=None):
    z = pg.vbetween(truth[a][None], truth[b][None])
    if disturb is not None:
        z = pg.vmul(z, pg.vexp(np.asarray(disturb, dtype=np.float64)[None]))
    return z[0]


def ring(seed=19):
    truth = circle_truth(48, 12.7)
    poses = drift(truth, seed)
    closures = [(0, 47, rel(truth, 0, 47), 4.0 * ODOM_INFO), (5, 45, rel(truth, 5, 45, DISAGREE), ODOM_INFO.copy())]
    return dict(poses=poses, truth=truth, odom_info=ODOM_INFO.copy(), closures=closures)


def shifted(scene, by=UTM):
    out = dict(scene)
    out["poses"] = scene["poses"].copy()
    out["poses"][:, 4:] += by
    out["truth"] = scene["truth"].copy()
    out["truth"][:, 4:] += by
    return out


def full_info(seed=3):
    """one full, non-diagonal SPD 6x6, symmetric to the bit"""
    rng = np.random.default_rng(seed)
    B = np.eye(6) + 0.1 * rng.normal(size=(6, 6))
    M = B @ ODOM_INFO @ B.T
    return (M + M.T) / 2.0


def ring_full(seed=19):
    s = ring(seed)
    M = full_info()
    s["odom_info"] = M
    s["closures"] = [(a, b, z, (4.0 * M if k == 0 else M.copy())) for k, (a, b, z, _) in enumerate(s["closures"])]
    return s


def two_laps(seed=23):
    """96 poses, two laps of the ring; three closures from the truth: mutually consistent"""
    truth = circle_truth(96, 12.7, per_lap=48)
    poses = drift(truth, seed)
    closures = [(a, b, rel(truth, a, b), 4.0 * ODOM_INFO) for a, b in ((2, 50), (20, 68), (40, 95))]
    return dict(poses=poses, truth=truth, odom_info=ODOM_INFO.copy(), closures=closures)


def chain(n, c, seed, how="spread", anchor=0):
    """a gently curving drive of n poses with c closures from a slightly different truth, placed as `how` says:
    spread — over the drive; edges — at the anchor, at the last pose, on adjacent poses (parallel to an odometry edge),
    twice on one pair, and given in reverse (a > b), cycled"""
    rng = np.random.default_rng(seed)
    truth = circle_truth(n, max(3.0, 0.25 * n), per_lap=max(n, 8))
    truth[:, 6] = 0.01 * np.arange(n)
    poses = drift(truth, seed, trans_frac=0.02, rot=1e-3) if n > 1 else truth.copy()
    pairs = []
    if how == "spread":
        for k in range(c):
            a = int(rng.integers(0, n))
            b = int((a + 1 + rng.integers(0, max(1, n - 1))) % n)
            if a == b:
                b = (a + 1) % n
            pairs.append((a, b))
    else:
        other = (anchor + n // 2) % n if (anchor + n // 2) % n != anchor else (anchor + 1) % n
        far = 0 if n - 1 != 0 and anchor != 0 else max(0, n - 2)
        menu = [(anchor, other), (far if far != n - 1 else 0, n - 1), (min(1, n - 2), min(1, n - 2) + 1), (anchor, other),
                (n - 1, 0), (n - 1, max(0, n - 2)), (other, anchor)]
        pairs = [menu[k % len(menu)] for k in range(c)]
    pairs = [(a, b) for a, b in pairs if a != b]
    closures = [(a, b, rel(truth, a, b, 0.02 * rng.normal(size=6) * np.array([1, 1, 1, 0.1, 0.1, 0.1])), ODOM_INFO * (1.0 + k % 3))
                for k, (a, b) in enumerate(pairs)]
    return dict(poses=poses, truth=truth, odom_info=ODOM_INFO.copy(), closures=closures)


ODOM_ANGLES = (1e-3, 0.2499, 0.2501, 0.6)
CLOSURE_ANGLES = (0.01, 0.2499, 0.2501, 1.5, 3.0)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def stepped(n, c, seed, anchor=0, how="edges", angles=CLOSURE_ANGLES, odom_angles=ODOM_ANGLES, trans=0.02, base=None):
    """chain(n, c, seed, how, anchor) with a start whose first linearisation decides (tests/graphsteps.py): scene["initial"]
    = poses * exp(e_k), the tangents e_k drawn once.  Poses of even k keep their rotation and poses of odd k turn by
    odom_angles[(k // 2) % 4] about an axis of their own, so the residuals of the two odometry edges at an odd pose have
    exactly that angle (to rounding): no odometry residual is zero, and the angles lie on either side of posegraph.h's
    kPgSeriesAngle = 0.25 rad.  An odd pose at which a closure ends turns by odom_angles[0] only: the closure is taken from
    the start, and a pose turned by 0.6 rad would swing a closure of 100 m by 60 m against the odometry, a start from
    which no step within three halvings decreases F on the long chains.  Every pose is also shifted by `trans` metres
    (normal).  Each closure's measurement is
    turned by the exp(.) that makes its residual at initial (u, angles[k % len] * axis) to rounding.  Every fifth start
    pose and every other closure carry the other sign of their quaternion (the same rotation; se3_log then meets
    qw < 0).  Translations of poses and of initial lie on the 2^-10 m grid.  base: another drive (poses, truth, odom_info,
    closures) in place of chain's."""
    s = chain(n, c, seed, how=how, anchor=anchor) if base is None else dict(base)
    rng = np.random.default_rng(seed + 7919)
    poses = s["poses"]
    n = len(poses)
    e = np.zeros((n, 6))
    e[:, :3] = trans * rng.normal(size=(n, 3))
    axes = rng.normal(size=(n, 3))
    theta = np.array(odom_angles)[(np.arange(n) // 2) % len(odom_angles)] * (np.arange(n) % 2)
    for a, b, _, _ in s["closures"]:                             # (a closure's ends: see above)
        theta[[a, b]] = np.minimum(theta[[a, b]], odom_angles[0])
    e[:, 3:] = theta[:, None] * axes / np.linalg.norm(axes, axis=1)[:, None]
    initial = pg.vmul(poses, pg.vexp(e))
    initial[:, 4:] = np.round(initial[:, 4:] * 1024.0) / 1024.0
    initial[3::5, :4] *= -1.0
    closures = []
    for k, (a, b, z, info) in enumerate(s["closures"]):
        r = np.concatenate([trans * rng.normal(size=3), angles[k % len(angles)] * _unit(rng)])
        # z exp(t) with t = log(z^-1 D exp(-r)), D = initial_a^-1 initial_b: the product itself, not through the logarithm
        z2 = pg.vmul(pg.vbetween(initial[a][None], initial[b][None]), pg.vexp(-r[None]))[0]
        if k % 2:
            z2[:4] *= -1.0
        closures.append((a, b, z2, info))
    s["closures"], s["initial"] = closures, initial
    return s


def edges(sage, scene):
    """the scene's closures as the library's records"""
    out = []
    for a, b, z, info in scene["closures"]:
        e = sage.GraphEdge()
        e.a, e.b = a, b
        e.z[:] = list(z)
        e.info[:] = list(np.asarray(info, dtype=np.float64).reshape(-1))
        out.append(e)
    return out


# ---- what the host and the GPU tests share ---------------------------------------------------------------------------------
STEP_TOL = 1e-9
SCENES = {"ring": ring, "ring_utm": lambda: shifted(ring()), "full_info": ring_full, "two_laps": two_laps}
_SCENE = {}


def scene(name):
    if name not in _SCENE:
        _SCENE[name] = SCENES[name]()
    return _SCENE[name]


def measured(name):
    s = scene(name)
    return pg.measured(name, s["poses"], s["odom_info"], s["closures"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def optimize(sage, s, where="host", **kw):
    return sage.graph_optimize(s["poses"], edges(sage, s), s["odom_info"], where=where, return_info=True, **kw)


def sequential(sage, s, order):
    """the closures applied one after another by sageicp_closure_corrections, in `order`"""
    import closureref as cr
    P = s["poses"].copy()
    for k in order:
        a, b, z, _ = s["closures"][k]
        _, P = sage.closure_corrections(P, a, b, cr.se3_mul(P[a], np.asarray(z)))
    return P
