"""The pair sets, scenes and cases of tests/test_gn_step_host.py and tests/test_gn_step_gpu.py, and the child process that
runs the RegisterFrame cases of the latter.

    python tests/gnstep_cases.py          one JSON line per case on stdout, in the order of CASES, flushed as it is done

Two families:

  pair sets  (PAIR_SETS x PAIR_N)  pairs handed to AlignClouds as they are.  A set is a base of BASE pairs; n pairs are the
             base tiled (pair i is pair i % BASE of the base), so the truth of 65,537 pairs is that of 257 with multiplicities.
  scenes     (SCENES x FRAMES x forms)  a map of 4,000 points, a frame of n and a guess; the first two iterations of
             RegisterFrame, stopped with SAGEICP_MAX_ITER, against tests/gnref.py over the oracle's pairs.

TAU is the bound on every ratio error / budget of a detector case: 4 x RHO_REF rounded up to a power of two, RHO_REF
the worst ratio of the fp64 ORACLE over the detector cases (measured by tests/test_gn_step_host.py, which fails if the
figure here is stale)."""
import json
import math
import os
import sys
import time

import numpy as np

import gnref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RHO_REF = 0.048
TAU = 0.25
MAX_TURN = 0.1                    # rank-deficient sets: the pose's logarithm is checked where gnref.Step.turn is below this

U = gnref.U

# ---- pair sets ---------------------------------------------------------------------------------------------------------
BASE = 257
PAIR_N = (1, 2, 3, 5, 6, 7, 255, 256, 257, 32767, 32768, 32769, 65537)
CENTRES = {"km4": (4321.0, -2750.0, 12.0), "km12": (12000.0, -9000.0, 40.0), "utm": (4e5, -5e6, 0.0)}
#              name        kernel   detector (both wrong restatements exceed the budget: test_gn_step_host.py)
PAIR_SETS = (("origin",     1 / 3,  True),
             ("km4",        1 / 3,  True),
             ("km12",       1 / 3,  True),
             ("collinear",  1 / 3,  False),      # rank deficient at every n: the residual check
             ("planar",     1 / 3,  True),
             ("identical",  1 / 3,  False),      # b = 0: the pose is the identity whatever the weights
             ("scale",      1e-3,   True),       # residuals of 1e3 m: weights of 1e-18
             ("k1e-3",      1e-3,   True),
             ("k1e3",       1e3,    True),
             ("theta1e-8",  1 / 3,  False),      # pairs that fit a motion exactly: x* does not depend on the weights
             ("theta1e-6",  1e-9,   True),       # (here fp64's rounding of the targets is a residual of its own, and
                                                 # the kernel is of the size of |r|^2: the weights do differ)
             ("utm",        1 / 3,  False))      # fp64 itself is ill-conditioned here: measured and reported only
PAIR_KERNEL = {name: k for name, k, _ in PAIR_SETS}
PAIR_DETECTOR = {name: d for name, _, d in PAIR_SETS}
PAIR_CASES = [(name, n) for name, _, _ in PAIR_SETS for n in PAIR_N]
PAIR_IDS = ["%s-n%d" % c for c in PAIR_CASES]


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-4:
        return np.eye(3) + W + 0.5 * W @ W
    return np.eye(3) + math.sin(th) / th * W + (1 - math.cos(th)) / th ** 2 * W @ W


_bases = {}


def pair_base(name):
    """-> source (BASE, 4), target (BASE, 4), centre of the set"""
    if name in _bases:
        return _bases[name]
    rng = np.random.default_rng(5300 + [s[0] for s in PAIR_SETS].index(name))
    c = np.array(CENTRES.get(name, (0.0, 0.0, 0.0)))
    local = rng.normal(scale=30.0, size=(BASE, 3)) * [1.0, 1.0, 0.2]
    noise = rng.normal(scale=0.05, size=(BASE, 3))
    R, t = rodrigues([0.002, -0.001, 0.005]), np.array([0.05, -0.03, 0.02])
    if name == "collinear":
        local = np.outer(rng.integers(-400, 400, size=BASE) / 8.0, [1.0, 0.5, 0.25])        # exactly on a line
    elif name == "planar":
        local = np.concatenate([rng.uniform(-40, 40, size=(BASE, 2)), np.zeros((BASE, 1))], axis=1)
    elif name == "scale":
        t = np.array([800.0, -500.0, 300.0])
    elif name.startswith("theta"):
        th = float(name[5:])
        # (the step is the motion itself: no noise)
        R, t, noise = rodrigues(th * np.array([0.6, -0.48, 0.64])), th * np.array([3.0, -2.0, 1.0]), 0.0
    s = local + c
    q = local @ R.T + c + t + noise
    if name == "identical":
        q = s.copy()
    lab = rng.choice([0.0, 10.0, 40.0], size=(BASE, 1))
    _bases[name] = (np.ascontiguousarray(np.hstack([s, lab])), np.ascontiguousarray(np.hstack([q, lab])), c)
    return _bases[name]


def pair_case(name, n):
    """-> source (n, 4), target (n, 4), kernel, the base's pairs in use, their multiplicities, eight points"""
    s, q, c = pair_base(name)
    idx = np.arange(n) % BASE
    m = min(n, BASE)
    return s[idx], q[idx], PAIR_KERNEL[name], (s[:m], q[:m]), gnref.tile(n, m), gnref.spread(c, [30.0, 30.0, 6.0])


_pair_truth = {}


def pair_truth(name, n):
    if (name, n) not in _pair_truth:
        _, _, k, (bs, bq), mult, _ = pair_case(name, n)
        _pair_truth[(name, n)] = gnref.Step(bs, bq, k, mult)
    return _pair_truth[(name, n)]


# ---- scenes ------------------------------------------------------------------------------------------------------------
MAX_DIST, SEM_TH = 3.0, 0.4
N_MAP = 4000
FRAMES = (17, 64, 65, 257, 1000)
LABELS = (0, 10, 40, 44, 70, 80)
EDGE = 1e-9                       # no pair, accepted or rejected, within this (relative) of MAX_DIST
#           name      kernel   detector
SCENES = (("origin",  1 / 3,   True),
          ("km4",     1 / 3,   True),
          ("km12",    1 / 3,   True),
          ("tiny",    1 / 3,   False),     # the frame within 1e-7 m and 1e-8 rad of its place: the pairs fit that motion exactly,
                                           # so x* does not depend on the weights
          ("far",     1 / 3,   False),     # no pairs: the pose is the guess
          ("utm",     1 / 3,   False),     # reported only
          ("trans",   1 / 3,   True))      # the frame in the sensor's coordinates, a guess that is a pure translation of kilometres
SCENE_KERNEL = {name: k for name, k, _ in SCENES}
SCENE_DETECTOR = {name: d for name, _, d in SCENES}
TRUE_TWIST = [0.25, -0.15, 0.05, 0.01, -0.005, 0.02]
TINY_TWIST = [6e-8, -4e-8, 2e-8, 6e-9, -4.8e-9, 6.4e-9]


def _case(scene, n, loop, lw, filt):
    return dict(id="%s-n%d-loop%d-lw%d-filt%d" % (scene, n, loop, lw, filt), scene=scene, n=n, loop=loop, lw=lw, filt=filt)


CASES = [_case(s, n, loop, lw, f) for s, _, _ in SCENES for n in FRAMES for loop in (0, 2) for lw in (1, 2, 3, 4) for f in (0, 1)]
IDS = [c["id"] for c in CASES]


def make_scene(oracle, scene, n):
    """-> voxel size, map points, frame, guess, the eight points (in the frame's coordinates)"""
    rng = np.random.default_rng(53000 + n)
    c = np.array(CENTRES.get("km4" if scene == "trans" else scene, (0.0, 0.0, 0.0)))
    if scene == "utm":
        c[1] = -1e6                         # (the map's voxel indices end at +-2^20: the furthest a map of 1 m voxels goes)
    local = rng.uniform(-7.0, 7.0, size=(N_MAP, 4))
    local[:, 2] *= 0.25
    local[:, 3] = rng.choice(LABELS, size=N_MAP)
    mp = local.copy()
    mp[:, :3] += c
    pick = rng.choice(N_MAP, size=n, replace=False)
    frame = local[pick].copy()
    if scene != "tiny":
        frame[:, :3] += rng.normal(size=(n, 3)) * 0.03
    # the frame is moved off its place by a small motion about the scene's centre ...
    back = oracle.se3_inv(oracle.se3_exp(TINY_TWIST if scene == "tiny" else TRUE_TWIST))
    frame = oracle.transform_points(back, frame)
    guess = np.array(oracle.IDENTITY, dtype=np.float64)
    if scene == "trans":
        guess[4:] = c                       # ... and stays in the sensor's coordinates
    else:
        frame[:, :3] += c
    if scene == "far":
        frame[:, :3] += 5000.0
    at = np.zeros(3) if scene == "trans" else c + (5000.0 if scene == "far" else 0.0)
    return 1.0, mp, np.ascontiguousarray(frame), guess, gnref.spread(at, [7.0, 7.0, 1.75])


def first_source(frame, guess):
    """the source points of iteration 1: the frame itself, or fl(p + t) under a pure translation (R = I: one rounding
    whatever the order of the operands)"""
    assert np.array_equal(guess[:4], [0.0, 0.0, 0.0, 1.0])
    s = frame.copy()
    s[:, :3] += guess[4:]
    return s


def pairs_clear_of_edge(om, s):
    """(pairs, whether no pair lies within EDGE of MAX_DIST)"""
    src, tgt = om.get_correspondences(s, MAX_DIST, SEM_TH, nthreads=1)
    lo, _ = om.get_correspondences(s, MAX_DIST * (1 - EDGE), SEM_TH, nthreads=1)
    hi, _ = om.get_correspondences(s, MAX_DIST * (1 + EDGE), SEM_TH, nthreads=1)
    return src, tgt, len(lo) == len(src) == len(hi)


def se3_mul_budget(guess, step):
    """the composition est * guess in fp64: 8u (|t_guess| + |t|) for the translation; for a guess that rotates, the
    product of the quaternions and its renormalisation on top (a handful of roundings of a unit quaternion: 8u rad,
    charged per metre of the points' distance from the origin by the caller)"""
    tn = math.sqrt(sum(float(v) ** 2 for v in step.t))
    return 8 * U * (float(np.linalg.norm(guess[4:7])) + tn)


class Env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Scene:
    """a scene, its maps and the truth of its first iteration, shared by the cases that use it"""

    def __init__(self, oracle, scene, n, sage=None):
        self.scene, self.n, self.kernel = scene, n, SCENE_KERNEL[scene]
        self.vs, mp, self.frame, self.guess, self.points = make_scene(oracle, scene, n)
        self.om = oracle.Map(self.vs, 100.0)
        self.om.add_points(mp)
        self.gm = None
        if sage is not None:
            self.gm = sage.VoxelHashMap(self.vs, 100.0, device=0)
            self.gm.AddPoints(mp)
        self.oracle = oracle
        src, tgt, self.clear1 = pairs_clear_of_edge(self.om, first_source(self.frame, self.guess))
        self.pairs1 = (src, tgt)
        self.truth1 = gnref.Step(src, tgt, self.kernel)
        self.second = {}

    def extra1(self):
        return se3_mul_budget(self.guess, self.truth1) if self.truth1.full_rank and self.scene == "trans" else 0.0

    def ratio1(self, pose, gamma):
        return self.truth1.ratio(pose, self.points, gamma, guess=self.guess, extra=self.extra1())

    def two_iterations(self):
        """whether the loop goes on after iteration 1 (its step is not below the 1e-4 of Registration.cpp:97)"""
        return self.truth1.n > 0 and self.truth1.x_norm >= 1e-4

    def truth2(self, P1):
        """the truth of the iteration that follows the pose P1: (Step, pairs clear of the edge)"""
        key = P1.tobytes()
        if key not in self.second:
            s = self.oracle.transform_points(P1, self.frame)
            src, tgt, clear = pairs_clear_of_edge(self.om, s)
            self.second[key] = (gnref.Step(src, tgt, self.kernel), clear)
        return self.second[key]

    def ratio2(self, P1, P2, gamma):
        """the device forms s again from the pristine frame and P1 in its own order of operations: every s is within
        4u |s| of the oracle's, charged to E_b at first order; est * P1 is a general composition: 8u per metre on top"""
        st, _ = self.truth2(P1)
        reach = max(float(np.linalg.norm(p)) for p in self.points) + float(np.linalg.norm(P1[4:7]))
        extra = se3_mul_budget(P1, st) + 8 * U * reach
        return st.ratio(P2, self.points, gamma, guess=P1, extra_b=st.perturbation(4 * U), extra=extra)


def main():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import oracle
    import sage_icp_amd as sage
    oracle.lib()
    shared = {}
    gamma = gnref.GAMMA_EPILOGUE

    def run(sc, c, max_iter):
        with Env(SAGEICP_LOOP=c["loop"], SAGEICP_LW=c["lw"], SAGEICP_FILTER=c["filt"], SAGEICP_MAX_ITER=max_iter):
            T, st = sage.register_frame(sc.frame, sc.gm, sc.guess, MAX_DIST, sc.kernel, SEM_TH, return_stats=True)
        status = sc.gm.loop_status()
        form = dict(single_launch=int(st.single_launch), lanes=int(st.lanes_per_query), compact=int(st.compact_scan),
                    timeouts=int(status.timeouts), last_fallback=int(status.last_fallback))
        return np.array(T, dtype=np.float64), st, form

    for c in CASES:
        t0 = time.time()
        key = (c["scene"], c["n"])
        if key not in shared:
            shared[key] = Scene(oracle, c["scene"], c["n"], sage)
        sc = shared[key]
        t1 = sc.truth1
        P1, s1, form1 = run(sc, c, 1)
        P1b, s1b, _ = run(sc, c, 1)
        out = dict(id=c["id"], same_map=sc.om.size() == sc.gm.size(), clear1=bool(sc.clear1), form1=form1,
                   pairs1=int(t1.n), n_corr1=int(s1.n_corr_hist[0]), iterations1=int(s1.iterations),
                   repeat_same=bool(np.array_equal(P1, P1b) and float(s1.last_step_norm) == float(s1b.last_step_norm)),
                   pose_is_guess=bool(np.array_equal(P1, sc.guess)), full_rank1=bool(t1.full_rank), two=bool(sc.two_iterations()))
        if t1.full_rank:
            out["ratio1"] = sc.ratio1(P1, gamma)
            out["theta1"], out["x_norm1"] = t1.theta, t1.x_norm
            out["step1"] = abs(float(s1.last_step_norm) - t1.x_norm) / (t1.budget_x(gamma) + 8 * U * t1.x_norm)
            out["converged1"] = int(s1.converged)
        P2, s2, form2 = run(sc, c, 2)
        out["form2"], out["iterations2"] = form2, int(s2.iterations)
        if t1.full_rank and sc.two_iterations():
            t2, clear2 = sc.truth2(P1)
            out.update(clear2=bool(clear2), pairs2=int(t2.n), n_corr2=[int(s2.n_corr_hist[0]), int(s2.n_corr_hist[1])],
                       full_rank2=bool(t2.full_rank))
            if t2.full_rank:
                out["ratio2"] = sc.ratio2(P1, P2, gamma)
                out["step2"] = abs(float(s2.last_step_norm) - t2.x_norm) / (
                    t2.budget_x(gamma, t2.perturbation(4 * U)) + 8 * U * t2.x_norm)
        else:
            out["same_after_two"] = bool(np.array_equal(P1, P2))
        out["seconds"] = round(time.time() - t0, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
