"""The registration quality report on the device (sageicp_registration_quality*, csrc/quality.hip) against the truth of
tests/qualityref.py over the ORACLE's pairs.  Needs a real MI355X:  python -m pytest tests -m gpu

Counts are compared bit for bit.  A real sum is held to |got - exact| <= gamma_serial(n_pairs) E, E the sum of the
magnitudes of its terms (qualityref.py): (16 + n) u bounds the roundings of a term plus any order of summation.  The
derived values are held to the forward bound of a backward-stable 6 x 6 factorisation of the RETURNED JTJ,
64 u cond2(JTJ) |C_exact|max, and the pose covariance to 8 u sum |terms| of the exact triple product of the returned
covariance.

The pass deals tiles of 256 queries to at most 256 workgroups and the reducer adds at most 256 slabs in one step
(quality.h): 256 * 256 + 1 queries are 257 tiles — workgroup 0 takes a second tile, the one place where the form changes.
256 * 257 + 1 (the scan of the compaction's second step) is run too.

The UTM scene is the same points shifted by (5e5, 5.5e6, 0) in a map of voxel 8.0: a map of voxel 1.0 refuses
coordinates beyond 2^20 voxels (AddPoints: SAGEICP_ERR_CAPACITY), so the scene cannot be held at voxel 1.0 at all."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import qualityref as qr
from gnref import U, _solve, gamma_serial

pytestmark = pytest.mark.gpu

LABELS = [0, 0, 10, 40, 44, 50, 70, 71, 80, 251]
SPECIAL = [10.9, 300.0, -3.0]          # class 10, other, other
TH = 0.4
KERNEL = 0.5
MD_ALL, MD_NONE, MD_MIXED = 1e3, 1e-7, 0.25
POSE = np.array([0.02, -0.05, 0.1, 0.99, 0.4, -0.3, 0.05])
POSE[:4] /= np.linalg.norm(POSE[:4])
UTM = np.array([5e5, 5.5e6, 0.0])
N_TILES2 = 256 * 256 + 1
N_SCAN2 = 256 * 257 + 1
COUNT_KEYS = ("n_queries", "n_pairs", "pairs_same_label", "pairs_unlabelled", "pairs_cross_label", "other_queries",
              "other_pairs")


def _map_points(seed=11, n=6000, span=6.0):
    rng = np.random.default_rng(seed)
    mp = rng.uniform(-span, span, size=(n, 4))
    mp[:, 2] *= 0.2
    mp[:, 3] = rng.choice(LABELS, size=n)
    return mp


class Scene:
    """the map of 6 000 random points as the product and the oracle hold it (shifted by `shift`), query sets by size,
    and per (n, max_dist, pose) the oracle's pairs, the product's report and the truth, each computed once"""

    def __init__(self, sage, oracle, shift=(0.0, 0.0, 0.0), voxel=1.0):
        self.sage, self.oracle, self.shift = sage, oracle, np.asarray(shift, dtype=np.float64)
        mp = _map_points()
        mp[:, :3] += self.shift
        self.a = sage.VoxelHashMap(voxel, 100.0)
        self.b = oracle.Map(voxel, 100.0, 20, 20)
        self.a.AddPoints(mp)
        self.b.add_points(mp)
        self.a.sync()
        self.stored = self.a.Pointcloud()
        self._q, self._pairs, self._report, self._truth = {}, {}, {}, {}

    def queries(self, n):
        """n map points (as stored), each moved by up to 0.3 per axis; the first rows carry the labels of SPECIAL"""
        if n not in self._q:
            rng = np.random.default_rng(1000 + n)
            q = self.stored[rng.integers(0, len(self.stored), size=n)].copy()
            q[:, :3] += rng.uniform(-0.3, 0.3, size=(n, 3))
            q[:, 3] = rng.choice(LABELS, size=n)
            q[:min(n, 3), 3] = SPECIAL[:min(n, 3)]
            self._q[n] = q
        return self._q[n]

    def moved(self, q, pose):
        return q if pose is None else self.sage.transform_points(pose, q)

    def pairs(self, n, md, pose):
        key = (n, md, pose is not None)
        if key not in self._pairs:
            self._pairs[key] = self.b.get_correspondences(self.moved(self.queries(n), pose), md, TH, with_index=True)
        return self._pairs[key]

    def report(self, n, md, pose):
        key = (n, md, pose is not None)
        if key not in self._report:
            self._report[key] = self.a.RegistrationQuality(self.queries(n), md, KERNEL, TH, pose=pose)
        return self._report[key]

    def truth(self, n, md, pose):
        key = (n, md, pose is not None)
        if key not in self._truth:
            src, tgt, _ = self.pairs(n, md, pose)
            self._truth[key] = qr.Quality(self.queries(n)[:, 3], src, tgt, KERNEL, derive=False)
        return self._truth[key]


@pytest.fixture(scope="module")
def scene(gpu_sage, oracle):
    return Scene(gpu_sage, oracle)


@pytest.fixture(scope="module")
def utm_scene(gpu_sage, oracle):
    return Scene(gpu_sage, oracle, shift=UTM, voxel=8.0)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda() if dtype is None else t.cuda().to(dtype)


def _check_counts(got, q_labels, src, tgt):
    want = qr.counts(q_labels, src, tgt)
    d = got.as_dict()
    assert got.valid == 1
    for k in COUNT_KEYS:
        assert d[k] == want[k], k
    assert np.array_equal(d["class_queries"], want["class_queries"])
    assert np.array_equal(d["class_pairs"], want["class_pairs"])
    assert got.pairs_same_label + got.pairs_unlabelled + got.pairs_cross_label == got.n_pairs
    assert int(d["class_queries"].sum()) + got.other_queries == got.n_queries
    assert int(d["class_pairs"].sum()) + got.other_pairs == got.n_pairs


# ---- counts, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", [None, POSE], ids=["nopose", "pose"])
@pytest.mark.parametrize("md", [MD_ALL, MD_NONE, MD_MIXED], ids=["all", "none", "mixed"])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1000, N_TILES2, N_SCAN2])
def test_counts(scene, n, md, pose):
    src, tgt, _ = scene.pairs(n, md, pose)
    got = scene.report(n, md, pose)
    if md == MD_ALL and pose is None:        # (moved by the pose, a query at the rim may find its 27 voxels empty)
        assert got.n_pairs == n
    elif md == MD_ALL:
        assert 0.9 * n <= got.n_pairs <= n
    elif md == MD_NONE:
        assert got.n_pairs == 0
    elif n >= 255:
        assert 0 < got.n_pairs < n
    _check_counts(got, scene.queries(n)[:, 3], src, tgt)
    if n >= 3:           # 300 and -3 land in `other`, 10.9 in class 10
        assert got.other_queries == 2 and got.class_queries[10] >= 1


# ---- the real sums --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", [None, POSE], ids=["nopose", "pose"])
@pytest.mark.parametrize("md", [MD_ALL, MD_NONE, MD_MIXED], ids=["all", "none", "mixed"])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1000])
def test_real_sums(scene, n, md, pose):
    ref = scene.truth(n, md, pose)
    got = scene.report(n, md, pose)
    assert got.n_pairs == ref.n
    worst, where = ref.sums_ratio(got.as_dict())
    print("n %d pairs %d: worst |got - exact| / (gamma_serial E) = %.3g at %s" % (n, ref.n, worst, where))
    assert worst <= 1.0, where


def test_real_sums_second_tile(scene):
    """257 tiles: workgroup 0's running sums and class sums go through a second tile"""
    ref = scene.truth(N_TILES2, MD_MIXED, None)
    got = scene.report(N_TILES2, MD_MIXED, None)
    assert got.n_pairs == ref.n > 1000
    worst, where = ref.sums_ratio(got.as_dict())
    print("pairs %d: worst |got - exact| / (gamma_serial E) = %.3g at %s" % (ref.n, worst, where))
    assert worst <= 1.0, where


# ---- the derived values ---------------------------------------------------------------------------------------------------
def _frac_matrix(M):
    return [[Fraction(float(v)) for v in row] for row in np.asarray(M, dtype=np.float64).reshape(6, 6)]


def _check_derived(got, pose):
    d = got.as_dict()
    n, nq = got.n_pairs, got.n_queries
    # fitness and rmse: the formulas on the returned sums, to 4 u relative
    assert abs(got.fitness - n / nq) <= 4 * U * (n / nq)
    want_rmse = math.sqrt(got.sum_r2 / n) if n else 0.0
    assert abs(got.rmse - want_rmse) <= 4 * U * want_rmse
    assert got.sum_w == d["JTJ"][0, 0] == d["JTJ"][1, 1] == d["JTJ"][2, 2]
    assert np.array_equal(d["JTJ"], d["JTJ"].T) and np.array_equal(d["info"], d["info"].T)
    assert d["info"][0, 0] == n
    if not got.covariance_valid:
        return None
    A = _frac_matrix(d["JTJ"])
    b = [Fraction(float(v)) for v in d["JTr"]]
    cond = float(np.linalg.cond(d["JTJ"], 2))
    eye = [[Fraction(int(i == j)) for j in range(6)] for i in range(6)]
    Ainv = _solve(A, eye)
    x = [-sum(Ainv[i][j] * b[j] for j in range(6)) for i in range(6)]
    s2 = Fraction(float(got.sum_w_r2)) / (3 * n - 6)
    C = [[s2 * v for v in row] for row in Ainv]
    bound = 64 * U * cond
    x_max = max(abs(float(v)) for v in x)
    err_x = max(abs(float(Fraction(float(g)) - w)) for g, w in zip(d["step"], x))
    c_max = max(abs(float(v)) for row in C for v in row)
    err_c = max(abs(float(Fraction(float(d["covariance"][i, j])) - C[i][j])) for i in range(6) for j in range(6))
    print("cond2 %.3g  step err %.3g of %.3g  covariance err %.3g of %.3g" % (cond, err_x, bound * x_max, err_c, bound * c_max))
    assert err_x <= bound * x_max
    assert err_c <= bound * c_max
    assert abs(got.step_norm - math.sqrt(sum(v * v for v in d["step"]))) <= 8 * U * got.step_norm
    # the pose covariance: the exact triple product of the RETURNED covariance
    t = (0.0, 0.0, 0.0) if pose is None else pose[4:7]
    P, E = qr.pose_covariance(_frac_matrix(d["covariance"]), t)
    for i in range(6):
        for j in range(6):
            err = abs(Fraction(float(d["covariance_pose"][i, j])) - P[i][j])
            assert err <= 8 * Fraction(U) * E[i][j], (i, j)
    if pose is None:
        assert np.array_equal(d["covariance_pose"], d["covariance"])
    return cond


@pytest.mark.parametrize("pose", [None, POSE], ids=["nopose", "pose"])
@pytest.mark.parametrize("md", [MD_ALL, MD_MIXED], ids=["all", "mixed"])
@pytest.mark.parametrize("n", [3, 255, 1000])
def test_derived_values(scene, n, md, pose):
    got = scene.report(n, md, pose)
    cond = _check_derived(got, pose)
    if md == MD_ALL:
        assert got.covariance_valid == 1 and cond is not None and got.fitness == (1.0 if pose is None else got.n_pairs / n)
        assert np.all(np.diag(got.as_dict()["covariance"]) > 0)


def _assert_nothing_derived(got):
    d = got.as_dict()
    assert got.valid == 1 and got.covariance_valid == 0
    assert got.step_norm == 0.0 and not d["step"].any() and not d["covariance"].any() and not d["covariance_pose"].any()


def test_no_covariance_without_three_pairs_in_general_position(scene):
    for n, md, pairs in ((257, MD_NONE, 0), (1, MD_ALL, 1), (2, MD_ALL, 2)):
        got = scene.report(n, md, None)
        assert got.n_pairs == pairs
        _assert_nothing_derived(got)
        _check_derived(got, None)
        assert got.rmse == 0.0 if pairs == 0 else got.rmse > 0.0
    # collinear queries: J depends on the queries only, JTJ is singular whatever the map's points are
    line = np.zeros((7, 4))
    line[:, 0] = np.linspace(-3.0, 3.0, 7)
    line[:, 1:3] = [2.0, 0.25]
    line[:, 3] = 40.0
    got = scene.a.RegistrationQuality(line, MD_ALL, KERNEL, TH)
    src, tgt, _ = scene.b.get_correspondences(line, MD_ALL, TH, with_index=True)
    _check_counts(got, line[:, 3], src, tgt)
    assert got.n_pairs == 7 and got.fitness == 1.0 and got.rmse > 0.0
    _assert_nothing_derived(got)


# ---- UTM ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("md", [MD_ALL, MD_MIXED], ids=["all", "mixed"])
def test_utm(utm_scene, md):
    s = utm_scene
    assert np.all(s.stored[:, 1] > 5.4e6) and len(s.stored) > 50
    src, tgt, _ = s.pairs(1000, md, None)
    got = s.report(1000, md, None)            # (SAGEICP_OK: the binding raises otherwise)
    _check_counts(got, s.queries(1000)[:, 3], src, tgt)
    assert got.n_pairs > 10
    ref = s.truth(1000, md, None)
    worst, where = ref.sums_ratio(got.as_dict())
    print("UTM pairs %d: worst |got - exact| / (gamma_serial E) = %.3g at %s" % (ref.n, worst, where))
    assert worst <= 1.0, where
    cond = _check_derived(got, None)
    print("UTM covariance_valid %d cond2 %s" % (got.covariance_valid, cond))


# ---- the same bits ----------------------------------------------------------------------------------------------------------
def test_same_bits_run_to_run_and_between_entries(scene):
    for n, md, pose in ((1000, MD_MIXED, POSE), (N_TILES2, MD_ALL, None)):
        q = scene.queries(n)
        want = bytes(scene.report(n, md, pose))
        assert bytes(scene.a.RegistrationQuality(q, md, KERNEL, TH, pose=pose)) == want
        dev = _dev(q)
        assert bytes(scene.a.RegistrationQuality(dev, md, KERNEL, TH, pose=pose)) == want
        assert bytes(scene.a.RegistrationQuality(dev, md, KERNEL, TH, pose=pose)) == want


def test_same_bits_other_layouts(scene):
    q = scene.queries(1000)[3:]              # (without the rows labelled 10.9, 300 and -3: uint8 cannot hold them)
    want = bytes(scene.a.RegistrationQuality(q, MD_MIXED, KERNEL, TH, pose=POSE))
    labels = _dev(q[:, 3].astype(np.uint8))
    assert bytes(scene.a.RegistrationQuality(_dev(q[:, :3]), MD_MIXED, KERNEL, TH, pose=POSE, labels=labels)) == want
    assert bytes(scene.a.RegistrationQuality(_dev(q), MD_MIXED, KERNEL, TH, pose=POSE,
                                             labels=_dev(q[:, 3].astype(np.int32)))) == want
    q = scene.queries(1000)
    q32 = q.astype(np.float32)
    want = bytes(scene.a.RegistrationQuality(q32.astype(np.float64), MD_MIXED, KERNEL, TH, pose=POSE))
    assert bytes(scene.a.RegistrationQuality(_dev(q32), MD_MIXED, KERNEL, TH, pose=POSE)) == want


def test_non_finite_rows_are_refused_on_the_device(scene):
    q = scene.queries(257).copy()
    q[200, 1] = np.nan
    with pytest.raises(scene.sage.SageIcpError) as e:
        scene.a.RegistrationQuality(_dev(q), MD_ALL, KERNEL, TH)
    assert e.value.code == scene.sage.ERR_INVALID and "not finite" in str(e.value)


def test_resident_map_stays_resident(scene):
    sage = scene.sage
    m = sage.VoxelHashMap(1.0, 100.0)
    m.UpdateOnDevice(_map_points(), sage.IDENTITY)
    assert m.resident()
    q = scene.queries(1000)
    a = m.RegistrationQuality(_dev(q), MD_MIXED, KERNEL, TH, pose=POSE)
    assert m.resident()
    b = m.RegistrationQuality(q, MD_MIXED, KERNEL, TH, pose=POSE)
    assert m.resident()
    assert a.valid == 1 and 0 < a.n_pairs < 1000 and bytes(a) == bytes(b)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------
def _quat_to_mat(q):
    x, y, z, w = q
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
            2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]


def _mat_apply(R, t, p):
    return [R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0],
            R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1],
            R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2]]


def _se3_mul(A, B):
    """csrc/se3_math.h's se3_mul, operation for operation"""
    ax, ay, az, aw = (float(v) for v in A[:4])
    bx, by, bz, bw = (float(v) for v in B[:4])
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by - ax * bz + ay * bw + az * bx
    z = aw * bz + ax * by - ay * bx + az * bw
    w = aw * bw - ax * bx - ay * by - az * bz
    inv = 1.0 / math.sqrt(x * x + y * y + z * z + w * w)
    t = _mat_apply(_quat_to_mat([ax, ay, az, aw]), [float(v) for v in A[4:7]], [float(v) for v in B[4:7]])
    return [x * inv, y * inv, z * inv, w * inv] + t


def _se3_inv(A):
    qi = [-float(A[0]), -float(A[1]), -float(A[2]), float(A[3])]
    t = _mat_apply(_quat_to_mat(qi), [0.0, 0.0, 0.0], [float(v) for v in A[4:7]])
    return qi + [-t[0], -t[1], -t[2]]


class _Threshold:
    """Pipeline::adaptive_threshold and the constant-velocity guess (csrc/pipeline.hpp; pipeline/sageICP.cpp:103-121,
    core/Threshold.cpp:29-50) from the poses, operation for operation: sigma of the NEXT frame"""

    def __init__(self, cfg):
        self.cfg, self.poses, self.sse2, self.num = cfg, [], 0.0, 0
        self.deviation = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
        self.guess = None

    def sigma(self):
        cfg, I = self.cfg, [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
        s = self._sigma()
        N = len(self.poses)
        prediction = _se3_mul(_se3_inv(self.poses[N - 2]), self.poses[N - 1]) if N >= 2 else I
        self.guess = _se3_mul(self.poses[-1] if N else I, prediction)
        return s

    def _sigma(self):
        cfg = self.cfg
        moved = False
        if self.poses:
            d = _se3_mul(_se3_inv(self.poses[0]), self.poses[-1])
            moved = math.sqrt(d[4] * d[4] + d[5] * d[5] + d[6] * d[6]) > 5.0 * cfg.min_motion_th
        if not moved:
            return cfg.initial_threshold
        q = self.deviation
        theta = 2.0 * math.atan2(math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), abs(q[3]))
        delta_rot = 2.0 * cfg.max_range * math.sin(theta / 2.0)
        delta_trans = math.sqrt(q[4] * q[4] + q[5] * q[5] + q[6] * q[6])
        err = delta_trans + delta_rot
        if err > cfg.min_motion_th:
            self.sse2 += err * err
            self.num += 1
        if self.num < 1:
            return cfg.initial_threshold
        return math.sqrt(self.sse2 / self.num)

    def registered(self, pose):
        self.deviation = _se3_mul(_se3_inv(self.guess), pose)
        self.poses.append([float(v) for v in pose])


def _clone_local_map(sage, p):
    cfg = p.config
    h = sage.lib().sageicp_map_clone(sage.lib().sageicp_pipeline_local_map(p._h))
    assert h
    return sage.VoxelHashMap(cfg.voxel_size_map, cfg.local_map_range, _handle=h)


def test_pipeline_report_equals_the_entry_on_the_map_before_the_update(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(7, 5, points_per_frame=20000)
    cfg = sage.make_pipeline_config()
    a, off = sage.SageICP(cfg), sage.SageICP(cfg)
    a.set_quality(True)
    th = _Threshold(cfg)
    adaptive = 0
    for k, f in enumerate(frames):
        before = _clone_local_map(sage, a)
        pose = a.RegisterFrame(f)[0]
        pose_off = off.RegisterFrame(f)[0]
        assert np.array_equal(pose, pose_off), "frame %d" % k
        assert not off.quality().valid
        sigma = th.sigma()
        th.registered(pose)
        adaptive += sigma != cfg.initial_threshold
        got = a.quality()
        if k == 0:
            assert got.valid == 0 and bytes(got) == bytes(sage.QUALITY_BYTES)
            continue
        want = before.RegistrationQuality(a.source(), 3.0 * sigma, sigma / 3.0, cfg.sem_th, pose=pose)
        assert got.valid == 1 and got.n_queries == a.source_size() and got.n_pairs > 100
        assert got.covariance_valid == 1 and 0.0 < got.fitness <= 1.0 and got.rmse > 0.0
        assert bytes(got) == bytes(want), "frame %d (sigma %r)" % (k, sigma)
    assert adaptive > 0, "the stream never left the initial threshold: the test would not see a wrong sigma"
    assert np.array_equal(a.LocalMap(), off.LocalMap())
    assert np.array_equal(np.array(a.poses()), np.array(off.poses()))
    a.reinitialize()
    assert bytes(a.quality()) == bytes(sage.QUALITY_BYTES)
    # after a restart: the first frame has no report, the second has; switching off drops it
    a.RegisterFrame(frames[0])
    assert a.quality().valid == 0
    a.RegisterFrame(frames[1])
    assert a.quality().valid == 1
    a.set_quality(False)
    assert a.quality().valid == 0
