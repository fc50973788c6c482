"""A batch of candidate poses scored in one pass and Relocalize on the device (sageicp_score_poses*, sageicp_relocalize*,
csrc/score.hip).  Needs a real MI355X:  python -m pytest tests -m gpu

The contract is bits: out[c] of a batch holds the same-named fields of sageicp_registration_quality at poses[c] alone,
whatever k, the chunking and the other candidates are — compared as bytes.  The shapes are the quality test's (a tile is
256 queries, 256 * 256 + 1 queries are the one place where a workgroup takes a second tile) times batches of 1, 2, 3 and
7 poses; n = 1 with 65 537 candidates is past any 16-bit grid dimension.  An independent truth stands beside the
single entry: the counts over the oracle's pairs, and the quality test's bound (16 + n_pairs) u sum |terms| on the real
sums (tests/qualityref.py).  Relocalize is compared with its definition — the Python composition of the public entries —
bit for bit, and with the oracle on the scene of tests/scoreref.py (its margins are checked in
tests/test_score_poses_host.py)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import qualityref as qr
import scoreref as sr
from gnref import gamma_serial

pytestmark = pytest.mark.gpu

LABELS = [0, 0, 10, 40, 44, 50, 70, 71, 80, 251]
SPECIAL = [10.9, 300.0, -3.0]
TH = 0.4
KERNEL = 0.5
MD_ALL, MD_NONE, MD_MIXED = 1e3, 1e-7, 0.25
POSE = np.array([0.02, -0.05, 0.1, 0.99, 0.4, -0.3, 0.05])
POSE[:4] /= np.linalg.norm(POSE[:4])
N_TILES2 = 256 * 256 + 1
SHARED = ("fitness", "rmse", "step_norm", "sum_r2", "sum_w", "sum_w_r2", "step", "JTr", "JTJ", "n_queries", "n_pairs",
          "pairs_same_label", "pairs_unlabelled", "pairs_cross_label", "valid")


def _map_points(seed=11, n=6000, span=6.0):
    """the map of tests/test_quality_gpu.py"""
    rng = np.random.default_rng(seed)
    mp = rng.uniform(-span, span, size=(n, 4))
    mp[:, 2] *= 0.2
    mp[:, 3] = rng.choice(LABELS, size=n)
    return mp


def _perturbed(seed):
    rng = np.random.default_rng(seed)
    p = POSE.copy()
    p[:4] += rng.uniform(-0.01, 0.01, size=4)
    p[:4] /= np.linalg.norm(p[:4])
    p[4:] += rng.uniform(-0.2, 0.2, size=3)
    return p


FAR = POSE.copy()
FAR[4:] += [500.0, 0.0, 0.0]
# POSE, small perturbations of it, one pose 500 m away (no pairs), one duplicate
POSES = np.array([POSE, _perturbed(1), FAR, _perturbed(2), POSE, _perturbed(3), _perturbed(4)])
I_FAR, I_DUP = 2, 4


def expected(q):
    """the PoseScore record of a Quality of the single entry"""
    r = np.zeros(1, dtype=_dtype())
    for f in SHARED:
        v = getattr(q, f)
        r[f][0] = np.array(v[:], dtype=np.float64).reshape(r[f][0].shape) if hasattr(v, "_length_") else v
    r["score"][0] = q.sum_w
    r["step_valid"][0] = q.covariance_valid
    return r


def _dtype():
    import sage_icp_amd
    return sage_icp_amd.POSE_SCORE_DTYPE


class Scene:
    def __init__(self, sage, oracle):
        self.sage = sage
        mp = _map_points()
        self.a = sage.VoxelHashMap(1.0, 100.0)
        self.b = oracle.Map(1.0, 100.0, 20, 20)
        self.a.AddPoints(mp)
        self.b.add_points(mp)
        self.a.sync()
        self.stored = self.a.Pointcloud()
        self._q, self._single = {}, {}

    def queries(self, n):
        """the query sets of tests/test_quality_gpu.py"""
        if n not in self._q:
            rng = np.random.default_rng(1000 + n)
            q = self.stored[rng.integers(0, len(self.stored), size=n)].copy()
            q[:, :3] += rng.uniform(-0.3, 0.3, size=(n, 3))
            q[:, 3] = rng.choice(LABELS, size=n)
            q[:min(n, 3), 3] = SPECIAL[:min(n, 3)]
            self._q[n] = q
        return self._q[n]

    def single(self, n, md, c):
        """the single entry at POSES[c], as a PoseScore record: computed once"""
        key = (n, md, c)
        if key not in self._single:
            self._single[key] = expected(self.a.RegistrationQuality(self.queries(n), md, KERNEL, TH, pose=POSES[c]))
        return self._single[key]

    def singles(self, n, md, k):
        return np.concatenate([self.single(n, md, c) for c in range(k)])


@pytest.fixture(scope="module")
def scene(gpu_sage, oracle):
    return Scene(gpu_sage, oracle)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda() if dtype is None else t.cuda().to(dtype)


def _assert_same(got, want):
    for f in got.dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    assert got.tobytes() == want.tobytes()


# ---- bit for bit against the single entry ---------------------------------------------------------------------------------
@pytest.mark.parametrize("md", [MD_ALL, MD_MIXED, MD_NONE], ids=["all", "mixed", "none"])
@pytest.mark.parametrize("k", [1, 2, 3, 7])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_batch_equals_single_entries(scene, n, k, md):
    got = scene.a.ScorePoses(scene.queries(n), POSES[:k], md, KERNEL, TH)
    assert got.shape == (k,)
    _assert_same(got, scene.singles(n, md, k))
    assert np.all(got["valid"] == 1) and np.all(got["n_queries"] == n)
    if md == MD_NONE:
        assert not got["n_pairs"].any() and not got["step_valid"].any()
    elif n >= 255:
        assert got["n_pairs"][0] > 0 and got["step_valid"][0] == 1 and got["score"][0] == got["sum_w"][0] > 0
    if k > I_FAR:           # 500 m away: a valid answer without pairs
        assert got["valid"][I_FAR] == 1 and got["n_pairs"][I_FAR] == 0 and got["step_valid"][I_FAR] == 0
        assert got["score"][I_FAR] == 0.0
    if k > I_DUP:
        assert got[I_DUP].tobytes() == got[0].tobytes()


@pytest.mark.parametrize("md", [MD_ALL, MD_MIXED, MD_NONE], ids=["all", "mixed", "none"])
def test_second_tile(scene, md):
    """257 tiles per candidate: workgroup 0 of every candidate takes a second tile"""
    got = scene.a.ScorePoses(scene.queries(N_TILES2), POSES[:3], md, KERNEL, TH)
    _assert_same(got, scene.singles(N_TILES2, md, 3))
    if md != MD_NONE:
        assert got["n_pairs"][0] > 1000 and got["n_pairs"][I_FAR] == 0


# ---- the chunking ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k", [(257, 7), (1000, 3)], ids=["3+3+1", "one-per-chunk"])
def test_chunking_does_not_change_a_bit(scene, n, k):
    want = scene.a.ScorePoses(scene.queries(n), POSES[:k], MD_MIXED, KERNEL, TH)
    old = os.environ.get("SAGEICP_SCORE_CHUNK_ROWS")
    os.environ["SAGEICP_SCORE_CHUNK_ROWS"] = "1000"
    try:
        got = scene.a.ScorePoses(scene.queries(n), POSES[:k], MD_MIXED, KERNEL, TH)
    finally:
        if old is None:
            del os.environ["SAGEICP_SCORE_CHUNK_ROWS"]
        else:
            os.environ["SAGEICP_SCORE_CHUNK_ROWS"] = old
    _assert_same(got, want)
    _assert_same(got, scene.singles(n, MD_MIXED, k))
    _assert_same(scene.a.ScorePoses(scene.queries(n), POSES[:k], MD_MIXED, KERNEL, TH), want)


# ---- many candidates ------------------------------------------------------------------------------------------------------
def test_more_candidates_than_a_16_bit_grid_dimension(scene):
    k = 65537
    poses = np.tile(POSE, (k, 1))
    where = {0: 1, 1: 3, k - 3: 5, k - 2: 6, k - 1: I_FAR}          # index in the batch: index in POSES
    for i, c in where.items():
        poses[i] = POSES[c]
    got = scene.a.ScorePoses(scene.queries(1), poses, MD_ALL, KERNEL, TH)
    for i, c in where.items():
        _assert_same(got[i:i + 1], scene.single(1, MD_ALL, c))
    rest = np.delete(got, list(where))
    assert len(rest) == k - 5 and rest.tobytes() == rest[:1].tobytes() * (k - 5)
    _assert_same(rest[:1], scene.single(1, MD_ALL, 0))
    assert rest["n_pairs"][0] == 1


# ---- an independent truth ---------------------------------------------------------------------------------------------------
def test_counts_and_sums_against_the_oracle(scene):
    n, k = 1000, 7
    q = scene.queries(n)
    got = scene.a.ScorePoses(q, POSES[:k], MD_MIXED, KERNEL, TH)
    truth = None
    for c in range(k):
        src, tgt, _ = scene.b.get_correspondences(scene.sage.transform_points(POSES[c], q), MD_MIXED, TH, with_index=True)
        want = qr.counts(q[:, 3], src, tgt)
        for f in ("n_queries", "n_pairs", "pairs_same_label", "pairs_unlabelled", "pairs_cross_label"):
            assert int(got[f][c]) == want[f], (c, f)
        if c == 0:
            truth = qr.Quality(q[:, 3], src, tgt, KERNEL, derive=False)
    assert 0 < got["n_pairs"][0] < n and truth.n == got["n_pairs"][0]
    # the real sums of candidate 0: |got - exact| <= (16 + n_pairs) u sum |terms|
    flat = {"sum_r2": got["sum_r2"][0], "sum_w": got["sum_w"][0], "sum_w_r2": got["sum_w_r2"][0]}
    for i in range(6):
        flat["JTr[%d]" % i] = got["JTr"][0][i]
        for j in range(6):
            flat["JTJ[%d][%d]" % (i, j)] = got["JTJ"][0][i, j]
    gamma = Fraction(gamma_serial(truth.n))
    worst, seen = 0.0, 0
    for name, exact, e in truth.flat():
        if name not in flat:
            continue
        seen += 1
        d = abs(Fraction(float(flat[name])) - exact)
        if d:
            assert e != 0, name
            worst = max(worst, float(d / (e * gamma)))
    print("pairs %d: worst |got - exact| / (gamma_serial E) = %.3g over %d sums" % (truth.n, worst, seen))
    assert seen == 3 + 6 + 36 and worst <= 1.0


# ---- entries and state ------------------------------------------------------------------------------------------------------
def test_device_entry_equals_host_entry(scene):
    q = scene.queries(1000)
    want = scene.singles(1000, MD_MIXED, 7)
    _assert_same(scene.a.ScorePoses(_dev(q), POSES, MD_MIXED, KERNEL, TH), want)
    _assert_same(scene.a.ScorePoses(_dev(q), POSES, MD_MIXED, KERNEL, TH), want)            # two calls
    _assert_same(scene.a.ScorePoses(q, POSES, MD_MIXED, KERNEL, TH), want)
    # float32 rows with separate uint8 labels (without the rows labelled 10.9, 300 and -3)
    q32 = q[3:].astype(np.float32)
    host = scene.a.ScorePoses(q32.astype(np.float64), POSES, MD_MIXED, KERNEL, TH)
    dev = scene.a.ScorePoses(_dev(q32[:, :3]), POSES, MD_MIXED, KERNEL, TH, labels=_dev(q32[:, 3].astype(np.uint8)))
    _assert_same(dev, host)
    assert host["n_pairs"][0] > 0


def test_empty_map_empty_frame_no_candidates(scene):
    sage = scene.sage
    empty = sage.VoxelHashMap(1.0, 100.0)
    q = scene.queries(257)
    for got in (empty.ScorePoses(q, POSES, MD_ALL, KERNEL, TH), empty.ScorePoses(_dev(q), POSES, MD_ALL, KERNEL, TH),
                scene.a.ScorePoses(np.zeros((0, 4)), POSES, MD_ALL, KERNEL, TH),
                scene.a.ScorePoses(torch.empty((0, 4), dtype=torch.float64, device="cuda"), POSES, MD_ALL, KERNEL, TH)):
        assert got.shape == (7,) and got.tobytes() == bytes(7 * sage.POSE_SCORE_BYTES)
    assert scene.a.ScorePoses(q, np.zeros((0, 7)), MD_ALL, KERNEL, TH).shape == (0,)
    assert scene.a.ScorePoses(_dev(q), np.zeros((0, 7)), MD_ALL, KERNEL, TH).shape == (0,)


def test_resident_map_stays_resident(scene):
    sage = scene.sage
    m = sage.VoxelHashMap(1.0, 100.0)
    m.UpdateOnDevice(_map_points(), sage.IDENTITY)
    assert m.resident()
    q = scene.queries(1000)
    stats, loops = m.table_stats(), bytes(m.loop_status())
    a = m.ScorePoses(_dev(q), POSES, MD_MIXED, KERNEL, TH)
    assert m.resident() and m.table_stats() == stats and bytes(m.loop_status()) == loops
    b = m.ScorePoses(q, POSES, MD_MIXED, KERNEL, TH)
    assert m.resident() and m.table_stats() == stats and bytes(m.loop_status()) == loops
    assert 0 < a["n_pairs"][0] < 1000 and a.tobytes() == b.tobytes()
    _assert_same(a[:1], expected(m.RegistrationQuality(q, MD_MIXED, KERNEL, TH, pose=POSE)))
    assert m.resident()


def test_non_finite_row_refuses_with_out_untouched(scene):
    sage = scene.sage
    q = scene.queries(257).copy()
    q[200, 1] = np.nan
    poses = np.ascontiguousarray(POSES)
    for device in (False, True):
        out = np.full(7 * sage.POSE_SCORE_BYTES, 0xAB, dtype=np.uint8)
        if device:
            t = _dev(q)
            f, stream = sage._device_rows(sage.DeviceFrame, t, None, 0, sage._FRAME_WORDS)
            rc = sage.lib().sageicp_score_poses_device(scene.a._h, C.byref(f), poses.ctypes.data_as(sage._dp), 7, MD_ALL,
                                                       KERNEL, TH, stream, out.ctypes.data)
        else:
            rc = sage.lib().sageicp_score_poses(scene.a._h, q.ctypes.data_as(sage._dp), 257, poses.ctypes.data_as(sage._dp),
                                                7, MD_ALL, KERNEL, TH, out.ctypes.data)
        assert rc == sage.ERR_INVALID and b"not finite" in sage.lib().sageicp_last_error()
        assert np.all(out == 0xAB)
    # and the handle answers as before
    _assert_same(scene.a.ScorePoses(scene.queries(257), POSES[:3], MD_MIXED, KERNEL, TH), scene.singles(257, MD_MIXED, 3))


def test_the_new_buffers_disturb_nothing(scene):
    sage = scene.sage
    q = scene.queries(1000)
    guess = _perturbed(9)
    quality = bytes(scene.a.RegistrationQuality(q, MD_MIXED, KERNEL, TH, pose=POSE))
    pose = sage.register_frame(q, scene.a, guess, 1.0, KERNEL, TH)
    scene.a.ScorePoses(q, POSES, MD_MIXED, KERNEL, TH)
    scene.a.ScorePoses(scene.queries(N_TILES2), POSES[:2], MD_ALL, KERNEL, TH)
    assert bytes(scene.a.RegistrationQuality(q, MD_MIXED, KERNEL, TH, pose=POSE)) == quality
    assert sage.register_frame(q, scene.a, guess, 1.0, KERNEL, TH).tobytes() == pose.tobytes()


# ---- Relocalize, end to end -------------------------------------------------------------------------------------------------
class Street:
    """the scene of tests/scoreref.py in the product and in the oracle, and the Python composition of the public entries
    that sageicp_relocalize is defined as"""

    def __init__(self, sage, oracle):
        self.sage = sage
        mp = sr.map_points()
        self.a = sage.VoxelHashMap(sr.VOXEL, 100.0)
        self.b = oracle.Map(sr.VOXEL, 100.0, 20, 20)
        self.a.AddPoints(mp)
        self.b.add_points(mp)
        self.rows, self.T = sr.scan(), sr.t_gt()
        self.args = (sr.MD, sr.KERNEL, sr.TH)
        self.cands = sage.relocalize_candidates(sr.PRIOR, **sr.GRID)
        self.scores = self.a.ScorePoses(self.rows, self.cands, *self.args)
        self.rank = sr.ranking(self.scores["score"])

    def composed(self, refine_top):
        sage, best = self.sage, None
        for r in range(min(refine_top, len(self.cands))):
            c = self.rank[r]
            pose, st = sage.register_frame(self.rows, self.a, self.cands[c], *self.args, return_stats=True)
            q = self.a.RegistrationQuality(self.rows, *self.args, pose=pose)
            if best is None or q.sum_w > best[1].sum_w:
                best = (pose, q, dict(best_candidate=int(c), best_candidate_score=float(self.scores["score"][c]),
                                      winner_rank=r, iterations=st.iterations, converged=st.converged))
        return best


@pytest.fixture(scope="module")
def street(gpu_sage, oracle):
    return Street(gpu_sage, oracle)


def test_relocalize_is_the_composition_of_the_public_entries(street):
    s = street
    pose, q, info = s.a.Relocalize(s.rows, sr.PRIOR, *s.args, refine_top=3, **sr.GRID)
    want_pose, want_q, want_info = s.composed(3)
    assert pose.tobytes() == want_pose.tobytes()
    assert bytes(q) == bytes(want_q) and q.valid == 1 and q.covariance_valid == 1
    assert info["candidates"] == len(s.cands) == sr.GRID_CANDIDATES and info["refined"] == 3
    for f, v in want_info.items():
        assert info[f] == v, f
    assert info["us_score"] > 0 and info["us_refine"] > 0 and info["us_wall"] >= info["us_score"]
    print("Relocalize: score %.0f us, refine %.0f us; winner rank %d, candidate %d" %
          (info["us_score"], info["us_refine"], info["winner_rank"], info["best_candidate"]))
    # the device-frame entry agrees with the host entry
    pose_d, q_d, info_d = s.a.Relocalize(_dev(s.rows), sr.PRIOR, *s.args, refine_top=3, **sr.GRID)
    assert pose_d.tobytes() == pose.tobytes() and bytes(q_d) == bytes(q)
    for f in ("candidates", "best_candidate", "best_candidate_score", "refined", "winner_rank", "iterations", "converged"):
        assert info_d[f] == info[f], f


def test_relocalize_against_the_oracle(street):
    s = street
    # the ranking: the oracle's scores put the same three candidates first (their margins: test_score_poses_host.py)
    ref_scores, ref_pairs = sr.score(s.b, s.rows, s.cands, *s.args)
    ref_rank = sr.ranking(ref_scores)
    assert list(s.rank[:3]) == list(ref_rank[:3])
    assert np.array_equal(s.scores["n_pairs"], ref_pairs)
    # scoreref's winner: the oracle's registration from each of the three, the largest sum_w at its result
    ref_poses = [s.b.register_frame(s.rows, s.cands[c], *s.args)[0] for c in ref_rank[:3]]
    ref_refined = [sr.score(s.b, s.rows, [p], *s.args)[0][0] for p in ref_poses]
    ref_winner = int(np.argmax(ref_refined))
    pose, q, info = s.a.Relocalize(s.rows, sr.PRIOR, *s.args, refine_top=3, **sr.GRID)
    assert info["best_candidate"] == ref_rank[ref_winner] and info["winner_rank"] == ref_winner
    # the suite's parity bar against the oracle's registration from that candidate
    d = sr.pose_error(pose, ref_poses[ref_winner])
    print("against the oracle from candidate %d: %.3g m / %.3g rad" % (info["best_candidate"], d[0], d[1]))
    assert d[0] <= 1e-7 and d[1] <= 1e-7
    lost = s.sage.register_frame(s.rows, s.a, sr.PRIOR, *s.args)
    d_lost, d_found = sr.pose_error(lost, s.T), sr.pose_error(pose, s.T)
    print("from the prior %.3f m from T_gt, relocalised %.4f m" % (d_lost[0], d_found[0]))
    assert d_lost[0] - d_found[0] > 1.0


def test_relocalize_without_refinement_returns_the_best_candidate(street):
    s = street
    pose, q, info = s.a.Relocalize(s.rows, sr.PRIOR, *s.args, refine_top=0, **sr.GRID)
    best = int(s.rank[0])
    assert pose.tobytes() == s.cands[best].tobytes()
    assert bytes(q) == bytes(s.a.RegistrationQuality(s.rows, *s.args, pose=s.cands[best]))
    assert info["best_candidate"] == best and info["best_candidate_score"] == s.scores["score"][best] == q.sum_w
    assert info["refined"] == 0 and info["winner_rank"] == 0 and info["iterations"] == 0 and info["converged"] == 0
