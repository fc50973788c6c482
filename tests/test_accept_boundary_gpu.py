"""Pairs ON the acceptance radius (tests/acceptscenes.py): every site that evaluates (nn - p).norm() < max_dist — the fused
epilogue of the search (csrc/icp_body.h: k_icp, the chained launches, k_loop, at every lane width and in both scan forms),
k_corr_flag (csrc/correspond.hip: GetCorrespondences on device frames, the quality report, ScorePoses) and the host entry's
own sqrt form (csrc/capi_query.hip) — against the oracle, which follows the same build switch.  Every comparison is for equality.

Rows lie within 4 ulps of T = accept_threshold(max_dist) on either side, many exactly on it and on its successor, and
hundreds of them change sides with the association of the three squares: a threshold one ulp off, `<` for `<=`, the other
association or a contracted multiply-add moves a count here.  The host entry searches on the device too, so it is tested
here and not on the CPU.  tests/test_sqnorm3_variant.py runs this file on the other build as well.

Needs a real MI355X:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest
import torch

import acceptscenes as acs
import qualityref as qr

pytestmark = pytest.mark.gpu

KERNEL = 0.5
CASES = [(name, n) for name in acs.CONFIGS for n in acs.SIZES[name]]
IDS = ["%s-%d" % c for c in CASES]
# the scenes are built here, at collection, on the CPU: each asserts its own preconditions as it is built (exact hits of T
# and of its successor, both sides populated, at least 20 deciders, irregular order; under a second for all of them)
for _name in acs.CONFIGS:
    acs.scene(_name)
acs.scene("v1.0_d0.7", acs.POSE)
COUNT_KEYS = ("n_queries", "n_pairs", "pairs_same_label", "pairs_unlabelled", "pairs_cross_label", "other_queries",
              "other_pairs")


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


class World:
    """one scene as the product and the oracle hold it, and the oracle's answer per frame size, computed once"""

    def __init__(self, sage, oracle, name, pose=None):
        self.sage, self.sc = sage, acs.scene(name, pose)
        self.a = sage.VoxelHashMap(self.sc.voxel, 100.0)
        self.b = oracle.Map(self.sc.voxel, 100.0, 20, 20)
        self.a.AddPoints(self.sc.map)
        self.b.add_points(self.sc.map)
        self.a.sync()
        self.md, self.th = self.sc.max_dist, self.sc.sem_th
        self._truth = {}

    def truth(self, n):
        """(src, tgt, idx) of the oracle for the first n rows (moved by the scene's pose, if it has one) — first held to
        what the scene's own arithmetic says, so that the rows are known to sit where they were put"""
        if n not in self._truth:
            got = self.b.get_correspondences(self.sc.moved[:n], self.md, self.th, with_index=True)
            for g, w in zip(got, self.sc.expect(n)):
                assert np.array_equal(g, w)
            self._truth[n] = got
        return self._truth[n]


@pytest.fixture(scope="module")
def worlds(gpu_sage, oracle):
    made = {}

    def get(name, pose=None):
        key = (name, pose is not None)
        if key not in made:
            made[key] = World(gpu_sage, oracle, name, pose)
        return made[key]
    return get


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    src, tgt, idx = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    assert np.array_equal(idx, want[2]), (len(idx), len(want[2]))
    assert np.array_equal(src, want[0]) and np.array_equal(tgt, want[1])


def _check_counts(got, q_labels, src, tgt):
    want = qr.counts(q_labels, src, tgt)
    d = got.as_dict()
    assert got.valid == 1
    for k in COUNT_KEYS:
        assert d[k] == want[k], (k, d[k], want[k])
    assert np.array_equal(d["class_queries"], want["class_queries"])
    assert np.array_equal(d["class_pairs"], want["class_pairs"])


# ---- GetCorrespondences ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_accept_boundary_host_rows(worlds, name, n):
    """sageicp_get_correspondences: the search on the device, the acceptance on the host in its sqrt form"""
    w = worlds(name)
    _same(w.a.GetCorrespondences(w.sc.frame(n), w.md, w.th, with_index=True), w.truth(n))


@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_accept_boundary_device_frames(worlds, scan_form, name, n):
    """sageicp_get_correspondences_device (k_corr_flag) at 1, 2, 4, 8 and 16 lanes per query"""
    w = worlds(name)
    q = _dev(w.sc.frame(n))
    for lw in range(5):
        with Env(SAGEICP_LW=lw):
            _same(w.a.GetCorrespondences(q, w.md, w.th, with_index=True), w.truth(n))


# ---- the quality report and the batch score --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_accept_boundary_quality_counts(worlds, name, n):
    w = worlds(name)
    src, tgt, idx = w.truth(n)
    frame = w.sc.frame(n)
    for rows in (frame, _dev(frame)):
        got = w.a.RegistrationQuality(rows, w.md, KERNEL, w.th)
        assert got.n_pairs == len(idx)
        _check_counts(got, frame[:, 3], src, tgt)


@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_accept_boundary_score_poses_at_the_identity(worlds, gpu_sage, name, n):
    w = worlds(name)
    src, tgt, idx = w.truth(n)
    want = qr.counts(w.sc.frame(n)[:, 3], src, tgt)
    frame = w.sc.frame(n)
    for rows in (frame, _dev(frame)):
        got = w.a.ScorePoses(rows, np.stack([gpu_sage.IDENTITY, gpu_sage.IDENTITY]), w.md, KERNEL, w.th)
        for c in range(2):
            assert int(got["n_pairs"][c]) == len(idx)
            for k in ("n_queries", "pairs_same_label", "pairs_unlabelled", "pairs_cross_label"):
                assert int(got[k][c]) == want[k], k


@pytest.mark.parametrize("n", acs.POSED_SIZES)
def test_accept_boundary_at_a_pose(worlds, gpu_sage, oracle, n):
    """the rows built so that the rows MOVED by the pose sit on the boundary: the truth is the oracle over
    transform_points' output; ScorePoses, the quality report and GetCorrespondences with pose= move the rows themselves"""
    w = worlds("v1.0_d0.7", acs.POSE)
    frame = w.sc.frame(n)
    moved = gpu_sage.transform_points(acs.POSE, frame)
    assert np.array_equal(moved, w.sc.moved[:n])            # the boundary is where the scene put it
    src, tgt, idx = w.b.get_correspondences(moved, w.md, w.th, with_index=True)
    _same((src, tgt, idx), w.truth(n))
    assert 0.4 * n < len(idx) < 0.6 * n
    # the raw rows at the identity are nowhere near the boundary's count: the pose is not ignored
    poses = np.stack([gpu_sage.IDENTITY, acs.POSE])
    for rows in (frame, _dev(frame)):
        got = w.a.ScorePoses(rows, poses, w.md, KERNEL, w.th)
        assert int(got["n_pairs"][1]) == len(idx)
        assert int(got["n_pairs"][0]) != len(idx)
        q = w.a.RegistrationQuality(rows, w.md, KERNEL, w.th, pose=acs.POSE)
        assert q.n_pairs == len(idx)
        _check_counts(q, frame[:, 3], src, tgt)
    _same(w.a.GetCorrespondences(_dev(frame), w.md, w.th, with_index=True, pose=acs.POSE), (src, tgt, idx))


# ---- RegisterFrame: the fused epilogue in every form ---------------------------------------------------------------------------
FORMS = ([("loop-lw%d" % lw, dict(SAGEICP_LOOP=2, SAGEICP_LW=lw), 1, 0) for lw in (1, 2, 3, 4)] +
         [("chained", dict(SAGEICP_LOOP=0), 0, 1)] +
         [("k_fin-lw%d" % lw, dict(SAGEICP_LOOP=0, SAGEICP_CHAIN=0, SAGEICP_LW=lw), 0, 0) for lw in (0, 1, 2, 3, 4)])


def _register(w, frame, env):
    before = w.a.loop_status().calls_chained
    with Env(**env):
        pose, st = w.sage.register_frame(frame, w.a, w.sage.IDENTITY, w.md, KERNEL, w.th, return_stats=True)
    return pose, st, w.a.loop_status().calls_chained - before


@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_accept_boundary_register_frame(worlds, scan_form, name, n):
    """n_corr_first of the identity guess, in every form of the loop.  So that two errors cannot cancel in one count: the
    frame of exactly the accepted rows reports all of them, the frame of exactly the rejected rows none — and then stops
    after one iteration on the guess itself."""
    w = worlds(name)
    frame = w.sc.frame(n)
    src, tgt, idx = w.truth(n)
    yes = np.zeros(n, dtype=bool)
    yes[idx] = True
    accepted, rejected = np.ascontiguousarray(frame[yes]), np.ascontiguousarray(frame[~yes])
    for form, env, single, chained in FORMS:
        # (the first count does not depend on how long the loop then runs)
        pose, st, ch = _register(w, frame, dict(env, SAGEICP_MAX_ITER=1))
        assert (st.single_launch, ch) == (single, chained), form
        assert st.n_corr_first == len(idx) and st.n_corr_hist[0] == len(idx), (form, st.n_corr_first, len(idx))
        if "SAGEICP_LW" in env:
            assert st.lanes_per_query == 1 << env["SAGEICP_LW"]
        assert st.compact_scan == (1 if scan_form == "compact" else 0)
        if len(accepted):
            pose, st, ch = _register(w, accepted, dict(env, SAGEICP_MAX_ITER=1))
            assert st.n_corr_first == len(accepted), (form, st.n_corr_first, len(accepted))
        if len(rejected):
            pose, st, ch = _register(w, rejected, env)
            assert (st.n_corr_first, st.n_corr_last, st.iterations, st.converged) == (0, 0, 1, 1), form
            assert pose.tobytes() == w.sage.IDENTITY.tobytes(), (form, pose)
