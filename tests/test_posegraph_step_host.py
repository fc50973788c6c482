"""One Gauss-Newton step of the pose-graph optimiser's host path (where = 1: block Thomas plus Woodbury; capi_posegraph.hip,
posegraph.h) held to the np.longdouble step of tests/posegraphref.py.  The cases, the checks and their bounds are
tests/graphsteps.py's, shared with tests/test_posegraph_step_gpu.py.  No GPU."""
import numpy as np
import pytest

import graphsteps as st

IDS = [st.case_id(c) for c in st.DENSE]


def test_the_scenes_decide():
    st.check_the_scenes_decide()


def test_the_shapes_cover_every_anchor_and_closure_count():
    pairs = {(kind, c) for i, (n, c, a, how) in enumerate(st.DENSE[:len(st.M_SIZES)]) for kind in st.ANCHORS if st._anchor(kind, n) == a}
    assert {(k, c) for k in st.ANCHORS for c in st.COUNTS} <= pairs
    assert sorted(n - 1 for n, _, _, _ in st.DENSE[:len(st.M_SIZES)]) == st.M_SIZES


def test_the_longdouble_step_solves_its_system():
    """the reference's own residual: 1e-19, against the fp64 restatement's 1e-14 ... 1e-12"""
    for case in st.DENSE:
        m = st.reference(case)
        assert m["rho"] <= 2.0 ** -60 and m["rho"] < 1e-4 * m["rho_ref"]


@pytest.mark.parametrize("case", st.DENSE, ids=IDS)
def test_one_step(sage, case):
    st.check_one_step(sage, "host", case)


@pytest.mark.parametrize("case", st.DENSE, ids=IDS)
def test_the_starts_numbers(sage, case):
    st.check_the_start(sage, "host", case)


@pytest.mark.parametrize("case", st.SECOND, ids=[st.case_id(c) for c in st.SECOND])
def test_a_second_step_from_the_first(sage, case):
    out = st.check_one_step(sage, "host", case)
    st.check_one_step(sage, "host", case, x0=out, tag="second-host")


@pytest.mark.parametrize("case", st.BEYOND, ids=[st.case_id(c) for c in st.BEYOND])
def test_one_step_beyond_the_dense_restatement(sage, case):
    st.check_beyond(sage, ("host",), st.scene_of(case), case[2], st.allowance())


def test_one_step_of_the_large_chain(sage):
    n = st.LARGE_N
    near = lambda k: np.arange(max(0, k - 2), min(n, k + 3))
    sample = np.unique(np.concatenate([np.arange(0, n, 37)] + [near(k) for k in (0, 5, 112200, 131000, 262143, 262144, 262145)]))
    st.check_beyond(sage, ("host",), st.large_scene(), 0, st.allowance(), sample, name="large")
