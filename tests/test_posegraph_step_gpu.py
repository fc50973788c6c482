"""One Gauss-Newton step of the pose-graph optimiser's device path (where = 2: block cyclic reduction k_pg_inv / k_pg_red /
k_pg_fwd / k_pg_bwd, the low-rank part k_pg_rhs_cols / k_pg_cap / k_pg_rhs_final, the refinement k_pg_resid;
csrc/posegraph.hip) held to the np.longdouble step of tests/posegraphref.py.  The cases, the checks and their bounds are
tests/graphsteps.py's, shared with tests/test_posegraph_step_host.py.

The shapes: every free size m = 1 ... 9 and 15 ... 17, 31 ... 33, 63 ... 65, 127 ... 129 (level sizes halve with floor: an
odd and an even size at every depth), anchors at 0, 1, n // 2, n - 2 and n - 1 against 0, 1, 2 and 7 closures at the anchor,
at the last pose, on adjacent poses, twice on a pair and reversed; 43 closures (1 + 6 * 43 = 259 columns, one beyond a
workgroup's 256 lanes in the idx / K, idx % K split); kPgMaxClosures = 256; a second step from the first one's output (the
scratch of the first is then stale); 1 000 and 4 097 poses (m = 4 096: even down to 1); and 262 146 poses, where every
first-level kernel has exactly one item for its second stride."""
import numpy as np
import pytest

import graphscenes as gs
import graphsteps as st

pytestmark = pytest.mark.gpu
IDS = [st.case_id(c) for c in st.DENSE]


@pytest.mark.parametrize("case", st.DENSE, ids=IDS)
def test_one_step(gpu_sage, case):
    st.check_one_step(gpu_sage, "device", case)


@pytest.mark.parametrize("case", st.DENSE, ids=IDS)
def test_the_starts_numbers(gpu_sage, case):
    st.check_the_start(gpu_sage, "device", case)


@pytest.mark.parametrize("case", st.SECOND, ids=[st.case_id(c) for c in st.SECOND])
def test_a_second_step_from_the_first(gpu_sage, case):
    """two iterations in one call reuse d_X, Gm and the level buffers of the first: their output is one step (held here to
    the reference computed at that point) from the output of a call of one iteration"""
    s, anchor = st.scene_of(case), case[2]
    first = st.check_one_step(gpu_sage, "device", case)
    second = st.check_one_step(gpu_sage, "device", case, x0=first, tag="second-device")
    corr, both, info = st.run(gpu_sage, s, anchor, "device", iterations=2)
    assert info["iterations"] == 2 and gs.bits(both) == gs.bits(second)


@pytest.mark.parametrize("case", st.BEYOND, ids=[st.case_id(c) for c in st.BEYOND])
def test_one_step_beyond_the_dense_restatement(gpu_sage, case):
    st.check_beyond(gpu_sage, ("host", "device"), st.scene_of(case), case[2], st.allowance())


def test_one_step_of_the_large_chain(gpu_sage):
    n = st.LARGE_N
    near = lambda k: np.arange(max(0, k - 2), min(n, k + 3))
    sample = np.unique(np.concatenate([np.arange(0, n, 37)] + [near(k) for k in (0, 5, 112200, 131000, 262143, 262144, 262145)]))
    st.check_beyond(gpu_sage, ("host", "device"), st.large_scene(), 0, st.allowance(), sample, name="large")


@pytest.mark.parametrize("case", [c for c in st.DENSE if c[1] == 256], ids=lambda c: st.case_id(c))
def test_the_same_bytes_on_two_runs(gpu_sage, case):
    s = st.scene_of(case)
    a, b = st.run(gpu_sage, s, case[2], "device"), st.run(gpu_sage, s, case[2], "device")
    assert gs.bits(a[0]) == gs.bits(b[0]) and gs.bits(a[1]) == gs.bits(b[1]) and a[2] == b[2]
