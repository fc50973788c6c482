"""One Gauss-Newton step of the ROBUST pose-graph optimiser's host path (sageicp_graph_optimize_robust, where = 1; DESIGN.md
D20: pg_robustify in HostSolver::linearize, pg_rho in cost_at) held to the np.longdouble step of tests/posegraphref.py on
tests/robustref.py's RobustGraph: the re-weighted H and g of one iteration, vertex by vertex, not only where a run ends.
The cases (graphsteps.ROBUST: the dense shapes with closures under Huber, Cauchy and Geman-McClure at the library's scale
and at a scale between the closures' terms), the checks and every bound are tests/graphsteps.py's, shared with
tests/test_posegraph_robust_step_gpu.py.  No GPU."""
import pytest

import graphscenes as gs
import graphsteps as st

IDS = [st.robust_id(rc) for rc in st.ROBUST]


def test_the_scenes_decide():
    st.check_the_scenes_decide(robust=True)


def test_the_cases_are_the_dense_ones_with_closures_under_every_kernel():
    with_closures = [c for c in st.DENSE if c[1] > 0]
    assert {(c, k) for c, k, which in st.ROBUST if which == "default"} == {(c, k) for c in with_closures for k in st.KERNELS}
    mid = {c for c, k, which in st.ROBUST if which == "mid"}
    assert mid == {c for c in with_closures if c[0] <= 17} | {(33, 3, 0, "spread")}
    assert {(c, k) for c, k, which in st.ROBUST if which == "mid"} == {(c, k) for c in mid for k in st.KERNELS}
    assert len(set(st.ROBUST)) == len(st.ROBUST) == 3 * (len(with_closures) + len(mid)) and len(set(IDS)) == len(IDS)
    assert st.scale_of(st.DENSE[1], "default") ** 2 == pytest.approx(16.81, rel=1e-15)


def test_the_longdouble_step_solves_its_system():
    """the reference's own residual under the kernels: 1e-19, against the fp64 restatement's 1e-14 ... 1e-12"""
    for case, kernel, which in st.ROBUST:
        m = st.reference(case, kernel=kernel, scale=st.scale_of(case, which))
        assert m["rho"] <= 2.0 ** -60 and m["rho"] < 1e-4 * m["rho_ref"]


@pytest.mark.parametrize("case,kernel,which", st.ROBUST, ids=IDS)
def test_one_step(sage, case, kernel, which):
    st.check_one_step(sage, "host", case, kernel=kernel, scale=st.scale_of(case, which))


@pytest.mark.parametrize("case,kernel,which", st.ROBUST, ids=IDS)
def test_the_starts_numbers(sage, case, kernel, which):
    st.check_the_start(sage, "host", case, kernel=kernel, scale=st.scale_of(case, which))


@pytest.mark.parametrize("case,kernel,which", st.ROBUST_SECOND, ids=[st.robust_id(rc) for rc in st.ROBUST_SECOND])
def test_a_second_step_from_the_first(sage, case, kernel, which):
    st.check_a_second_step(sage, "host", case, kernel=kernel, scale=st.scale_of(case, which))


@pytest.mark.parametrize("case,kernel,which", st.ROBUST_BEYOND, ids=[st.robust_id(rc) for rc in st.ROBUST_BEYOND])
def test_one_step_beyond_the_dense_restatement(sage, case, kernel, which):
    st.check_beyond(sage, ("host",), st.scene_of(case), case[2], st.allowance(robust=True), kernel=kernel, scale=st.scale_of(case, which))


@pytest.mark.parametrize("case", st.SECOND + ["two_laps"], ids=[st.case_id(c) for c in st.SECOND] + ["two_laps"])
def test_huber_beyond_every_term_is_the_plain_entry(sage, case):
    """one iteration from the stepped start on the cases of SECOND; a full run on graphscenes' two laps"""
    if case == "two_laps":
        return st.check_huber_beyond_every_term(sage, "host", gs.scene(case))
    s = st.scene_of(case)
    st.check_huber_beyond_every_term(sage, "host", s, initial=s["initial"], anchor=case[2], max_iterations=1, max_halvings=st.MAX_HALVINGS)
