"""One Gauss-Newton step of the ROBUST pose-graph optimiser's device path (sageicp_graph_optimize_robust, where = 2;
k_pg_lin<true> and k_pg_cost<true> of csrc/posegraph.hip with pg_robustify, pg_rho and pg_rho_weight of posegraph.h under
all three kernels, then the plain solve on the scaled blocks) held to the np.longdouble step of
tests/posegraphref.py on tests/robustref.py's RobustGraph.  The cases, the checks and every bound are tests/graphsteps.py's,
shared with tests/test_posegraph_robust_step_host.py.

Huber runs on the device here at both scales, with closures on both of its branches in one step (20 of the cases); Cauchy
and Geman-McClure with weights from 6e-8 to 1.  A second iteration in one call reuses the `lin` buffer the first left
scaled; 1 000 and 4 097 poses lie beyond the dense restatement; 256 closures under Huber give the same bytes twice."""
import numpy as np
import pytest

import graphscenes as gs
import graphsteps as st

pytestmark = pytest.mark.gpu
IDS = [st.robust_id(rc) for rc in st.ROBUST]


@pytest.mark.parametrize("case,kernel,which", st.ROBUST, ids=IDS)
def test_one_step(gpu_sage, case, kernel, which):
    st.check_one_step(gpu_sage, "device", case, kernel=kernel, scale=st.scale_of(case, which))


@pytest.mark.parametrize("case,kernel,which", st.ROBUST, ids=IDS)
def test_the_starts_numbers(gpu_sage, case, kernel, which):
    st.check_the_start(gpu_sage, "device", case, kernel=kernel, scale=st.scale_of(case, which))


@pytest.mark.parametrize("case,kernel,which", st.ROBUST_SECOND, ids=[st.robust_id(rc) for rc in st.ROBUST_SECOND])
def test_a_second_step_from_the_first(gpu_sage, case, kernel, which):
    st.check_a_second_step(gpu_sage, "device", case, kernel=kernel, scale=st.scale_of(case, which))


@pytest.mark.parametrize("case,kernel,which", st.ROBUST_BEYOND, ids=[st.robust_id(rc) for rc in st.ROBUST_BEYOND])
def test_one_step_beyond_the_dense_restatement(gpu_sage, case, kernel, which):
    st.check_beyond(gpu_sage, ("host", "device"), st.scene_of(case), case[2], st.allowance(robust=True), kernel=kernel,
                    scale=st.scale_of(case, which))


@pytest.mark.parametrize("case", st.SECOND + ["two_laps"], ids=[st.case_id(c) for c in st.SECOND] + ["two_laps"])
def test_huber_beyond_every_term_is_the_plain_entry(gpu_sage, case):
    """one iteration from the stepped start on the cases of SECOND; a full run on graphscenes' two laps"""
    if case == "two_laps":
        return st.check_huber_beyond_every_term(gpu_sage, "device", gs.scene(case))
    s = st.scene_of(case)
    st.check_huber_beyond_every_term(gpu_sage, "device", s, initial=s["initial"], anchor=case[2], max_iterations=1, max_halvings=st.MAX_HALVINGS)


def test_the_same_bytes_on_two_runs(gpu_sage):
    case = (66, 256, 33, "spread")
    s = st.scene_of(case)
    a, b = (st.run(gpu_sage, s, case[2], "device", kernel="huber", scale=st.scale_of(case, "default")) for _ in range(2))
    assert gs.bits(a[0]) == gs.bits(b[0]) and gs.bits(a[1]) == gs.bits(b[1])
    assert set(a[2]) == set(b[2]) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    assert a[2]["iterations"] == 1 and a[2]["where"] == 2 and (a[2]["closure_weight"] < 1.0).any()
