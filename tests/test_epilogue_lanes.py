"""The Gauss-Newton epilogue spreads the 16 pair terms of a query over its lanes (kernels.hip, icp_body and
wave_terms_to_wgacc): lane ci of a query computes components ci K .. ci K + K - 1, K = 16 / lanes per query.
The block sums keep their association, so the headline frame (c2) and c1, at full size, must register to ONE
pose, to the bit, at every lane width of both loops — the width of 1 still computes all 16 terms on one lane —
and that pose must match the oracle.

Needs a real MI355X:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("name", ["c2", "c1"])
def test_full_frames_are_bit_identical_at_every_lane_width(gpu_sage, oracle, name):
    from sage_icp_amd import synthetic as syn
    w = syn.make_workload(name, lambda: gpu_sage.VoxelHashMap(syn.WORKLOADS[name]["voxel"], 100.0))
    p = syn.PARAMS["cold"]
    runs = []
    for loop in (0, 2):
        for lw in range(0 if loop == 0 else 1, 5):
            with Env(SAGEICP_LOOP=loop, SAGEICP_LW=lw):
                pose, st = gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"],
                                                   p["sem_th"], return_stats=True)
            assert st.lanes_per_query == 1 << lw
            assert loop or st.single_launch == 0
            runs.append((loop, lw, pose, st))
    assert any(loop and st.single_launch for loop, _, _, st in runs), "no width ran the one-launch loop"
    _, _, pose0, st0 = runs[0]
    for loop, lw, pose, st in runs[1:]:
        assert np.array_equal(pose, pose0), (loop, lw)
        assert st.iterations == st0.iterations and st.converged == st0.converged
        assert list(st.n_corr_hist) == list(st0.n_corr_hist)
        assert st.last_step_norm == st0.last_step_norm

    om = oracle.Map(w["voxel"], 100.0)
    om.add_points(w["stream"])
    opose, ost = om.register_frame(w["scan"], oracle.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"])
    e = oracle.se3_log(oracle.se3_mul(oracle.se3_inv(opose), pose0))
    assert np.linalg.norm(e[:3]) < 1e-7 and np.linalg.norm(e[3:]) < 1e-7
    assert st0.iterations == ost.iterations and st0.converged == ost.converged
    assert st0.n_corr_first == ost.n_corr_first and st0.n_corr_last == ost.n_corr_last
