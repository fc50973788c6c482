"""The solving wave of the one-launch loop publishes every pose once per XCD (kernels.h, kLoopPoseCopies); a
workgroup polls the copy of the XCD it is believed to run on.  That belief is a matter of speed only: every copy is
the whole pose.  SAGEICP_LOOP_POSE_MAP moves the workgroups onto other copies — all onto copy 0, or workgroup b onto
copy (b + 3) & 7 — and the poses must stay what they are, to the bit; a launch whose waits time out must still fall
back, whichever copies are in use; so must the chained launches, which read the same block.  (The time-out cases show
that the fall-back still works with the new layout; they cannot show that every copy's done word is written on an
abort: a polling wave also leaves on the abort word, which is the real exit.)

Needs a real MI355X:  python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAPS = (0, 1, 2)          # b & 7 (default) | copy 0 | (b + 3) & 7


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


def _register(gpu_sage, w, p, **env):
    with Env(**env):
        return gpu_sage.register_frame(w["scan"], w["map"], gpu_sage.IDENTITY, p["max_dist"], p["kernel"], p["sem_th"],
                                       return_stats=True)


def _workload(gpu_sage, name, scale=1.0):
    from sage_icp_amd import synthetic as syn
    return syn.make_workload(name, lambda: gpu_sage.VoxelHashMap(syn.WORKLOADS[name]["voxel"], 100.0), scale=scale)


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_any_copy_of_the_pose_is_the_pose(gpu_sage, name):
    from sage_icp_amd import synthetic as syn
    w = _workload(gpu_sage, name)
    p = syn.PARAMS["cold"]
    runs = [_register(gpu_sage, w, p, SAGEICP_LOOP=2, SAGEICP_LOOP_POSE_MAP=m) for m in MAPS]
    ref, sref = _register(gpu_sage, w, p, SAGEICP_LOOP=0, SAGEICP_CHAIN=0)       # k_icp + k_fin: no shared block at all
    assert sref.single_launch == 0
    for pose, st in runs:
        assert st.single_launch == 1, "the frame was expected to fit the one-launch loop"
        assert np.array_equal(pose, runs[0][0]) and np.array_equal(pose, ref)
        assert st.iterations == sref.iterations and st.converged == sref.converged
        assert list(st.n_corr_hist) == list(sref.n_corr_hist)
        assert st.last_step_norm == sref.last_step_norm
    assert w["map"].loop_status().timeouts == 0


@pytest.mark.parametrize("pose_map", MAPS)
def test_timed_out_launch_falls_back_with_every_copy_in_use(gpu_sage, pose_map):
    from sage_icp_amd import synthetic as syn
    w = _workload(gpu_sage, "c2", 0.05)
    p = syn.PARAMS["cold"]
    a, sa = _register(gpu_sage, w, p, SAGEICP_LOOP=2, SAGEICP_LOOP_POSE_MAP=pose_map)
    assert sa.single_launch == 1
    s0 = w["map"].loop_status()
    b, sb = _register(gpu_sage, w, p, SAGEICP_LOOP=2, SAGEICP_LOOP_POSE_MAP=pose_map, SAGEICP_LOOP_TIMEOUT_TICKS=1,
                      SAGEICP_LOOP_COOLDOWN=0)
    assert sb.single_launch == 0 and np.array_equal(a, b)
    s1 = w["map"].loop_status()
    assert (s1.last_fallback, s1.timeouts) == (1, s0.timeouts + 1)
    assert s1.calls_single_launch == s0.calls_single_launch


@pytest.mark.parametrize("pose_map", MAPS)
def test_chained_launches_follow_the_copies(gpu_sage, pose_map):
    """the launches chained beside the solving wave poll the same block: one pose whichever copy, also when every wait
    of theirs gives up at once and the frame is registered again with k_fin"""
    from sage_icp_amd import synthetic as syn
    w = _workload(gpu_sage, "c2", 0.05)
    p = syn.PARAMS["cold"]
    ref, sref = _register(gpu_sage, w, p, SAGEICP_LOOP=0, SAGEICP_CHAIN=0)
    s0 = w["map"].loop_status()
    a, sa = _register(gpu_sage, w, p, SAGEICP_LOOP=0, SAGEICP_LOOP_POSE_MAP=pose_map)
    assert w["map"].loop_status().calls_chained == s0.calls_chained + 1
    b, sb = _register(gpu_sage, w, p, SAGEICP_LOOP=0, SAGEICP_LOOP_POSE_MAP=pose_map, SAGEICP_LOOP_TIMEOUT_TICKS=1)
    assert w["map"].loop_status().calls_chained == s0.calls_chained + 1
    for pose, st in ((a, sa), (b, sb)):
        assert st.single_launch == 0 and np.array_equal(pose, ref)
        assert st.iterations == sref.iterations and list(st.n_corr_hist) == list(sref.n_corr_hist)
