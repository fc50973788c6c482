"""The streams and events a map and a pipeline create lazily (csrc/dev_buffer.h: OwnedStream, OwnedEvent) are all alive
when the handles are destroyed, eight times over in one process: every round computes what the first did, to the bit,
and handles that were never used go without a call."""
import numpy as np
import pytest
import torch

import dynscenes

DEV = "cuda:0"
ROUNDS = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _stats(st):
    return (st.iterations, st.n_corr_first, st.n_corr_last, list(st.n_corr_hist))


def _inputs():
    rng = np.random.default_rng(17)
    # a floor and two walls, 400 points; the scan: 256 of them seen from 0.2 m and 1 degree away
    n = 400
    u, v = rng.uniform(8.0, 20.0, n), rng.uniform(-6.0, 6.0, n)
    which = np.arange(n) % 3
    xyz = np.where((which == 0)[:, None], np.column_stack([u, v, np.full(n, -1.5)]),
                   np.where((which == 1)[:, None], np.column_stack([u, np.full(n, 6.0), 0.25 * v]),
                            np.column_stack([np.full(n, 20.0), v, 0.25 * (u - 14.0)])))
    world = np.ascontiguousarray(np.column_stack([xyz, np.full(n, 40.0)]))
    a = np.deg2rad(1.0)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    scan = world[rng.permutation(n)[:256]].copy()
    scan[:, :3] = (scan[:, :3] - np.array([0.2, -0.1, 0.0])) @ R
    # cars in two rows, landmarks under some of them, a road: the vehicle filter finds clusters and keeps a few
    scene, _ = dynscenes.bumper_rows(13, n_cars=(6, 4))
    frames = []
    for k in range(4):
        f = scene.copy()
        f[:, 0] -= 0.15 * k
        frames.append(np.ascontiguousarray(f))
    return np.ascontiguousarray(world), np.ascontiguousarray(scan), frames


def _round(sage, world, scan, frames):
    """one map and one pipeline, used so that every stream and event they can hold exists, then destroyed; returns
    what they computed"""
    out = []
    m = sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints(world)
    for level in (2, 0):           # 2: an event around every kernel of every iteration; 0: the one-launch loop
        sage.set_profiling(level)
        pose, st = sage.register_frame(scan, m, sage.IDENTITY, 3.0, 1.0, 0.05, return_stats=True)
        out.append((_bits(pose), _stats(st)))
    assert st.single_launch == 1   # (the solving wave's stream and event exist)
    rows = m.Pointcloud(device=True)                 # the map's event for the caller's stream
    assert rows.shape == (m.size(), 4)
    out.append(_bits(rows.cpu().numpy()))
    sage.set_profiling(1)
    p = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
    dev = [torch.from_numpy(f).to(DEV) for f in frames]
    res = [p.RegisterFrame(dev[0])]
    announced = p.prefetch(frames[2])                # prepared in the other set of buffers while frame 1 registers
    res.append(p.RegisterFrame(dev[1]))
    assert p.dynamic_filter_info()["clusters"] >= 1  # (the filter got past its early return)
    res.append(p.RegisterFrame(announced))           # ... which is the current set from here on
    res.append(p.RegisterFrame(dev[3]))
    for pose, _, _, n_source, st in res:
        out.append((_bits(pose), n_source, _stats(st)))
    out.append(_bits(p.poses()))
    p.__del__()
    m.__del__()
    assert p._h is None and m._h is None
    return out


@pytest.mark.gpu
def test_handles_created_and_destroyed_eight_times_compute_the_same(gpu_sage):
    world, scan, frames = _inputs()
    try:
        # (every call of the binding raises unless it returned SAGEICP_OK)
        first = _round(gpu_sage, world, scan, frames)
        for k in range(1, ROUNDS):
            assert _round(gpu_sage, world, scan, frames) == first, "round %d" % k
    finally:
        gpu_sage.set_profiling(0)


@pytest.mark.gpu
def test_handles_never_used_are_destroyed(gpu_sage):
    m = gpu_sage.VoxelHashMap(1.0, 100.0)
    p = gpu_sage.SageICP(gpu_sage.make_pipeline_config(dynamic_vehicle_filter=True))
    p.__del__()
    m.__del__()
    assert p._h is None and m._h is None
    # ... and the library goes on working
    world, scan, _ = _inputs()
    m = gpu_sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints(world)
    assert m.size() > 0
    gpu_sage.register_frame(scan, m, gpu_sage.IDENTITY, 3.0, 1.0, 0.05)
