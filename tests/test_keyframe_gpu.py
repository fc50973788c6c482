"""Key-frame selection by occupancy overlap on the device (csrc/keyframe.hip): the stand-alone grid entries bit for bit
against the restatement tests/keyframe_ref.py (random frames, the truncation quirk, cell edges and bounds, H != W, the
global-atomic path of large grids, empty / single / million-point frames, a pose, device frames), and the pipeline's
selection frame by frame against a host replay of the node's logic over the pipeline's own poses and the raw frames —
through host rows, device tensors, prefetch, the dynamic filter and deskew — with the poses unchanged, reinitialize /
reset, an empty first key grid, and the refusals."""
import math
import os

import numpy as np
import pytest
import torch

import keyframe_ref as kr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCH = ((-51.2, 51.2), (-51.2, 51.2), (-4.0, 2.4))
NEAR = ((-20.0, 20.0), (-20.0, 20.0), (-4.0, 2.4))
NEAR_OCC = (64, 64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _cloud(rng, n, spread=70.0, zs=(-6.0, 4.0)):
    f = np.empty((n, 4))
    f[:, 0] = rng.uniform(-spread, spread, n)
    f[:, 1] = rng.uniform(-spread, spread, n)
    f[:, 2] = rng.uniform(zs[0], zs[1], n)
    f[:, 3] = rng.integers(0, 100, n)
    return f


# ---- the stand-alone entries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_frames_match_the_restatement(gpu_sage, seed):
    f = _cloud(np.random.default_rng(seed), 120000)
    g = gpu_sage.occupancy_grid(f, LAUNCH, (128, 128))
    ref = kr.grid(f, LAUNCH, (128, 128))
    assert 1000 < ref.sum() < 128 * 128
    assert np.array_equal(g, ref)


def test_asymmetric_bounds_hit_the_truncation_quirk(gpu_sage):
    b = ((-60.0, 50.0), (-45.0, 55.5), (-3.0, 2.0))
    rng = np.random.default_rng(7)
    f = _cloud(rng, 50000, spread=70.0)
    # values (x + bx_hi) / x_res in (-1, 0): x in (-60, -50) with x_res = 110 / 100 = 1.1 -> truncated to column 0
    band = _cloud(rng, 200)
    band[:, 0] = rng.uniform(-51.09, -50.01, 200)
    band[:, 2] = 0.0
    f = np.concatenate([f, band])
    g = gpu_sage.occupancy_grid(f, b, (97, 100))
    ref = kr.grid(f, b, (97, 100))
    assert np.array_equal(g, ref)
    vx = (band[:, 0] + 50.0) / (110.0 / 100)
    assert np.all((vx > -1) & (vx < 0)) and ref[:, 0].sum() > 0


@pytest.mark.parametrize("occ", [(100, 37), (37, 100), (128, 128), (1, 1)])
def test_cell_edges_and_bounds(gpu_sage, occ):
    H, W = occ
    b = ((-30.0, 25.0), (-12.5, 40.0), (-2.0, 3.0))
    xr, yr = (b[0][1] - b[0][0]) / W, (b[1][1] - b[1][0]) / H
    xs = np.concatenate([b[0][0] + xr * np.arange(W + 1), -b[0][1] + xr * np.arange(-1, W + 2),
                         [b[0][0], b[0][1], np.nextafter(b[0][0], -1e9), np.nextafter(b[0][1], 1e9)]])
    ys = np.concatenate([b[1][0] + yr * np.arange(H + 1), -b[1][1] + yr * np.arange(-1, H + 2),
                         [b[1][0], b[1][1], np.nextafter(b[1][0], -1e9), np.nextafter(b[1][1], 1e9)]])
    X, Y = np.meshgrid(xs, ys)
    f = np.zeros((X.size * 3, 4))
    f[:, 0] = np.tile(X.ravel(), 3)
    f[:, 1] = np.tile(Y.ravel(), 3)
    f[:, 2] = np.repeat([b[2][0], b[2][1], np.nextafter(b[2][1], 1e9)], X.size)
    g = gpu_sage.occupancy_grid(f, b, occ)
    assert g.shape == occ
    assert np.array_equal(g, kr.grid(f, b, occ))


def test_large_grid_takes_the_global_path_and_both_paths_agree(gpu_sage, monkeypatch):
    f = _cloud(np.random.default_rng(11), 300000, spread=55.0)
    g = gpu_sage.occupancy_grid(f, LAUNCH, (2048, 1024))
    assert np.array_equal(g, kr.grid(f, LAUNCH, (2048, 1024)))
    lds = gpu_sage.occupancy_grid(f, LAUNCH, (128, 128))
    monkeypatch.setenv("SAGEICP_OCC_GLOBAL", "1")
    glob = gpu_sage.occupancy_grid(f, LAUNCH, (128, 128))
    assert np.array_equal(lds, glob) and np.array_equal(lds, kr.grid(f, LAUNCH, (128, 128)))


@pytest.mark.parametrize("n", [0, 1, 1 << 20])
def test_frame_sizes(gpu_sage, n):
    f = _cloud(np.random.default_rng(n + 5), n)
    g = gpu_sage.occupancy_grid(f, LAUNCH, (128, 128))
    assert np.array_equal(g, kr.grid(f, LAUNCH, (128, 128)))
    if n == 1:
        f = np.array([[1.0, 2.0, 0.0, 3.0]])
        g = gpu_sage.occupancy_grid(f, LAUNCH, (128, 128))
        assert g.sum() == 1 and np.array_equal(g, kr.grid(f, LAUNCH, (128, 128)))


def test_with_a_pose_the_grid_is_that_of_the_transformed_frame(gpu_sage):
    rng = np.random.default_rng(13)
    f = _cloud(rng, 80000)
    q = rng.normal(size=4)
    pose = np.concatenate([q / np.linalg.norm(q), rng.uniform(-5, 5, 3)])
    moved = gpu_sage.transform_points(pose, f)
    assert np.array_equal(_bits(moved), _bits(kr.transform(pose, f)))     # the restatement is k_tf's arithmetic
    g = gpu_sage.occupancy_grid(f, LAUNCH, (128, 128), pose=pose)
    assert np.array_equal(g, kr.grid(moved, LAUNCH, (128, 128)))
    assert not np.array_equal(g, kr.grid(f, LAUNCH, (128, 128)))


def test_device_frames_give_the_grid_of_the_same_converted_values(gpu_sage):
    rng = np.random.default_rng(17)
    f = _cloud(rng, 60000)
    pose = np.array([0.0, 0.0, np.sin(0.2), np.cos(0.2), 1.5, -2.0, 0.1])
    for dt in (torch.float32, torch.float64):
        t = torch.from_numpy(f).to(DEV).to(dt)
        host = t.double().cpu().numpy()
        for p in (None, pose):
            want = gpu_sage.occupancy_grid(host, LAUNCH, (100, 37), pose=p)
            assert np.array_equal(want, kr.grid(host if p is None else kr.transform(p, host), LAUNCH, (100, 37)))
            assert np.array_equal(gpu_sage.occupancy_grid(t, LAUNCH, (100, 37), pose=p), want)
        wide = torch.zeros((len(f), 6), dtype=dt, device=DEV)          # strided rows, labels apart
        wide[:, :3] = t[:, :3]
        lab = torch.from_numpy(f[:, 3].astype(np.int32)).to(DEV)
        assert np.array_equal(gpu_sage.occupancy_grid(wide, LAUNCH, (100, 37), pose=pose, labels=lab),
                              gpu_sage.occupancy_grid(host, LAUNCH, (100, 37), pose=pose))
    torch.cuda.synchronize()


def test_standalone_refuses_non_finite_coordinates(gpu_sage):
    f = _cloud(np.random.default_rng(19), 1000)
    f[500, 1] = np.nan
    for frame in (f, torch.from_numpy(f).to(DEV)):
        with pytest.raises(gpu_sage.SageIcpError) as e:
            gpu_sage.occupancy_grid(frame, LAUNCH, (128, 128))
        assert e.value.code == gpu_sage.ERR_INVALID
    g = f.copy()
    g[500, 1] = 0.0
    with pytest.raises(gpu_sage.SageIcpError):
        gpu_sage.occupancy_grid(g, LAUNCH, (128, 128), pose=[0, 0, 0, 1, np.inf, 0, 0])


# ---- the pipeline ----------------------------------------------------------------------------------------------------
def _street(n_frames=14, n=20000):
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(41, n_frames, points_per_frame=n, step=(1.5, 0.0, 0.0), yaw_step_deg=3.0)
    return [np.ascontiguousarray(f, dtype=np.float64) for f in frames]


def _replay(frames, poses, bounds, occ, th):
    r = kr.Replay(bounds, occ, th)
    return [r.step(f, p, i) for i, (f, p) in enumerate(zip(frames, poses))]


def _threshold(frames, poses, bounds=NEAR, occ=NEAR_OCC):
    """the first threshold (of a fixed list) under which the replay takes at least 3 key frames after the first and
    rejects at least 3 frames: both branches run"""
    for th in np.round(np.arange(0.02, 1.0, 0.01), 2):
        s = _replay(frames, poses, bounds, occ, th)
        takes = sum(x["is_key_frame"] for x in s[1:])
        if takes >= 3 and len(s) - 1 - takes >= 3:
            return float(th)
    raise AssertionError("no threshold gives both branches on this stream")


def _check(step, info, grid, k):
    assert info["enabled"]
    assert info["is_key_frame"] == step["is_key_frame"], k
    if math.isnan(step["overlap"]):
        assert math.isnan(info["overlap"]), k
    else:
        assert _bits([info["overlap"]])[0] == _bits([step["overlap"]])[0], k
    assert np.array_equal(_bits(info["key_pose"]), _bits(step["key_pose"])), k
    assert info["key_frame_index"] == step["key_frame_index"] and info["key_frames"] == step["key_frames"], k
    assert (info["key_occupied"], info["intersect"]) == (step["key_occupied"], step["intersect"]), k
    assert np.array_equal(grid, step["key_grid"]), k


def _run(sage, frames, mode, th, cfg=None, timestamps=None, select=True):
    p = sage.SageICP(cfg if cfg is not None else sage.make_pipeline_config())
    if select:
        p.set_key_frames(True, NEAR, NEAR_OCC, th)
    infos, grids, sources = [], [], []
    nxt = None
    for k, f in enumerate(frames):
        if mode == "prefetch":
            cur = nxt if nxt is not None else f
            nxt = p.prefetch(frames[k + 1]) if k + 1 < len(frames) else None
            p.RegisterFrame(cur)
        elif mode == "device":
            p.RegisterFrame(torch.from_numpy(f).to(DEV))
        elif mode == "timestamps":
            p.RegisterFrame(f, timestamps[k])
        else:
            p.RegisterFrame(f)
        sources.append(p.source())
        if select:
            infos.append(p.key_frame_info())
            grids.append(p.key_frame_grid())
    return p, infos, grids, sources


@pytest.fixture(scope="module")
def street(gpu_sage):
    frames = _street()
    off, _, _, src_off = _run(gpu_sage, frames, "host", 0.0, select=False)
    poses = off.poses()
    return frames, poses, src_off, _threshold(frames, poses)


@pytest.mark.parametrize("mode", ["host", "device", "prefetch"])
def test_pipeline_selection_matches_the_replay(gpu_sage, street, mode):
    frames, poses_off, src_off, th = street
    p, infos, grids, sources = _run(gpu_sage, frames, mode, th)
    poses = p.poses()
    # selection changes nothing of the registration
    assert np.array_equal(_bits(poses), _bits(poses_off))
    for a, b in zip(sources, src_off):
        assert np.array_equal(_bits(a), _bits(b))
    steps = _replay(frames, poses, NEAR, NEAR_OCC, th)
    for k, (s, i, g) in enumerate(zip(steps, infos, grids)):
        _check(s, i, g, k)
    assert sum(i["is_key_frame"] for i in infos[1:]) >= 3 and sum(not i["is_key_frame"] for i in infos[1:]) >= 3
    dev = p.key_frame_grid(device=True)
    assert dev.device.type == "cuda" and np.array_equal(dev.cpu().numpy(), grids[-1])


def test_pipeline_selection_under_the_dynamic_filter(gpu_sage, street):
    frames = street[0]                                  # (cars among the labels: the filter removes points)
    cfg = gpu_sage.make_pipeline_config(dynamic_vehicle_filter=True)
    off, _, _, _ = _run(gpu_sage, frames, "host", 0.0, cfg=cfg, select=False)
    th = _threshold(frames, off.poses())
    cfg = gpu_sage.make_pipeline_config(dynamic_vehicle_filter=True)
    p, infos, grids, _ = _run(gpu_sage, frames, "host", th, cfg=cfg)
    assert p.dynamic_filter_info()["vehicle_points"] > 0
    assert np.array_equal(_bits(p.poses()), _bits(off.poses()))
    for k, (s, i, g) in enumerate(zip(_replay(frames, p.poses(), NEAR, NEAR_OCC, th), infos, grids)):
        _check(s, i, g, k)


def test_pipeline_selection_reads_the_raw_frame_under_deskew(gpu_sage):
    from sage_icp_amd import synthetic_skew as sk
    S = sk.make_skewed_stream(seed=0x6B, n_frames=12, az_steps=512)
    frames, stamps = S["frames"], S["timestamps"]
    cfg = gpu_sage.make_pipeline_config(deskew=True)
    off, _, _, _ = _run(gpu_sage, frames, "timestamps", 0.0, cfg=cfg, timestamps=stamps, select=False)
    poses = off.poses()
    th = _threshold(frames, poses)
    p, infos, grids, _ = _run(gpu_sage, frames, "timestamps", th, cfg=gpu_sage.make_pipeline_config(deskew=True),
                              timestamps=stamps)
    assert p.deskew_info()[0]
    assert np.array_equal(_bits(p.poses()), _bits(poses))
    for k, (s, i, g) in enumerate(zip(_replay(frames, poses, NEAR, NEAR_OCC, th), infos, grids)):
        _check(s, i, g, k)
    # the test tells the raw rows from the deskewed ones: deskewed, some frame draws another grid
    differs = 0
    for k in range(3, len(frames)):
        d = gpu_sage.deskew_scan(frames[k], stamps[k], poses[k - 2], poses[k - 1])
        differs += not np.array_equal(kr.grid(d, NEAR, NEAR_OCC), kr.grid(frames[k], NEAR, NEAR_OCC))
    assert differs > 0


def test_reinitialize_keeps_the_state_and_reset_clears_it(gpu_sage, street):
    frames, _, _, th = street
    p = gpu_sage.SageICP()
    p.set_key_frames(True, NEAR, NEAR_OCC, th)
    for f in frames[:5]:
        p.RegisterFrame(f)
    info, grid = p.key_frame_info(), p.key_frame_grid()
    assert info["key_frames"] >= 1 and grid.sum() > 0
    p.reinitialize()
    after = p.key_frame_info()
    assert after.keys() == info.keys()
    for k in info:
        a, b = np.atleast_1d(after[k]).astype(np.float64), np.atleast_1d(info[k]).astype(np.float64)
        assert np.array_equal(_bits(a), _bits(b)), k
    assert np.array_equal(p.key_frame_grid(), grid)
    p.key_frame_reset()
    r = p.key_frame_info()
    assert r["key_frames"] == 0 and not r["is_key_frame"] and math.isnan(r["overlap"])
    assert p.key_frame_grid().sum() == 0
    p.RegisterFrame(frames[5])
    r = p.key_frame_info()
    assert r["is_key_frame"] and math.isnan(r["overlap"]) and r["key_frames"] == 1
    assert r["key_frame_index"] == len(p.poses()) - 1
    assert np.array_equal(p.key_frame_grid(), kr.grid(frames[5], NEAR, NEAR_OCC))


def test_an_empty_first_key_grid_never_switches(gpu_sage, street):
    frames = street[0]
    p = gpu_sage.SageICP()
    p.set_key_frames(True, NEAR, NEAR_OCC, 0.99)
    first = frames[0].copy()
    first[:, 2] += 50.0                                 # every point above bz_hi
    p.RegisterFrame(first)
    assert p.key_frame_info()["is_key_frame"] and p.key_frame_grid().sum() == 0
    for f in frames[1:6]:
        p.RegisterFrame(f)
        i = p.key_frame_info()
        assert not i["is_key_frame"] and math.isnan(i["overlap"]) and i["key_occupied"] == 0
        assert i["key_frames"] == 1 and i["key_frame_index"] == 0


@pytest.mark.parametrize("bounds,occ,th", [
    (((-1.0, 1.0), (-1.0, 1.0), (-1.0, float("nan"))), (8, 8), 0.5),
    (((-1.0, 1.0), (3.0, 3.0), (-1.0, 1.0)), (8, 8), 0.5),
    (((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), (4097, 8), 0.5),
    (((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), (8, 8), float("-inf")),
])
def test_refused_configurations_leave_the_selection_as_it_was(gpu_sage, street, bounds, occ, th):
    frames = street[0]
    p = gpu_sage.SageICP()
    p.set_key_frames(True, NEAR, NEAR_OCC, 0.5)
    p.RegisterFrame(frames[0])
    before = p.key_frame_info()
    with pytest.raises(gpu_sage.SageIcpError) as e:
        p.set_key_frames(True, bounds, occ, th)
    assert e.value.code == gpu_sage.ERR_INVALID
    assert p.key_frame_info()["key_frames"] == before["key_frames"] == 1
    assert np.array_equal(p.key_frame_grid(), kr.grid(frames[0], NEAR, NEAR_OCC))


def test_non_finite_frames_are_refused_only_while_selecting(gpu_sage, street):
    frames = street[0]
    bad = frames[2].copy()
    bad[100, 0] = np.nan
    bad[200, 2] = np.inf
    p = gpu_sage.SageICP()
    p.set_key_frames(True, NEAR, NEAR_OCC, 0.5)
    p.RegisterFrame(frames[0])
    p.RegisterFrame(frames[1])
    info, grid = p.key_frame_info(), p.key_frame_grid()
    for frame in (bad, torch.from_numpy(bad).to(DEV)):
        with pytest.raises(gpu_sage.SageIcpError):
            p.RegisterFrame(frame)
        assert len(p.poses()) == 2
        again = p.key_frame_info()
        assert again["key_frames"] == info["key_frames"] and again["is_key_frame"] == info["is_key_frame"]
        assert np.array_equal(_bits([again["overlap"]]), _bits([info["overlap"]]))
        assert np.array_equal(p.key_frame_grid(), grid)
    # off, the same frame registers (the crop drops the points, as the reference's Preprocess does)
    p.set_key_frames(False)
    p.RegisterFrame(bad)
    assert len(p.poses()) == 3
    assert not p.key_frame_info()["enabled"]
    with pytest.raises(gpu_sage.SageIcpError):
        p.key_frame_grid()
