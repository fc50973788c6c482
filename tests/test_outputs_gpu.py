"""Outputs in device memory (sageicp_pipeline_source*, sageicp_map_pointcloud_device; csrc/egress.hip and the templated
gathers of map_update.hip): the registered source cloud is the preprocessing chain's output through every entry, the
device rows are the host rows in every layout the egress writes, the local map comes out bit for bit in both map modes
and either residency, the caller's stream is followed, memory that is not device memory is refused, and registration
is unchanged by any of it."""
import ctypes
import os

import numpy as np
import pytest
import torch

DEV = "cuda:0"


@pytest.fixture
def oracle_ref(oracle):
    """the oracle in mode 3: bucket order and the reference's erase-while-iterating sweep (reference-order maps)"""
    oracle.set_robin_order(3)
    yield oracle
    oracle.set_robin_order(False)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _sorted(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a[np.lexsort(a.T[::-1])]


def _stream(n_frames, n=30000, seed=31):
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(seed, n_frames, points_per_frame=n)
    return [np.ascontiguousarray(f, dtype=np.float64) for f in frames]


def _chain(sage, frame, cfg, ds=None, **pre):
    """Preprocess, then VoxelDownsample at 0.5 and 1.5 (pipeline/sageICP.cpp:57-67, 97-101)"""
    ds = ds or sage.voxel_downsample
    labels, sizes = sage.KITTI_VOXEL_LABELS, sage.KITTI_VOXEL_SIZE
    p = sage.preprocess(frame, cfg.max_range, cfg.min_range, cfg.label_max_range, **pre)
    return ds(ds(p, labels, sizes, 0.5), labels, sizes, 1.5)


def _oracle_ds(oracle):
    return lambda f, labels, sizes, scale: oracle.voxel_downsample(f, labels, sizes, scale)


# ---- 1. the source is the preprocessing chain's output ------------------------------------------------------------------
@pytest.mark.gpu
def test_source_is_the_preprocessing_chain(gpu_sage, oracle, reference_emission_order):
    # (each level keeps the first point of a voxel in its input's order: the oracle's chain is the product's in the
    # emission order they share, bucket order)
    sage = gpu_sage
    cfg = sage.make_pipeline_config()
    p = sage.SageICP(cfg)
    assert p.source().shape == (0, 4)
    for k, f in enumerate(_stream(20)):
        n_source = p.RegisterFrame(f)[3]
        src = p.source()
        assert src.shape == (n_source, 4), k
        want = _sorted(_chain(sage, f, cfg))
        assert np.array_equal(_bits(_sorted(src)), _bits(want)), k
        assert np.array_equal(_bits(want), _bits(_sorted(_chain(sage, f, cfg, ds=_oracle_ds(oracle))))), k
    p.reinitialize()
    assert p.source().shape == (0, 4)


@pytest.mark.gpu
def test_reference_source_order_is_the_chain_row_for_row(gpu_sage, oracle, reference_emission_order):
    sage = gpu_sage
    cfg = sage.make_pipeline_config()
    os.environ["SAGEICP_SOURCE_REFERENCE_ORDER"] = "1"
    try:
        p = sage.SageICP(cfg)
        for k, f in enumerate(_stream(20)):
            n_source = p.RegisterFrame(f)[3]
            src = p.source()
            assert src.shape == (n_source, 4), k
            assert np.array_equal(_bits(src), _bits(_chain(sage, f, cfg))), k
            assert np.array_equal(_bits(src), _bits(_chain(sage, f, cfg, ds=_oracle_ds(oracle)))), k
            d = p.source(device=True)
            assert np.array_equal(_bits(d.cpu().numpy()), _bits(src)), k
    finally:
        del os.environ["SAGEICP_SOURCE_REFERENCE_ORDER"]


# ---- 2. deskew and the dynamic vehicle filter -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_source_with_deskew_is_the_chain_of_the_deskewed_frame(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic_skew as sk
    S = sk.make_skewed_stream(seed=0x5E, n_frames=8, az_steps=2048)
    cfg = sage.make_pipeline_config(deskew=True)
    p = sage.SageICP(cfg)
    for k, (f, t) in enumerate(zip(S["frames"], S["timestamps"])):
        P = p.poses()
        g = sage.deskew_scan(f, t, P[-2], P[-1]) if len(P) > 2 else f
        p.RegisterFrame(f, t)
        assert p.deskew_info()[0] == (k >= 3), k
        assert np.array_equal(_bits(_sorted(p.source())), _bits(_sorted(_chain(sage, g, cfg)))), k


@pytest.mark.gpu
def test_source_with_the_dynamic_filter_is_the_chain_of_the_filtered_frame(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic_dynamic as sd
    frames, _ = sd.make_dynamic_stream(21, 8, n=40000)
    cfg = sage.make_pipeline_config(dynamic_vehicle_filter=True)
    p = sage.SageICP(cfg)
    vehicles = sage.KITTI_VOXEL_LABELS[5]
    for k, f in enumerate(frames):
        p.RegisterFrame(f)
        assert p.dynamic_filter_info()["points_removed"] > 0, k
        want = _chain(sage, f, cfg, dynamic_vehicle_filter=True, dy_th=0.5, dynamic_labels=vehicles,
                      landmark_labels=(44, 48))
        assert np.array_equal(_bits(_sorted(p.source())), _bits(_sorted(want))), k


@pytest.mark.gpu
def test_a_refused_register_call_leaves_no_source(gpu_sage):
    """every way a register call can fail, before or inside the registration, leaves a 0-row source (not the last
    frame's cloud)"""
    sage = gpu_sage
    from sage_icp_amd import synthetic_skew as sk
    S = sk.make_skewed_stream(seed=0x5E, n_frames=6, az_steps=2048)
    F = [np.ascontiguousarray(f, dtype=np.float64) for f in S["frames"]]
    T = [np.ascontiguousarray(t, dtype=np.float64) for t in S["timestamps"]]
    p = sage.SageICP(sage.make_pipeline_config(deskew=True))
    L = sage.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    pose = np.empty(7)

    def device_frame_in_host_memory():
        f = sage.DeviceFrame(F[1].ctypes.data, 32, sage.DTYPE_FLOAT64, 0, None, 0, len(F[1]))
        return L.sageicp_pipeline_register_frame_device(p._h, ctypes.byref(f), None, None, pose.ctypes.data_as(dp),
                                                        None, None, None, None)

    def nan_timestamp():
        t = T[1].copy()
        t[17] = np.nan
        return L.sageicp_pipeline_register_frame_timestamps(p._h, F[1].ctypes.data_as(dp), t.ctypes.data_as(dp),
                                                            len(F[1]), pose.ctypes.data_as(dp), None, None, None, None)

    def null_timestamps():
        return L.sageicp_pipeline_register_frame_timestamps(p._h, F[1].ctypes.data_as(dp), None, len(F[1]),
                                                            pose.ctypes.data_as(dp), None, None, None, None)

    def null_pose_out():
        return L.sageicp_pipeline_register_frame(p._h, F[1].ctypes.data_as(dp), len(F[1]), None, None, None, None,
                                                 None)

    def nan_label():                # refused inside the registration, by the preprocessing (a point the crop keeps)
        f = F[1].copy()
        r = np.linalg.norm(f[:, :3], axis=1)
        f[int(np.flatnonzero((r > 10.0) & (r < 40.0))[0]), 3] = np.nan
        return L.sageicp_pipeline_register_frame_timestamps(p._h, f.ctypes.data_as(dp), T[1].ctypes.data_as(dp),
                                                            len(f), pose.ctypes.data_as(dp), None, None, None, None)

    k = 0
    for name, refused in (("device frame in host memory", device_frame_in_host_memory),
                          ("NaN timestamp", nan_timestamp), ("NULL timestamps", null_timestamps),
                          ("NULL pose_out", null_pose_out), ("NaN label", nan_label)):
        p.RegisterFrame(F[k % len(F)], T[k % len(T)])
        k += 1
        assert p.source_size() > 0 and len(p.source(device=True)) == p.source_size(), name
        poses = len(p.poses())
        assert refused() == sage.ERR_INVALID, name
        assert len(p.poses()) == poses, name
        assert p.source_size() == 0, name
        assert p.source().shape == (0, 4), name
        assert p.source(device=True).shape == (0, 4), name
        out = torch.full((8, 4), 3.0, dtype=torch.float64, device=DEV)
        assert p.source(out=out).shape == (0, 4) and (out == 3.0).all(), name


# ---- 3. prefetch and device frames ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_source_is_the_same_with_prefetch_and_for_device_frames(gpu_sage):
    sage = gpu_sage
    frames = _stream(8)
    a, b, c = sage.SageICP(), sage.SageICP(), sage.SageICP()
    mine = frames[0]
    for k, f in enumerate(frames):
        ra = a.RegisterFrame(f)
        # frame k + 1 is prepared on the other buffers under frame k's registration
        nxt = b.prefetch(frames[k + 1]) if k + 1 < len(frames) else None
        rb = b.RegisterFrame(mine)
        mine = nxt
        t, lab = torch.from_numpy(f).to(DEV), None
        if k % 2:        # float32 rows with int64 labels apart: the same values (the synthetic xyz are float32 values)
            t = torch.from_numpy(f[:, :3].astype(np.float32)).to(DEV)
            lab = torch.from_numpy(f[:, 3].astype(np.int64)).to(DEV)
        rc = c.RegisterFrame(t, labels=lab)
        sa, sb = a.source(), b.source()
        if nxt is not None:
            b.prefetch_wait()         # the worker filled the other buffers: the source is still this frame's
        assert np.array_equal(_bits(sa), _bits(b.source())), k
        assert np.array_equal(_bits(sa), _bits(sb)), k
        assert np.array_equal(ra[0], rb[0]) and ra[3] == rb[3] == len(sa), k
        assert np.array_equal(_bits(sa), _bits(c.source())), k
        assert np.array_equal(ra[0], rc[0]), k


# ---- 4. device layouts against the host rows ---------------------------------------------------------------------------
def _registered(sage, n_frames=3):
    p = sage.SageICP()
    for f in _stream(n_frames):
        p.RegisterFrame(f)
    return p


@pytest.mark.gpu
def test_device_source_layouts_match_the_host_rows(gpu_sage):
    p = _registered(gpu_sage)
    host = p.source()
    n = len(host)
    assert n > 1000
    d64 = p.source(device=True)
    assert d64.dtype == torch.float64 and d64.device == torch.device(DEV) and d64.shape == (n, 4)
    assert np.array_equal(_bits(d64.cpu().numpy()), _bits(host))
    d32 = p.source(device=True, dtype=torch.float32)
    assert d32.dtype == torch.float32
    assert np.array_equal(d32.cpu().numpy().view(np.uint32), host.astype(np.float32).view(np.uint32))
    for ldt, ndt in ((torch.uint8, np.uint8), (torch.int32, np.int32), (torch.int64, np.int64)):
        for xdt, nx in ((torch.float64, np.float64), (torch.float32, np.float32)):
            out = torch.full((n, 3), -7.0, dtype=xdt, device=DEV)
            lab = torch.full((n,), 99, dtype=ldt, device=DEV)
            o, l = p.source(out=out, labels_out=lab)
            assert o.shape == (n, 3) and l.shape == (n,)
            assert np.array_equal(o.cpu().numpy(), host[:, :3].astype(nx)), (ldt, xdt)
            assert np.array_equal(l.cpu().numpy(), host[:, 3].astype(np.int64).astype(ndt)), (ldt, xdt)


@pytest.mark.gpu
@pytest.mark.parametrize("xdt", [torch.float64, torch.float32])
def test_strided_destinations_leave_the_guard_columns_alone(gpu_sage, xdt):
    p = _registered(gpu_sage)
    host = p.source()
    n = len(host)
    wide = torch.full((n, 6), 1234.5, dtype=xdt, device=DEV)
    got = p.source(out=wide[:, 0:4])
    assert np.array_equal(got.cpu().numpy(), host.astype(xdt == torch.float32 and np.float32 or np.float64))
    assert (wide[:, 4:] == 1234.5).all()
    # x, y, z in columns 1-3 of a 5-wide tensor, the labels in column 2 of a 3-wide int tensor
    wide = torch.full((n, 5), 1234.5, dtype=xdt, device=DEV)
    li = torch.full((n, 3), -5, dtype=torch.int32, device=DEV)
    o, l = p.source(out=wide[:, 1:4], labels_out=li[:, 2])
    assert np.array_equal(o.cpu().numpy(), host[:, :3].astype(o.cpu().numpy().dtype))
    assert np.array_equal(l.cpu().numpy(), host[:, 3].astype(np.int32))
    assert (wide[:, 0] == 1234.5).all() and (wide[:, 4] == 1234.5).all()
    assert (li[:, :2] == -5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["source", "local_map"])
def test_aligned_float64_rows_with_labels_apart_leave_column_3_alone(gpu_sage, what):
    """(n, 4) float64 rows with the labels in a tensor of their own: a 32-B stride, so x, y go out as one 16-B store
    and z alone — column 3 keeps its sentinel"""
    p = _registered(gpu_sage)
    host = p.source() if what == "source" else p.LocalMap()
    call = p.source if what == "source" else p.LocalMap
    n = len(host)
    for ldt, ndt in ((torch.uint8, np.uint8), (torch.int32, np.int32), (torch.int64, np.int64)):
        rows = torch.full((n, 4), 1234.5, dtype=torch.float64, device=DEV)
        lab = torch.full((n,), 7, dtype=ldt, device=DEV)
        o, l = call(out=rows[:, :3], labels_out=lab)
        assert o.stride(0) == 4 and rows.data_ptr() % 16 == 0
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(host[:, :3])), ldt
        assert np.array_equal(l.cpu().numpy(), host[:, 3].astype(np.int64).astype(ndt)), ldt
        assert (rows[:, 3] == 1234.5).all(), ldt


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["source", "local_map"])
def test_a_short_destination_gets_exactly_its_rows(gpu_sage, what):
    p = _registered(gpu_sage)
    host = p.source() if what == "source" else p.LocalMap()
    call = p.source if what == "source" else p.LocalMap
    n = len(host)
    for cap in (1, 255, 257, n // 3):
        out = torch.full((cap + 50, 4), -3.0, dtype=torch.float64, device=DEV)
        got = call(out=out[:cap])
        assert got.shape == (cap, 4)
        assert np.array_equal(_bits(out[:cap].cpu().numpy()), _bits(host[:cap])), cap
        assert (out[cap:] == -3.0).all(), cap
        lab = torch.full((cap + 50,), 77, dtype=torch.int64, device=DEV)
        o3 = torch.full((cap, 3), -3.0, dtype=torch.float32, device=DEV)
        call(out=o3, labels_out=lab[:cap])
        assert np.array_equal(lab[:cap].cpu().numpy(), host[:cap, 3].astype(np.int64)), cap
        assert (lab[cap:] == 77).all(), cap
    empty = torch.empty((0, 4), dtype=torch.float64, device=DEV)
    assert call(out=empty).shape == (0, 4)


@pytest.mark.gpu
def test_a_label_that_does_not_fit_is_refused(gpu_sage):
    sage = gpu_sage
    frames = _stream(2)
    for f in frames:
        f[f[:, 3] == 40, 3] = 259.0       # a SemanticKITTI moving class: out of uint8's range
    # a label group for SemanticKITTI's moving classes, so that their points are kept
    cfg = sage.make_pipeline_config(voxel_labels=sage.KITTI_VOXEL_LABELS + [list(range(252, 260))],
                                    voxel_size=sage.KITTI_VOXEL_SIZE + [1.0])
    p = sage.SageICP(cfg)
    for f in frames:
        p.RegisterFrame(f)
    host = p.source()
    assert (host[:, 3] == 259).any()
    n = len(host)
    out = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    with pytest.raises(sage.SageIcpError) as e:
        p.source(out=out, labels_out=torch.empty(n, dtype=torch.uint8, device=DEV))
    assert e.value.code == sage.ERR_INVALID and "label" in str(e.value)
    with pytest.raises(sage.SageIcpError):
        p.LocalMap(out=torch.empty((p.LocalMap().shape[0], 3), device=DEV),
                   labels_out=torch.empty(p.LocalMap().shape[0], dtype=torch.uint8, device=DEV))
    o, l = p.source(out=out, labels_out=torch.empty(n, dtype=torch.int32, device=DEV))
    assert np.array_equal(l.cpu().numpy(), host[:, 3].astype(np.int32))
    # after a refusal the next call works
    assert np.array_equal(_bits(p.source(device=True).cpu().numpy()), _bits(host))


# ---- 5. the local map -----------------------------------------------------------------------------------------------------
def _c2_map(sage, reference_order, resident):
    from sage_icp_amd import synthetic as syn

    def new_map():
        m = sage.VoxelHashMap(1.0, 1e6)
        return m.set_reference_order(True) if reference_order else m
    w = syn.make_workload("c2", new_map)
    m = w["map"]
    if resident:
        m.UpdateOnDevice(w["scan"][:5000], w["T_gt"])
        assert m.resident()
    else:
        assert not m.resident()
    assert m.size() >= 1_000_000
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
@pytest.mark.parametrize("reference_order", [False, True], ids=["pool_order", "reference_order"])
def test_device_local_map_matches_the_host_rows(gpu_sage, reference_order, resident):
    m = _c2_map(gpu_sage, reference_order, resident)
    host = m.Pointcloud()
    assert m.resident() == resident
    d = m.Pointcloud(device=True)
    assert d.shape == host.shape and d.dtype == torch.float64
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(host))
    d32 = m.Pointcloud(device=True, dtype=torch.float32)
    assert np.array_equal(d32.cpu().numpy().view(np.uint32), host.astype(np.float32).view(np.uint32))
    o, l = m.Pointcloud(out=torch.empty((len(host), 3), dtype=torch.float32, device=DEV),
                        labels_out=torch.empty(len(host), dtype=torch.int32, device=DEV))
    assert np.array_equal(o.cpu().numpy(), host[:, :3].astype(np.float32))
    assert np.array_equal(l.cpu().numpy(), host[:, 3].astype(np.int32))
    assert m.resident() == resident
    assert np.array_equal(_bits(m.Pointcloud()), _bits(host))


@pytest.mark.gpu
def test_two_pass_local_map_matches_the_fused_one(gpu_sage):
    m = _c2_map(gpu_sage, False, True)
    fused = m.Pointcloud(device=True, dtype=torch.float32)
    os.environ["SAGEICP_EGRESS_TWO_PASS"] = "1"
    try:
        two = m.Pointcloud(device=True, dtype=torch.float32)
    finally:
        del os.environ["SAGEICP_EGRESS_TWO_PASS"]
    assert torch.equal(fused, two)


@pytest.mark.gpu
def test_reference_order_pipeline_local_map_is_the_oracles_row_for_row(gpu_sage, oracle_ref):
    sage = gpu_sage
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(21, 12, points_per_frame=20000, step=(2.5, 0.0, 0.0), max_range=30.0)
    cfg = sage.make_pipeline_config(max_range=30.0, local_map_range=30.0)
    os.environ["SAGEICP_MAP_REFERENCE_ORDER"] = "1"
    try:
        a = sage.SageICP(cfg)
    finally:
        del os.environ["SAGEICP_MAP_REFERENCE_ORDER"]
    b = oracle_ref.Pipeline(cfg)
    for k, f in enumerate(frames):
        a.RegisterFrame(f)
        b.register_frame(f)
        if k % 4 == 3:
            ma, mb = a.LocalMap(device=True).cpu().numpy(), b.local_map()
            assert np.array_equal(_bits(ma), _bits(a.LocalMap())), k
            assert ma.shape == mb.shape, k
            assert np.array_equal(ma[:, 3], mb[:, 3]), k
            assert np.allclose(ma[:, :3], mb[:, :3], rtol=0, atol=1e-8), k


# ---- 6. the caller's stream -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["source", "local_map"])
def test_the_write_follows_the_callers_stream(gpu_sage, what):
    p = _registered(gpu_sage)
    host = p.source() if what == "source" else p.LocalMap()
    call = p.source if what == "source" else p.LocalMap
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        out = torch.empty((len(host), 4), dtype=torch.float64, device=DEV)
        torch.cuda._sleep(200_000_000)
        out.fill_(float("nan"))               # lands only after the delay: the rows must land after it
        got = call(out=out)
        # the call is synchronous: the rows are in place now, whatever the stream does next
        snap = got.clone()
        out.fill_(float("nan"))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(snap.cpu().numpy()), _bits(host))


# ---- 7. memory that is not device memory ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_memory_that_is_not_device_memory_is_refused(gpu_sage):
    sage = gpu_sage
    p = _registered(sage, 2)
    n = len(p.source())
    L = sage.lib()
    h = L.sageicp_pipeline_local_map(p._h)
    host = np.full((n, 4), 5.0)
    pinned = torch.full((n, 4), 5.0, dtype=torch.float64).pin_memory()
    for ptr in (host.ctypes.data, pinned.data_ptr()):
        d = sage.DevicePoints(ptr, 32, sage.DTYPE_FLOAT64, 0, None, 0, n)
        k = ctypes.c_uint64(0)
        assert L.sageicp_pipeline_source_device(p._h, ctypes.byref(d), None, ctypes.byref(k)) == sage.ERR_INVALID
        assert "device memory" in L.sageicp_last_error().decode()
        assert L.sageicp_map_pointcloud_device(h, ctypes.byref(d), None, ctypes.byref(k)) == sage.ERR_INVALID
    # a device tensor with its labels in host memory
    dev = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    d = sage.DevicePoints(dev.data_ptr(), 24, sage.DTYPE_FLOAT64, sage.DTYPE_INT64, host.ctypes.data, 8, n)
    k = ctypes.c_uint64(0)
    assert L.sageicp_pipeline_source_device(p._h, ctypes.byref(d), None, ctypes.byref(k)) == sage.ERR_INVALID
    assert (host == 5.0).all() and (pinned == 5.0).all()
    with pytest.raises(ValueError):
        p.source(out=torch.empty((n, 4), dtype=torch.float64))
    with pytest.raises(ValueError):
        p.LocalMap(out=torch.empty((n, 4), dtype=torch.float64))


# ---- 8. registration is unchanged ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exports_between_frames_leave_the_registration_alone(gpu_sage):
    sage = gpu_sage
    frames = _stream(10)
    a, b = sage.SageICP(), sage.SageICP()
    for k, f in enumerate(frames):
        ra, rb = a.RegisterFrame(f), b.RegisterFrame(f)
        assert np.array_equal(_bits(ra[0]), _bits(rb[0])) and ra[3] == rb[3], k
        b.source(device=True)
        b.LocalMap(device=True, dtype=torch.float32)
        b.source(out=torch.empty((ra[3], 3), dtype=torch.float32, device=DEV),
                 labels_out=torch.empty(ra[3], dtype=torch.int64, device=DEV))
        b.LocalMap(device=True)
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))
    assert np.array_equal(_bits(a.LocalMap()), _bits(b.LocalMap()))
