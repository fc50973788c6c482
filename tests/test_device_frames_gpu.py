"""Frames that are already on the GPU (sageicp_device_frame, csrc/ingest.hip): a torch tensor registered through the
pipeline or made a resident Frame gives, bit for bit, what the same values give as host rows — every format the
ingest kernel reads, the dynamic vehicle filter, deskew with device timestamps, non-finite input, the order of the
caller's stream, announcements — and memory that is not device memory of the library's runtime is refused."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_result(ra, rb, what):
    (pa, _, _, na, sa), (pb, _, _, nb, sb) = ra, rb
    assert np.array_equal(_bits(pa), _bits(pb)), what
    assert na == nb, what
    assert (sa.iterations, sa.n_corr_first, sa.n_corr_last) == (sb.iterations, sb.n_corr_first, sb.n_corr_last), what
    assert list(sa.n_corr_hist) == list(sb.n_corr_hist), what


def _same_state(a, b):
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))
    assert np.array_equal(_bits(a.LocalMap()), _bits(b.LocalMap()))


def _street(n_frames):
    from sage_icp_amd import synthetic as syn
    frames, truth = syn.make_stream(31, n_frames, points_per_frame=30000)
    return [np.ascontiguousarray(f, dtype=np.float64) for f in frames], truth


def _street_and_ring():
    """12 street frames of 30k points, then a 64-beam ring scan of 122k points seen from the last pose"""
    from sage_icp_amd import synthetic as syn
    frames, truth = _street(12)
    ring = syn.make_ring_scan(np.random.default_rng(32), truth[-1], az_steps=2400)
    assert len(ring) >= 120000
    return frames + [np.ascontiguousarray(ring, dtype=np.float64)]


def _stream_parity(sage, host_frames, device_frames, cfg=None):
    cfg = cfg if cfg is not None else sage.make_pipeline_config()
    a, b = sage.SageICP(cfg), sage.SageICP(cfg)
    for k, (h, d) in enumerate(zip(host_frames, device_frames)):
        ra = a.RegisterFrame(h)
        rb = b.RegisterFrame(d[0], labels=d[1]) if isinstance(d, tuple) else b.RegisterFrame(d)
        _same_result(ra, rb, "frame %d" % k)
    _same_state(a, b)


@pytest.mark.gpu
def test_fp64_xyzl_tensor_stream_matches_host_rows(gpu_sage):
    frames = _street_and_ring()
    _stream_parity(gpu_sage, frames, [torch.from_numpy(f).to(DEV) for f in frames])


def _f32_host(f, labels):
    h = np.empty((len(f), 4))
    h[:, :3] = f[:, :3].astype(np.float32).astype(np.float64)
    h[:, 3] = labels.astype(np.float64)
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["f32_n4_u8", "f32_n4_i64", "f32_xyzl", "f32_n3_i32", "f32_n6_view_strided_labels",
                                    "f64_n6_view_strided_labels"])
def test_float32_and_strided_layouts_match_host_rows(gpu_sage, layout):
    frames = _street_and_ring()
    rng = np.random.default_rng(5)
    host, dev = [], []
    for f in frames:
        n = len(f)
        lab = f[:, 3].astype(np.int64)
        assert lab.min() >= 0 and lab.max() < 256
        xyz32 = torch.from_numpy(f[:, :3].astype(np.float32))
        garbage = torch.from_numpy(rng.uniform(-1e30, 1e30, n).astype(np.float32))      # "intensity"
        host.append(_f32_host(f, lab))
        if layout.startswith("f32_n4"):
            t = torch.cat([xyz32, garbage[:, None]], 1).to(DEV)
            L = torch.from_numpy(lab.astype(np.uint8 if layout.endswith("u8") else np.int64)).to(DEV)
            dev.append((t, L))
        elif layout == "f32_xyzl":
            dev.append(torch.cat([xyz32, torch.from_numpy(lab.astype(np.float32))[:, None]], 1).to(DEV))
        elif layout == "f32_n3_i32":
            dev.append((xyz32.to(DEV), torch.from_numpy(lab.astype(np.int32)).to(DEV)))
        else:
            dt = torch.float32 if layout.startswith("f32") else torch.float64
            w = torch.full((n, 6), float("nan"), dtype=dt)
            w[:, :3] = torch.from_numpy(f[:, :3].astype(np.float32)).to(dt)
            w[:, 3] = garbage.to(dt)
            twice = torch.full((2 * n,), -7, dtype=torch.int64)
            twice[::2] = torch.from_numpy(lab)
            dev.append((w.to(DEV), twice.to(DEV)[::2]))
            assert dev[-1][0].stride() == (6, 1) and dev[-1][1].stride() == (2,)
    _stream_parity(gpu_sage, host, dev)


@pytest.mark.gpu
def test_dynamic_vehicle_filter_on_device_frames(gpu_sage):
    from sage_icp_amd import synthetic_dynamic as sd
    frames, _ = sd.make_dynamic_stream(23, 6, n=40000)
    frames = [np.ascontiguousarray(f, dtype=np.float64) for f in frames]
    cfg = gpu_sage.make_pipeline_config(dynamic_vehicle_filter=True)
    a, b = gpu_sage.SageICP(cfg), gpu_sage.SageICP(cfg)
    removed = 0
    for k, f in enumerate(frames):
        _same_result(a.RegisterFrame(f), b.RegisterFrame(torch.from_numpy(f).to(DEV)), "frame %d" % k)
        ia, ib = a.dynamic_filter_info(), b.dynamic_filter_info()
        keys = ("vehicle_points", "landmark_points", "clusters", "clusters_kept", "points_removed")
        assert [ia[x] for x in keys] == [ib[x] for x in keys]
        removed += ia["points_removed"]
    assert removed > 0             # the filter did something
    _same_state(a, b)


@pytest.mark.gpu
def test_deskew_with_device_timestamps_matches_host_timestamps(gpu_sage):
    from sage_icp_amd import synthetic_skew as sk
    S = sk.make_skewed_stream(seed=0x5F, n_frames=6, az_steps=1024)
    cfg = gpu_sage.make_pipeline_config(deskew=True)
    a, b = gpu_sage.SageICP(cfg), gpu_sage.SageICP(cfg)
    applied = 0
    for k, (f, t) in enumerate(zip(S["frames"], S["timestamps"])):
        _same_result(a.RegisterFrame(f, t), b.RegisterFrame(torch.from_numpy(f).to(DEV),
                                                            timestamps=torch.from_numpy(t).to(DEV)), "frame %d" % k)
        (xa, da), (xb, db) = a.deskew_info(), b.deskew_info()
        assert xa == xb and np.array_equal(_bits(da), _bits(db))
        applied += xa
        if k == 3:                 # a non-finite stamp on a later frame: refused, no pose, nothing changed
            bad = t.copy()
            bad[len(bad) // 3] = np.nan
            for p, frame, ts in ((a, f, bad), (b, torch.from_numpy(f).to(DEV), torch.from_numpy(bad).to(DEV))):
                with pytest.raises(gpu_sage.SageIcpError) as e:
                    p.RegisterFrame(frame, ts)
                assert e.value.code == gpu_sage.ERR_INVALID and "timestamp" in str(e.value)
            assert len(a.poses()) == len(b.poses()) == k + 1
    assert applied == 3
    _same_state(a, b)
    # ... and on the very first frame
    c = gpu_sage.SageICP(cfg)
    bad = S["timestamps"][0].copy()
    bad[-1] = np.inf
    with pytest.raises(gpu_sage.SageIcpError) as e:
        c.RegisterFrame(torch.from_numpy(S["frames"][0]).to(DEV), timestamps=torch.from_numpy(bad).to(DEV))
    assert e.value.code == gpu_sage.ERR_INVALID
    assert len(c.poses()) == 0
    # deskew off: the timestamps are not read, even non-finite ones
    d, e2 = gpu_sage.SageICP(gpu_sage.make_pipeline_config()), gpu_sage.SageICP(gpu_sage.make_pipeline_config())
    _same_result(d.RegisterFrame(S["frames"][0]),
                 e2.RegisterFrame(torch.from_numpy(S["frames"][0]).to(DEV), timestamps=torch.from_numpy(bad).to(DEV)),
                 "deskew off")


@pytest.mark.gpu
def test_non_finite_rows_give_the_host_outcome(gpu_sage):
    frames = _street(4)[0]
    a, b = gpu_sage.SageICP(), gpu_sage.SageICP()
    for k, f in enumerate(frames[:2]):
        _same_result(a.RegisterFrame(f), b.RegisterFrame(torch.from_numpy(f).to(DEV)), "frame %d" % k)
    nan_xyz = frames[2].copy()
    nan_xyz[::997, 1] = np.nan                     # dropped by the crop, like the reference's Preprocess()
    nan_label = frames[3].copy()
    r = np.linalg.norm(nan_label[:, :3], axis=1)
    nan_label[np.flatnonzero((r > 6.0) & (r < 40.0))[::50], 3] = np.nan     # kept points: the frame is refused
    for k, f in enumerate((nan_xyz, nan_label, frames[3])):
        outcome = []
        for p, x in ((a, f), (b, torch.from_numpy(f).to(DEV))):
            try:
                outcome.append(("ok", p.RegisterFrame(x)))
            except gpu_sage.SageIcpError as e:
                outcome.append((e.code, None))
        assert outcome[0][0] == outcome[1][0], (k, outcome[0][0], outcome[1][0])
        if outcome[0][0] == "ok":
            _same_result(outcome[0][1], outcome[1][1], "case %d" % k)
        _same_state(a, b)
    assert len(a.poses()) == 4                      # the NaN-label frame was refused, the others registered


@pytest.mark.gpu
def test_resident_frame_from_a_tensor(gpu_sage):
    frames = _street_and_ring()
    m = gpu_sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints(frames[0])
    P = dict(max_correspondence_distance=3.0, kernel=1.0, sem_th=0.05)
    for k, f in enumerate((frames[1], frames[-1])):
        ph, sh = gpu_sage.register_frame(f, m, gpu_sage.IDENTITY, return_stats=True, **P)
        fr = gpu_sage.Frame(m, torch.from_numpy(f).to(DEV))
        assert fr.n == len(f)
        pd, sd = gpu_sage.register_frame(fr, m, gpu_sage.IDENTITY, return_stats=True, **P)
        assert np.array_equal(_bits(ph), _bits(pd)), k
        assert (sh.iterations, sh.n_corr_first, sh.n_corr_last) == (sd.iterations, sd.n_corr_first, sd.n_corr_last)
        # float32 rows + separate int64 labels, against the same values as host rows
        lab = f[:, 3].astype(np.int64)
        h = _f32_host(f, lab)
        fr32 = gpu_sage.Frame(m, torch.from_numpy(f[:, :3].astype(np.float32)).to(DEV),
                              labels=torch.from_numpy(lab).to(DEV))
        ph32 = gpu_sage.register_frame(h, m, gpu_sage.IDENTITY, **P)
        assert np.array_equal(_bits(ph32), _bits(gpu_sage.register_frame(fr32, m, gpu_sage.IDENTITY, **P)))


def _delay(stream):
    """keep `stream` busy for a while (tens of ms at least) before what is enqueued next"""
    try:
        torch.cuda._sleep(200_000_000)
    except (AttributeError, RuntimeError):
        x = torch.randn(4096, 4096, device=DEV)
        for _ in range(40):
            x = torch.tanh(x @ x)


@pytest.mark.gpu
def test_the_call_follows_the_callers_stream_and_then_lets_go(gpu_sage):
    frames = _street(4)[0]
    a, b = gpu_sage.SageICP(), gpu_sage.SageICP()
    ref = [a.RegisterFrame(f) for f in frames]
    src = [torch.from_numpy(f).to(DEV) for f in frames]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        t = torch.empty((len(frames[0]), 4), dtype=torch.float64, device=DEV)
        t.fill_(float("nan"))
        _delay(s)
        t.copy_(src[0])                 # lands only after the delay: the call must wait for it
        _same_result(ref[0], b.RegisterFrame(t), "frame 0")
        for k in (1, 2, 3):
            # the call has returned: nothing reads `t` any more, so it can be refilled at once
            t = t if len(frames[k]) == t.shape[0] else torch.empty((len(frames[k]), 4), dtype=torch.float64, device=DEV)
            t.copy_(src[k])
            _same_result(ref[k], b.RegisterFrame(t), "frame %d" % k)
            t.fill_(float("nan"))
    torch.cuda.synchronize()
    _same_state(a, b)


@pytest.mark.gpu
def test_device_frame_consumes_an_announcement_like_a_host_frame(gpu_sage):
    frames = _street(5)[0]
    a, b = gpu_sage.SageICP(), gpu_sage.SageICP()
    ref = [a.RegisterFrame(f) for f in frames]
    _same_result(ref[0], b.RegisterFrame(frames[0]), "frame 0")
    nxt = b.prefetch(frames[2])                       # announces the frame after the next one
    _same_result(ref[1], b.RegisterFrame(torch.from_numpy(frames[1]).to(DEV)), "frame 1 (device)")
    _same_result(ref[2], b.RegisterFrame(nxt), "frame 2 (announced)")
    b.prefetch(frames[4])                             # announced, but a device frame comes instead: dropped
    _same_result(ref[3], b.RegisterFrame(torch.from_numpy(frames[3]).to(DEV)), "frame 3 (device)")
    _same_result(ref[4], b.RegisterFrame(frames[4]), "frame 4")
    _same_state(a, b)


@pytest.mark.gpu
def test_memory_that_is_not_device_memory_is_refused(gpu_sage):
    p = gpu_sage.SageICP()
    host = np.zeros((1000, 4))
    pinned = torch.zeros((1000, 4), dtype=torch.float64).pin_memory()
    dev = torch.zeros((1000, 4), dtype=torch.float64, device=DEV)
    out = np.empty(7)
    for what, ptr, lab in (("host", host.ctypes.data, None), ("pinned", pinned.data_ptr(), None),
                           ("host labels", dev.data_ptr(), host.ctypes.data)):
        f = gpu_sage.DeviceFrame(ptr, 32, gpu_sage.DTYPE_FLOAT64, gpu_sage.DTYPE_INT64 if lab else 0, lab,
                                 8 if lab else 0, 1000)
        rc = gpu_sage.lib().sageicp_pipeline_register_frame_device(
            p._h, ctypes.byref(f), None, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None,
            None)
        assert rc == gpu_sage.ERR_INVALID, what
        assert "not device memory" in gpu_sage.lib().sageicp_last_error().decode(), what
        m = gpu_sage.VoxelHashMap(1.0, 100.0)
        assert not gpu_sage.lib().sageicp_frame_from_device(m._h, ctypes.byref(f), None), what
    assert len(p.poses()) == 0
    # the refusals left no error behind: the next call works
    f0 = _street(1)[0][0]
    ok = gpu_sage.SageICP()
    _same_result(p.RegisterFrame(f0), ok.RegisterFrame(torch.from_numpy(f0).to(DEV)), "after refusals")


@pytest.mark.gpu
def test_library_loaded_before_torch_refuses_tensors(gpu_sage):
    """Loaded first, the library may sit beside a second HIP runtime that torch brings: a tensor is refused with the
    remedy in the message, before any call reaches the library's device code."""
    child = r"""
import os, sys
sys.path.insert(0, %r)
import sage_icp_amd as sage
sage.lib()
import torch
p = sage.SageICP()
t = torch.zeros((1000, 4), dtype=torch.float64, device="cuda:0")
try:
    p.RegisterFrame(t)
    print("NOT REFUSED", sorted(set(sage._hip_runtimes().values())))
    sys.stdout.flush()
    os._exit(3)
except sage.SageIcpError as e:
    assert e.code == sage.ERR_INVALID, e
    assert "import torch before the first sage_icp_amd call" in str(e), e
    print("refused:", e)
sys.stdout.flush()
os._exit(0)          # the library's runtime was never used: nothing of it to tear down
""" % ROOT
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "refused:" in r.stdout
