"""sensor_msgs/PointCloud2 payloads unpacked and packed on the device (csrc/msg.hip), against the numpy
restatement of tests/pc2ref.py.  Every comparison is bit for bit: the casts are exact, the fp64 division of the stamps
is correctly rounded on both sides, packing is data movement.  Unpacked rows and stamps are observed through what the
pipeline does with them — the pose, n_source, source() and deskew_info of a frame registered as a message against the
same values registered as host rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pc2ref

DEV = "cuda:0"
F32, F64, U8, U32 = pc2ref.FLOAT32, pc2ref.FLOAT64, pc2ref.UINT8, pc2ref.UINT32
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4099)

# name -> (fields, point_step): x, y, z float32, the label uint8 or float32, then 't' (uint32) and 'time' (float64)
# where the record has room.  The kernel stages records of up to 64 bytes through LDS: 65 is the first beyond.
LAYOUTS = {
    "tight13": ([("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("label", 12, U8)], 13),
    "16": ([("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("label", 12, F32)], 16),
    "ref21": ([("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("label", 12, U8), ("t", 13, U32)], 21),
    "22": ([("x", 1, F32), ("y", 5, F32), ("z", 9, F32), ("label", 13, F32), ("t", 18, U32)], 22),
    "32": ([("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("label", 12, U8), ("t", 16, U32), ("time", 24, F64)], 32),
    "48": ([("x", 8, F32), ("y", 12, F32), ("z", 16, F32), ("label", 24, F32), ("time", 32, F64), ("t", 44, U32)], 48),
    "64": ([("x", 59, F32), ("y", 4, F32), ("z", 33, F32), ("label", 63, U8), ("t", 9, U32), ("time", 49, F64)], 64),
    "65": ([("x", 3, F32), ("y", 7, F32), ("z", 11, F32), ("label", 15, U8), ("t", 17, U32), ("time", 21, F64)], 65),
    "1024": ([("x", 1000, F32), ("y", 1004, F32), ("z", 1008, F32), ("label", 1012, F32), ("t", 1016, U32),
              ("time", 9, F64)], 1024),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _layout(sage, name, time_field=None):
    fields, step = LAYOUTS[name]
    off = {f[0]: f[1] for f in fields}
    typ = {f[0]: f[2] for f in fields}
    lay = sage.MsgLayout(step, off["x"], off["y"], off["z"], off["label"],
                         sage.DTYPE_UINT8 if typ["label"] == U8 else sage.DTYPE_FLOAT32, 0, 0)
    if time_field:
        lay.time_kind, lay.time_offset = (1 if time_field == "t" else 2), off[time_field]
    return lay


_FRAMES = {}


def _frames(n_frames=10, n=30000, seed=31):
    """synthetic street frames (x, y, z are float32 values, integer labels), shared and never written"""
    key = (n_frames, n, seed)
    if key not in _FRAMES:
        from sage_icp_amd import synthetic as syn
        frames, _ = syn.make_stream(seed, n_frames, points_per_frame=n)
        fs = [np.ascontiguousarray(f, dtype=np.float64) for f in frames]
        for f in fs:
            assert np.array_equal(f[:, :3], f[:, :3].astype(np.float32)) and f[:, 3].min() >= 0 and f[:, 3].max() <= 255
            f.setflags(write=False)
        _FRAMES[key] = fs
    return _FRAMES[key]


def _blob(name, rows, t=None, time=None):
    fields, step = LAYOUTS[name]
    cols = {"x": rows[:, 0], "y": rows[:, 1], "z": rows[:, 2], "label": rows[:, 3]}
    names = [f[0] for f in fields]
    if "t" in names:
        cols["t"] = t if t is not None else 0xDEADBEEF
    if "time" in names:
        cols["time"] = time if time is not None else np.nan
    return pc2ref.build_blob(fields, step, cols, len(rows))


def _on_device(blob, offset):
    """the blob in device memory at a base that is `offset` bytes past a 16-byte boundary"""
    big = torch.empty(len(blob) + 16, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    view = big[offset:offset + len(blob)]
    view.copy_(torch.from_numpy(blob))
    return view


def _same(ra, rb, a, b, what):
    assert np.array_equal(_bits(ra[0]), _bits(rb[0])), what
    assert ra[3] == rb[3], what
    for k in ("iterations", "converged", "n_queries", "n_corr_first", "n_corr_last"):
        assert getattr(ra[4], k) == getattr(rb[4], k), (what, k)
    assert np.array_equal(_bits(a.source()), _bits(b.source())), what


# every point survives the two down-sampling levels: source() then holds every row of the frame the crop keeps
FINE = dict(voxel_size=[0.001] * 6)


# ---- unpack ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,deskew", [(n, d) for n in sorted(LAYOUTS) for d in (False, True)
                                         if not d or any(f[0] in ("t", "time") for f in LAYOUTS[n][0])])
def test_unpacked_rows_and_stamps_are_the_host_rows(gpu_sage, name, deskew):
    """(deskew on needs a time field: the 13- and 16-byte records have no room for one)"""
    sage = gpu_sage
    fields, step = LAYOUTS[name]
    time_fields = [f[0] for f in fields if f[0] in ("t", "time")]
    base = _frames(4, 4099, seed=7)
    rng = np.random.default_rng(sum(name.encode()))
    a, b = sage.SageICP(sage.make_pipeline_config(deskew=deskew, **FINE)), sage.SageICP(sage.make_pipeline_config(deskew=deskew, **FINE))
    for f in base[:3]:                      # a map and three poses: the frames that follow are deskewed
        ts = rng.random(len(f))
        a.RegisterFrame(f, ts)
        b.RegisterFrame(f, ts)
    k = 0
    for n in SIZES:
        for place in ("host", 0, 1, 2, 3):
            rows = base[3][(np.arange(n) + 13 * k) % len(base[3])]
            k += 1
            tf = time_fields[k % len(time_fields)] if time_fields else None
            t = rng.integers(0, 100000, n, dtype=np.uint32)
            time = rng.random(n)
            blob = _blob(name, rows, t, time)
            want_rows = pc2ref.read_rows(blob, fields, step, n)
            assert np.array_equal(_bits(want_rows), _bits(rows))
            # with deskew off the time field is never read: whatever the layout says about it
            lay = _layout(sage, name, tf)
            data = blob if place == "host" else _on_device(blob, place)
            ra = a.RegisterFrameBytes(data, n, lay)
            if deskew:
                rb = b.RegisterFrame(want_rows, pc2ref.read_timestamps(blob, fields, step, n, tf))
                assert a.deskew_info()[0] and np.array_equal(_bits(a.deskew_info()[1]), _bits(b.deskew_info()[1]))
            else:
                rb = b.RegisterFrame(want_rows)
            _same(ra, rb, a, b, (n, place, tf))
            # the crop keeps every point of these frames between 5 and 100 m, and no two share a 0.5 mm voxel
            assert ra[3] >= 0.8 * np.count_nonzero((np.linalg.norm(rows[:, :3], axis=1) > 5.0) &
                                                   (np.linalg.norm(rows[:, :3], axis=1) < 100.0)), (n, place)
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["all_zero", "max_1", "epoch"])
@pytest.mark.parametrize("name", ["ref21", "65"])
def test_uint32_stamps_are_normalised_by_their_maximum(gpu_sage, name, case):
    sage = gpu_sage
    fields, step = LAYOUTS[name]
    base = _frames(5, 4099, seed=7)
    n = 4099                               # 16 workgroups and 3 records
    rng = np.random.default_rng(5)
    if case == "all_zero":
        t = np.zeros(n, dtype=np.uint32)            # the maximum is below 1: the stamps stay as cast
    elif case == "max_1":
        t = (rng.random(n) < 0.5).astype(np.uint32)
        t[100] = 1
    else:                                           # epoch-like values near 2^32, the maximum in the very last record
        t = (np.uint64(4294960000) + rng.integers(0, 7000, n).astype(np.uint64)).astype(np.uint32)
        t[-1] = 4294967295
        assert t[:-1].max() < t[-1]
    want_t = pc2ref.normalize_timestamps(t.astype(np.float64))
    if case == "all_zero":
        assert not want_t.any()
    if case == "epoch":
        assert want_t[-1] == 1.0 and want_t.min() > 0.99999
    cfg = dict(deskew=True, **FINE)
    a, b = sage.SageICP(sage.make_pipeline_config(**cfg)), sage.SageICP(sage.make_pipeline_config(**cfg))
    for f in base[:3]:
        ts = rng.random(len(f))
        a.RegisterFrame(f, ts)
        b.RegisterFrame(f, ts)
    for place, f in (("host", base[3]), (1, base[4])):
        blob = _blob(name, f, t)
        assert np.array_equal(pc2ref.read_timestamps(blob, fields, step, n, "t"), want_t)
        data = blob if place == "host" else _on_device(blob, place)
        ra = a.RegisterFrameBytes(data, n, _layout(sage, name, "t"))
        rb = b.RegisterFrame(f, want_t)
        assert a.deskew_info()[0]
        _same(ra, rb, a, b, (case, place))


@pytest.mark.gpu
def test_a_blob_one_byte_short_is_refused(gpu_sage):
    sage = gpu_sage
    f = _frames(4, 4099, seed=7)[0]
    blob = _blob("ref21", f)
    lay = _layout(sage, "ref21")
    for data in (blob[:-1], _on_device(blob, 0)[:-1]):
        p = sage.SageICP()
        with pytest.raises(sage.SageIcpError) as e:
            p.RegisterFrameBytes(data, len(f), lay)
        assert e.value.code == sage.ERR_INVALID and "n * point_step" in str(e.value)
        assert len(p.poses()) == 0 and p.source_size() == 0
    # host memory handed to the device entry is refused, not copied
    p = sage.SageICP()
    pinned = torch.from_numpy(blob.copy()).pin_memory()
    pose = np.empty(7)
    for ptr in (blob.ctypes.data, pinned.data_ptr()):
        rc = sage.lib().sageicp_pipeline_register_frame_msg_device(
            p._h, ptr, len(blob), len(f), ctypes.byref(lay), None, pose.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
            None, None, None, None)
        assert rc == sage.ERR_INVALID and "device memory" in sage.lib().sageicp_last_error().decode()
    assert len(p.poses()) == 0


@pytest.mark.gpu
def test_values_that_are_not_finite_meet_the_rules_of_host_rows(gpu_sage):
    sage = gpu_sage
    frames = _frames(4, 4099, seed=7)
    a, b = sage.SageICP(), sage.SageICP()
    for f in frames[:2]:
        a.RegisterFrame(f)
        b.RegisterFrame(f)
    # a NaN coordinate: Preprocess() drops the point, as it does in host rows
    f = frames[2].copy()
    f[17, 0] = np.nan
    f[4000, 2] = np.inf
    ra = a.RegisterFrameBytes(_blob("16", f), len(f), _layout(sage, "16"))
    rb = b.RegisterFrame(f)
    _same(ra, rb, a, b, "NaN coordinate")
    # a NaN label of a point the crop keeps: the whole call is refused, no pose pushed, as for host rows
    f = frames[3].copy()
    r = np.linalg.norm(f[:, :3], axis=1)
    f[int(np.flatnonzero((r > 10.0) & (r < 40.0))[0]), 3] = np.nan
    for call in (lambda: a.RegisterFrameBytes(_blob("16", f), len(f), _layout(sage, "16")),
                 lambda: a.RegisterFrameBytes(_on_device(_blob("16", f), 2), len(f), _layout(sage, "16")),
                 lambda: b.RegisterFrame(f)):
        with pytest.raises(sage.SageIcpError) as e:
            call()
        assert e.value.code == sage.ERR_INVALID
    assert len(a.poses()) == len(b.poses()) == 3 and a.source_size() == 0
    # with key frames on a coordinate that is not finite refuses the frame
    a.set_key_frames(True)
    f = frames[3].copy()
    f[5, 1] = np.nan
    with pytest.raises(sage.SageIcpError) as e:
        a.RegisterFrameBytes(_blob("16", f), len(f), _layout(sage, "16"))
    assert e.value.code == sage.ERR_INVALID and len(a.poses()) == 3
    # a float64 stamp that is not finite, deskew on: refused on the first frame
    c = sage.SageICP(sage.make_pipeline_config(deskew=True))
    time = np.random.default_rng(1).random(len(frames[0]))
    time[-1] = np.inf
    with pytest.raises(sage.SageIcpError) as e:
        c.RegisterFrameBytes(_blob("32", frames[0], None, time), len(frames[0]), _layout(sage, "32", "time"))
    assert e.value.code == sage.ERR_INVALID and "timestamp" in str(e.value) and len(c.poses()) == 0


# ---- stream parity -----------------------------------------------------------------------------------------------------
FIVE = [("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("label", 12, U8), ("rgb", 13, U32)]               # the node's own
SIX = [("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("intensity", 12, F32), ("label", 16, F32), ("t", 20, U32)]


def _message(sage, fields, step, rows, t=None, device=False):
    cols = {"x": rows[:, 0], "y": rows[:, 1], "z": rows[:, 2], "label": rows[:, 3]}
    if t is not None:
        cols["t"] = t
    blob = pc2ref.build_blob(fields, step, cols, len(rows))
    data = _on_device(blob, 0) if device else bytes(blob)
    return sage.PointCloud2([sage.PointField(*f) for f in fields], step, data, width=len(rows))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["plain", "deskew", "dynamic_filter", "key_frames", "all_on"])
def test_a_stream_of_messages_is_the_stream_of_host_rows(gpu_sage, mode):
    """all_on: deskew, the dynamic filter and key frames together, and a fourth pipeline fed the rows as a device frame
    (a tensor of rows and a tensor of the normalised stamps): every source meets the same keep-raw, deskew and filter"""
    sage = gpu_sage
    deskew, dyn, keys = mode in ("deskew", "all_on"), mode in ("dynamic_filter", "all_on"), mode in ("key_frames", "all_on")
    if dyn:
        from sage_icp_amd import synthetic_dynamic as sd
        frames = [np.ascontiguousarray(f, dtype=np.float64) for f in sd.make_dynamic_stream(21, 10, n=30000)[0]]
    else:
        frames = _frames(10)
    # the float32-rounded values: what a message can carry
    frames = [np.column_stack([f[:, :3].astype(np.float32).astype(np.float64), f[:, 3]]) for f in frames]
    cfg = dict(deskew=deskew, dynamic_vehicle_filter=dyn)
    # host message, device message, host rows; all_on: and a device frame
    pipes = [sage.SageICP(sage.make_pipeline_config(**cfg)) for _ in range(4 if mode == "all_on" else 3)]
    others = [p for p in pipes if p is not pipes[2]]
    if keys:
        for p in pipes:
            p.set_key_frames(True)
    fields, step = (SIX, 24) if deskew else (FIVE, 21)
    rng = np.random.default_rng(3)
    for k, f in enumerate(frames):
        t = rng.integers(0, 100000, len(f), dtype=np.uint32) if deskew else None
        ts = pc2ref.normalize_timestamps(t.astype(np.float64)) if deskew else None
        host, dev = _message(sage, fields, step, f, t), _message(sage, fields, step, f, t, device=True)
        ra, rb = pipes[0].RegisterFrame(host), pipes[1].RegisterFrame(dev)
        rc = pipes[2].RegisterFrame(f, ts) if deskew else pipes[2].RegisterFrame(f)
        _same(ra, rc, pipes[0], pipes[2], (k, "host message"))
        _same(rb, rc, pipes[1], pipes[2], (k, "device message"))
        if mode == "all_on":
            rd = pipes[3].RegisterFrame(torch.from_numpy(f).to(DEV), timestamps=torch.from_numpy(ts).to(DEV))
            _same(rd, rc, pipes[3], pipes[2], (k, "device frame"))
        if deskew:
            assert all(p.deskew_info()[0] == (k >= 3) for p in pipes), k
        if dyn:
            info = [p.dynamic_filter_info() for p in pipes]
            assert info[2]["vehicle_points"] > 0
            for key in ("vehicle_points", "landmark_points", "clusters", "clusters_kept", "points_removed"):
                assert all(i[key] == info[2][key] for i in info), (k, key)
        if keys:
            info = [p.key_frame_info() for p in pipes]
            for key in ("is_key_frame", "key_frame_index", "key_frames", "key_occupied", "intersect"):
                assert all(i[key] == info[2][key] for i in info), (k, key)
    for p in others:
        assert np.array_equal(_bits(p.poses()), _bits(pipes[2].poses()))
        assert np.array_equal(_bits(p.LocalMap()), _bits(pipes[2].LocalMap()))
    if keys:
        assert pipes[2].key_frame_info()["key_frames"] >= 1
        for p in others:
            assert np.array_equal(p.key_frame_grid(), pipes[2].key_frame_grid())


@pytest.mark.gpu
def test_a_message_frame_consumes_a_prefetch_announcement(gpu_sage):
    sage = gpu_sage
    frames = _frames(10)[:5]
    a, b = sage.SageICP(), sage.SageICP()
    for k, f in enumerate(frames):
        ra = a.RegisterFrame(f)
        if k in (1, 2):          # announced, then a message frame is registered: the announcement is dropped
            b.prefetch(frames[k + 1])
            rb = b.RegisterFrame(_message(sage, FIVE, 21, f, device=k == 2))
        else:
            rb = b.RegisterFrame(f)
        _same(ra, rb, a, b, k)
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))


# ---- pack ---------------------------------------------------------------------------------------------------------------
COLORS = {l: (l * 0x010305 + 7) if l % 3 else -(l * 977 + 1) for l in range(256)}      # every third one negative
COLORS.update({256: 1, 1000: 2, -1: 3, -40: 4})                                       # keys that can never match


def _registered(sage, n_frames=3, **cfg):
    p = sage.SageICP(sage.make_pipeline_config(**cfg))
    for f in _frames(10)[:n_frames]:
        p.RegisterFrame(f)
    return p


def _dev_out(nbytes, offset, fill=0xEE):
    big = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)
    assert big.data_ptr() % 16 == 0
    return big, big[offset:offset + nbytes]


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["source", "resident_map", "host_map", "reference_order_map"])
def test_packed_records_are_the_reference_packer_of_the_rows(gpu_sage, what):
    sage = gpu_sage
    if what == "reference_order_map":
        os.environ["SAGEICP_MAP_REFERENCE_ORDER"] = "1"
    try:
        p = _registered(sage, map_update_on_device=what != "host_map")
    finally:
        os.environ.pop("SAGEICP_MAP_REFERENCE_ORDER", None)
    if what == "source":
        rows, call = p.source(), p.source_msg
    else:
        rows, call = p.LocalMap(), p.LocalMapMsg
        h = sage.lib().sageicp_pipeline_local_map(p._h)
        assert bool(sage.lib().sageicp_map_resident(h)) == (what != "host_map")      # (a reference-order map is resident too)
        assert (sage.lib().sageicp_map_reference_order(h) == 1) == (what == "reference_order_map")
    n = len(rows)
    assert n > 1000
    want = pc2ref.pack(rows, COLORS)
    assert (want[:, 12] == rows[:, 3]).all() and (np.ascontiguousarray(want[:, 13:17]).view("<u4") >= 0x80000000).any()
    got = call(COLORS)
    assert got.dtype == np.uint8 and got.shape == (n, 21) and np.array_equal(got, want)
    d = call(COLORS, device=True)
    assert d.dtype == torch.uint8 and d.shape == (n, 21) and np.array_equal(d.cpu().numpy(), want)
    for offset in (0, 1, 4):              # 16-byte stores, byte stores, dword stores
        big, out = _dev_out(n * 21, offset)
        r = call(COLORS, out=out)
        assert r.shape == (n, 21) and r.data_ptr() == out.data_ptr()
        assert np.array_equal(out.cpu().numpy().reshape(n, 21), want), offset
        assert (big[:offset] == 0xEE).all() and (big[offset + n * 21:] == 0xEE).all(), offset
    # cap: exactly min(cap, n) records, not a byte beyond them
    for cap in (0, 1, 255, 256, 257, n, n + 5):
        k = min(cap, n)
        for offset in (0, 1):
            big, out = _dev_out(cap * 21, offset)
            r = call(COLORS, out=out)
            assert r.shape == (k, 21), (cap, offset)
            flat = big.cpu().numpy()
            assert np.array_equal(flat[offset:offset + k * 21].reshape(k, 21), want[:k]), (cap, offset)
            assert (flat[:offset] == 0xEE).all() and (flat[offset + k * 21:] == 0xEE).all(), (cap, offset)
        host = np.full(cap * 21 + 32, 0xEE, dtype=np.uint8)
        r = call(COLORS, out=host[:cap * 21])
        assert r.shape == (k, 21) and np.array_equal(r, want[:k]), cap
        assert (host[k * 21:] == 0xEE).all(), cap
    # the rows are where they were
    assert np.array_equal(_bits(p.source() if what == "source" else p.LocalMap()), _bits(rows))


@pytest.mark.gpu
def test_label_and_colour_rules(gpu_sage):
    sage = gpu_sage
    pts = np.array([[1.5, 2.5, 3.5, 255.0], [10.25, -4.0, 0.5, -0.5], [20.0, 7.0, 1.0, 40.9], [-30.0, 3.0, 2.0, 7.0]])
    m = sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints(pts)
    rows = m.Pointcloud()
    assert sorted(rows[:, 3]) == [-0.5, 7.0, 40.9, 255.0]
    colors = {255: 0x00FF00FF, 0: -1, 40: -2147483648, 7: 0x7FFFFFFF, 300: 9, 256: 8, -1: 5}
    want = pc2ref.pack(rows, colors)
    for got in (m.PointcloudMsg(colors), m.PointcloudMsg(colors, device=True).cpu().numpy()):
        assert np.array_equal(got, want)
    by_label = {int(r[12]): r for r in want}
    assert sorted(by_label) == [0, 7, 40, 255]                                  # -0.5 gives 0, 40.9 gives 40
    assert by_label[0][13:17].tobytes() == b"\xff\xff\xff\xff"                  # a negative colour wraps to uint32
    assert by_label[40][13:17].tobytes() == b"\x00\x00\x00\x80"
    assert by_label[255][13:17].tobytes() == b"\xff\x00\xff\x00" and not want[:, 17:].any()
    # a label without a colour: the reference's .at throws
    for missing in (255, 0, 40):
        c = {k: v for k, v in colors.items() if k != missing}
        with pytest.raises(KeyError):
            pc2ref.pack(rows, c)
        for kw in (dict(), dict(device=True)):
            with pytest.raises(sage.SageIcpError) as e:
                m.PointcloudMsg(c, **kw)
            assert e.value.code == sage.ERR_INVALID and "colour" in str(e.value)
    # keys above 255 never match: label 256 is out of the record's range whatever the table says
    m256 = sage.VoxelHashMap(1.0, 100.0)
    m256.AddPoints(np.array([[1.0, 1.0, 1.0, 256.0], [2.0, 2.0, 2.0, 7.0]]))
    m_neg = sage.VoxelHashMap(1.0, 100.0)
    m_neg.AddPoints(np.array([[1.0, 1.0, 1.0, -1.0]]))
    for bad in (m256, m_neg):
        with pytest.raises(ValueError):
            pc2ref.pack(bad.Pointcloud(), colors)
        for kw in (dict(), dict(device=True)):
            with pytest.raises(sage.SageIcpError) as e:
                bad.PointcloudMsg(colors, **kw)
            assert e.value.code == sage.ERR_INVALID and "label" in str(e.value)
    # after a refusal the next call works
    assert np.array_equal(m.PointcloudMsg(colors), want)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["source", "local_map"])
def test_the_records_follow_the_callers_stream(gpu_sage, what):
    p = _registered(gpu_sage)
    rows = p.source() if what == "source" else p.LocalMap()
    call = p.source_msg if what == "source" else p.LocalMapMsg
    want = pc2ref.pack(rows, COLORS)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        out = torch.empty((len(rows), 21), dtype=torch.uint8, device=DEV)
        torch.cuda._sleep(200_000_000)
        out.fill_(0xEE)                       # lands only after the delay: the records must land after it
        got = call(COLORS, out=out)
        snap = got.clone()                    # the call is synchronous: the records are in place now
        out.fill_(0xEE)
    torch.cuda.synchronize()
    assert np.array_equal(snap.cpu().numpy(), want)


@pytest.mark.gpu
def test_host_memory_given_to_a_device_entry_is_refused(gpu_sage):
    sage = gpu_sage
    p = _registered(sage, 2)
    n = p.source_size()
    L = sage.lib()
    h = L.sageicp_pipeline_local_map(p._h)
    c = sage._msg_colors(COLORS)
    host = np.full(n * 21, 5, dtype=np.uint8)
    pinned = torch.full((n * 21,), 5, dtype=torch.uint8).pin_memory()
    k = ctypes.c_uint64(0)
    for ptr in (host.ctypes.data, pinned.data_ptr()):
        assert L.sageicp_pipeline_source_msg_device(p._h, ctypes.byref(c), ptr, n, None, ctypes.byref(k)) == sage.ERR_INVALID
        assert "device memory" in L.sageicp_last_error().decode()
        assert L.sageicp_map_pointcloud_msg_device(h, ctypes.byref(c), ptr, n, None, ctypes.byref(k)) == sage.ERR_INVALID
        assert "device memory" in L.sageicp_last_error().decode()
    assert (host == 5).all() and (pinned == 5).all()
    with pytest.raises(ValueError):
        p.source_msg(COLORS, out=torch.empty(n * 21, dtype=torch.uint8))
    with pytest.raises(ValueError):
        p.LocalMapMsg(COLORS, out=torch.empty((n, 21), dtype=torch.float32, device=DEV))


# ---- round trip --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_source_records_fed_back_in_register_the_float32_rounded_source(gpu_sage, device):
    sage = gpu_sage
    p = _registered(sage)
    src = p.source()
    msg = sage.output_pointcloud2(p.source_msg(COLORS, device=device))
    assert len(msg.fields) == 5 and msg.width == len(src)
    a, b = sage.SageICP(sage.make_pipeline_config(**FINE)), sage.SageICP(sage.make_pipeline_config(**FINE))
    rounded = np.column_stack([src[:, :3].astype(np.float32).astype(np.float64), src[:, 3]])
    ra, rb = a.RegisterFrame(msg), b.RegisterFrame(rounded)
    _same(ra, rb, a, b, "round trip")
    # on an empty map nothing moves the rows: what was registered is the rounded source, point for point
    got = a.source()
    assert len(got) >= 0.9 * len(rounded)
    assert {r.tobytes() for r in got} <= {r.tobytes() for r in rounded}
