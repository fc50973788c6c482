"""The archive of a map on the GPU (include/sageicp.h "the archive of a map"): what a device-side update
evicts, appended by archive.hip's kernels, against the plain restatement (tests/archiveref.py), the oracle (reference-order
mode) and the host path's bytes; the LATEST / SESSION selections and the sinks of an export.  Every comparison is on bytes."""
import contextlib
import ctypes
import gc
import os

import numpy as np
import pytest

import archiveref as ar
import pc2ref
from test_archive_host import _map, _ref, oracle_log, reference_order_stream

pytestmark = pytest.mark.gpu

try:
    import torch
    DEV = torch.device("cuda", 0)
except ImportError:          # (collected without torch on a CPU box: every test here is marked gpu)
    torch = None

COLORS = {71: 0x112233, 0: 0x445566, 40: 0x0A0B0C, 48: 1, 50: 2, 70: 3, 80: 4, 10: 5}


def _run(sage, entry, steps, m=None, ref=None, check=True, **over):
    if m is None:
        m = _map(sage, **{k: v for k, v in over.items() if k != "max_rows"}).set_archive(True, over.get("max_rows", 0))
    ref = ref if ref is not None else _ref(**over)
    for k, (pts, origin) in enumerate(steps):
        ar.apply_step(m, entry, pts, origin)
        ar.ref_step(ref, pts, origin)
        if check:
            ar.assert_equal_to_ref(m, ref, "%s step %d" % (entry, k))
    return m, ref


@contextlib.contextmanager
def _managed(nbytes):
    """nbytes of managed memory (hipMallocManaged of the HIP runtime the process has loaded), every byte 0x55; freed on
    the way out.  Only the host touches it here: the entries under test refuse it before any device work."""
    hip = ctypes.CDLL(None)
    hip.hipMallocManaged.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_uint]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    p = ctypes.c_void_p()
    assert hip.hipMallocManaged(ctypes.byref(p), nbytes, 1) == 0 and p.value      # 1: hipMemAttachGlobal
    try:
        ctypes.memset(p.value, 0x55, nbytes)
        yield p.value
    finally:
        assert hip.hipFree(p) == 0


def _state(m):
    st = m.loop_status()
    return m.resident(), m.table_stats(), tuple(getattr(st, f) for f, _ in st._fields_)


# ---- the device append ---------------------------------------------------------------------------------------------------
def test_walk_through_the_device_update_equals_the_restatement_and_the_host_path(gpu_sage):
    sage = gpu_sage
    m = _map(sage).set_archive(True)
    assert m.archive_info()["device_bytes"] == 0           # the first eviction goes into an archive without a buffer
    m, ref = _run(sage, "device", ar.walk(), m=m)
    h, _ = _run(sage, "update_pose", ar.walk(), check=False)
    assert m.resident() and not h.resident()
    assert m.ArchivedPointcloud("all").tobytes() == h.ArchivedPointcloud("all").tobytes()
    assert np.asarray(m.archive_voxels()).tobytes() == np.asarray(h.archive_voxels()).tobytes()
    assert m.Pointcloud().tobytes() == h.Pointcloud().tobytes() == ref.pointcloud().tobytes()
    info = m.archive_info()
    assert info["device_rows"] == info["rows"] > 100 and info["host_rows"] == 0 and info["device_bytes"] >= 32 * info["rows"]
    # the same sequence again: the same bytes
    m2, _ = _run(sage, "device", ar.walk(), check=False)
    assert m2.ArchivedPointcloud("all").tobytes() == m.ArchivedPointcloud("all").tobytes()
    assert np.asarray(m2.archive_voxels()).tobytes() == np.asarray(m.archive_voxels()).tobytes()
    assert m2.archive_info() == info


def test_reference_order_mode_on_the_device_against_the_oracle(gpu_sage, oracle):
    sage = gpu_sage
    oracle.set_robin_order(3)
    try:
        stream = reference_order_stream(frames=11, n=1000, grid=1024)         # (on a grid: rows in the sensor frame + the translation is exact)
        calls, final = oracle_log(oracle, stream)
    finally:
        oracle.set_robin_order(False)
    m = sage.VoxelHashMap(1.0, 40.0, 5, 5, [40, 48, 50]).set_reference_order(True).set_archive(True)
    h = sage.VoxelHashMap(1.0, 40.0, 5, 5, [40, 48, 50]).set_reference_order(True).set_archive(True)
    log = []
    for k, (pts, centre) in enumerate(stream):
        m.UpdateOnDevice(ar.sensor_rows(pts, centre), ar.pose_of(centre))
        h.Update(ar.sensor_rows(pts, centre), ar.pose_of(centre))
        log += [(key, rows, k) for key, rows in calls[k]]
        assert m.ArchivedPointcloud("all").tobytes() == ar.rows_of(log).tobytes(), "call %d" % k
        assert np.asarray(m.archive_voxels()).tobytes() == ar.records_of(log).tobytes(), "call %d" % k
    assert m.resident() and np.array_equal(m.Pointcloud(), final)
    assert m.ArchivedPointcloud("all").tobytes() == h.ArchivedPointcloud("all").tobytes()
    mi, hi = m.archive_info(), h.archive_info()
    assert {k: mi[k] for k in ("rows", "voxels", "updates", "full")} == {k: hi[k] for k in ("rows", "voxels", "updates", "full")}
    # SESSION: the tail is Pointcloud() in bucket order
    live = ar.keys_of(final, 1.0)
    want = ar.session(log, live, final)
    assert m.ArchivedPointcloud("session").tobytes() == want.tobytes()


def _line(n, x0=0.0):
    """n one-row voxels along y at x0"""
    p = np.zeros((n, 4))
    p[:, 0] = x0 + 0.5
    p[:, 1] = np.arange(n) + 0.5
    p[:, 2] = 0.5
    p[:, 3] = 71.0
    return p


@pytest.mark.parametrize("n", [255, 256, 257])
def test_one_update_evicts_n_one_row_voxels_and_then_every_voxel(gpu_sage, n):
    """the workgroup edge of the counts kernel and the second tile of the scan; then an update that evicts all there is"""
    sage = gpu_sage
    P = dict(ar.PARAMS, max_distance=1000.0)
    m = sage.VoxelHashMap(P["voxel_size"], P["max_distance"], 20, 20, [40]).set_archive(True)
    ref = ar.ArchiveRef(**dict(P, basic_labels=(40,)))
    steps = [(np.concatenate([_line(n, 3000.0), _line(40, 0.0)]), (0.5, 0.5, 0.5)),       # the far line goes as it arrives
             (ar.walk()[1][0], (0.5, 0.5, 0.5)),
             (np.zeros((0, 4)), (-5000.0, 0.5, 0.5))]                                     # every voxel
    for k, (pts, origin) in enumerate(steps):
        ar.apply_step(m, "device", pts, origin)
        ar.ref_step(ref, pts, origin)
        ar.assert_equal_to_ref(m, ref, "step %d" % k)
    assert ref.evicted_by_call[0] == n and m.num_voxels() == 0 and ref.evicted_by_call[2] > 40


@pytest.mark.parametrize("blocks", [1173, 1174, 1175, 1176])
def test_an_update_whose_block_bound_meets_the_scratch_capacity(gpu_sage, blocks):
    """The append scans bound + 1 counts (bound = blocks so far + n) in scratch the update keeps from frame to frame; the
    scratch grows to nb + nb / 2 + 1024 entries when a frame needs nb.  After a first update of 100 one-row voxels it holds
    1175 entries (1174, had the extra entry been forgotten): the second update's bound is walked over those sizes, evicts
    every voxel, and the log must be the restatement's — the first selected block included."""
    sage = gpu_sage
    P = dict(ar.PARAMS, max_distance=1000.0, basic_labels=(40,))
    m = sage.VoxelHashMap(1.0, 1000.0, 20, 20, [40]).set_archive(True)
    ref = ar.ArchiveRef(**P)
    steps = [(_line(100, 0.0), (0.5, 0.5, 0.5)),
             (_line(blocks - 100, 2.0), (-5000.0, 0.5, 0.5))]
    for k, (pts, origin) in enumerate(steps):
        ar.apply_step(m, "device", pts, origin)
        ar.ref_step(ref, pts, origin)
        ar.assert_equal_to_ref(m, ref, "step %d" % k)
    assert ref.evicted_by_call == [0, blocks] and m.num_voxels() == 0


def test_reallocations_keep_the_contents(gpu_sage):
    sage = gpu_sage
    rng = np.random.default_rng(8)
    steps = []
    for f in range(24):
        pts = np.zeros((400, 4))
        pts[:, 0] = 6 * f + rng.integers(0, 6 * 64, size=400) / 64.0
        pts[:, 1] = rng.integers(0, 8 * 64, size=400) / 64.0
        pts[:, 2] = rng.integers(0, 64, size=400) / 64.0
        pts[:, 3] = 71.0
        steps.append((pts, (6.0 * f + 3.0, 4.0, 0.5)))
    big, ref = _run(sage, "device", steps, check=False, max_distance=9.0)
    os.environ["SAGEICP_ARCHIVE_INITIAL_ROWS"] = "64"
    try:
        m = _map(sage, max_distance=9.0).set_archive(True)
        caps = set()
        for pts, origin in steps:
            ar.apply_step(m, "device", pts, origin)
            caps.add(m.archive_info()["device_bytes"])
    finally:
        del os.environ["SAGEICP_ARCHIVE_INITIAL_ROWS"]
    assert len(caps) >= 4, "the buffer was meant to be re-allocated several times"
    assert m.archive_info()["rows"] > 3000
    ar.assert_equal_to_ref(m, ref)
    assert m.ArchivedPointcloud("all").tobytes() == big.ArchivedPointcloud("all").tobytes()
    assert np.asarray(m.archive_voxels()).tobytes() == np.asarray(big.archive_voxels()).tobytes()


@pytest.mark.parametrize("short", [0, 1], ids=["at_a_voxel_end", "one_row_short"])
def test_limit_cuts_inside_one_device_update(gpu_sage, short):
    sage = gpu_sage
    full = _ref()
    for pts, origin in ar.walk():
        ar.ref_step(full, pts, origin)
    # a voxel in the middle of a call that evicts several, of more than one row
    at, ends = 0, []
    for _, rows, serial in full.log:
        at += len(rows)
        ends.append((at, serial, len(rows)))
    j = next(i for i in range(1, len(ends) - 1) if ends[i][1] == ends[i - 1][1] == ends[i + 1][1] and ends[i][2] > 1 and i > 8)
    max_rows = ends[j][0] - short
    m, ref = _run(sage, "device", ar.walk(), max_rows=max_rows)
    info = m.archive_info()
    assert info["full"] == 1 and info["rows"] == (ends[j][0] if not short else ends[j - 1][0])
    assert info["rows"] + info["dropped_rows"] == full.rows_held() and info["voxels"] + info["dropped_voxels"] == len(full.log)
    assert m.ArchivedPointcloud("all").tobytes() == ar.rows_of(ar.limited(full.log, max_rows)).tobytes()


def test_host_and_device_evictions_interleave_into_one_log(gpu_sage):
    sage = gpu_sage
    steps = ar.walk()
    m, ref = _map(sage).set_archive(True), _ref()
    _run(sage, "update", steps[:4], m=m, ref=ref)                 # on the host copy of a map that is not resident
    i = m.archive_info()
    assert not m.resident() and i["host_rows"] == i["rows"] > 0 and i["device_rows"] == 0
    _run(sage, "device", steps[4:7], m=m, ref=ref)                # the pending tail goes up behind nothing, then the device appends
    i = m.archive_info()
    assert m.resident() and i["host_rows"] == 0 and i["device_rows"] == i["rows"]
    held = i["rows"]
    _run(sage, "remove_far", steps[7:9], m=m, ref=ref)            # downloads the map; the archive stays where it is
    i = m.archive_info()
    assert not m.resident() and i["device_rows"] == held and i["host_rows"] == i["rows"] - held > 0
    _run(sage, "device", steps[9:], m=m, ref=ref)
    i = m.archive_info()
    assert i["host_rows"] == 0 and i["device_rows"] == i["rows"] == ref.rows_held()


def test_a_refused_device_update_leaves_the_archive_unchanged(gpu_sage):
    sage = gpu_sage
    m, ref = _run(sage, "device", ar.walk()[:5])
    info, rows, rec = m.archive_info(), m.ArchivedPointcloud("all").tobytes(), np.asarray(m.archive_voxels()).tobytes()
    far = ar.pose_of((900.0, 0.0, 0.0))          # would evict everything
    bad = [np.array([[1.5, 0.5, 0.5, 71.0], [np.nan, 0.0, 0.0, 0.0]]), np.array([[1.5, 0.5, 0.5, 71.0], [3.0e6, 0.0, 0.0, 0.0]])]
    for pts, code in zip(bad, (sage.ERR_INVALID, sage.ERR_CAPACITY)):
        with pytest.raises(sage.SageIcpError) as e:
            m.UpdateOnDevice(pts, far)
        assert e.value.code == code
        assert m.archive_info() == info
        assert m.ArchivedPointcloud("all").tobytes() == rows and np.asarray(m.archive_voxels()).tobytes() == rec
    _run(sage, "device", ar.walk()[5:8], m=m, ref=ref)


# ---- LATEST and SESSION ------------------------------------------------------------------------------------------------
def _check_selections(m, ref):
    before = _state(m)
    pc = m.Pointcloud()
    live = ar.keys_of(pc, ref.vs)
    want_latest = ar.rows_of(ar.latest(ref.log, live))
    assert m.ArchivedPointcloud("latest").tobytes() == want_latest.tobytes()
    got = m.ArchivedPointcloud("session")
    assert got.tobytes() == ar.session(ref.log, live, pc).tobytes()
    keys = ar.keys_of(got, ref.vs)
    runs = [k for i, k in enumerate(keys) if i == 0 or keys[i - 1] != k]
    assert len(runs) == len(set(runs)), "a key appears twice in the session's map"
    assert _state(m) == before
    return want_latest


@pytest.mark.parametrize("entry", ["device", "update"], ids=["resident", "host"])
def test_latest_and_session_against_the_restatement(gpu_sage, entry):
    sage = gpu_sage
    steps = ar.walk()
    m = _map(sage).set_archive(True)
    ref = _ref()
    assert m.ArchivedPointcloud("session").shape == (0, 4)
    _run(sage, entry, steps[:2], m=m, ref=ref)                    # an empty archive: SESSION is Pointcloud()
    assert ref.rows_held() == 0
    assert m.ArchivedPointcloud("session").tobytes() == m.Pointcloud().tobytes() and len(m.ArchivedPointcloud("latest")) == 0
    for k in range(2, len(steps)):
        _run(sage, entry, steps[k:k + 1], m=m, ref=ref, check=False)
        _check_selections(m, ref)
    # two archived generations of a key, a key archived and live again, a key archived once: all in the walk
    keys = [k for k, _, _ in ref.log]
    live = set(ar.keys_of(m.Pointcloud(), 1.0))
    assert any(keys.count(k) > 1 for k in keys) and any(k in live for k in keys) and any(keys.count(k) == 1 for k in keys)
    m.Clear()                                                    # an empty map: SESSION is LATEST, nothing is live
    ref2 = ar.rows_of(ar.latest(ref.log, []))
    assert m.ArchivedPointcloud("session").tobytes() == m.ArchivedPointcloud("latest").tobytes() == ref2.tobytes()
    assert m.archive_info()["rows"] == ref.rows_held()


def test_257_keys_and_257_generations_of_one_key(gpu_sage):
    sage = gpu_sage
    P = dict(ar.PARAMS, max_distance=1000.0, basic_labels=(40,))
    m = sage.VoxelHashMap(1.0, 1000.0, 20, 20, [40]).set_archive(True)
    ref = ar.ArchiveRef(**P)
    _run(sage, "device", [(_line(257, 3000.0), (0.5, 0.5, 0.5))], m=m, ref=ref)
    _check_selections(m, ref)
    for g in range(257):                                           # one far voxel, born and evicted 257 times
        p = np.array([[5000.25, 0.5, 0.5, 71.0], [5000.5, 0.5 + g / 1024.0, 0.5, 71.0]])
        _run(sage, "device", [(p, (0.5, 0.5, 0.5))], m=m, ref=ref, check=False)
    ar.assert_equal_to_ref(m, ref)
    latest = _check_selections(m, ref)
    assert len(latest) == 257 + 2 and m.archive_info()["voxels"] == 514


def test_latest_and_session_exports_beyond_one_stride_of_the_gather(gpu_sage):
    """The gathers launch 2048 x 256 lanes, a lane per row, and stride over the rest: an export of 538,240 rows takes a
    second trip for its last 13,952.  ALL is a plain copy of the log, so LATEST is built from it with numpy: the log without
    the superseded records, in log order.  300 voxels have a second generation, so the selection is not the identity."""
    sage = gpu_sage
    rows, again = ar.big_sheet()
    voxels = ar.BIG_SIDE * ar.BIG_SIDE
    assert len(rows) == voxels * ar.BIG_COUNT == 538240 > ar.GATHER_STRIDE == 524288 and len(again) == 300 * 40
    m = _map(sage, max_distance=ar.BIG_MAX_DISTANCE).set_archive(True)
    for pts, origin in ar.big_sheet_steps():
        ar.apply_step(m, "device", pts, origin)
    info = m.archive_info()
    assert m.resident() and m.num_voxels() == 0 and info["full"] == 0
    assert info["device_rows"] == info["rows"] == len(rows) + len(again) and info["voxels"] == voxels + ar.BIG_AGAIN
    log = m.ArchivedPointcloud("all")
    rec = np.asarray(m.archive_voxels())
    assert (rec["count"] == ar.BIG_COUNT).all() and np.array_equal(rec["first_row"], ar.BIG_COUNT * np.arange(len(rec)))
    assert (rec["update"][:voxels] == 1).all() and (rec["update"][voxels:] == 3).all()
    # the log itself (one update evicted 538,240 rows: the append's gather strides too): per voxel the rows offered, the
    # first generation before the second
    assert ar.by_voxel(log).tobytes() == ar.by_voxel(np.concatenate([rows, again])).tobytes()
    key = (rec["x"].astype(np.int64) * ar.BIG_SIDE + rec["y"]) * 2 + rec["z"]
    assert rec["z"].min() == rec["z"].max() == 0 and len(np.unique(key)) == voxels
    kept = np.ones(len(rec), dtype=bool)
    kept[:voxels] = ~np.isin(key[:voxels], key[voxels:])             # superseded: a later record has the key (nothing is live)
    assert (~kept).sum() == ar.BIG_AGAIN and np.flatnonzero(~kept)[0] < voxels // 10
    want = log[np.repeat(kept, rec["count"])]
    got = m.ArchivedPointcloud("latest")
    assert len(got) == len(want) == len(rows)
    assert got.tobytes() == want.tobytes()
    tail = len(got) - ar.GATHER_STRIDE
    assert tail == 13952 and got[-tail:].tobytes() == want[-tail:].tobytes()         # what the second trip writes
    assert want[-tail:].tobytes() != log[ar.GATHER_STRIDE:len(got)].tobytes()        # ... and not from the same log position
    # per voxel, the rows offered last
    born_again = np.isin(ar.by_voxel(rows)[:, :2].astype(np.int64) @ [ar.BIG_SIDE, 1], (key[voxels:] // 2))
    final = np.concatenate([ar.by_voxel(rows)[~born_again], again])
    assert len(final) == len(rows) and ar.by_voxel(got).tobytes() == ar.by_voxel(final).tobytes()
    # SESSION: nothing is live, so it is LATEST; through the device sink the same bytes
    assert m.Pointcloud().shape == (0, 4) and m.ArchivedPointcloud("session").tobytes() == want.tobytes()
    assert m.ArchivedPointcloud("latest", device=True).cpu().numpy().tobytes() == want.tobytes()
    assert m.ArchivedPointcloud("latest", first=ar.GATHER_STRIDE - 5).tobytes() == want[ar.GATHER_STRIDE - 5:].tobytes()


# ---- sinks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "latest", "session"])
def test_sinks_of_an_export(gpu_sage, which):
    sage = gpu_sage
    m, ref = _run(sage, "device", ar.walk()[:9], check=False)
    host = m.ArchivedPointcloud(which)
    n = len(host)
    assert n > 50
    d = m.ArchivedPointcloud(which, device=True)
    assert d.dtype == torch.float64 and d.cpu().numpy().tobytes() == host.tobytes()
    d32 = m.ArchivedPointcloud(which, device=True, dtype=torch.float32)
    assert np.array_equal(d32.cpu().numpy().view(np.uint32), host.astype(np.float32).view(np.uint32))
    for ldt, npdt in ((torch.uint8, np.uint8), (torch.int32, np.int32), (torch.int64, np.int64)):
        o, l = m.ArchivedPointcloud(which, out=torch.empty((n, 3), dtype=torch.float32, device=DEV),
                                    labels_out=torch.empty(n, dtype=ldt, device=DEV))
        assert np.array_equal(o.cpu().numpy(), host[:, :3].astype(np.float32)) and np.array_equal(l.cpu().numpy(), host[:, 3].astype(npdt))
    # the label apart as float32 (the C entry: the binding's tensors take the integer types)
    xyz = torch.empty((n, 3), dtype=torch.float64, device=DEV)
    lab = torch.empty(n, dtype=torch.float32, device=DEV)
    dp = sage.DevicePoints(xyz.data_ptr(), 24, sage.DTYPE_FLOAT64, sage.DTYPE_FLOAT32, lab.data_ptr(), 4, n)
    k = ctypes.c_uint64(0)
    torch.cuda.synchronize()
    assert sage.lib().sageicp_map_archive_rows_device(m._h, sage.ARCHIVE_WHICH[which], 0, ctypes.byref(dp), None, ctypes.byref(k)) == 0
    assert k.value == n and xyz.cpu().numpy().tobytes() == np.ascontiguousarray(host[:, :3]).tobytes()
    assert np.array_equal(lab.cpu().numpy(), host[:, 3].astype(np.float32))
    # ranges: first in a voxel's middle, a short destination, first at and past the end
    for first in (0, 3, n, n + 4):
        assert m.ArchivedPointcloud(which, first=first).tobytes() == host[first:].tobytes()
        out = torch.full((5, 4), -3.0, dtype=torch.float64, device=DEV)
        got = m.ArchivedPointcloud(which, first=first, out=out)
        k = min(5, max(0, n - first))
        assert len(got) == k and got.cpu().numpy().tobytes() == host[first:first + k].tobytes()
        assert (out[k:] == -3.0).all()
    # records, host and device, under a colour table
    rec = m.ArchivedPointcloudMsg(COLORS, which)
    assert rec.shape == (n, 21)
    assert np.array_equal(rec, pc2ref.pack(host, COLORS))
    drec = m.ArchivedPointcloudMsg(COLORS, which, device=True)
    assert np.array_equal(drec.cpu().numpy(), rec)
    part = m.ArchivedPointcloudMsg(COLORS, which, first=7, out=np.zeros((4, 21), dtype=np.uint8))
    assert np.array_equal(part, rec[7:11])
    dpart = m.ArchivedPointcloudMsg(COLORS, which, first=7, out=torch.zeros((4, 21), dtype=torch.uint8, device=DEV))
    assert np.array_equal(dpart.cpu().numpy(), rec[7:11])
    with pytest.raises(sage.SageIcpError) as e:                     # a missing colour
        m.ArchivedPointcloudMsg({0: 1}, which)
    assert e.value.code == sage.ERR_INVALID
    # host, pinned and managed destinations are refused, by the rows entry and by the records entry, and left untouched
    L = sage.lib()
    k = ctypes.c_uint64(0)
    w = sage.ARCHIVE_WHICH[which]
    colors = sage._msg_colors(COLORS)
    hostbuf = np.full((n, 4), 5.0)
    pinned = torch.full((n, 4), 5.0, dtype=torch.float64).pin_memory()
    with _managed(32 * n) as managed:
        for ptr in (hostbuf.ctypes.data, pinned.data_ptr(), managed):
            dp = sage.DevicePoints(ptr, 32, sage.DTYPE_FLOAT64, 0, None, 0, n)
            assert L.sageicp_map_archive_rows_device(m._h, w, 0, ctypes.byref(dp), None, ctypes.byref(k)) == sage.ERR_INVALID
            assert "device memory" in L.sageicp_last_error().decode()
            assert L.sageicp_map_archive_msg_device(m._h, w, 0, ctypes.byref(colors), ptr, n, None, ctypes.byref(k)) == sage.ERR_INVALID
            assert "device memory" in L.sageicp_last_error().decode()
        assert ctypes.string_at(managed, 32 * n) == b"\x55" * (32 * n)
    assert (hostbuf == 5.0).all() and (pinned == 5.0).all()


def test_a_label_that_does_not_fit_is_refused(gpu_sage):
    sage = gpu_sage
    m = sage.VoxelHashMap(1.0, 3.0, 20, 20, [40]).set_archive(True)
    m.UpdateOnDevice(np.array([[50.5, 0.5, 0.5, 300.0], [0.5, 0.5, 0.5, 71.0]]), ar.pose_of((0.5, 0.5, 0.5)))
    assert m.archive_info()["rows"] == 1
    with pytest.raises(sage.SageIcpError) as e:
        m.ArchivedPointcloud("all", out=torch.empty((1, 3), dtype=torch.float32, device=DEV),
                             labels_out=torch.empty(1, dtype=torch.uint8, device=DEV))
    assert e.value.code == sage.ERR_INVALID
    with pytest.raises(sage.SageIcpError) as e:
        m.ArchivedPointcloudMsg({300: 1, 71: 2}, "session")
    assert e.value.code == sage.ERR_INVALID


# ---- the pipeline --------------------------------------------------------------------------------------------------------
FIVE = [("x", 0, 7), ("y", 4, 7), ("z", 8, 7), ("label", 12, 2), ("rgb", 13, 6)]      # the node's own fields (FLOAT32, UINT8, UINT32)


def _as(sage, form, f):
    """a frame as host rows, as a device frame (a tensor on the GPU), or as a PointCloud2 message"""
    if form == "device":
        return torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64)).to(DEV)
    if form == "msg":
        cols = {"x": f[:, 0], "y": f[:, 1], "z": f[:, 2], "label": f[:, 3]}
        blob = pc2ref.build_blob(FIVE, 17, cols, len(f))
        return sage.PointCloud2([sage.PointField(*fld) for fld in FIVE], 17, bytes(blob), width=len(f))
    return f


def _pipeline_run(sage, frames, on_device, archive, check=None, form="rows"):
    cfg = sage.make_pipeline_config(max_range=30.0, local_map_range=30.0, map_update_on_device=on_device)
    p = sage.SageICP(cfg)
    if archive:
        p.set_archive(True)
    seen = 0
    for k, f in enumerate(frames):
        pose = p.RegisterFrame(_as(sage, form, f))[0]
        if check and archive:
            seen = check(p, np.asarray(pose), seen, k)
    return p


def _frames():
    from sage_icp_amd import synthetic as syn
    return syn.make_stream(21, 30, points_per_frame=3000, step=(2.5, 0.0, 0.0), max_range=30.0)[0]


def _voxel_keys(rows, voxel_size):
    """the voxel of every row (fp64 divide, truncation toward zero), as an (n, 3) integer array"""
    return np.trunc(np.asarray(rows)[:, :3] / voxel_size).astype(np.int64)


def _frame_checks():
    """after every frame: each newly archived voxel's first row lies farther than local_map_range from the pose's
    translation, no newly archived key is live in LocalMap(), and SESSION's keys are distinct"""
    def check(p, pose, seen, k):
        rec = p.archive_voxels()
        if len(rec) > seen:
            rows = p.SessionMap("all")
            new = rec[seen:]
            d = rows[new.first_row.astype(np.int64)][:, :3] - pose[4:7]
            assert ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] > 30.0 * 30.0 * (1 - 1e-12)).all(), k
            live = set(map(tuple, _voxel_keys(p.LocalMap(), 0.8).tolist()))
            assert not any((int(r.x), int(r.y), int(r.z)) in live for r in new), k
        keys = _voxel_keys(p.SessionMap(), 0.8)
        runs = keys[np.concatenate([[True], (keys[1:] != keys[:-1]).any(axis=1)])] if len(keys) else keys
        assert len(np.unique(runs, axis=0)) == len(runs), "frame %d: a key appears twice in the session's map" % k
        return len(rec)
    return check


def test_pipeline_archives_what_its_frames_evict(gpu_sage):
    sage = gpu_sage
    frames = _frames()
    a = _pipeline_run(sage, frames, True, True, _frame_checks())
    b = _pipeline_run(sage, frames, False, True)
    c = _pipeline_run(sage, frames, True, False)
    assert a.archive_info()["rows"] > 1000 and a.archive_info()["host_rows"] == 0 and b.archive_info()["device_rows"] == 0
    assert a.SessionMap("all").tobytes() == b.SessionMap("all").tobytes()
    assert np.asarray(a.archive_voxels()).tobytes() == np.asarray(b.archive_voxels()).tobytes()
    assert a.poses().tobytes() == b.poses().tobytes() == c.poses().tobytes()
    assert a.LocalMap().tobytes() == c.LocalMap().tobytes()
    assert c.archive_info()["rows"] == 0
    # reinitialize() empties the window, not the session
    held = a.archive_info()["rows"]
    a.reinitialize()
    assert a.local_map_size() == 0 and a.archive_info()["rows"] == held


@pytest.mark.parametrize("form", ["device", "msg"])
def test_device_frames_and_messages_archive_what_host_rows_archive(gpu_sage, form):
    """a device frame and a PointCloud2 frame go through the same per-frame checks, and archive the same bytes"""
    sage = gpu_sage
    frames = _frames()
    a = _pipeline_run(sage, frames, True, True)
    d = _pipeline_run(sage, frames, True, True, _frame_checks(), form=form)
    assert a.archive_info()["rows"] > 500
    assert d.SessionMap("all").tobytes() == a.SessionMap("all").tobytes()
    assert np.asarray(d.archive_voxels()).tobytes() == np.asarray(a.archive_voxels()).tobytes()
    assert d.poses().tobytes() == a.poses().tobytes()


def test_of_a_map_on_two_copies_only_the_first_archives(gpu_sage):
    """the one GPU twice: every update runs on both copies, the log holds each evicted voxel once"""
    sage = gpu_sage
    m = _map(sage)
    m.set_devices([0, 0])
    m.set_archive(True)
    assert m.num_devices() == 2
    one, ref = _run(sage, "device", ar.walk(), check=False)
    _run(sage, "device", ar.walk(), m=m, ref=_ref())
    assert m.archive_info() == one.archive_info()
    assert m.ArchivedPointcloud("all").tobytes() == one.ArchivedPointcloud("all").tobytes()
    _run(sage, "update", ar.walk()[:6], m=m, ref=ref, check=False)       # ... and on the host copies
    _run(sage, "update", ar.walk()[:6], m=one, ref=_ref(), check=False)
    assert m.ArchivedPointcloud("all").tobytes() == one.ArchivedPointcloud("all").tobytes()


# ---- lifetime --------------------------------------------------------------------------------------------------------------
def test_clone_of_a_resident_map_with_a_device_resident_archive(gpu_sage):
    sage = gpu_sage
    steps = ar.walk()
    m, ref = _run(sage, "device", steps[:7], check=False)
    c = m.clone()
    assert c.resident() and c.archive_info()["device_rows"] == m.archive_info()["device_rows"] > 0
    ar.assert_equal_to_ref(c, ref, "the clone")
    kept = m.ArchivedPointcloud("all").tobytes()
    _run(sage, "device", steps[7:], m=c, ref=ref)                 # the clone goes on alone
    assert m.ArchivedPointcloud("all").tobytes() == kept
    m.archive_clear()
    assert m.archive_info()["device_bytes"] == 0 and m.archive_info()["rows"] == 0
    ar.assert_equal_to_ref(c, ref, "the clone after the original was cleared")


def test_destroy_releases_the_archives_device_memory(gpu_sage):
    sage = gpu_sage
    rng = np.random.default_rng(5)
    pts = np.zeros((200000, 4))
    pts[:, :3] = rng.uniform(-300, 300, size=(200000, 3)) * [1.0, 1.0, 0.1]
    pts[:, 3] = 71.0
    here, away = ar.pose_of((0.0, 0.0, 0.0)), ar.pose_of((5000.0, 0.0, 0.0))

    def cycle():
        m = sage.VoxelHashMap(1.0, 1000.0).set_archive(True)
        m.UpdateOnDevice(pts, here)
        m.UpdateOnDevice(np.zeros((0, 4)), away)
        assert m.archive_info()["device_rows"] == len(pts)
        c = m.clone()
        assert c.archive_info()["device_rows"] == len(pts)
        del m, c
        gc.collect()

    cycle()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    cycles = 12
    for _ in range(cycles):
        cycle()
    torch.cuda.synchronize()
    lost = free_before - torch.cuda.mem_get_info(0)[0]
    held = cycles * 2 * 32 * len(pts)           # the rows of the archive and of its clone, every cycle
    assert lost < held / 4, "%.1f MB of device memory not returned after %d cycles" % (lost / 2**20, cycles)
