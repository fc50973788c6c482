"""The archive of a map on the CPU (include/sageicp.h "the archive of a map"): what the host copy's sweep
evicts, logged in order, against the plain restatement (tests/archiveref.py) and — in reference-order mode — against the
oracle alone.  Every comparison is on bytes.  No GPU: a handle that never touches a device keeps a working archive."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import archiveref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _map(sage, **over):
    p = dict(ar.PARAMS, **over)
    return sage.VoxelHashMap(p["voxel_size"], p["max_distance"], p["basic"], p["critical"], list(p["basic_labels"]))


def _ref(**over):
    return ar.ArchiveRef(**dict(ar.PARAMS, **over))


def test_off_by_default_and_empty(sage):
    m = _map(sage)
    info = m.archive_info()
    assert set(info.values()) == {0}, info
    assert m.ArchivedPointcloud("all").shape == (0, 4) and len(m.archive_voxels()) == 0
    for pts, origin in ar.walk()[:4]:           # evicts, and nothing is kept
        m.Update(pts, np.array(origin))
    assert set(m.archive_info().values()) == {0}


def test_the_walk_evicts_what_it_was_built_to_evict():
    ref = _ref()
    for pts, origin in ar.walk():
        ar.ref_step(ref, pts, origin)
    counts = {len(r) for _, r, _ in ref.log}
    assert counts >= {1, 4, 5, 8, 9, 16, 17, 40}, sorted(counts)
    per_call = ref.evicted_by_call
    assert 0 in per_call and 1 in per_call and any(n > 3 for n in per_call)
    step_all = [i for i, (_, o) in enumerate(ar.walk()) if o[0] == 500.5][0]
    assert per_call[step_all] > 0 and ref.log and ar.walk()[step_all][0].shape[0] == 0      # n == 0 evicts, every voxel goes
    keys = [k for k, _, _ in ref.log]
    assert len(set(keys)) < len(keys), "a key was meant to be archived in two generations"


@pytest.mark.parametrize("entry", ["remove_far", "update", "update_pose"])
def test_walk_through_each_host_entry_equals_the_restatement(sage, entry):
    m, ref = _map(sage).set_archive(True), _ref()
    assert m.archive_info()["enabled"] == 1
    for k, (pts, origin) in enumerate(ar.walk()):
        ar.apply_step(m, entry, pts, origin)
        ar.ref_step(ref, pts, origin)
        ar.assert_equal_to_ref(m, ref, "%s step %d" % (entry, k))
        assert m.Pointcloud().tobytes() == ref.pointcloud().tobytes()
    info = m.archive_info()
    assert info["device_rows"] == 0 and info["device_bytes"] == 0 and info["host_rows"] == info["rows"] > 100
    # a freed block was taken by a new voxel and evicted again: two records share a block's rows region over time — the
    # serials of one key's generations differ
    rec = m.archive_voxels()
    by_key = {}
    for r in rec:
        by_key.setdefault((r.x, r.y, r.z), []).append(int(r.update))
    assert any(len(set(v)) > 1 for v in by_key.values())
    # switched off: it keeps what it holds and takes nothing more
    m.set_archive(False)
    before = m.ArchivedPointcloud("all").tobytes()
    m.Update(np.zeros((0, 4)), np.array([900.0, 0.0, 0.0]))
    assert m.ArchivedPointcloud("all").tobytes() == before and m.archive_info()["updates"] == info["updates"]


def _cloud(rng, n, centre, spread=45.0):
    p = np.zeros((n, 4))
    p[:, :3] = centre + rng.uniform(-spread, spread, size=(n, 3)) * [1.0, 1.0, 0.1]
    p[:, 3] = rng.choice([0, 40, 48, 50, 70, 71, 80, 10], size=n)
    return p


def reference_order_stream(seed=100, frames=14, n=1500, grid=0):
    """[(rows in the map frame, sensor position)]; grid: coordinates and positions rounded to multiples of 1 / grid, so
    that rows - position and back is exact"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(frames):
        centre = np.array([9.0 * f, 2.0 * np.sin(f / 3.0), 0.0])
        if f == 9:
            centre[0] = 18.0                 # a jump back: evicted ground is seen again
        if grid:
            centre = np.round(centre * grid) / grid
            pts = _cloud(rng, n, np.zeros(3))
            pts[:, :3] = np.round(pts[:, :3] * grid) / grid + centre
        else:
            pts = _cloud(rng, n, centre)
        out.append((pts, centre))
    return out


def oracle_log(oracle, stream, vs=1.0, md=40.0):
    """per call, the evicted voxels (key, rows) from the oracle in mode 3 alone; and the oracle's final Pointcloud()"""
    om = oracle.Map(vs, md, 5, 5, [40, 48, 50])
    calls = []
    for pts, centre in stream:
        om.add_points(pts)
        before = om.pointcloud()
        om.remove_far(centre)
        calls.append(ar.evicted_groups(before, om.pointcloud(), vs))
    return calls, om.pointcloud()


def test_reference_order_mode_against_the_oracle(sage, oracle):
    oracle.set_robin_order(3)
    try:
        stream = reference_order_stream()
        calls, final = oracle_log(oracle, stream)
    finally:
        oracle.set_robin_order(False)
    m = sage.VoxelHashMap(1.0, 40.0, 5, 5, [40, 48, 50]).set_reference_order(True).set_archive(True)
    d = sage.VoxelHashMap(1.0, 40.0, 5, 5, [40, 48, 50]).set_archive(True)          # the default sweep, for contrast
    log, skipped_then_archived = [], False
    for k, (pts, centre) in enumerate(stream):
        m.Update(pts, centre)
        d.Update(pts, centre)
        log += [(key, rows, k) for key, rows in calls[k]]
        assert m.ArchivedPointcloud("all").tobytes() == ar.rows_of(log).tobytes(), "call %d" % k
        assert np.asarray(m.archive_voxels()).tobytes() == ar.records_of(log).tobytes(), "call %d" % k
        # a voxel the sweep skipped survives its frame: far from the sensor, still in the map, archived by a later call
        pc = m.Pointcloud()
        far_keys = {key for key, p in zip(ar.keys_of(pc, 1.0), pc) if np.linalg.norm(p[:3] - centre) > 40.0 + 2.0}
        if far_keys and any(key in far_keys for later in calls[k + 1:] for key, _ in later):
            skipped_then_archived = True
    assert skipped_then_archived
    assert np.array_equal(m.Pointcloud(), final)
    # the order of eviction is not ascending block order: the default map archives the same voxels of a call in another order
    rm, rd = m.archive_voxels(), d.archive_voxels()
    first = [(r.x, r.y, r.z) for r in rm if r.update == rm[0].update]
    first_d = [(r.x, r.y, r.z) for r in rd if r.update == rm[0].update]
    assert len(first) > 10 and first != first_d[:len(first)] and set(first) <= set(first_d)


def _ends(ref_log):
    at, out = 0, []
    for _, rows, _ in ref_log:
        at += len(rows)
        out.append(at)
    return out


@pytest.mark.parametrize("cut", ["at_a_voxel_end", "one_row_short", "no_room"])
def test_limit_keeps_the_longest_prefix_of_whole_voxels(sage, cut):
    full = _ref()
    for pts, origin in ar.walk():
        ar.ref_step(full, pts, origin)
    ends = _ends(full.log)
    j = len(ends) // 2
    assert full.log[j][1] and len(full.log[j][1]) > 1
    max_rows = {"at_a_voxel_end": ends[j], "one_row_short": ends[j] - 1, "no_room": 0}[cut]
    m = _map(sage)
    if cut == "no_room":
        # 0 rows of room: the limit is set to what the archive holds once it holds something
        m.set_archive(True)
        ref = _ref()
        steps = ar.walk()
        k0 = next(i for i in range(len(steps)) if sum(full.evicted_by_call[:i + 1]) > 0)
        for pts, origin in steps[:k0 + 1]:
            ar.apply_step(m, "update", pts, origin)
            ar.ref_step(ref, pts, origin)
        held = m.archive_info()["rows"]
        assert held > 0
        m.set_archive(True, held)
        ref.max_rows = held
        rest = steps[k0 + 1:]
    else:
        m.set_archive(True, max_rows)
        ref = _ref(max_rows=max_rows)
        rest = ar.walk()
    for pts, origin in rest:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
        ar.assert_equal_to_ref(m, ref, cut)
    info = m.archive_info()
    assert info["full"] == 1 and info["dropped_voxels"] > 0 and info["rows"] <= info["max_rows"]
    assert info["rows"] + info["dropped_rows"] == full.rows_held()
    want = ar.limited(full.log, info["max_rows"])
    assert m.ArchivedPointcloud("all").tobytes() == ar.rows_of(want).tobytes()
    if cut == "at_a_voxel_end":
        assert info["rows"] == max_rows
    if cut == "one_row_short":
        assert info["rows"] == ends[j - 1]
    # full is sticky: raising the limit does not reopen it; lowering it below the rows held is refused
    m.set_archive(True, 0)
    m.Update(ar.walk()[0][0], np.array([0.5, 1.0, 0.5]))
    m.Update(np.zeros((0, 4)), np.array([700.0, 0.0, 0.0]))
    after = m.archive_info()
    assert after["full"] == 1 and after["rows"] == info["rows"] and after["dropped_voxels"] > info["dropped_voxels"]
    with pytest.raises(sage.SageIcpError) as e:
        m.set_archive(True, info["rows"] - 1)
    assert e.value.code == sage.ERR_INVALID


def test_refused_calls_leave_the_archive_unchanged(sage):
    m, ref = _map(sage).set_archive(True), _ref()
    for pts, origin in ar.walk()[:5]:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    info, rows, rec = m.archive_info(), m.ArchivedPointcloud("all").tobytes(), np.asarray(m.archive_voxels()).tobytes()
    far = np.array([900.0, 0.0, 0.0])            # would evict everything
    bad = [np.array([[1.5, 0.5, 0.5, 71.0], [np.nan, 0.0, 0.0, 0.0]]), np.array([[1.5, 0.5, 0.5, 71.0], [1048576.0, 0.0, 0.0, 0.0]])]
    for pts, code in zip(bad, (sage.ERR_INVALID, sage.ERR_CAPACITY)):
        for call in (lambda: m.Update(pts, far), lambda: m.Update(pts, ar.pose_of(far))):
            with pytest.raises(sage.SageIcpError) as e:
                call()
            assert e.value.code == code
            assert m.archive_info() == info
            assert m.ArchivedPointcloud("all").tobytes() == rows and np.asarray(m.archive_voxels()).tobytes() == rec
    ar.assert_equal_to_ref(m, ref)


def test_clear_keeps_the_archive_and_archive_clear_restarts_it(sage):
    m, ref = _map(sage).set_archive(True, 100000), _ref(max_rows=100000)
    steps = ar.walk()
    for pts, origin in steps[:6]:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    m.Clear()
    assert m.size() == 0
    ar.assert_equal_to_ref(m, ref, "after Clear()")
    m.archive_clear()
    info = m.archive_info()
    assert info["enabled"] == 1 and info["max_rows"] == 100000
    assert {k: v for k, v in info.items() if k not in ("enabled", "max_rows")} == dict.fromkeys(
        [k for k in info if k not in ("enabled", "max_rows")], 0)
    ref2 = _ref(max_rows=100000)
    for pts, origin in steps[:6]:                # the same walk again: serials from 0
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref2, pts, origin)
    ar.assert_equal_to_ref(m, ref2, "after archive_clear()")
    assert int(m.archive_voxels()[0].update) == ref2.log[0][2]


def test_a_clone_carries_a_deep_copy(sage):
    m, ref = _map(sage).set_archive(True), _ref()
    steps = ar.walk()
    for pts, origin in steps[:6]:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    c = m.clone()
    assert c.archive_info() == m.archive_info()
    ar.assert_equal_to_ref(c, ref, "the clone")
    kept = m.ArchivedPointcloud("all").tobytes()
    for pts, origin in steps[6:9]:               # the clone goes on alone
        ar.apply_step(c, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    ar.assert_equal_to_ref(c, ref, "the clone, later")
    assert m.ArchivedPointcloud("all").tobytes() == kept and len(c.ArchivedPointcloud("all")) > len(kept) // 32
    m.archive_clear()
    ar.assert_equal_to_ref(c, ref, "the clone after the original was cleared")


def test_ranges_of_an_export(sage):
    m, ref = _map(sage).set_archive(True), _ref()
    for pts, origin in ar.walk()[:8]:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    rows = ar.rows_of(ref.log)
    total = len(rows)
    rec = ar.records_of(ref.log)
    mid = int(next(r for r in rec if r["count"] > 2)["first_row"]) + 1           # a voxel's middle
    L = sage.lib()
    n = ctypes.c_uint64(0)
    for first in (0, mid, total, total + 5):
        got = m.ArchivedPointcloud("all", first=first)
        assert got.tobytes() == rows[first:].tobytes(), first
        assert L.sageicp_map_archive_rows(m._h, 0, first, None, 0, ctypes.byref(n)) == 0 and n.value == total
        # cap smaller than the rest: nothing beyond it is written
        buf = np.full((7, 4), -1.0)
        assert L.sageicp_map_archive_rows(m._h, 0, first, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 3,
                                          ctypes.byref(n)) == 0
        k = min(3, max(0, total - first))
        assert n.value == total and buf[:k].tobytes() == rows[first:first + k].tobytes() and (buf[k:] == -1.0).all()
    out = np.zeros(2, dtype=ar.VOXEL_DTYPE)
    assert L.sageicp_map_archive_voxels(m._h, 3, out.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(n)) == 0
    assert n.value == len(rec) and out.tobytes() == rec[3:5].tobytes()
    assert L.sageicp_map_archive_rows(m._h, 7, 0, None, 0, ctypes.byref(n)) == sage.ERR_INVALID


def test_environment_switch(sage):
    os.environ["SAGEICP_MAP_ARCHIVE"] = "1"
    os.environ["SAGEICP_MAP_ARCHIVE_MAX_ROWS"] = "77"
    try:
        m = _map(sage)
    finally:
        del os.environ["SAGEICP_MAP_ARCHIVE"]
        del os.environ["SAGEICP_MAP_ARCHIVE_MAX_ROWS"]
    off = _map(sage)
    assert off.archive_info()["enabled"] == 0
    info = m.archive_info()
    assert info["enabled"] == 1 and info["max_rows"] == 77
    ref = _ref(max_rows=77)
    for pts, origin in ar.walk()[:6]:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    ar.assert_equal_to_ref(m, ref)
    assert m.archive_info()["rows"] > 0


def test_environment_limit_is_a_64_bit_count(sage):
    os.environ["SAGEICP_MAP_ARCHIVE"] = "1"
    os.environ["SAGEICP_MAP_ARCHIVE_MAX_ROWS"] = "5000000000"           # beyond 2^32
    try:
        m = _map(sage)
    finally:
        del os.environ["SAGEICP_MAP_ARCHIVE"]
        del os.environ["SAGEICP_MAP_ARCHIVE_MAX_ROWS"]
    assert m.archive_info()["max_rows"] == 5000000000 and m.archive_info()["enabled"] == 1


def test_serials_count_the_calls_made_while_the_archive_is_on(sage):
    """off and on again: the calls in between take no serial and archive nothing, the count goes on where it stopped"""
    m, ref = _map(sage).set_archive(True), _ref()
    steps = ar.walk()
    for pts, origin in steps[:5]:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    m.set_archive(False)
    off = mapref_only(steps[5:7], m, ref)
    assert m.archive_info()["updates"] == 5 and off
    m.set_archive(True)
    for pts, origin in steps[7:10]:
        ar.apply_step(m, "update", pts, origin)
        ar.ref_step(ref, pts, origin)
    ar.assert_equal_to_ref(m, ref, "after off and on")
    assert m.archive_info()["updates"] == 8


def mapref_only(steps, m, ref):
    """steps taken with the archive off: the library's map and the restatement's map move on, the restatement's log
    does not (its evictions are put back out of the log); True if something was evicted meanwhile"""
    evicted = 0
    for pts, origin in steps:
        ar.apply_step(m, "update", pts, origin)
        held, calls, n = len(ref.log), ref.updates, len(ref.evicted_by_call)
        ar.ref_step(ref, pts, origin)
        evicted += ref.evicted_by_call[-1]
        del ref.log[held:]
        del ref.evicted_by_call[n:]
        ref.updates = calls
    return evicted > 0


def test_latest_and_session_are_compute_entries(sage):
    """without a device they answer SAGEICP_ERR_NO_DEVICE (with one they answer: tests/test_archive_gpu.py)"""
    m = _map(sage).set_archive(True)
    for pts, origin in ar.walk()[:6]:
        ar.apply_step(m, "update", pts, origin)
    n = ctypes.c_uint64(0)
    want = sage.ERR_NO_DEVICE if sage.device_count() < 1 else 0
    for which in (1, 2):
        assert sage.lib().sageicp_map_archive_rows(m._h, which, 0, None, 0, ctypes.byref(n)) == want
    assert sage.lib().sageicp_map_archive_rows(m._h, 0, 0, None, 0, ctypes.byref(n)) == 0 and n.value > 0


def test_struct_layouts_match_the_header(sage, tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){printf("%zu %zu %zu %zu %zu", '
           'sizeof(sageicp_archive_info), sizeof(sageicp_archive_voxel), offsetof(sageicp_archive_voxel, first_row), '
           'offsetof(sageicp_archive_info, rows), offsetof(sageicp_archive_info, device_bytes));return 0;}')
    exe = str(tmp_path / "archive_layout_probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(sage.ArchiveInfo), 32, 16, sage.ArchiveInfo.rows.offset, sage.ArchiveInfo.device_bytes.offset]
    assert sage.ARCHIVE_VOXEL_DTYPE.itemsize == 32 and ar.VOXEL_DTYPE == sage.ARCHIVE_VOXEL_DTYPE


SHIM_PROBE = r"""
#include "sage_icp/core/VoxelHashMap.hpp"
std::vector<Eigen::Vector4d> archived(const sage_icp::VoxelHashMap &m) { return m.ArchivedPointcloud(); }
std::vector<Eigen::Vector4d> session(const sage_icp::VoxelHashMap &m) { return m.SessionPointcloud(); }
"""


def test_shim_extension_members_type_check(tmp_path):
    """the two extension members of the header shim against the stand-in Eigen (tests/shim_stubs), as
    tests/test_shim_compile.py checks the rest"""
    src = tmp_path / "archive_user.cpp"
    src.write_text(SHIM_PROBE)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
