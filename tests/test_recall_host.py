"""Recall on the CPU (include/sageicp.h "recall"): the symbols and the struct, the argument checks (made before
any device work, so they answer without a GPU), the header shim's member, and the restatement (tests/recallref.py) against
the only route the library offered before — the SESSION rows into a second map, then remove_far — in plain Python."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import archiveref as ar
import mapref
import recallref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CENTRES = ((0.5, 1.0, 0.5), (8.5, 1.0, 0.5), (500.5, 1.0, 0.5))      # the start, the middle, the far jump
RADII = (0.0, 3.0, 6.5, math.inf)
CHECKPOINTS = (7, 11, len(ar.walk()))                                  # steps made before a recall


def _map(sage, **over):
    p = dict(ar.PARAMS, **over)
    return sage.VoxelHashMap(p["voxel_size"], p["max_distance"], p["basic"], p["critical"], list(p["basic_labels"]),
                             device=over.get("device", 0))


def test_symbols_and_struct(sage, tmp_path):
    lib = sage.lib()
    assert lib.sageicp_map_recall and lib.sageicp_pipeline_recall
    assert lib.sageicp_abi_version() == 4
    fields = ["voxels", "rows", "archive_voxels", "archive_rows", "map_voxels", "map_rows", "session_voxels", "session_rows"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){printf("%zu", sizeof(sageicp_recall_info));'
           + "".join('printf(" %%zu", offsetof(sageicp_recall_info, %s));' % f for f in fields) + "return 0;}")
    exe = str(tmp_path / "recall_layout_probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(sage.RecallInfo)] + [getattr(sage.RecallInfo, f).offset for f in fields]
    assert got == [64] + list(range(0, 64, 8))
    assert [f for f, _ in sage.RecallInfo._fields_] == fields


def test_every_refused_call_leaves_the_destination_as_it_was(sage):
    lib, dp = sage.lib(), ctypes.POINTER(ctypes.c_double)
    pts = ar.walk()[0][0]
    src = _map(sage).set_archive(True)
    src.AddPoints(pts)
    centre = np.array([0.5, 1.0, 0.5])
    info = sage.RecallInfo()

    def refused(s, c, radius, d, held):
        cp = None if c is None else np.ascontiguousarray(c, dtype=np.float64).ctypes.data_as(dp)
        rc = lib.sageicp_map_recall(None if s is None else s._h, cp, radius, None if d is None else d._h, ctypes.byref(info))
        assert rc == sage.ERR_INVALID, (rc, lib.sageicp_last_error())
        if d is not None:
            assert d.Pointcloud().tobytes() == held.tobytes() and d.num_voxels() > 0

    def filled(**over):
        d = _map(sage, **over)
        d.AddPoints(pts[:40])
        return d, d.Pointcloud()

    dst, held = filled()
    refused(None, centre, 3.0, dst, held)
    refused(src, centre, 3.0, None, None)
    refused(src, None, 3.0, dst, held)
    refused(src, centre, 3.0, src, src.Pointcloud())                           # dst == src
    assert lib.sageicp_pipeline_recall(None, centre.ctypes.data_as(dp), 3.0, dst._h, None) == sage.ERR_INVALID
    for bad in (math.nan, math.inf, -math.inf):
        for axis in range(3):
            c = centre.copy()
            c[axis] = bad
            refused(src, c, 3.0, dst, held)
    for radius in (-1.0, -0.0 - 1e-300, -math.inf, math.nan):
        refused(src, centre, radius, dst, held)
    for over in (dict(voxel_size=0.5), dict(basic=19), dict(critical=21), dict(basic=21, critical=19),
                 dict(basic_labels=(40, 44)), dict(basic_labels=(40, 48, 44))):
        refused(src, centre, 3.0, *filled(**over))
    ro = _map(sage).set_reference_order(True)
    ro.AddPoints(pts[:40])
    refused(src, centre, 3.0, ro, ro.Pointcloud())
    refused(src, centre, 3.0, *filled(device=1))                               # another device than src's
    wide = _map(sage)
    wide.set_devices([0, 0])
    wide.AddPoints(pts[:40])
    refused(src, centre, 3.0, wide, wide.Pointcloud())
    # +inf and 0 are radii; past the checks the call is device work
    for radius in (math.inf, 0.0):
        d, held = filled()
        rc = lib.sageicp_map_recall(src._h, centre.ctypes.data_as(dp), radius, d._h, None)
        if sage.device_count() < 1:
            assert rc == sage.ERR_NO_DEVICE and d.Pointcloud().tobytes() == held.tobytes()
        else:
            assert rc == 0 and d.resident()


def test_python_entries_check_their_arguments(sage):
    src = _map(sage)
    with pytest.raises(ValueError):
        src.Recall((0.0, 1.0), 3.0)
    with pytest.raises(sage.SageIcpError):
        src.Recall((0.0, 1.0, 2.0), -3.0)
    assert callable(sage.SageICP.Recall)


def test_shim_recall_type_checks():
    """the Recall member of the header shim against the stand-in Eigen (tests/shim_stubs), as tests/test_shim_compile.py
    checks the rest"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_stubs", "recall_user.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def sessions_of_the_walk():
    """[(steps made, the SESSION rows, how many of them are the LATEST part)] at the checkpoints, from the restatements"""
    ref = ar.ArchiveRef(**ar.PARAMS)
    out = []
    for k, (pts, origin) in enumerate(ar.walk()):
        ar.ref_step(ref, pts, origin)
        if k + 1 in CHECKPOINTS:
            cloud = ref.pointcloud()
            live = ar.keys_of(cloud, ar.PARAMS["voxel_size"])
            out.append((k + 1, ar.session(ref.log, live, cloud), len(ar.rows_of(ar.latest(ref.log, live)))))
    return out


def test_the_restatement_equals_the_existing_route_in_plain_python():
    vs = ar.PARAMS["voxel_size"]
    seen = set()
    for steps, session, n_arc in sessions_of_the_walk():
        if steps == 11:
            assert n_arc == len(session) > 0, "everything was meant to be evicted by then"
        for centre in CENTRES:
            for radius in RADII:
                twin = mapref.MapRef(**dict(ar.PARAMS, max_distance=radius))
                twin.add_points(session)
                twin.remove_far(centre)
                got, voxels = recallref.recall(session, vs, centre, radius)
                assert got.tobytes() == twin.pointcloud().tobytes(), (steps, centre, radius)
                assert voxels == twin.num_voxels() and len(got) == twin.size()
                i = recallref.info(session, n_arc, vs, centre, radius)
                assert i["rows"] == len(got) and i["voxels"] == voxels and i["session_rows"] == len(session)
                if radius == math.inf:
                    assert got.tobytes() == session.tobytes()
                seen.add("all" if len(got) == len(session) else "none" if len(got) == 0 else "some")
                if 0 < i["archive_voxels"] and 0 < i["map_voxels"]:
                    seen.add("both parts")
    assert seen == {"all", "none", "some", "both parts"}, seen
