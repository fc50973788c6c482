"""The session rebuild on the CPU (include/sageicp.h "session rebuild"): the closed form of the retention
policy (csrc/rebuild_rule.h) against a transcription of VoxelBlock::AddPoint as a stand-alone program, plain and under the
sanitizers; the symbols and the struct; the argument checks (made before any device work, so they answer without a GPU);
the header shim's members."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import archiveref as ar
import mapref
import rebuildref
from test_recall_host import _map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_rebuild_rule_check(tmp_path, flags):
    """every label sequence of length <= 9 at seven policies, seeded runs of 15 .. 320 arrivals, groups of 16 and of 64"""
    exe = str(tmp_path / "rebuild_rule_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "sage-icp_amd", "csrc"), os.path.join(ROOT, "tests", "rebuild_rule_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rebuild_rule_check: ok" in r.stdout
    for pair in ("(basic 1, critical 0)", "(basic 1, critical 1)", "(basic 2, critical 2)", "(basic 3, critical 1)", "(basic 2, critical 0)"):
        assert pair + ": 29523 sequences" in r.stdout


def test_symbols_and_struct(sage, tmp_path):
    lib = sage.lib()
    assert lib.sageicp_map_session_rebuild and lib.sageicp_pipeline_session_rebuild
    assert lib.sageicp_abi_version() == 4
    assert {"sageicp_map_session_rebuild", "sageicp_pipeline_session_rebuild"} <= set(sage.EXPORTED_SYMBOLS)
    fields = list(rebuildref.INFO_FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){printf("%zu", sizeof(sageicp_rebuild_info));'
           + "".join('printf(" %%zu", offsetof(sageicp_rebuild_info, %s));' % f for f in fields) + "return 0;}")
    exe = str(tmp_path / "rebuild_layout_probe")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src, text=True, check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(sage.RebuildInfo)] + [getattr(sage.RebuildInfo, f).offset for f in fields]
    assert got == [64] + list(range(0, 64, 8))
    assert [f for f, _ in sage.RebuildInfo._fields_] == fields
    assert callable(sage.VoxelHashMap.RebuildSession) and callable(sage.SageICP.RebuildSessionMap)


IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def test_every_refused_call_leaves_the_destination_as_it_was(sage):
    lib, dp = sage.lib(), ctypes.POINTER(ctypes.c_double)
    pts = ar.walk()[0][0]
    src = _map(sage).set_archive(True)
    src.AddPoints(pts)
    centre = np.array([0.5, 1.0, 0.5])
    pos = np.array([[0.5, 1.0, 0.5], [2.5, 1.0, 0.5]])
    corr = np.array([IDENTITY, IDENTITY])
    info = sage.RebuildInfo()

    def call(s, which, p, c, n, ctr, radius, d):
        as_p = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)
        return lib.sageicp_map_session_rebuild(None if s is None else s._h, which, as_p(p), as_p(c), n, as_p(ctr), radius,
                                               None if d is None else d._h, ctypes.byref(info))

    def refused(d, held, s=src, which=sage.SESSION, p=pos, c=corr, n=2, ctr=centre, radius=3.0):
        rc = call(s, which, p, c, n, ctr, radius, d)
        assert rc == sage.ERR_INVALID, (rc, lib.sageicp_last_error())
        if d is not None:
            assert d.Pointcloud().tobytes() == held.tobytes() and d.num_voxels() > 0

    def filled(**over):
        d = _map(sage, **over)
        d.AddPoints(pts[:40])
        return d, d.Pointcloud()

    dst, held = filled()
    # dst's refusals are recall's
    refused(None, None)
    refused(src, src.Pointcloud())                                             # dst == src
    for over in (dict(voxel_size=0.5), dict(basic=19), dict(critical=21), dict(basic=21, critical=19),
                 dict(basic_labels=(40, 44)), dict(basic_labels=(40, 48, 44))):
        refused(*filled(**over))
    ro = _map(sage).set_reference_order(True)
    ro.AddPoints(pts[:40])
    refused(ro, ro.Pointcloud())
    refused(*filled(device=1))                                                 # another device than src's
    wide = _map(sage)
    wide.set_devices([0, 0])
    wide.AddPoints(pts[:40])
    refused(wide, wide.Pointcloud())
    # src, which, positions, corrections, n: the corrected export's
    refused(dst, held, s=None)
    refused(dst, held, p=None)
    refused(dst, held, c=None)
    refused(dst, held, n=0)
    refused(dst, held, n=1 << 32)
    for which in (-1, 3, 7):
        refused(dst, held, which=which)
    for bad in (math.nan, math.inf, -math.inf):
        p = pos.copy()
        p[1, 2] = bad
        refused(dst, held, p=p)
        for col in (0, 3, 6):
            c = corr.copy()
            c[1, col] = bad
            refused(dst, held, c=c)
        # the centre and the radius, when a centre is given
        for axis in range(3):
            ctr = centre.copy()
            ctr[axis] = bad
            refused(dst, held, ctr=ctr)
    for radius in (-1.0, -0.0 - 1e-300, -math.inf, math.nan):
        refused(dst, held, radius=radius)
    assert lib.sageicp_pipeline_session_rebuild(None, sage.SESSION, corr.ctypes.data_as(dp), 2, None, 0.0, dst._h, None) == sage.ERR_INVALID
    assert dst.Pointcloud().tobytes() == held.tobytes()
    # past the checks the call is device work; without a centre the radius is not looked at
    for ctr, radius in ((centre, math.inf), (centre, 0.0), (None, math.nan), (None, -1.0)):
        d, held = filled()
        rc = call(src, sage.SESSION, pos, corr, 2, ctr, radius, d)
        if sage.device_count() < 1:
            assert rc == sage.ERR_NO_DEVICE and d.Pointcloud().tobytes() == held.tobytes()
        else:
            assert rc == 0 and d.resident()


def test_python_entries_check_their_arguments(sage):
    src = _map(sage)
    pos, corr = np.zeros((2, 3)), np.array([IDENTITY, IDENTITY])
    with pytest.raises(ValueError):
        src.RebuildSession(pos, corr, center=(0.0, 1.0), radius=3.0)
    with pytest.raises(ValueError):
        src.RebuildSession(pos, corr[:1])
    with pytest.raises(sage.SageIcpError):
        src.RebuildSession(pos, corr, center=(0.0, 1.0, 2.0), radius=-3.0)
    with pytest.raises(KeyError):
        src.RebuildSession(pos, corr, which="everything")


def test_shim_rebuild_type_checks():
    """the RebuiltMap members of the header shim against the stand-in Eigen (tests/shim_stubs), as tests/test_shim_compile.py
    checks the rest"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "tests", "shim_stubs"), "-I", os.path.join(ROOT, "sage-icp_amd", "shim"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim_stubs", "rebuild_user.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_restatement_merges_and_crops_by_the_final_first_row():
    """rebuildref.rebuild_rows on a hand-made case: at policy (3, 2) slot 0 is unlabelled and a later labelled row replaces
    it; the crop looks at the replacer"""
    params = dict(voxel_size=1.0, basic=3, critical=2, basic_labels=(40, 44, 48))
    rows = np.array([[0.25, 0.5, 0.5, 0.0], [0.5, 0.5, 0.5, 71.0], [0.5, 0.25, 0.5, 71.0], [0.75, 0.5, 0.5, 44.0],
                     [5.5, 0.5, 0.5, 71.0]])
    cloud, info = rebuildref.rebuild_rows(rows, params)
    assert cloud.tobytes() == rows[[3, 1, 2, 4]].tobytes()
    assert info == dict(voxels=2, rows=4, session_rows=5, built_voxels=2, built_rows=4, cropped_voxels=0, cropped_rows=0)
    # the original first row is 0.25 from the centre, the replacer 0.75
    cloud, info = rebuildref.rebuild_rows(rows, params, center=(0.0, 0.5, 0.5), radius=0.5)
    assert len(cloud) == 0 and info["cropped_voxels"] == 2 and info["cropped_rows"] == 4
    cloud, info = rebuildref.rebuild_rows(rows, params, center=(0.0, 0.5, 0.5), radius=0.75)        # on the radius: kept
    assert cloud.tobytes() == rows[[3, 1, 2]].tobytes() and info["cropped_voxels"] == 1 and info["cropped_rows"] == 1
    assert mapref.KEY_LIMIT == 1 << 20
