"""The batch score of candidate poses and Relocalize (sageicp_score_poses*, sageicp_relocalize*): what needs
no GPU — the layout of the three structs, the candidate grid, the refusals (before any device is asked: they hold on a
machine without one) and, with the oracle, the condition under which tests/test_score_poses_gpu.py may compare winners:
that on its scene the ranking by sum_w finds the basin and has margins far above fp64 noise."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import scoreref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP4 = 4 * 2.0 ** -52


# ---- layout and symbols ---------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(sage):
    structs = (("sageicp_pose_score", sage.PoseScore), ("sageicp_relocalize_params", sage.RelocalizeParams),
               ("sageicp_relocalize_info", sage.RelocalizeInfo))
    body = ""
    for name, ty in structs:
        body += 'printf("%%zu", sizeof(%s));' % name
        body += "".join('printf(" %%zu", offsetof(%s, %s));' % (name, f) for f, _ in ty._fields_)
        body += 'printf("\\n");'
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){%sprintf("%%d\\n", SAGEICP_ABI_VERSION);return 0;}' % body
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        lines = subprocess.check_output([os.path.join(d, "t")]).decode().splitlines()
    for (name, ty), line in zip(structs, lines):
        got = [int(x) for x in line.split()]
        assert got[0] == C.sizeof(ty), name
        assert got[1:] == [getattr(ty, f).offset for f, _ in ty._fields_], name
    assert C.sizeof(sage.PoseScore) == sage.POSE_SCORE_BYTES == 488
    assert C.sizeof(sage.RelocalizeParams) == 80 and C.sizeof(sage.RelocalizeInfo) == 64
    assert int(lines[3]) == sage.ABI_VERSION == 4
    # the record array of ScorePoses lays the same struct out
    assert sage.POSE_SCORE_DTYPE.itemsize == 488
    for f, _ in sage.PoseScore._fields_:
        assert sage.POSE_SCORE_DTYPE.fields[f][1] == getattr(sage.PoseScore, f).offset, f


def test_new_symbols_are_exported(sage):
    L = C.CDLL(sage.LIB_PATH)
    for n in ("sageicp_score_poses", "sageicp_score_poses_device", "sageicp_relocalize_candidates", "sageicp_relocalize",
              "sageicp_relocalize_device"):
        assert hasattr(L, n) and n in sage.EXPORTED_SYMBOLS, n
    assert L.sageicp_abi_version() == 4


# ---- the candidate grid ---------------------------------------------------------------------------------------------------
PRIOR = np.array([0.05, -0.02, 0.3, 0.95, 12.5, -7.25, 1.5])
PRIOR[:4] /= np.linalg.norm(PRIOR[:4])


def _close(got, want):
    return np.all(np.abs(got - want) <= ULP4 * np.abs(want))


def test_all_zero_params_give_the_prior(sage):
    for prior in (PRIOR, np.array([-0.0, 0.0, -0.0, 1.0, -0.0, 0.0, -0.0])):
        got = sage.relocalize_candidates(prior)
        assert got.shape == (1, 7) and got.tobytes() == np.asarray(prior, dtype=np.float64).tobytes()


@pytest.mark.parametrize("kw, k", [
    (dict(xy=(2.0, 1.0)), 25), (dict(z=(1.0, 0.5)), 5), (dict(yaw=(0.3, 0.1)), 2 * sr.axis_steps(0.3, 0.1) + 1),
    (dict(xy=(0.9, 1.0), z=(0.4, 0.5), yaw=(0.09, 0.1)), 1),          # extent < step
    (dict(xy=(3.0, 1.5)), 25), (dict(z=(0.75, 0.25)), 7),             # extent == m * step exactly
    (dict(xy=(5.0, -1.0), z=(5.0, 0.0), yaw=(1.0, -0.1)), 1),         # a step that is negative or zero
    (dict(xy=(1.0, 1.0), z=(0.5, 0.5), yaw=(0.1, 0.1)), 81),
    (sr.GRID, sr.GRID_CANDIDATES),
], ids=["xy", "z", "yaw", "extent<step", "xy-exact", "z-exact", "step<=0", "all", "grid"])
def test_candidates(sage, kw, k):
    got = sage.relocalize_candidates(PRIOR, **kw)
    want = sr.candidates(PRIOR, **kw)
    assert len(want) == k and got.shape == (k, 7)
    assert _close(got, want)
    assert np.all(np.abs(np.linalg.norm(got[:, :4], axis=1) - 1.0) <= ULP4)
    # the order: yaw outermost, then x, then y, z innermost, each ascending; the middle one is the prior itself
    my, mx, mz = sr.axis_steps(*kw.get("yaw", (0, 0))), sr.axis_steps(*kw.get("xy", (0, 0))), sr.axis_steps(*kw.get("z", (0, 0)))
    g = got.reshape(2 * my + 1, 2 * mx + 1, 2 * mx + 1, 2 * mz + 1, 7)
    assert g[my, mx, mx, mz].tobytes() == PRIOR.tobytes()
    yaw_of = 2.0 * np.arctan2(g[:, 0, 0, 0, 2], g[:, 0, 0, 0, 3])
    assert np.all(np.diff(yaw_of) > 0) and np.all(np.diff(g[0, :, 0, 0, 4]) > 0)
    assert np.all(np.diff(g[0, 0, :, 0, 5]) > 0) and np.all(np.diff(g[0, 0, 0, :, 6]) > 0)
    assert np.all(g[..., :4] == g[:, :1, :1, :1, :4]) and np.all(g[..., 4] == g[:1, :, :1, :1, 4])


def test_cap_below_k_writes_cap_poses_and_reports_k(sage):
    full = sage.relocalize_candidates(PRIOR, **sr.GRID)
    part, k = sage.relocalize_candidates(PRIOR, cap=10, **sr.GRID)
    assert k == sr.GRID_CANDIDATES and part.tobytes() == full[:10].tobytes()
    # nothing beyond cap is written
    buf = np.full((12, 7), 7.5)
    p = sage._relocalize_params(**sr.GRID)
    n = C.c_uint64(0)
    prior = np.ascontiguousarray(PRIOR)
    assert sage.lib().sageicp_relocalize_candidates(prior.ctypes.data_as(sage._dp), C.byref(p), buf.ctypes.data_as(sage._dp),
                                                    10, C.byref(n)) == 0
    assert n.value == sr.GRID_CANDIDATES and np.all(buf[10:] == 7.5) and buf[:10].tobytes() == full[:10].tobytes()


@pytest.mark.parametrize("kw", [dict(xy=(512.5, 1.0)), dict(xy=(1e300, 1e-300)), dict(yaw=(float("nan"), 0.1)),
                                dict(z=(1.0, float("inf")))], ids=["2^20+", "huge", "nan", "inf"])
def test_candidates_refused(sage, kw):
    with pytest.raises(sage.SageIcpError) as e:
        sage.relocalize_candidates(PRIOR, **kw)
    assert e.value.code == sage.ERR_INVALID
    bad = PRIOR.copy()
    bad[5] = np.nan
    with pytest.raises(sage.SageIcpError) as e:
        sage.relocalize_candidates(bad, xy=(1.0, 1.0))
    assert e.value.code == sage.ERR_INVALID


def test_largest_grid_is_taken(sage):
    # 1024 x 1024 = 2^20 exactly... the grid is odd per axis: 1023 x 1023 x 1 passes, 1025 x 1025 does not
    _, k = sage.relocalize_candidates(PRIOR, xy=(511.0, 1.0), cap=1)
    assert k == 1023 * 1023


# ---- refusals: before any device is asked -----------------------------------------------------------------------------------
PATTERN = 0xAB


def _call(sage, m, rows, n, poses, k, kernel=0.5, out="pattern", device_frame=None):
    L = sage.lib()
    buf = np.full(4 * 488, PATTERN, dtype=np.uint8)
    outp = None if out is None else buf.ctypes.data
    rp = None if rows is None else rows.ctypes.data_as(sage._dp)
    pp = None if poses is None else poses.ctypes.data_as(sage._dp)
    if device_frame is not None:
        fp = None if device_frame == "null" else C.byref(device_frame)
        rc = L.sageicp_score_poses_device(m, fp, pp, k, 1.0, kernel, 0.4, None, outp)
    else:
        rc = L.sageicp_score_poses(m, rp, n, pp, k, 1.0, kernel, 0.4, outp)
    assert np.all(buf == PATTERN), "out was written"
    return rc, (L.sageicp_last_error() or b"").decode()


def test_refusals_leave_out_untouched(sage):
    m = sage.VoxelHashMap(1.0, 100.0)
    rows = np.ones((5, 4))
    poses = np.tile(sage.IDENTITY, (4, 1))
    INV = sage.ERR_INVALID
    assert _call(sage, None, rows, 5, poses, 4)[0] == INV                       # NULL map
    assert _call(sage, m._h, rows, 5, poses, 4, out=None)[0] == INV             # NULL out
    assert _call(sage, m._h, rows, 5, None, 4)[0] == INV                        # NULL poses
    assert _call(sage, m._h, None, 5, poses, 4)[0] == INV                       # NULL rows with n > 0
    assert _call(sage, m._h, rows, 5, poses, (1 << 20) + 1)[0] == INV           # k > 2^20 (before a pose is read)
    assert _call(sage, m._h, rows, (1 << 26) - 3, poses, 4)[0] == INV           # n > 2^26 - 4 (before a row is read)
    for kernel in (0.0, -1.0, float("nan"), float("inf")):
        assert _call(sage, m._h, rows, 5, poses, 4, kernel=kernel)[0] == INV
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 3, 6):
            p = poses.copy()
            p[2, col] = bad
            rc, msg = _call(sage, m._h, rows, 5, p, 4)
            assert rc == INV and "pose 2 of 4" in msg, msg
    # the device entry: the same refusals, and its own
    f = sage.DeviceFrame()
    assert _call(sage, None, None, 0, poses, 4, device_frame=f)[0] == INV
    assert _call(sage, m._h, None, 0, poses, 4, device_frame="null")[0] == INV
    assert _call(sage, m._h, None, 0, None, 4, device_frame=f)[0] == INV
    assert _call(sage, m._h, None, 0, poses, 4, out=None, device_frame=f)[0] == INV
    assert _call(sage, m._h, None, 0, poses, (1 << 20) + 1, device_frame=f)[0] == INV
    assert _call(sage, m._h, None, 0, poses, 4, kernel=0.0, device_frame=f)[0] == INV
    p = poses.copy()
    p[2, 5] = np.nan
    rc, msg = _call(sage, m._h, None, 0, p, 4, device_frame=f)
    assert rc == INV and "pose 2 of 4" in msg
    f.n, f.xyz_dtype, f.xyz, f.xyz_stride = 5, 99, 256, 32                       # a layout no frame has
    assert _call(sage, m._h, None, 0, poses, 4, device_frame=f)[0] == INV
    # k == 0: fine, nothing read or written
    assert _call(sage, None, None, 5, None, 0, out=None)[0] == 0
    assert _call(sage, None, None, 0, None, 0, device_frame="null")[0] == 0


def test_empty_map_and_empty_frame_need_no_device(sage):
    m = sage.VoxelHashMap(1.0, 100.0)
    poses = np.tile(sage.IDENTITY, (3, 1))
    for rows in (np.ones((5, 4)), np.zeros((0, 4))):
        got = m.ScorePoses(rows, poses, 1.0, 0.5, 0.4)
        assert got.shape == (3,) and got.tobytes() == bytes(3 * 488)
    pose, q, info = m.Relocalize(np.ones((5, 4)), PRIOR, 1.0, 0.5, 0.4, xy=(2.0, 1.0))
    assert pose.tobytes() == PRIOR.tobytes() and q.valid == 0 and bytes(q) == bytes(sage.QUALITY_BYTES)
    assert info["candidates"] == 25 and info["refined"] == 0 and info["iterations"] == 0
    with pytest.raises(sage.SageIcpError) as e:
        m.Relocalize(np.ones((5, 4)), PRIOR, 1.0, 0.5, 0.4, refine_top=17)
    assert e.value.code == sage.ERR_INVALID
    with pytest.raises(sage.SageIcpError) as e:
        m.Relocalize(np.ones((5, 4)), PRIOR, 1.0, 0.0, 0.4)
    assert e.value.code == sage.ERR_INVALID


# ---- the reference ranking on the scene of the end-to-end test -----------------------------------------------------------------
def test_reference_ranking_finds_the_basin_with_margins(oracle):
    """The condition under which the GPU test may compare winners, checked: plain registration from the prior is lost,
    the ranking by sum_w over the 637-candidate grid leads into the basin, and the margins between the scores that decide
    are far above fp64 noise (an fp64 sum of <= 2000 positive terms is off by <= 2000 u = 2.3e-13 relative)."""
    m = oracle.Map(sr.VOXEL, 100.0, 20, 20)
    m.add_points(sr.map_points())
    rows, T = sr.scan(), sr.t_gt()
    cands = sr.candidates(sr.PRIOR, **sr.GRID)
    assert len(cands) == sr.GRID_CANDIDATES == 637
    lost, _ = m.register_frame(rows, sr.PRIOR, sr.MD, sr.KERNEL, sr.TH)
    d_lost = sr.pose_error(lost, T)
    print("from the prior: %.3f m / %.3f rad from T_gt" % d_lost)
    assert d_lost[0] > 1.0
    s, pairs = sr.score(m, rows, cands, sr.MD, sr.KERNEL, sr.TH)
    rank = sr.ranking(s)
    m12 = (s[rank[0]] - s[rank[1]]) / s[rank[0]]
    m34 = (s[rank[2]] - s[rank[3]]) / s[rank[2]]
    print("best %d (%.6f), then %d, %d | %d; margins %.3g, %.3g" % (rank[0], s[rank[0]], rank[1], rank[2], rank[3], m12, m34))
    assert m12 >= 1e-6 and m34 >= 1e-6
    refined = []
    for r in rank[:3]:
        pose, _ = m.register_frame(rows, cands[r], sr.MD, sr.KERNEL, sr.TH)
        refined.append(sr.score(m, rows, [pose], sr.MD, sr.KERNEL, sr.TH)[0][0])
        d = sr.pose_error(pose, T)
        print("candidate %d refines to %.4f m / %.2g rad, sum_w %.6f" % (r, d[0], d[1], refined[-1]))
        if r == rank[0]:
            assert d[0] <= 0.05 and d[1] <= 2e-3
    top = sorted(refined)
    assert min((top[1] - top[0]) / top[1], (top[2] - top[1]) / top[2]) >= 1e-6
