"""Key-frame selection without a GPU: known answers of the restatement tests/keyframe_ref.py (the reference's quirks:
the upper bound as the offset, truncation toward zero, inclusive bounds, H != W orientation, NaN overlap), the header's
new structs against their ctypes mirrors, and the refusals that happen before any device is asked for."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import keyframe_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = ((-10.0, 10.0), (-10.0, 10.0), (-5.0, 5.0))


def _rows(*xyz):
    return np.array([[x, y, z, 0.0] for x, y, z in xyz], dtype=np.float64)


def test_upper_bound_is_the_offset():
    # x_res = 20 / 4 = 5: x = -10 lands in int((-10 + 10) / 5) = 0, x = -5 in 1, x = 0 in 2 (with symmetric bounds
    # the upper and the lower bound give the same offset: the asymmetric box below tells them apart)
    g = kr.grid(_rows((-10.0, -10.0, 0.0), (-5.0, -10.0, 0.0), (0.0, -10.0, 0.0)), SYM, (4, 4))
    assert g[0].tolist() == [1, 1, 1, 0]
    # bounds x in [-60, 50], W = 11: x_res = 10; x = -60 -> (-60 + 50) / 10 = -1.0, not > -1: no cell; x = -55 ->
    # -0.5 -> cell 0 (truncation toward zero); x = -40 -> 1; x = 0 -> 5 (a lower-bound offset would give 6)
    b = ((-60.0, 50.0), (-10.0, 10.0), (-5.0, 5.0))
    g = kr.grid(_rows((-60.0, 0.0, 0.0)), b, (2, 11))
    assert g.sum() == 0
    g = kr.grid(_rows((-55.0, 0.0, 0.0)), b, (2, 11))
    assert g.sum() == 1 and g[:, 0].sum() == 1
    g = kr.grid(_rows((0.0, 0.0, 0.0)), b, (2, 11))
    assert g[:, 5].sum() == 1 and g.sum() == 1
    # x in [-50.5, -50) maps to (-0.05, 0]: cell 0; x = 45 -> 9.5 -> 9; x = 50 -> 10 -> 10 (the last column)
    g = kr.grid(_rows((-50.4, 0.0, 0.0), (45.0, 0.0, 0.0), (50.0, 0.0, 0.0)), b, (2, 11))
    assert g[:, 0].sum() == 1 and g[:, 9].sum() == 1 and g[:, 10].sum() == 1


def test_truncation_cell_of_values_in_minus_one_zero():
    # bounds y in [-60, 50], H = 11: y = -58 -> (-58 + 50) / 10 = -0.8 -> int(-0.8) = 0: row 0
    b = ((-10.0, 10.0), (-60.0, 50.0), (-5.0, 5.0))
    g = kr.grid(_rows((0.0, -58.0, 0.0)), b, (11, 4))
    assert g[0].sum() == 1 and g.sum() == 1
    # y = -50.0 -> 0 exactly, y = -59.99 -> -0.999 -> 0, y = -60.0 -> -1.0: out
    g = kr.grid(_rows((0.0, -50.0, 0.0), (0.0, -59.99, 0.0), (0.0, -60.0, 0.0)), b, (11, 4))
    assert g[0].sum() == 1 and g.sum() == 1


def test_bounds_are_inclusive_and_x_hi_falls_out_as_W():
    # on the bounds: z = -5 and z = 5 pass the filter; x = bx_hi = 10 passes it but occ_x = (10 + 10) / 5 = 4 == W:
    # no cell
    g = kr.grid(_rows((0.0, 0.0, -5.0)), SYM, (4, 4))
    assert g.sum() == 1
    g = kr.grid(_rows((0.0, 0.0, 5.0)), SYM, (4, 4))
    assert g.sum() == 1
    g = kr.grid(_rows((0.0, 0.0, 5.000000000000001)), SYM, (4, 4))
    assert g.sum() == 0
    g = kr.grid(_rows((10.0, 0.0, 0.0)), SYM, (4, 4))
    assert g.sum() == 0
    g = kr.grid(_rows((0.0, 10.0, 0.0)), SYM, (4, 4))
    assert g.sum() == 0
    # the largest double below 10 falls out too: x + bx_hi rounds to 20 before the division
    g = kr.grid(_rows((np.nextafter(10.0, 0.0), 0.0, 0.0)), SYM, (4, 4))
    assert g.sum() == 0
    g = kr.grid(_rows((9.999, 0.0, 0.0)), SYM, (4, 4))
    assert g[:, 3].sum() == 1
    g = kr.grid(_rows((10.000000000000002, 0.0, 0.0), (-10.000000000000002, 0.0, 0.0)), SYM, (4, 4))
    assert g.sum() == 0


def test_rows_are_y_and_columns_are_x():
    # H = 2 rows (y), W = 5 columns (x): x_res = 4, y_res = 10
    g = kr.grid(_rows((-9.0, 1.0, 0.0)), SYM, (2, 5))
    assert g.shape == (2, 5)
    # occ_x = int(1 / 4) = 0, occ_y = int(11 / 10) = 1
    assert g[1, 0] == 1 and g.sum() == 1
    g = kr.grid(_rows((1.0, -9.0, 0.0)), SYM, (2, 5))
    # occ_x = int(11 / 4) = 2, occ_y = int(1 / 10) = 0
    assert g[0, 2] == 1 and g.sum() == 1


def test_overlap_counts_and_nan():
    key = np.array([[1, 1, 0], [0, 1, 0]], dtype=np.uint8)
    cur = np.array([[1, 0, 1], [0, 1, 1]], dtype=np.uint8)
    ov, inter, total = kr.overlap(key, cur)
    assert (inter, total) == (2, 3) and ov == 2.0 / 3.0
    ov, inter, total = kr.overlap(np.zeros((3, 3), np.uint8), np.ones((3, 3), np.uint8))
    assert (inter, total) == (0, 0) and math.isnan(ov)
    assert not (ov < 0.5)          # the node never switches on a NaN overlap


def test_replay_never_switches_after_an_empty_key_grid():
    r = kr.Replay(SYM, (8, 8), 0.9)
    far = _rows((100.0, 100.0, 0.0))
    near = _rows((1.0, 1.0, 0.0), (-3.0, 2.0, 1.0))
    s = r.step(far, [0, 0, 0, 1, 0, 0, 0], 0)
    assert s["is_key_frame"] and math.isnan(s["overlap"]) and s["key_grid"].sum() == 0
    for i in range(1, 4):
        s = r.step(near, [0, 0, 0, 1, 0.1 * i, 0, 0], i)
        assert not s["is_key_frame"] and math.isnan(s["overlap"]) and s["key_frame_index"] == 0


def test_replay_switches_below_the_threshold_and_stores_the_untransformed_grid():
    r = kr.Replay(SYM, (20, 20), 0.5)
    pts = _rows(*[(x, y, 0.0) for x in np.linspace(-9, 9, 10) for y in np.linspace(-9, 9, 10)])
    r.step(pts, [0, 0, 0, 1, 0, 0, 0], 0)
    s = r.step(pts, [0, 0, 0, 1, 0.1, 0, 0], 1)        # a small move: most cells overlap
    assert not s["is_key_frame"] and s["overlap"] > 0.5
    moved = [0, 0, 0, 1, 7.0, 0.0, 0.0]
    s = r.step(pts, moved, 2)
    assert s["is_key_frame"] and s["overlap"] < 0.5 and s["key_frame_index"] == 2
    assert np.array_equal(s["key_grid"], kr.grid(pts, SYM, (20, 20)))
    assert np.array_equal(s["key_pose"], moved)


def test_se3_restatement_inverts():
    a = np.array([0.1, -0.2, 0.3, 0.9, 1.0, 2.0, -3.0])
    a[:4] /= np.linalg.norm(a[:4])
    e = kr.se3_mul(kr.se3_inv(a), a)
    assert np.allclose(e, [0, 0, 0, 1, 0, 0, 0], atol=1e-12)
    p = _rows((1.0, 2.0, 3.0))
    assert np.allclose(kr.transform(kr.se3_inv(a), kr.transform(a, p)), p, atol=1e-12)


def test_header_structs_match_the_ctypes_mirrors(sage):
    fields_p = [f for f, _ in sage.OccupancyParams._fields_]
    fields_i = [f for f, _ in sage.KeyFrameInfo._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){'
           'printf("%zu %zu", sizeof(sageicp_occupancy_params), sizeof(sageicp_key_frame_info));' +
           "".join('printf(" %%zu", offsetof(sageicp_occupancy_params, %s));' % f for f in fields_p) +
           "".join('printf(" %%zu", offsetof(sageicp_key_frame_info, %s));' % f for f in fields_i) +
           'printf(" %d", SAGEICP_ABI_VERSION);return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"),
                               "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[0] == ctypes.sizeof(sage.OccupancyParams) == 64
    assert got[1] == ctypes.sizeof(sage.KeyFrameInfo) == 104
    k = len(fields_p)
    assert got[2:2 + k] == [getattr(sage.OccupancyParams, f).offset for f in fields_p]
    assert got[2 + k:-1] == [getattr(sage.KeyFrameInfo, f).offset for f in fields_i]
    assert got[-1] == sage.ABI_VERSION == 4


def test_launch_file_defaults(sage):
    p = sage.occupancy_params()
    assert [list(b) for b in p.bounds] == [[-51.2, 51.2], [-51.2, 51.2], [-4.0, 2.4]]
    assert (p.occ_h, p.occ_w, p.overlap_th) == (128, 128, 0.5)


@pytest.mark.parametrize("bounds,occ,th", [
    (((-1.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0)), (8, 8), 0.5),
    (((-1.0, float("inf")), (-1.0, 1.0), (-1.0, 1.0)), (8, 8), 0.5),
    (((1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), (8, 8), 0.5),
    (((-1.0, 1.0), (2.0, -2.0), (-1.0, 1.0)), (8, 8), 0.5),
    (((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), (0, 8), 0.5),
    (((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), (8, 4097), 0.5),
    (((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), (8, 8), float("nan")),
    (((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), (8, 8), float("inf")),
])
def test_refused_configurations_before_any_device(sage, bounds, occ, th):
    p = sage.occupancy_params(bounds, occ, th)
    g = np.zeros(occ[0] * occ[1] + 1, dtype=np.uint8)
    rc = sage.lib().sageicp_occupancy_grid(None, 0, None, ctypes.byref(p), g.ctypes.data_as(ctypes.c_void_p), 0)
    assert rc == sage.ERR_INVALID
    assert "occupancy" in sage.lib().sageicp_last_error().decode() or "overlap" in sage.lib().sageicp_last_error().decode()


def test_pipeline_key_frame_entries_refuse_null(sage):
    L = sage.lib()
    info = sage.KeyFrameInfo()
    assert L.sageicp_pipeline_key_frame_info(None, ctypes.byref(info)) == sage.ERR_INVALID
    assert L.sageicp_pipeline_key_frame_reset(None) == sage.ERR_INVALID
    assert L.sageicp_pipeline_set_key_frames(None, 1, None) == sage.ERR_INVALID
    assert L.sageicp_pipeline_key_frame_grid(None, None, 0) == sage.ERR_INVALID
