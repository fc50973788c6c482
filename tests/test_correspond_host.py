"""GetCorrespondences on a device frame into device memory (sageicp_get_correspondences_device, csrc/correspond.hip) —
what is decided without a GPU: the entry exists, and everything wrong with its arguments that can be known on the host
is refused before any device query (FAKE pointers are never looked at); the Python binding refuses bad arguments before
any call into the library."""
import ctypes

import numpy as np
import pytest
import torch

from test_outputs_host import BAD_LAYOUTS, FAKE, U8

# (test_outputs_host's table of bad layouts serves the frame as well: what it does to a destination a frame refuses too —
# the float label types it uses in well-formed places are no label types of a frame)
POSE = (0.0, 0.0, 0.0, 1.0, 0.5, -0.25, 0.125)


@pytest.fixture
def vmap(sage):
    return sage.VoxelHashMap(1.0, 100.0)


def _points(sage, base=FAKE, **kw):
    d = sage.DevicePoints(base, 32, sage.DTYPE_FLOAT64, 0, None, 0, 1000)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _frame(sage, **kw):
    f = sage.DeviceFrame(FAKE + (1 << 30), 32, sage.DTYPE_FLOAT64, 0, None, 0, 1000)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _call(sage, vmap, frame="default", pose=None, src="default", tgt="default", idx=FAKE + (3 << 20), idx_cap=1000,
          n_out="default", handle="default"):
    """the entry with valid FAKE arguments (three destinations 1 MiB apart, 32 000 B each), one or more replaced"""
    frame = _frame(sage) if frame == "default" else frame
    src = _points(sage, FAKE + (1 << 20)) if src == "default" else src
    tgt = _points(sage, FAKE + (2 << 20)) if tgt == "default" else tgt
    n = ctypes.c_uint64(12345)
    pp = None if pose is None else np.asarray(pose, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = sage.lib().sageicp_get_correspondences_device(
        vmap._h if handle == "default" else handle, None if frame is None else ctypes.byref(frame), pp, 1.0, 0.5,
        None if src is None else ctypes.byref(src), None if tgt is None else ctypes.byref(tgt), idx, idx_cap, None,
        ctypes.byref(n) if n_out == "default" else n_out)
    return rc, sage.lib().sageicp_last_error().decode(), n.value


def _refused_on_the_host(sage, rc, msg, n):
    assert rc == sage.ERR_INVALID, (rc, msg)
    assert "device memory" not in msg and "no HIP device" not in msg, msg      # not on where anything points
    assert n == 12345                                                         # nothing reported for a refused call


def test_the_entry_exists(sage):
    assert hasattr(sage.lib(), "sageicp_get_correspondences_device")
    assert sage.lib().sageicp_abi_version() == 4


@pytest.mark.parametrize("which", ["src", "tgt"])
@pytest.mark.parametrize("case", sorted(BAD_LAYOUTS))
def test_a_bad_destination_is_refused_before_any_device_query(sage, vmap, which, case):
    rc, msg, n = _call(sage, vmap, **{which: _points(sage, FAKE + (1 << 20), **BAD_LAYOUTS[case])})
    _refused_on_the_host(sage, rc, msg, n)
    assert "device points" in msg, msg


@pytest.mark.parametrize("case", sorted(BAD_LAYOUTS))
def test_a_bad_frame_is_refused_before_any_device_query(sage, vmap, case):
    rc, msg, n = _call(sage, vmap, frame=_frame(sage, **BAD_LAYOUTS[case]))
    _refused_on_the_host(sage, rc, msg, n)
    assert "device frame" in msg, msg


def test_a_frame_refuses_float_labels_and_too_many_rows(sage, vmap):
    for kw in (dict(label=FAKE, label_stride=4, label_dtype=sage.DTYPE_FLOAT32),
               dict(label=FAKE, label_stride=8, label_dtype=sage.DTYPE_FLOAT64), dict(n=(1 << 26) - 3)):
        _refused_on_the_host(sage, *_call(sage, vmap, frame=_frame(sage, **kw)))


@pytest.mark.parametrize("caps", [(1000, 999, 1000), (1000, 1000, 999), (999, 1000, 1000), (0, 1000, 1000)])
def test_unequal_caps_are_refused(sage, vmap, caps):
    rc, msg, n = _call(sage, vmap, src=_points(sage, FAKE + (1 << 20), cap=caps[0]),
                       tgt=_points(sage, FAKE + (2 << 20), cap=caps[1]), idx_cap=caps[2])
    _refused_on_the_host(sage, rc, msg, n)
    assert "equal" in msg, msg


def test_caps_of_absent_destinations_are_not_compared(sage, vmap):
    # (an index capacity without an index array says nothing; the call goes on to ask for the device)
    rc, msg, _ = _call(sage, vmap, idx=None, idx_cap=7)
    assert "equal" not in msg, msg


@pytest.mark.parametrize("off", [1, 2, 4, 7])
def test_a_misaligned_index_pointer_is_refused(sage, vmap, off):
    rc, msg, n = _call(sage, vmap, idx=FAKE + (3 << 20) + off)
    _refused_on_the_host(sage, rc, msg, n)
    assert "8-byte aligned" in msg, msg


OVERLAPS = {
    "src_is_tgt": dict(src=(0, {}), tgt=(0, {})),
    "tgt_starts_inside_src": dict(src=(0, {}), tgt=(31992, {})),
    "tgt_ends_inside_src": dict(src=(32000 - 8, {}), tgt=(0, {})),
    "interleaved_rows": dict(src=(0, dict(xyz_stride=64)), tgt=(32, dict(xyz_stride=64))),
    "idx_inside_src": dict(src=(0, {}), idx=16000),
    "idx_tail_inside_tgt": dict(tgt=(8000 - 8, {}), idx=0),
    "tgt_labels_inside_src": dict(src=(0, {}), tgt=(1 << 20, dict(label=FAKE + 100, label_stride=1, label_dtype=U8,
                                                                  xyz_stride=24))),
    "src_labels_inside_idx": dict(src=(1 << 20, dict(label=FAKE + (2 << 20) + 7999, label_stride=8, label_dtype=5,
                                                     xyz_stride=24)), idx=2 << 20),
}


@pytest.mark.parametrize("case", sorted(OVERLAPS))
def test_overlapping_destinations_are_refused(sage, vmap, case):
    c = OVERLAPS[case]
    kw = {}
    for which, default in (("src", 5 << 20), ("tgt", 6 << 20)):
        off, fields = c.get(which, (default, {}))
        kw[which] = _points(sage, FAKE + off, **fields)
    kw["idx"] = FAKE + c.get("idx", 7 << 20)
    rc, msg, n = _call(sage, vmap, **kw)
    _refused_on_the_host(sage, rc, msg, n)
    assert "overlap" in msg, msg


def test_destinations_that_touch_do_not_overlap(sage, vmap):
    # back to back, and a destination's own labels inside its own rows' stride: past the host's checks
    rc, msg, _ = _call(sage, vmap, src=_points(sage, FAKE), tgt=_points(sage, FAKE + 32000), idx=FAKE + 64000)
    assert "overlap" not in msg, msg
    rc, msg, _ = _call(sage, vmap, src=_points(sage, FAKE, xyz_stride=32, label=FAKE + 24, label_stride=32, label_dtype=5))
    assert "overlap" not in msg, msg


def test_a_destination_may_alias_the_frame(sage, vmap):
    rc, msg, _ = _call(sage, vmap, frame=_frame(sage, xyz=FAKE), src=_points(sage, FAKE))
    assert "overlap" not in msg, msg


def test_null_arguments_are_refused(sage, vmap):
    _refused_on_the_host(sage, *_call(sage, vmap, frame=None))
    _refused_on_the_host(sage, *_call(sage, vmap, handle=None))
    _refused_on_the_host(sage, *_call(sage, vmap, n_out=None))


@pytest.mark.parametrize("at", range(7))
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_pose_that_is_not_finite_is_refused(sage, vmap, at, bad):
    pose = list(POSE)
    pose[at] = bad
    rc, msg, n = _call(sage, vmap, pose=pose)
    _refused_on_the_host(sage, rc, msg, n)
    assert "pose" in msg, msg


def test_three_nulls_on_an_empty_frame_count_0_pairs_without_a_device(sage, vmap):
    rc, msg, n = _call(sage, vmap, frame=_frame(sage, xyz=None, n=0), src=None, tgt=None, idx=None, idx_cap=0)
    assert rc == 0 and n == 0, msg


# ---- the Python binding: refused before any call into the library ------------------------------------------------------
def _no_library_calls(monkeypatch, sage):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sage, "lib", boom)


def _meta(shape, dtype=torch.float64):
    return torch.empty(shape, dtype=dtype, device="meta")


def test_host_input_refuses_the_device_arguments(sage, vmap, monkeypatch):
    _no_library_calls(monkeypatch, sage)
    q = np.zeros((4, 4))
    for kw in (dict(labels=np.zeros(4, dtype=np.uint8)), dict(pose=POSE), dict(dtype=torch.float32)):
        with pytest.raises(ValueError):
            vmap.GetCorrespondences(q, 1.0, 0.5, **kw)
        with pytest.raises(ValueError):
            vmap.GetCorrespondences(torch.zeros((4, 4), dtype=torch.float64), 1.0, 0.5, **kw)


BAD_FRAMES = {
    "not_a_gpu": dict(pts=lambda: _meta((10, 4))),
    "1-D": dict(pts=lambda: _meta(40)),
    "3-D": dict(pts=lambda: _meta((10, 4, 1))),
    "3_columns_without_labels": dict(pts=lambda: _meta((10, 3))),
    "2_columns_with_labels": dict(pts=lambda: _meta((10, 2)), labels=lambda: _meta(10, torch.int64)),
    "column_stride_2": dict(pts=lambda: _meta((10, 8))[:, ::2]),
    "float16": dict(pts=lambda: _meta((10, 4), torch.float16)),
    "int64_points": dict(pts=lambda: _meta((10, 4), torch.int64)),
    "float_labels": dict(pts=lambda: _meta((10, 4)), labels=lambda: _meta(10, torch.float32)),
    "int16_labels": dict(pts=lambda: _meta((10, 4)), labels=lambda: _meta(10, torch.int16)),
    "2-D_labels": dict(pts=lambda: _meta((10, 4)), labels=lambda: _meta((10, 1), torch.uint8)),
    "short_labels": dict(pts=lambda: _meta((10, 4)), labels=lambda: _meta(9, torch.uint8)),
    "cpu_labels": dict(pts=lambda: _meta((10, 4)), labels=lambda: torch.zeros(10, dtype=torch.int64)),
    "numpy_labels": dict(pts=lambda: _meta((10, 4)), labels=lambda: np.zeros(10, dtype=np.uint8)),
}


@pytest.mark.parametrize("case", sorted(BAD_FRAMES))
def test_binding_refuses_a_bad_frame_before_any_library_call(sage, vmap, monkeypatch, case):
    kw = {k: v() for k, v in BAD_FRAMES[case].items()}
    _no_library_calls(monkeypatch, sage)
    with pytest.raises(ValueError):
        vmap.GetCorrespondences(kw.pop("pts"), 1.0, 0.5, **kw)


def test_binding_words_a_bad_frame_as_every_device_frame(sage, vmap):
    with pytest.raises(ValueError, match="a device frame is float32 or float64"):
        vmap.GetCorrespondences(_meta((10, 4), torch.float16), 1.0, 0.5)
    with pytest.raises(ValueError, match="the frame is on meta"):
        vmap.GetCorrespondences(_meta((10, 4)), 1.0, 0.5)
