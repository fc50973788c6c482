"""Frames in device memory (sageicp_device_frame, csrc/ingest.hip) — what is decided without a GPU: the C entries refuse
a bad layout before any device query, and the Python binding refuses a bad tensor before any call into the library."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000001000          # never dereferenced: every case below fails before the memory is looked at


def _frame(sage, **kw):
    f = sage.DeviceFrame(FAKE, 32, sage.DTYPE_FLOAT64, 0, None, 0, 1000)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


BAD_LAYOUTS = {
    "xyz_dtype_0": dict(xyz_dtype=0),
    "xyz_dtype_int64": dict(xyz_dtype=5),
    "xyz_dtype_99": dict(xyz_dtype=99),
    "stride_below_3_f64": dict(xyz_stride=16, label=FAKE, label_stride=1, label_dtype=3),
    "stride_below_3_f32": dict(xyz_dtype=1, xyz_stride=8, label=FAKE, label_stride=1, label_dtype=3),
    "stride_3_without_label_column": dict(xyz_stride=24),
    "stride_not_a_multiple": dict(xyz_stride=36),
    "stride_0": dict(xyz_stride=0),
    "label_dtype_float": dict(label=FAKE, label_stride=8, label_dtype=2),
    "label_dtype_99": dict(label=FAKE, label_stride=8, label_dtype=99),
    "label_stride_0": dict(label=FAKE, label_stride=0, label_dtype=5),
    "label_stride_not_a_multiple": dict(label=FAKE, label_stride=6, label_dtype=4),
    "xyz_null": dict(xyz=None),
    "too_many_points": dict(n=1 << 26),
}


@pytest.fixture
def pipeline(sage):
    return sage.SageICP()


@pytest.fixture
def vmap(sage):
    return sage.VoxelHashMap(1.0, 100.0)


def _register(sage, p, f, ts=None):
    out = np.empty(7)
    icp, tot, ns = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0)
    st = sage.Stats()
    return sage.lib().sageicp_pipeline_register_frame_device(
        p._h, ctypes.byref(f) if f is not None else None, ts, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        ctypes.byref(icp), ctypes.byref(tot), ctypes.byref(ns), ctypes.byref(st))


@pytest.mark.parametrize("case", sorted(BAD_LAYOUTS))
def test_pipeline_entry_refuses_a_bad_layout_before_any_device_query(sage, pipeline, case):
    f = _frame(sage, **BAD_LAYOUTS[case])
    assert _register(sage, pipeline, f) == sage.ERR_INVALID
    msg = sage.lib().sageicp_last_error().decode()
    assert "device frame" in msg or "too large" in msg, msg
    assert "device memory" not in msg          # refused on its layout, not on where it points
    assert sage.lib().sageicp_pipeline_num_poses(pipeline._h) == 0


@pytest.mark.parametrize("case", sorted(BAD_LAYOUTS))
def test_frame_from_device_refuses_a_bad_layout_before_any_device_query(sage, case):
    m = sage.VoxelHashMap(1.0, 100.0)
    f = _frame(sage, **BAD_LAYOUTS[case])
    assert not sage.lib().sageicp_frame_from_device(m._h, ctypes.byref(f), None)
    msg = sage.lib().sageicp_last_error().decode()
    assert "device frame" in msg or "too large" in msg, msg


@pytest.mark.parametrize("case", sorted(BAD_LAYOUTS))
def test_occupancy_grid_device_refuses_a_bad_layout_before_any_device_query(sage, case):
    f = _frame(sage, **BAD_LAYOUTS[case])
    params = sage.occupancy_params()            # valid: only the layout is wrong
    grid = np.zeros(params.occ_h * params.occ_w, dtype=np.uint8)
    assert sage.lib().sageicp_occupancy_grid_device(ctypes.byref(f), None, ctypes.byref(params),
                                                    grid.ctypes.data_as(ctypes.c_void_p), None) == sage.ERR_INVALID
    msg = sage.lib().sageicp_last_error().decode()
    assert "device frame" in msg or "too large" in msg, msg
    assert "device memory" not in msg


def test_null_frame_and_null_handles(sage, pipeline):
    assert _register(sage, pipeline, None) == sage.ERR_INVALID
    f = _frame(sage)
    out = np.empty(7)
    L = sage.lib()
    assert L.sageicp_pipeline_register_frame_device(None, ctypes.byref(f), None, None,
                                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                    None, None, None, None) == sage.ERR_INVALID
    assert L.sageicp_pipeline_register_frame_device(pipeline._h, ctypes.byref(f), None, None, None,
                                                    None, None, None, None) == sage.ERR_INVALID
    m = sage.VoxelHashMap(1.0, 100.0)
    assert not L.sageicp_frame_from_device(m._h, None, None)
    assert not L.sageicp_frame_from_device(None, ctypes.byref(f), None)


def test_device_frame_struct_layout_matches_header(sage):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){printf("%zu", '
           'sizeof(sageicp_device_frame));' +
           "".join('printf(" %%zu", offsetof(sageicp_device_frame, %s));' % f for f, _ in sage.DeviceFrame._fields_) +
           'printf(" %d %d %d %d %d", SAGEICP_DTYPE_FLOAT32, SAGEICP_DTYPE_FLOAT64, SAGEICP_DTYPE_UINT8, '
           'SAGEICP_DTYPE_INT32, SAGEICP_DTYPE_INT64);return 0;}')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o",
                               os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[0] == ctypes.sizeof(sage.DeviceFrame)
    assert got[1:8] == [getattr(sage.DeviceFrame, f).offset for f, _ in sage.DeviceFrame._fields_]
    assert got[8:] == [sage.DTYPE_FLOAT32, sage.DTYPE_FLOAT64, sage.DTYPE_UINT8, sage.DTYPE_INT32, sage.DTYPE_INT64]


# ---- the Python binding: refused before any call into the library ------------------------------------------------------
def _no_library_calls(monkeypatch, sage):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sage, "lib", boom)


META_CASES = {
    "1-D": (lambda: torch.empty(400, device="meta"), None),
    "3-D": (lambda: torch.empty((10, 4, 1), device="meta"), None),
    "3_columns_without_labels": (lambda: torch.empty((10, 3), device="meta"), None),
    "2_columns_with_labels": (lambda: torch.empty((10, 2), device="meta"),
                              lambda: torch.empty(10, dtype=torch.int64, device="meta")),
    "column_stride_2": (lambda: torch.empty((10, 8), device="meta")[:, ::2], None),
    "float16": (lambda: torch.empty((10, 4), dtype=torch.float16, device="meta"), None),
    "int64_points": (lambda: torch.empty((10, 4), dtype=torch.int64, device="meta"), None),
    "float_labels": (lambda: torch.empty((10, 4), device="meta"), lambda: torch.empty(10, device="meta")),
    "2-D_labels": (lambda: torch.empty((10, 4), device="meta"),
                   lambda: torch.empty((10, 1), dtype=torch.uint8, device="meta")),
    "short_labels": (lambda: torch.empty((10, 4), device="meta"),
                     lambda: torch.empty(9, dtype=torch.uint8, device="meta")),
    "numpy_labels": (lambda: torch.empty((10, 4), device="meta"), lambda: np.zeros(10, dtype=np.uint8)),
    "not_a_gpu": (lambda: torch.empty((10, 4), device="meta"), None),
}


@pytest.mark.parametrize("case", sorted(META_CASES))
def test_binding_refuses_a_bad_tensor_before_any_library_call(sage, pipeline, vmap, monkeypatch, case):
    make_pts, make_labels = META_CASES[case]
    pts, labels = make_pts(), (make_labels() if make_labels else None)
    m = vmap
    _no_library_calls(monkeypatch, sage)
    with pytest.raises(ValueError):
        pipeline.RegisterFrame(pts, labels=labels)
    with pytest.raises(ValueError):
        sage.Frame(m, pts, labels=labels)


def test_binding_refuses_bad_device_timestamps_before_any_library_call(sage, pipeline, monkeypatch):
    pts = torch.empty((10, 4), device="meta")
    _no_library_calls(monkeypatch, sage)
    for ts in (np.zeros(10), torch.zeros(10), torch.empty(10, dtype=torch.float32, device="meta"),
               torch.empty(9, dtype=torch.float64, device="meta"),
               torch.empty(20, dtype=torch.float64, device="meta")[::2]):
        with pytest.raises(ValueError):
            pipeline.RegisterFrame(pts, timestamps=ts)


def test_labels_with_host_input_are_refused_before_any_library_call(sage, pipeline, vmap, monkeypatch):
    m = vmap
    frame = np.zeros((10, 4))
    _no_library_calls(monkeypatch, sage)
    for labels in (np.zeros(10, dtype=np.uint8), torch.zeros(10, dtype=torch.int64)):
        for pts in (frame, torch.from_numpy(frame)):
            with pytest.raises(ValueError):
                pipeline.RegisterFrame(pts, labels=labels)
            with pytest.raises(ValueError):
                sage.Frame(m, pts, labels=labels)


def test_one_hip_runtime_check_reads_the_process_maps():
    """Loaded before torch, the library and torch may map two HIP runtimes (a wheel that bundles its own): the check
    refuses exactly then.  Imported first, torch's runtime is the only one.  (No device is touched.)"""
    child = r"""
import sys
sys.path.insert(0, %r)
first = sys.argv[1]
if first == "torch":
    import torch
import sage_icp_amd as sage
sage.lib()
import torch
n = len(set(sage._hip_runtimes().values()))
try:
    sage._check_one_hip_runtime()
    refused = False
except sage.SageIcpError as e:
    refused = True
    assert e.code == sage.ERR_INVALID and "import torch before" in str(e), e
assert refused == (n > 1), (n, refused)
print(n, refused)
""" % ROOT
    results = {}
    for first in ("torch", "library"):
        r = subprocess.run([sys.executable, "-c", child, first], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        results[first] = r.stdout.split()
    assert results["torch"] == ["1", "False"]
