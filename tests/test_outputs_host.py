"""Outputs into device memory (sageicp_device_points, csrc/egress.hip) — what is decided without a GPU: the entries exist,
a bad destination is refused before any device query, a fresh pipeline has no source cloud, and the Python binding
refuses a bad tensor before any call into the library."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F0000001000          # never dereferenced: every case below fails before the memory is looked at
U8, I32, I64, F32, F64 = 3, 4, 5, 1, 2


def _points(sage, **kw):
    d = sage.DevicePoints(FAKE, 32, sage.DTYPE_FLOAT64, 0, None, 0, 1000)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD_LAYOUTS = {
    "xyz_dtype_0": dict(xyz_dtype=0),
    "xyz_dtype_uint8": dict(xyz_dtype=U8),
    "xyz_dtype_int32": dict(xyz_dtype=I32),
    "xyz_dtype_int64": dict(xyz_dtype=I64),
    "xyz_dtype_99": dict(xyz_dtype=99),
    "stride_below_3_f64": dict(xyz_stride=16, label=FAKE, label_stride=1, label_dtype=U8),
    "stride_below_3_f32": dict(xyz_dtype=F32, xyz_stride=8, label=FAKE, label_stride=4, label_dtype=F32),
    "stride_3_without_label_column": dict(xyz_stride=24),
    "stride_3_without_label_column_f32": dict(xyz_dtype=F32, xyz_stride=12),
    "stride_not_a_multiple": dict(xyz_stride=36),
    "stride_not_a_multiple_f32": dict(xyz_dtype=F32, xyz_stride=18),
    "stride_0": dict(xyz_stride=0),
    "label_dtype_0": dict(label=FAKE, label_stride=8, label_dtype=0),
    "label_dtype_99": dict(label=FAKE, label_stride=8, label_dtype=99),
    "label_stride_0": dict(label=FAKE, label_stride=0, label_dtype=I64),
    "label_stride_0_uint8": dict(label=FAKE, label_stride=0, label_dtype=U8),
    "label_stride_not_a_multiple_int32": dict(label=FAKE, label_stride=6, label_dtype=I32),
    "label_stride_not_a_multiple_float32": dict(label=FAKE, label_stride=6, label_dtype=F32),
    "label_stride_not_a_multiple_float64": dict(label=FAKE, label_stride=12, label_dtype=F64),
    "label_stride_below_float64": dict(label=FAKE, label_stride=4, label_dtype=F64),
    "xyz_null": dict(xyz=None),
    "xyz_null_with_labels": dict(xyz=None, label=FAKE, label_stride=1, label_dtype=U8),
}


@pytest.fixture
def pipeline(sage):
    return sage.SageICP()


@pytest.fixture
def vmap(sage):
    return sage.VoxelHashMap(1.0, 100.0)


def _entries(sage, pipeline, vmap):
    L = sage.lib()
    return {"source_device": lambda d, n: L.sageicp_pipeline_source_device(pipeline._h, d, None, n),
            "map_pointcloud_device": lambda d, n: L.sageicp_map_pointcloud_device(vmap._h, d, None, n)}


def test_the_three_entries_exist(sage):
    L = sage.lib()
    for name in ("sageicp_pipeline_source", "sageicp_pipeline_source_device", "sageicp_map_pointcloud_device"):
        assert hasattr(L, name), name


@pytest.mark.parametrize("entry", ["source_device", "map_pointcloud_device"])
@pytest.mark.parametrize("case", sorted(BAD_LAYOUTS))
def test_a_bad_destination_is_refused_before_any_device_query(sage, pipeline, vmap, entry, case):
    d = _points(sage, **BAD_LAYOUTS[case])
    n = ctypes.c_uint64(12345)
    assert _entries(sage, pipeline, vmap)[entry](ctypes.byref(d), ctypes.byref(n)) == sage.ERR_INVALID
    msg = sage.lib().sageicp_last_error().decode()
    assert "device points" in msg, msg
    assert "device memory" not in msg          # refused on its layout, not on where it points
    assert n.value == 12345                    # nothing reported for a refused call


@pytest.mark.parametrize("entry", ["source_device", "map_pointcloud_device"])
def test_null_destination_handle_and_count_are_refused(sage, pipeline, vmap, entry):
    L = sage.lib()
    d = _points(sage)
    n = ctypes.c_uint64(0)
    call = _entries(sage, pipeline, vmap)[entry]
    assert call(None, ctypes.byref(n)) == sage.ERR_INVALID
    assert call(ctypes.byref(d), None) == sage.ERR_INVALID
    if entry == "source_device":
        assert L.sageicp_pipeline_source_device(None, ctypes.byref(d), None, ctypes.byref(n)) == sage.ERR_INVALID
    else:
        assert L.sageicp_map_pointcloud_device(None, ctypes.byref(d), None, ctypes.byref(n)) == sage.ERR_INVALID


def test_host_source_refuses_null_arguments(sage, pipeline):
    L = sage.lib()
    n = ctypes.c_uint64(0)
    out = np.empty((4, 4))
    assert L.sageicp_pipeline_source(None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 4,
                                     ctypes.byref(n)) == sage.ERR_INVALID
    assert L.sageicp_pipeline_source(pipeline._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 4,
                                     None) == sage.ERR_INVALID
    assert L.sageicp_pipeline_source(pipeline._h, None, 4, ctypes.byref(n)) == sage.ERR_INVALID


def test_a_fresh_pipeline_has_a_0_row_source(sage, pipeline):
    L = sage.lib()
    n = ctypes.c_uint64(99)
    out = np.full((4, 4), 7.0)
    assert L.sageicp_pipeline_source(pipeline._h, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    n.value = 99
    assert L.sageicp_pipeline_source(pipeline._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 4,
                                     ctypes.byref(n)) == 0
    assert n.value == 0 and (out == 7.0).all()
    # a valid layout of cap 0 asks nothing of the device either
    d = _points(sage, xyz=None, cap=0)
    n.value = 99
    assert L.sageicp_pipeline_source_device(pipeline._h, ctypes.byref(d), None, ctypes.byref(n)) == 0 and n.value == 0
    assert pipeline.source().shape == (0, 4) and pipeline.source().dtype == np.float64
    assert pipeline.source_size() == 0 and pipeline.local_map_size() == 0
    pipeline.reinitialize()
    assert pipeline.source().shape == (0, 4)


def test_a_refused_register_call_leaves_a_0_row_source(sage, pipeline):
    L = sage.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    f = np.zeros((4, 4))
    assert L.sageicp_pipeline_register_frame(pipeline._h, f.ctypes.data_as(dp), 4, None, None, None, None,
                                             None) == sage.ERR_INVALID
    assert L.sageicp_pipeline_register_frame_device(pipeline._h, None, None, None, None, None, None, None,
                                                    None) == sage.ERR_INVALID
    assert pipeline.source_size() == 0


def test_an_empty_map_reports_0_rows_to_a_cap_0_destination(sage, vmap):
    d = _points(sage, xyz=None, cap=0)
    n = ctypes.c_uint64(99)
    assert sage.lib().sageicp_map_pointcloud_device(vmap._h, ctypes.byref(d), None, ctypes.byref(n)) == 0
    assert n.value == 0


def test_local_map_without_arguments_keeps_its_host_rows(sage, pipeline, vmap):
    lm = pipeline.LocalMap()
    assert isinstance(lm, np.ndarray) and lm.shape == (0, 4) and lm.dtype == np.float64
    pc = vmap.Pointcloud()
    assert isinstance(pc, np.ndarray) and pc.shape == (0, 4) and pc.dtype == np.float64


def test_device_points_struct_layout_matches_header(sage):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){printf("%zu", '
           'sizeof(sageicp_device_points));' +
           "".join('printf(" %%zu", offsetof(sageicp_device_points, %s));' % f for f, _ in sage.DevicePoints._fields_) +
           'return 0;}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o",
                               os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[0] == ctypes.sizeof(sage.DevicePoints)
    assert got[1:] == [getattr(sage.DevicePoints, f).offset for f, _ in sage.DevicePoints._fields_]


# ---- the Python binding: refused before any call into the library ------------------------------------------------------
def _no_library_calls(monkeypatch, sage):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sage, "lib", boom)


def _meta(shape, dtype=torch.float64):
    return torch.empty(shape, dtype=dtype, device="meta")


BAD_TENSORS = {
    "cpu_tensor": dict(out=lambda: torch.empty((10, 4), dtype=torch.float64)),
    "numpy_out": dict(out=lambda: np.empty((10, 4))),
    "not_a_gpu": dict(out=lambda: _meta((10, 4))),
    "1-D": dict(out=lambda: _meta(40)),
    "3-D": dict(out=lambda: _meta((10, 4, 1))),
    "3_columns_without_labels": dict(out=lambda: _meta((10, 3))),
    "2_columns_with_labels": dict(out=lambda: _meta((10, 2)), labels_out=lambda: _meta(10, torch.int64)),
    "column_stride_2": dict(out=lambda: _meta((10, 8))[:, ::2]),
    "overlapping_rows": dict(out=lambda: _meta((1, 4)).expand(10, 4)),
    "float16": dict(out=lambda: _meta((10, 4), torch.float16)),
    "int64_points": dict(out=lambda: _meta((10, 4), torch.int64)),
    "float_labels": dict(out=lambda: _meta((10, 4)), labels_out=lambda: _meta(10, torch.float32)),
    "int16_labels": dict(out=lambda: _meta((10, 4)), labels_out=lambda: _meta(10, torch.int16)),
    "2-D_labels": dict(out=lambda: _meta((10, 4)), labels_out=lambda: _meta((10, 1), torch.uint8)),
    "short_labels": dict(out=lambda: _meta((10, 4)), labels_out=lambda: _meta(9, torch.uint8)),
    "long_labels": dict(out=lambda: _meta((10, 4)), labels_out=lambda: _meta(11, torch.int32)),
    "cpu_labels": dict(out=lambda: _meta((10, 4)), labels_out=lambda: torch.zeros(10, dtype=torch.int64)),
    "numpy_labels": dict(out=lambda: _meta((10, 4)), labels_out=lambda: np.zeros(10, dtype=np.uint8)),
    "labels_without_out": dict(labels_out=lambda: _meta(10, torch.uint8)),
    "dtype_mismatch": dict(out=lambda: _meta((10, 4)), dtype=torch.float32),
    "dtype_without_device": dict(dtype=torch.float32),
}


@pytest.mark.parametrize("case", sorted(BAD_TENSORS))
def test_binding_refuses_a_bad_tensor_before_any_library_call(sage, pipeline, vmap, monkeypatch, case):
    kw = {k: (v() if callable(v) else v) for k, v in BAD_TENSORS[case].items()}
    _no_library_calls(monkeypatch, sage)
    for call in (pipeline.source, pipeline.LocalMap, vmap.Pointcloud):
        with pytest.raises(ValueError):
            call(**kw)


@pytest.mark.parametrize("dtype", [torch.float16, torch.int32, np.float32])
def test_binding_refuses_a_device_dtype_it_does_not_write(sage, pipeline, vmap, monkeypatch, dtype):
    _no_library_calls(monkeypatch, sage)
    for call in (pipeline.source, pipeline.LocalMap, vmap.Pointcloud):
        with pytest.raises(ValueError):
            call(device=True, dtype=dtype)
