"""sensor_msgs/PointCloud2 at the library's two ends, the part that needs no device: the reference's
field-name rules in the Python binding and in the C++ header (sage-icp_amd/shim_ros/sageicp_msg.hpp, on a stub message
type), every refusal of the C ABI that comes before a device is looked for, the outgoing record's field table, and the
empty frame."""
import array
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pc2ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64, U8, U32 = pc2ref.FLOAT32, pc2ref.FLOAT64, pc2ref.UINT8, pc2ref.UINT32
XYZ = [("x", 0, F32), ("y", 4, F32), ("z", 8, F32)]
NO_TIME = "Field 't', 'timestamp', or 'time'  does not exist"         # ros/ros2/Utils.hpp:63, as written there


def _msg(sage, fields, step, n=0, data=b"", **kw):
    return sage.PointCloud2([sage.PointField(*f) for f in fields], step, data, width=n, **kw)


def _lay(l):
    return (l.point_step, l.x_offset, l.y_offset, l.z_offset, l.label_offset, l.label_dtype, l.time_kind, l.time_offset)


# ---- field-name rules, Python binding ---------------------------------------------------------------------------------
def test_five_fields_read_a_uint8_label_any_other_count_a_float32_one(sage):
    five = _msg(sage, XYZ + [("label", 12, U8), ("rgb", 13, U32)], 21)
    assert _lay(sage.pointcloud2_layout(five, False)) == (21, 0, 4, 8, 12, sage.DTYPE_UINT8, 0, 0)
    four = _msg(sage, XYZ + [("label", 12, F32)], 16)
    assert _lay(sage.pointcloud2_layout(four, False)) == (16, 0, 4, 8, 12, sage.DTYPE_FLOAT32, 0, 0)
    six = _msg(sage, [("pad", 0, U8), ("x", 1, F32), ("y", 5, F32), ("z", 9, F32), ("label", 13, F32), ("ring", 17, U8)], 22)
    assert _lay(sage.pointcloud2_layout(six, False)) == (22, 1, 5, 9, 13, sage.DTYPE_FLOAT32, 0, 0)
    # the switch is on the COUNT: a float32 label in five fields, a uint8 label in four, would be reinterpreted
    with pytest.raises(ValueError, match="'label'.*FLOAT32.*UINT8.*five"):
        sage.pointcloud2_layout(_msg(sage, XYZ + [("label", 12, F32), ("rgb", 16, U32)], 20), False)
    with pytest.raises(ValueError, match="'label'.*UINT8.*FLOAT32.*4 fields"):
        sage.pointcloud2_layout(_msg(sage, XYZ + [("label", 12, U8)], 13), False)


def test_the_last_time_field_wins_and_its_name_decides_the_kind(sage):
    base = XYZ + [("label", 12, F32)]
    m = _msg(sage, base + [("t", 16, U32), ("time", 24, F64)], 32)
    assert _lay(sage.pointcloud2_layout(m, True))[6:] == (2, 24)
    assert _lay(sage.pointcloud2_layout(m, False))[6:] == (0, 0)           # not asked for: not looked at
    m = _msg(sage, base + [("time", 16, F64), ("timestamp", 24, U32)], 28)
    assert _lay(sage.pointcloud2_layout(m, True))[6:] == (1, 24)
    # (x, y, z, label, t are five fields: the label of such a message is read as UINT8)
    m = _msg(sage, XYZ + [("label", 12, U8), ("t", 16, U32)], 20)
    assert _lay(sage.pointcloud2_layout(m, True)) == (20, 0, 4, 8, 12, sage.DTYPE_UINT8, 1, 16)


def test_refusals_name_the_field(sage):
    base = XYZ + [("label", 12, F32)]
    with pytest.raises(ValueError) as e:
        sage.pointcloud2_layout(_msg(sage, base, 16), True)
    assert str(e.value) == NO_TIME
    sage.pointcloud2_layout(_msg(sage, base, 16), False)                    # raised only when stamps are asked for
    ring = base + [("ring", 16, U8)]                                        # (six fields with the time field)
    with pytest.raises(ValueError, match="'t' is declared FLOAT64.*UINT32"):
        sage.pointcloud2_layout(_msg(sage, ring + [("t", 20, F64)], 28), True)
    with pytest.raises(ValueError, match="'timestamp' is declared FLOAT32.*UINT32"):
        sage.pointcloud2_layout(_msg(sage, ring + [("timestamp", 20, F32)], 24), True)
    with pytest.raises(ValueError, match="'time' is declared UINT32.*FLOAT64"):
        sage.pointcloud2_layout(_msg(sage, ring + [("time", 20, U32)], 24), True)
    for k, name in enumerate("xyz"):
        f = [list(x) for x in base]
        f[k][2] = F64
        with pytest.raises(ValueError, match="'%s' is declared FLOAT64.*FLOAT32" % name):
            sage.pointcloud2_layout(_msg(sage, f, 24), False)
    for missing in ("x", "y", "z", "label"):
        with pytest.raises(ValueError, match="Field %s does not exist" % missing):
            sage.pointcloud2_layout(_msg(sage, [f for f in base if f[0] != missing], 16), False)
    with pytest.raises(ValueError, match="big-endian"):
        sage.pointcloud2_layout(_msg(sage, base, 16, is_bigendian=True), False)


def test_register_frame_of_a_message_refuses_timestamps_and_labels(sage):
    p = sage.SageICP()
    m = _msg(sage, XYZ + [("label", 12, F32)], 16)
    with pytest.raises(ValueError):
        p.RegisterFrame(m, timestamps=np.zeros(0))
    with pytest.raises(ValueError):
        p.RegisterFrame(m, labels=np.zeros(0))


# ---- field-name rules, C++ binding -------------------------------------------------------------------------------------
def test_cpp_binding_applies_the_same_rules(sage, tmp_path):
    exe = str(tmp_path / "msg_user")
    lib_dir = os.path.join(ROOT, "sage-icp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "sage-icp_amd", "shim_ros"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim_stubs", "msg_user.cpp"),
                           "-L", lib_dir, "-l:libsageicp_hip.so", "-Wl,-rpath," + lib_dir, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    u8, f32 = sage.DTYPE_UINT8, sage.DTYPE_FLOAT32
    assert got["five_u8"] == "ok step=21 x=0 y=4 z=8 label=12/%d time=0/0" % u8
    assert got["four_f32"] == "ok step=16 x=0 y=4 z=8 label=12/%d time=0/0" % f32
    assert got["five_f32"].startswith("error: field 'label' is declared FLOAT32; it is read as UINT8")
    assert got["four_u8"].startswith("error: field 'label' is declared UINT8; it is read as FLOAT32")
    assert got["x_f64"].startswith("error: field 'x' is declared FLOAT64; it is read as FLOAT32")
    assert got["no_label"] == "error: Field label does not exist"
    assert got["last_time"] == "ok step=32 x=0 y=4 z=8 label=12/%d time=2/24" % f32
    assert got["time_not_asked"] == "ok step=32 x=0 y=4 z=8 label=12/%d time=0/0" % f32
    assert got["last_t"] == "ok step=28 x=0 y=4 z=8 label=12/%d time=1/24" % f32
    assert got["no_time"] == "error: " + NO_TIME
    assert got["t_f64"].startswith("error: field 't' is declared FLOAT64; it is read as UINT32")
    assert got["time_u32"].startswith("error: field 'time' is declared UINT32; it is read as FLOAT64")
    assert got["five_with_t"] == "ok step=20 x=0 y=4 z=8 label=12/%d time=1/16" % u8
    assert "big-endian" in got["bigendian"]
    fields = "".join("%s:%d:%d:%d," % f for f in pc2ref.OUTPUT_FIELDS)
    assert got["prepare_output"] == "step=21 width=7 height=1 row_step=147 data=147 fields=" + fields
    assert got["round_trip"] == "ok step=21 x=0 y=4 z=8 label=12/%d time=0/0" % u8
    assert got["colors"] == "n=3"
    assert got["empty_frame"] == "ok n_source=0 poses=1"
    assert got["empty_source"] == "ok width=0 data=0"
    # the Python binding words its refusals the same way
    with pytest.raises(ValueError) as e:
        sage.pointcloud2_layout(_msg(sage, XYZ + [("label", 12, F32), ("rgb", 16, U32)], 20), False)
    assert got["five_f32"] == "error: " + str(e.value)


# ---- validation through the C ABI, no device present -----------------------------------------------------------------
def _layout(sage, **kw):
    l = sage.MsgLayout(16, 0, 4, 8, 12, sage.DTYPE_FLOAT32, 0, 0)
    for k, v in kw.items():
        setattr(l, k, v)
    return l


BAD_LAYOUTS = {
    "point_step_0": dict(point_step=0),
    "point_step_1025": dict(point_step=1025),
    "x_ends_beyond": dict(x_offset=13),
    "y_ends_beyond": dict(y_offset=14),
    "z_ends_beyond": dict(z_offset=0xFFFFFFFE),
    "f32_label_ends_beyond": dict(label_offset=13),
    "u8_label_ends_beyond": dict(label_offset=16, label_dtype=3),
    "label_dtype_float64": dict(label_dtype=2),
    "label_dtype_int32": dict(label_dtype=4),
    "label_dtype_0": dict(label_dtype=0),
    "time_kind_3": dict(time_kind=3),
    "time_kind_negative": dict(time_kind=-1),
    "u32_time_ends_beyond": dict(time_kind=1, time_offset=13),
    "f64_time_ends_beyond": dict(time_kind=2, time_offset=9),
}


def _call(sage, p, data, data_bytes, n, layout, device):
    L = sage.lib()
    pose = np.empty(7)
    dp = ctypes.POINTER(ctypes.c_double)
    lp = ctypes.byref(layout) if layout is not None else None
    if device:
        return L.sageicp_pipeline_register_frame_msg_device(p._h, data, data_bytes, n, lp, None, pose.ctypes.data_as(dp),
                                                            None, None, None, None)
    return L.sageicp_pipeline_register_frame_msg(p._h, data, data_bytes, n, lp, pose.ctypes.data_as(dp), None, None, None,
                                                 None)


@pytest.mark.parametrize("device", [False, True], ids=["host_blob", "device_blob"])
@pytest.mark.parametrize("case", sorted(BAD_LAYOUTS))
def test_a_bad_layout_is_refused_before_any_device_is_looked_for(sage, case, device):
    p = sage.SageICP()
    blob = np.zeros(16 * 8, dtype=np.uint8)
    assert _call(sage, p, blob.ctypes.data, blob.size, 8, _layout(sage, **BAD_LAYOUTS[case]), device) == sage.ERR_INVALID, \
        sage.lib().sageicp_last_error()
    assert "device" not in sage.lib().sageicp_last_error().decode()
    assert len(p.poses()) == 0


@pytest.mark.parametrize("device", [False, True], ids=["host_blob", "device_blob"])
def test_bad_arguments_are_refused_before_any_device_is_looked_for(sage, device):
    p = sage.SageICP()
    L = sage.lib()
    blob = np.zeros(16 * 8, dtype=np.uint8)
    ok = _layout(sage)
    assert _call(sage, p, blob.ctypes.data, blob.size, 8, None, device) == sage.ERR_INVALID              # NULL layout
    assert "layout" in L.sageicp_last_error().decode()
    assert _call(sage, p, blob.ctypes.data, blob.size - 1, 8, ok, device) == sage.ERR_INVALID           # one byte short
    assert "n * point_step" in L.sageicp_last_error().decode()
    assert _call(sage, p, blob.ctypes.data, 1 << 40, (1 << 26) - 3, ok, device) == sage.ERR_INVALID     # n > 2^26 - 4
    assert "too large" in L.sageicp_last_error().decode()
    assert _call(sage, p, None, blob.size, 8, ok, device) == sage.ERR_INVALID                            # NULL data, n > 0
    assert "NULL" in L.sageicp_last_error().decode()
    # deskew on and no time field: refused, no pose pushed
    p.set_deskew(True)
    assert _call(sage, p, blob.ctypes.data, blob.size, 8, ok, device) == sage.ERR_INVALID
    assert "time" in L.sageicp_last_error().decode()
    assert len(p.poses()) == 0
    # a valid message gets as far as the device
    p.set_deskew(False)
    if sage.device_count() < 1:
        assert _call(sage, p, blob.ctypes.data, blob.size, 8, ok, device) == sage.ERR_NO_DEVICE


def test_a_colour_table_with_null_arrays_is_refused(sage):
    p = sage.SageICP()
    L = sage.lib()
    n = ctypes.c_uint64(7)
    out = np.zeros(21, dtype=np.uint8)
    keys = (ctypes.c_int32 * 2)(1, 2)
    h = L.sageicp_pipeline_local_map(p._h)
    for c in (sage.MsgColors(None, None, 2), sage.MsgColors(keys, None, 2), sage.MsgColors(None, keys, 2)):
        assert L.sageicp_pipeline_source_msg(p._h, ctypes.byref(c), out.ctypes.data, 1, ctypes.byref(n)) == sage.ERR_INVALID
        assert L.sageicp_pipeline_source_msg_device(p._h, ctypes.byref(c), out.ctypes.data, 1, None,
                                                    ctypes.byref(n)) == sage.ERR_INVALID
        assert L.sageicp_map_pointcloud_msg(h, ctypes.byref(c), out.ctypes.data, 1, ctypes.byref(n)) == sage.ERR_INVALID
        assert L.sageicp_map_pointcloud_msg_device(h, ctypes.byref(c), out.ctypes.data, 1, None,
                                                   ctypes.byref(n)) == sage.ERR_INVALID
        assert "colour" in L.sageicp_last_error().decode()
    # an empty table and no table are fine: nothing to write yet, so nothing to look up
    for c in (sage.MsgColors(None, None, 0), None):
        cp = ctypes.byref(c) if c is not None else None
        assert L.sageicp_pipeline_source_msg(p._h, cp, out.ctypes.data, 1, ctypes.byref(n)) == 0 and n.value == 0
        assert L.sageicp_map_pointcloud_msg(h, cp, out.ctypes.data, 1, ctypes.byref(n)) == 0 and n.value == 0
    assert not out.any()
    assert p.source_msg({}).shape == (0, 21) and p.LocalMapMsg({40: 1}).shape == (0, 21)
    assert sage.VoxelHashMap(1.0, 100.0).PointcloudMsg(None).shape == (0, 21)


# ---- the outgoing record's field table -----------------------------------------------------------------------------------
def test_output_field_table(sage):
    got = [(f.name, f.offset, f.datatype, f.count) for f in sage.msg_output_fields()]
    assert got == pc2ref.OUTPUT_FIELDS
    assert [f[1] for f in got] == [0, 4, 8, 12, 13] and sage.MSG_POINT_STEP == pc2ref.OUTPUT_STEP == 21
    # a cap below the count: the count comes back, only `cap` entries are written
    buf = (sage.MsgField * 3)()
    assert sage.lib().sageicp_msg_output_fields(buf, 2) == 5
    assert buf[1].name == b"y" and buf[2].name == b""
    assert sage.lib().sageicp_msg_output_fields(None, 0) == 5
    # pc2ref's packer writes that layout
    rec = pc2ref.pack([[1.5, -2.25, 3.0, 40.9]], {40: -2})
    assert rec.shape == (1, 21)
    assert rec[0, :12].tobytes() == np.array([1.5, -2.25, 3.0], dtype="<f4").tobytes()
    assert rec[0, 12] == 40 and rec[0, 13:17].tobytes() == b"\xfe\xff\xff\xff" and not rec[0, 17:].any()
    m = sage.output_pointcloud2(rec)
    assert (m.point_step, m.width, m.height, m.row_step) == (21, 1, 1, 21)
    assert _lay(sage.pointcloud2_layout(m, False)) == (21, 0, 4, 8, 12, sage.DTYPE_UINT8, 0, 0)


# ---- the empty frame -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deskew", [False, True])
def test_an_empty_frame_succeeds_on_both_paths_without_a_device(sage, deskew):
    fields = XYZ + [("label", 12, F32), ("ring", 16, U8), ("t", 20, U32)]
    lay = sage.MsgLayout(24, 0, 4, 8, 12, sage.DTYPE_FLOAT32, 1, 20)
    for device in (False, True):
        p = sage.SageICP()
        p.set_deskew(deskew)
        assert _call(sage, p, None, 0, 0, lay, device) == 0, sage.lib().sageicp_last_error()
        assert len(p.poses()) == 1 and np.array_equal(p.poses()[0], sage.IDENTITY)
        assert p.source_size() == 0
    # through the binding, with every kind of host data
    for data in (b"", bytearray(), array.array("B"), np.zeros(0, dtype=np.uint8)):
        p = sage.SageICP()
        p.set_deskew(deskew)
        pose, _, _, n_source, _ = p.RegisterFrame(_msg(sage, fields, 24, 0, data))
        assert np.array_equal(pose, sage.IDENTITY) and n_source == 0 and len(p.poses()) == 1
        assert p.source_msg({0: 0}).shape == (0, 21)
