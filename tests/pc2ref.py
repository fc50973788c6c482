"""An independent numpy restatement of the odometry node's PointCloud2 conversions (ros/ros2/Utils.hpp:55-198), for the
message tests: blobs of any layout are built and read through structured dtypes with explicit offsets and itemsize; the
21-byte packer looks colours up in a dict.  Everything here is exact: casts float32 -> float64 and uint -> float64 lose
nothing, numpy's float64 division is correctly rounded, packing is data movement."""
import numpy as np

# sensor_msgs/PointField datatype codes
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = 1, 2, 3, 4, 5, 6, 7, 8
NP_OF = {UINT8: "u1", UINT32: "<u4", FLOAT32: "<f4", FLOAT64: "<f8"}

# CreatePointCloud2Msg, Utils.hpp:104-128: (name, offset, datatype, count); point_step 21
OUTPUT_FIELDS = [("x", 0, FLOAT32, 1), ("y", 4, FLOAT32, 1), ("z", 8, FLOAT32, 1), ("label", 12, UINT8, 1),
                 ("rgb", 13, UINT32, 1)]
OUTPUT_STEP = 21


def record_dtype(fields, point_step):
    """fields: [(name, offset, datatype code)]; a structured dtype of itemsize point_step (unaligned fields allowed)"""
    return np.dtype({"names": [f[0] for f in fields], "formats": [NP_OF[f[2]] for f in fields],
                     "offsets": [f[1] for f in fields], "itemsize": point_step})


def build_blob(fields, point_step, columns, n, fill=0xA5):
    """n records as a 1-D uint8 array; columns: {name: values}; the bytes no field covers are `fill`"""
    raw = np.full(n * point_step, fill, dtype=np.uint8)
    rec = raw.view(record_dtype(fields, point_step)) if n else None
    for name, v in columns.items():
        if n:
            rec[name] = v
    return raw


def read_rows(blob, fields, point_step, n):
    """PointCloud2ToEigen: (n, 4) float64 of x, y, z, label, each a plain cast"""
    rec = np.asarray(blob, dtype=np.uint8)[:n * point_step].view(record_dtype(fields, point_step))
    out = np.empty((n, 4), dtype=np.float64)
    for k, name in enumerate(("x", "y", "z", "label")):
        out[:, k] = rec[name].astype(np.float64)
    return out


def normalize_timestamps(t):
    """NormalizeTimestamps, Utils.hpp:68-77"""
    t = np.asarray(t, dtype=np.float64)
    if t.size == 0:
        return t.copy()
    m = t.max()
    return t.copy() if m < 1.0 else t / m


def read_timestamps(blob, fields, point_step, n, name):
    """GetTimestamps: uint32 stamps of 't' / 'timestamp' normalised, float64 stamps of 'time' as they are"""
    rec = np.asarray(blob, dtype=np.uint8)[:n * point_step].view(record_dtype(fields, point_step))
    if name in ("t", "timestamp"):
        return normalize_timestamps(rec[name].astype(np.float64))
    return rec[name].astype(np.float64)


def pack(rows, colors):
    """EigenToPointCloud2's data: (n, 21) uint8.  colors: {int: int}.  KeyError where the reference's .at throws;
    ValueError where static_cast<uint8_t> is undefined (trunc(label) outside [0, 255])"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    n = len(rows)
    out = np.zeros(n, dtype=record_dtype([(f[0], f[1], f[2]) for f in OUTPUT_FIELDS], OUTPUT_STEP))
    lab = np.trunc(rows[:, 3])
    if n and (lab.min() < 0 or lab.max() > 255):
        raise ValueError("label outside [0, 255]")
    lab = lab.astype(np.int64)
    out["x"], out["y"], out["z"] = rows[:, 0].astype(np.float32), rows[:, 1].astype(np.float32), rows[:, 2].astype(np.float32)
    out["label"] = lab.astype(np.uint8)
    out["rgb"] = np.array([colors[int(l)] & 0xFFFFFFFF for l in lab], dtype=np.uint32)
    return out.view(np.uint8).reshape(n, OUTPUT_STEP)
