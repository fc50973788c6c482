"""ctypes front of tests/dynfilter_ref.cpp, the independent CPU restatement of Preprocess() with the dynamic vehicle
filter on (core/Preprocessing.cpp:95-172).  Compiled once per process with g++ -O2 -ffp-contract=off into a temporary
directory (nothing is written into the tree)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dynfilter_ref.cpp")
KITTI_VEHICLES = (10, 11, 13, 15, 16, 18, 20)
_lib = []


def lib():
    if not _lib:
        d = tempfile.mkdtemp(prefix="dynref_")
        so = os.path.join(d, "dynref.so")
        flags = ["-DSQNORM_A"] if os.environ.get("SAGE_SQNORM3_ORDER", "2") == "0" else []
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra",
                               "-Werror"] + flags + [SRC, "-o", so])
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int)
        L.dynref_preprocess.restype = C.c_int
        L.dynref_preprocess.argtypes = [dp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, ip, C.c_int,
                                        ip, C.c_int, dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.dynref_emission_order.restype = None
        L.dynref_emission_order.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        _lib.append(L)
    return _lib[0]


def _ints(v):
    v = list(v)
    return (C.c_int * max(len(v), 1))(*v), len(v)


def preprocess(frame, max_range=100.0, min_range=5.0, label_max_range=50.0, dy_th=0.5, dynamic_labels=KITTI_VEHICLES,
               landmark_labels=(44, 48)):
    """(filtered (m, 4) array, info dict); raises ValueError for a non-finite label of a kept point"""
    f = np.ascontiguousarray(frame, dtype=np.float64).reshape(-1, 4)
    out = np.empty((max(len(f), 1), 4))
    dl, nd = _ints(dynamic_labels)
    ll, nl = _ints(landmark_labels)
    m = C.c_uint64(0)
    info = (C.c_uint64 * 5)()
    rc = lib().dynref_preprocess(f.ctypes.data_as(C.POINTER(C.c_double)), len(f), max_range, min_range,
                                 label_max_range, dy_th, dl, nd, ll, nl, out.ctypes.data_as(C.POINTER(C.c_double)),
                                 C.byref(m), info)
    if rc:
        raise ValueError("non-finite label")
    keys = ("vehicle_points", "landmark_points", "clusters", "clusters_kept", "points_removed")
    return out[:m.value].copy(), dict(zip(keys, [int(x) for x in info]))


def emission_order(sizes):
    s = np.ascontiguousarray(sizes, dtype=np.uint32)
    out = np.zeros(max(len(s), 1), dtype=np.uint32)
    lib().dynref_emission_order(s.ctypes.data_as(C.c_void_p), len(s), out.ctypes.data_as(C.c_void_p))
    return out[:len(s)].copy()


# ---- known-answer scenes (min_range 0.1, max_range 100, label_max_range 50; vehicles 10, landmarks 44) -----------------
KAT_RANGES = dict(max_range=100.0, min_range=0.1, label_max_range=50.0)


def kat_scenes():
    """{name: (frame, dy_th, expected filtered frame)} — small scenes whose answer follows from the reference by hand"""
    S = {}
    other = [[3.0, 4.0, 0.0, 40.0], [0.05, 0.0, 0.0, 40.0], [120.0, 0.0, 0.0, 40.0], [60.0, 0.0, 0.0, 44.0]]
    crop_other = [[3.0, 4.0, 0.0, 40.0], [60.0, 0.0, 0.0, 0.0]]      # 0.05 m and 120 m are cropped, 60 m zeroed

    # a chain of vehicle points 0.49 m apart is one cluster; a landmark under each point keeps it
    chain = [[10.0 + 0.49 * k, 1.0, 0.0, 10.0] for k in range(6)]
    under = [[10.0 + 0.49 * k, 1.0, -0.3, 44.0] for k in range(6)]
    f = np.array(other[:2] + chain[:3] + under + chain[3:] + other[2:])
    S["chain_0.49_one_cluster"] = (f, 0.5, np.array(crop_other[:1] + under + crop_other[1:] + chain))
    # exactly 0.5 m apart (exact in fp32): d2 == 0.25f is no neighbour -> singletons -> all dropped
    spaced = [[10.0 + 0.5 * k, 1.0, 0.0, 10.0] for k in range(6)]
    under5 = [[10.0 + 0.5 * k, 1.0, -0.3, 44.0] for k in range(6)]
    f = np.array(spaced + under5 + other)
    S["exactly_0.5_not_linked"] = (f, 0.5, np.array(under5 + crop_other))
    # a 4-point cluster is dropped even with landmarks everywhere
    four = [[20.0 + 0.1 * k, 0.0, 0.0, 10.0] for k in range(4)]
    under4 = [[20.0 + 0.1 * k, 0.0, -0.2, 44.0] for k in range(4)]
    f = np.array(four + under4)
    S["four_points_dropped"] = (f, 0.0, np.array(under4))
    # 10 points 0.3 m apart; landmark k sits 0.45 m beside point k only: count = number of landmarks.
    # dy_th 0.5 -> static_cast<int>(5.0) = 5: count 5 is dropped, count 6 kept
    ten = [[30.0 + 0.3 * k, 0.0, 0.0, 10.0] for k in range(10)]
    for c in (5, 6):
        beside = [[30.0 + 0.3 * k, 0.45, 0.0, 44.0] for k in range(c)]
        f = np.array(ten + beside)
        S["count_%d_of_10" % c] = (f, 0.5, np.array(beside + (ten if c == 6 else [])))
    # no vehicles: the crop-only output
    f = np.array(other + [[7.0, 1.0, 1.0, 48.0], [8.0, 0.0, 0.0, 11.0]])
    S["no_vehicles"] = (f, 0.5, np.array(crop_other[:1] + crop_other[1:] + [[7.0, 1.0, 1.0, 48.0], [8.0, 0.0, 0.0, 11.0]]))
    return S


def crop_only(frame, max_range=100.0, min_range=5.0, label_max_range=50.0):
    """Preprocess() with the filter off (Preprocessing.cpp:173-187), same association of the norm"""
    f = np.array(frame, dtype=np.float64).reshape(-1, 4)
    x, y, z = f[:, 0], f[:, 1], f[:, 2]
    norm = np.sqrt((x * x + y * y) + z * z)
    keep = (norm < max_range) & (norm > min_range)
    f[norm > label_max_range, 3] = 0.0
    return f[keep]
