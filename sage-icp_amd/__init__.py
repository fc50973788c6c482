"""sage_icp_amd — Python binding (ctypes) of libsageicp_hip.so, the MI355X implementation of
SAGE-ICP's registration hot path, for tests and bench.py.

The product is the C-ABI shared library (include/sageicp.h) and the C++ header shim in
shim/; this module only mirrors the reference's interface names on top of it:

    VoxelHashMap            sage_icp::VoxelHashMap   (cpp/sage_icp/core/VoxelHashMap.hpp:35-107)
    register_frame()        sage_icp::RegisterFrame  (cpp/sage_icp/core/Registration.hpp:34-39)
    transform_points()      sage_icp::TransformPoints(cpp/sage_icp/core/Registration.hpp:32)
    align_clouds()          AlignClouds              (cpp/sage_icp/core/Registration.cpp:59-94)

There is no CPU fallback: if the library has not been built, importing a compute symbol raises;
if no HIP device is present every compute call raises SageIcpError(SAGEICP_ERR_NO_DEVICE).
The directory is named `sage-icp_amd`; import it as `sage_icp_amd` through the loader module
/sage_icp_amd.py at the repo root.
"""
import ctypes as C
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAGE_SQNORM3_ORDER=0 in the environment loads the build with the rounds-1-3 association of the 3-term
# squared norms (csrc/sageicp_types.h; default 2 = what Eigen 3.4's reductions evaluate, per call site):
# libsageicp_hip.v0.so, built by build.py next to the default
SQNORM3_ORDER = 0 if os.environ.get("SAGE_SQNORM3_ORDER", "2") == "0" else 2
if os.environ.get("SAGE_SQNORM3_ORDER", "2") not in ("0", "2"):
    import warnings
    warnings.warn("SAGE_SQNORM3_ORDER=%r: only the builds 0 and 2 exist — using 2" % os.environ["SAGE_SQNORM3_ORDER"])
LIB_PATH = os.path.join(_HERE, "libsageicp_hip.v0.so" if SQNORM3_ORDER == 0 else "libsageicp_hip.so")
if os.environ.get("SAGEICP_VARIANT_LIB"):      # measurement only: a variant build of the same library (profiles/)
    LIB_PATH = os.path.abspath(os.environ["SAGEICP_VARIANT_LIB"])

_dp = C.POINTER(C.c_double)
_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)
_u8p = C.POINTER(C.c_uint8)

ABI_VERSION = 4          # SAGEICP_ABI_VERSION of include/sageicp.h
ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_RCCL, ERR_CAPACITY = -1, -2, -3, -4, -5
UNIQUE_ID_BYTES = 128
P2P_HANDLE_BYTES = 64

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64)
DTYPE_FLOAT32, DTYPE_FLOAT64, DTYPE_UINT8, DTYPE_INT32, DTYPE_INT64 = 1, 2, 3, 4, 5     # SAGEICP_DTYPE_*


class SageIcpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sageicp error %d: %s" % (code, msg))
        self.code = code


class Stats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32),
        ("converged", C.c_int32),
        ("n_queries", C.c_uint64),
        ("n_corr_first", C.c_uint64),
        ("n_corr_last", C.c_uint64),
        ("last_step_norm", C.c_double),
        ("us_wall", C.c_double),
        ("us_upload", C.c_double),
        ("us_nn", C.c_double),
        ("us_fin", C.c_double),
        ("nn_launches", C.c_uint32),
        ("single_launch", C.c_uint32),
        ("sum_candidates", C.c_uint64),
        ("n_corr_hist", C.c_uint32 * 64),
        ("pairs_evaluated", C.c_uint64),
        ("lanes_per_query", C.c_uint32),
        ("compact_scan", C.c_uint32),
    ]


class CommInfo(C.Structure):
    """sageicp_comm_info"""
    _fields_ = [("rank", C.c_int32), ("nranks", C.c_int32), ("device", C.c_int32),
                ("has_rccl", C.c_int32), ("rccl_ranks", C.c_int32), ("rccl_rank", C.c_int32),
                ("p2p_connected", C.c_int32), ("p2p_enabled", C.c_int32), ("p2p_poisoned", C.c_int32),
                ("reserved", C.c_int32 * 7)]


class PipelineConfig(C.Structure):
    """sageicp_pipeline_config == sageConfig (pipeline/sageICP.hpp:39-65)"""
    _fields_ = [
        ("voxel_size_map", C.c_double), ("max_range", C.c_double), ("min_range", C.c_double),
        ("label_max_range", C.c_double), ("local_map_range", C.c_double),
        ("basic_points_per_voxel", C.c_int), ("critical_points_per_voxel", C.c_int),
        ("basic_parts_labels", C.POINTER(C.c_int)), ("n_basic_parts_labels", C.c_int),
        ("min_motion_th", C.c_double), ("initial_threshold", C.c_double), ("sem_th", C.c_double),
        ("n_groups", C.c_int),
        ("group_label_counts", C.POINTER(C.c_int)), ("group_labels", C.POINTER(C.c_int)),
        ("group_voxel_size", C.POINTER(C.c_double)),
        ("device", C.c_int),
        ("map_update_on_device", C.c_int),
    ]


class DynFilterInfo(C.Structure):
    """sageicp_dynfilter_info: what Preprocess()'s dynamic vehicle filter did to a frame"""
    _fields_ = [("vehicle_points", C.c_uint64), ("landmark_points", C.c_uint64), ("clusters", C.c_uint64),
                ("clusters_kept", C.c_uint64), ("points_removed", C.c_uint64), ("us_wall", C.c_double),
                ("us_host", C.c_double), ("us_device", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DeviceFrame(C.Structure):
    """sageicp_device_frame: a raw frame in device memory (xyz rows, labels in column 3 or apart)"""
    _fields_ = [("xyz", C.c_void_p), ("xyz_stride", C.c_uint64), ("xyz_dtype", C.c_int32), ("label_dtype", C.c_int32),
                ("label", C.c_void_p), ("label_stride", C.c_uint64), ("n", C.c_uint64)]


class DevicePoints(C.Structure):
    """sageicp_device_points: a destination in device memory (xyz rows, labels in column 3 or apart), cap rows"""
    _fields_ = [("xyz", C.c_void_p), ("xyz_stride", C.c_uint64), ("xyz_dtype", C.c_int32), ("label_dtype", C.c_int32),
                ("label", C.c_void_p), ("label_stride", C.c_uint64), ("cap", C.c_uint64)]


class MsgLayout(C.Structure):
    """sageicp_msg_layout: an incoming PointCloud2's fields as PointCloud2ToEigen / GetTimestamps read them"""
    _fields_ = [("point_step", C.c_uint32), ("x_offset", C.c_uint32), ("y_offset", C.c_uint32), ("z_offset", C.c_uint32),
                ("label_offset", C.c_uint32), ("label_dtype", C.c_int32), ("time_kind", C.c_int32),
                ("time_offset", C.c_uint32)]


class MsgColors(C.Structure):
    """sageicp_msg_colors: the node's color_list as (key, value) pairs"""
    _fields_ = [("keys", C.POINTER(C.c_int32)), ("values", C.POINTER(C.c_int32)), ("n", C.c_uint32)]


class MsgField(C.Structure):
    """sageicp_msg_field: one entry of the outgoing record's field table"""
    _fields_ = [("name", C.c_char * 8), ("offset", C.c_uint32), ("datatype", C.c_int32), ("count", C.c_uint32)]


MSG_POINT_STEP = 21      # SAGEICP_MSG_POINT_STEP


class Quality(C.Structure):
    """sageicp_quality: how good a pose is — fitness, rmse, the Gauss-Newton system and the step still left, covariances,
    and which classes produced the pairs (include/sageicp.h states every field)"""
    _fields_ = [("fitness", C.c_double), ("rmse", C.c_double), ("step_norm", C.c_double),
                ("sum_r2", C.c_double), ("sum_w", C.c_double), ("sum_w_r2", C.c_double),
                ("step", C.c_double * 6), ("JTr", C.c_double * 6),
                ("JTJ", C.c_double * 36), ("info", C.c_double * 36),
                ("covariance", C.c_double * 36), ("covariance_pose", C.c_double * 36),
                ("class_sum_r2", C.c_double * 256), ("other_sum_r2", C.c_double),
                ("n_queries", C.c_uint64), ("n_pairs", C.c_uint64),
                ("pairs_same_label", C.c_uint64), ("pairs_unlabelled", C.c_uint64), ("pairs_cross_label", C.c_uint64),
                ("other_queries", C.c_uint64), ("other_pairs", C.c_uint64),
                ("class_queries", C.c_uint32 * 256), ("class_pairs", C.c_uint32 * 256),
                ("valid", C.c_int32), ("covariance_valid", C.c_int32)]
    _MATRICES = ("JTJ", "info", "covariance", "covariance_pose")

    def as_dict(self):
        """plain Python numbers; the four matrices as (6, 6) numpy arrays, the other arrays as 1-D numpy arrays"""
        d = {}
        for k, ty in self._fields_:
            v = getattr(self, k)
            if k in self._MATRICES:
                v = np.array(v[:], dtype=np.float64).reshape(6, 6)
            elif hasattr(ty, "_length_"):
                v = np.array(v[:], dtype=np.uint32 if ty._type_ is C.c_uint32 else np.float64)
            d[k] = v
        d["valid"], d["covariance_valid"] = bool(self.valid), bool(self.covariance_valid)
        return d


QUALITY_BYTES = 5464     # sizeof(sageicp_quality)
assert C.sizeof(Quality) == QUALITY_BYTES


class PoseScore(C.Structure):
    """sageicp_pose_score: one candidate pose of a batch — bit for bit the same-named fields of the Quality of that pose
    alone; step_valid is its covariance_valid, score (the ranking key) its sum_w"""
    _fields_ = [("score", C.c_double), ("fitness", C.c_double), ("rmse", C.c_double), ("step_norm", C.c_double),
                ("sum_r2", C.c_double), ("sum_w", C.c_double), ("sum_w_r2", C.c_double),
                ("step", C.c_double * 6), ("JTr", C.c_double * 6), ("JTJ", C.c_double * 36),
                ("n_queries", C.c_uint64), ("n_pairs", C.c_uint64),
                ("pairs_same_label", C.c_uint64), ("pairs_unlabelled", C.c_uint64), ("pairs_cross_label", C.c_uint64),
                ("valid", C.c_int32), ("step_valid", C.c_int32)]


POSE_SCORE_BYTES = 488   # sizeof(sageicp_pose_score)
assert C.sizeof(PoseScore) == POSE_SCORE_BYTES
# the structs of ScorePoses as a numpy record array
POSE_SCORE_DTYPE = np.dtype([("score", "<f8"), ("fitness", "<f8"), ("rmse", "<f8"), ("step_norm", "<f8"),
                             ("sum_r2", "<f8"), ("sum_w", "<f8"), ("sum_w_r2", "<f8"),
                             ("step", "<f8", (6,)), ("JTr", "<f8", (6,)), ("JTJ", "<f8", (6, 6)),
                             ("n_queries", "<u8"), ("n_pairs", "<u8"),
                             ("pairs_same_label", "<u8"), ("pairs_unlabelled", "<u8"), ("pairs_cross_label", "<u8"),
                             ("valid", "<i4"), ("step_valid", "<i4")])
assert POSE_SCORE_DTYPE.itemsize == POSE_SCORE_BYTES


class RelocalizeParams(C.Structure):
    """sageicp_relocalize_params: the candidate grid around a prior, how many of the best to refine, the registration's
    parameters"""
    _fields_ = [("xy_extent", C.c_double), ("xy_step", C.c_double), ("z_extent", C.c_double), ("z_step", C.c_double),
                ("yaw_extent", C.c_double), ("yaw_step", C.c_double),
                ("refine_top", C.c_uint32), ("reserved", C.c_uint32),
                ("max_correspondence_distance", C.c_double), ("kernel", C.c_double), ("sem_th", C.c_double)]


class RelocalizeInfo(C.Structure):
    """sageicp_relocalize_info: what Relocalize did"""
    _fields_ = [("candidates", C.c_uint64), ("best_candidate", C.c_uint64), ("best_candidate_score", C.c_double),
                ("refined", C.c_uint32), ("winner_rank", C.c_uint32), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("us_score", C.c_double), ("us_refine", C.c_double), ("us_wall", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ArchiveInfo(C.Structure):
    """sageicp_archive_info"""
    _fields_ = [("enabled", C.c_int32), ("full", C.c_int32), ("rows", C.c_uint64), ("voxels", C.c_uint64),
                ("dropped_rows", C.c_uint64), ("dropped_voxels", C.c_uint64), ("max_rows", C.c_uint64), ("updates", C.c_uint64),
                ("device_rows", C.c_uint64), ("host_rows", C.c_uint64), ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RecallInfo(C.Structure):
    """sageicp_recall_info"""
    _fields_ = [(k, C.c_uint64) for k in ("voxels", "rows", "archive_voxels", "archive_rows", "map_voxels", "map_rows",
                                          "session_voxels", "session_rows")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RebuildInfo(C.Structure):
    """sageicp_rebuild_info"""
    _fields_ = [(k, C.c_uint64) for k in ("voxels", "rows", "session_voxels", "session_rows", "built_voxels", "built_rows",
                                          "cropped_voxels", "cropped_rows")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


ARCHIVE_ALL, ARCHIVE_LATEST, SESSION = 0, 1, 2          # SAGEICP_ARCHIVE_ALL / _LATEST, SAGEICP_SESSION
ARCHIVE_WHICH = {"all": ARCHIVE_ALL, "latest": ARCHIVE_LATEST, "session": SESSION}
# sageicp_archive_voxel
ARCHIVE_VOXEL_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("z", "<i4"), ("count", "<u4"), ("first_row", "<u8"), ("update", "<u8")])


class ClosureInfo(C.Structure):
    """sageicp_closure_info"""
    _fields_ = [("delta", C.c_double * 7), ("angle", C.c_double), ("shift", C.c_double), ("path", C.c_double),
                ("i", C.c_uint64), ("j", C.c_uint64)]

    def as_dict(self):
        return dict(delta=np.array(self.delta[:]), angle=self.angle, shift=self.shift, path=self.path, i=int(self.i), j=int(self.j))


class GraphEdge(C.Structure):
    """sageicp_graph_edge: a closure of the pose graph, z = T_a_b with its 6x6 information"""
    _fields_ = [("a", C.c_uint64), ("b", C.c_uint64), ("z", C.c_double * 7), ("info", C.c_double * 36)]


class GraphParams(C.Structure):
    """sageicp_graph_params"""
    _fields_ = [("anchor", C.c_uint64), ("max_iterations", C.c_uint32), ("max_halvings", C.c_uint32), ("step_tol", C.c_double),
                ("where", C.c_uint32), ("reserved", C.c_uint32)]


class GraphInfo(C.Structure):
    """sageicp_graph_info"""
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("grad_max", C.c_double), ("step_last", C.c_double),
                ("max_shift", C.c_double), ("iterations", C.c_uint32), ("halvings", C.c_uint32), ("status", C.c_uint32),
                ("where", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


GRAPH_WHERE = {"auto": 0, "host": 1, "device": 2}
GRAPH_KERNEL = {"none": 0, "huber": 1, "cauchy": 2, "gm": 3}


class GraphRobust(C.Structure):
    """sageicp_graph_robust: the robust kernel on the closures of a pose graph"""
    _fields_ = [("kernel", C.c_uint32), ("anneal", C.c_uint32), ("scale", C.c_double), ("anneal_factor", C.c_double),
                ("stage_iterations", C.c_uint32), ("reserved", C.c_uint32)]


class GraphRobustInfo(C.Structure):
    """sageicp_graph_robust_info"""
    _fields_ = [("scale2_first", C.c_double), ("stages", C.c_uint32), ("outliers", C.c_uint32)]


class OccupancyParams(C.Structure):
    """sageicp_occupancy_params: the bird's-eye grid of key-frame selection (bounds of x, y, z; H rows, W columns)"""
    _fields_ = [("bounds", (C.c_double * 2) * 3), ("occ_h", C.c_int32), ("occ_w", C.c_int32), ("overlap_th", C.c_double)]


class KeyFrameInfo(C.Structure):
    """sageicp_key_frame_info: what key-frame selection decided for the last frame registered"""
    _fields_ = [("enabled", C.c_int32), ("is_key_frame", C.c_int32), ("overlap", C.c_double),
                ("key_frame_index", C.c_uint64), ("key_frames", C.c_uint64), ("key_occupied", C.c_uint64),
                ("intersect", C.c_uint64), ("key_pose", C.c_double * 7)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "key_pose"}
        d["enabled"], d["is_key_frame"] = bool(self.enabled), bool(self.is_key_frame)
        d["key_pose"] = np.array(self.key_pose[:], dtype=np.float64)
        return d


# the key-frame parameters of ros/launch/odometry*.launch.py (key_frame_bounds, key_frame_occ_size, key_frame_overlap)
KEY_FRAME_BOUNDS = ((-51.2, 51.2), (-51.2, 51.2), (-4.0, 2.4))
KEY_FRAME_OCC_SIZE = (128, 128)
KEY_FRAME_OVERLAP = 0.5


def occupancy_params(bounds=KEY_FRAME_BOUNDS, occ_size=KEY_FRAME_OCC_SIZE, overlap=KEY_FRAME_OVERLAP):
    """OccupancyParams from the launch files' form: bounds ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)), occ_size (H, W)"""
    b = [[float(v) for v in ax] for ax in bounds]
    if len(b) != 3 or any(len(ax) != 2 for ax in b):
        raise ValueError("bounds are ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi))")
    h, w = (int(v) for v in occ_size)
    p = OccupancyParams()
    for a in range(3):
        p.bounds[a][0], p.bounds[a][1] = b[a]
    p.occ_h, p.occ_w, p.overlap_th = h, w, float(overlap)
    return p


class PlaceParams(C.Structure):
    """sageicp_place_params: the polar grid of a place descriptor (rings R, sectors S), the heights mapped to bytes 1 and
    255, and the rank of every class (0: ignored)"""
    _fields_ = [("min_range", C.c_double), ("max_range", C.c_double), ("z_lo", C.c_double), ("z_hi", C.c_double),
                ("rings", C.c_int32), ("sectors", C.c_int32), ("rank", C.c_uint8 * 256)]


class PlaceQuery(C.Structure):
    """sageicp_place_query"""
    _fields_ = [("min_similarity", C.c_double), ("exclude_last", C.c_uint64), ("top_k", C.c_uint32), ("h_tol", C.c_uint32)]


class PlaceMatch(C.Structure):
    """sageicp_place_match"""
    _fields_ = [("similarity", C.c_double), ("yaw", C.c_double), ("pose", C.c_double * 7), ("prior", C.c_double * 7),
                ("index", C.c_uint64), ("tag", C.c_uint64),
                ("agree", C.c_uint32), ("n_query", C.c_uint32), ("n_entry", C.c_uint32), ("shift", C.c_uint32)]


class PlaceInfo(C.Structure):
    """sageicp_place_info: what place recognition did for the last frame registered"""
    _fields_ = [("matches", PlaceMatch * 16), ("entries", C.c_uint64), ("enabled", C.c_int32), ("described", C.c_int32),
                ("n_matches", C.c_uint32), ("reserved", C.c_uint32)]


PLACE_PARAMS_BYTES, PLACE_QUERY_BYTES, PLACE_MATCH_BYTES, PLACE_INFO_BYTES = 296, 24, 160, 2584
assert (C.sizeof(PlaceParams), C.sizeof(PlaceQuery), C.sizeof(PlaceMatch), C.sizeof(PlaceInfo)) == \
    (PLACE_PARAMS_BYTES, PLACE_QUERY_BYTES, PLACE_MATCH_BYTES, PLACE_INFO_BYTES)
# the structs of PlaceDB.match as a numpy record array
PLACE_MATCH_DTYPE = np.dtype([("similarity", "<f8"), ("yaw", "<f8"), ("pose", "<f8", (7,)), ("prior", "<f8", (7,)),
                              ("index", "<u8"), ("tag", "<u8"),
                              ("agree", "<u4"), ("n_query", "<u4"), ("n_entry", "<u4"), ("shift", "<u4")])
assert PLACE_MATCH_DTYPE.itemsize == PLACE_MATCH_BYTES
PLACE_MAX_CELLS = 16384  # rings * sectors at most: two u32 planes of that many cells are one workgroup's LDS


def place_params(min_range=3.0, max_range=50.0, z_lo=-3.0, z_hi=7.0, rings=20, sectors=60, rank=None):
    """PlaceParams.  rank: a dict {class: rank} (the classes it does not name get 0: ignored), a sequence of 256 ranks,
    or None for rank 1 for every class but 0"""
    p = PlaceParams()
    p.min_range, p.max_range, p.z_lo, p.z_hi = float(min_range), float(max_range), float(z_lo), float(z_hi)
    p.rings, p.sectors = int(rings), int(sectors)
    if rank is None:
        table = [0] + [1] * 255
    elif isinstance(rank, dict):
        table = [0] * 256
        for c, r in rank.items():
            table[int(c)] = int(r)
    else:
        table = [int(r) for r in rank]
        if len(table) != 256:
            raise ValueError("rank holds one entry per class 0 .. 255")
    for c, r in enumerate(table):
        p.rank[c] = r
    return p


def place_query(top_k=1, h_tol=0, exclude_last=0, min_similarity=0.0):
    q = PlaceQuery()
    q.top_k, q.h_tol, q.exclude_last, q.min_similarity = int(top_k), int(h_tol), int(exclude_last), float(min_similarity)
    return q


# the SemanticKITTI parameter sets of ros/launch/odometry*.launch.py
KITTI_VOXEL_LABELS = [[40, 44, 48, 49], [50, 51, 52], [70, 72], [60, 71, 80, 81, 99], [0],
                      [10, 11, 13, 15, 16, 18, 20]]
KITTI_VOXEL_SIZE = [0.6, 1.0, 0.9, 0.8, 1.0, 0.6]


def make_pipeline_config(voxel_size_map=0.8, max_range=100.0, min_range=5.0, label_max_range=50.0,
                         local_map_range=100.0, basic=20, critical=20,
                         basic_parts_labels=(40, 44, 48, 49, 50, 70, 72), min_motion_th=0.1,
                         initial_threshold=2.0, sem_th=0.05, voxel_labels=None, voxel_size=None,
                         device=0, map_update_on_device=True, dynamic_vehicle_filter=False,
                         dynamic_vehicle_filter_th=0.5, dynamic_vehicle_voxid=5, dynamic_remove_lankmark=(44, 48),
                         deskew=False):
    """defaults: ros/launch/odometry_gt.launch.py (pre-labelled scans, dynamic filter off); odometry.launch.py sets
    dynamic_vehicle_filter=True.  The four dynamic_* settings (sageConfig's names) are kept on the returned object
    only — the C struct has no room for them — and SageICP() applies them through
    sageicp_pipeline_set_dynamic_vehicle_filter; likewise `deskew` (sageConfig::deskew, off in every launch file),
    applied through sageicp_pipeline_set_deskew."""
    voxel_labels = KITTI_VOXEL_LABELS if voxel_labels is None else voxel_labels
    voxel_size = KITTI_VOXEL_SIZE if voxel_size is None else voxel_size
    assert len(voxel_labels) == len(voxel_size)
    keep = {}
    keep["basic"] = (C.c_int * len(basic_parts_labels))(*basic_parts_labels)
    keep["counts"] = (C.c_int * len(voxel_labels))(*[len(g) for g in voxel_labels])
    flat = [l for g in voxel_labels for l in g]
    keep["labels"] = (C.c_int * len(flat))(*flat)
    keep["sizes"] = (C.c_double * len(voxel_size))(*voxel_size)
    cfg = PipelineConfig(voxel_size_map, max_range, min_range, label_max_range, local_map_range,
                         basic, critical, keep["basic"], len(basic_parts_labels), min_motion_th,
                         initial_threshold, sem_th, len(voxel_labels), keep["counts"],
                         keep["labels"], keep["sizes"], device, 1 if map_update_on_device else 0)
    cfg._keep = keep          # the arrays must outlive the struct
    cfg._dynamic = dict(enable=bool(dynamic_vehicle_filter), dy_th=float(dynamic_vehicle_filter_th),
                        voxid=int(dynamic_vehicle_voxid), landmarks=tuple(dynamic_remove_lankmark))
    cfg._deskew = bool(deskew)
    return cfg


# every symbol include/sageicp.h declares: (name, restype, argtypes)
_SIGNATURES = [
    ("sageicp_abi_version", C.c_int, []),
    ("sageicp_last_error", C.c_char_p, []),
    ("sageicp_device_count", C.c_int, []),
    ("sageicp_set_profiling", None, [C.c_int]),
    ("sageicp_set_counting", None, [C.c_int]),
    ("sageicp_reload_env", None, []),
    ("sageicp_map_loop_status", C.c_int, [C.c_void_p, C.c_void_p]),
    ("sageicp_set_downsample_order", None, [C.c_int]),
    ("sageicp_robin_iteration_order", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    ("sageicp_robin_sweep", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, _u64p, C.c_void_p, _u64p]),
    ("sageicp_map_create", C.c_void_p,
     [C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int]),
    ("sageicp_map_destroy", None, [C.c_void_p]),
    ("sageicp_map_set_devices", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    ("sageicp_map_num_devices", C.c_int, [C.c_void_p]),
    ("sageicp_map_set_reference_order", C.c_int, [C.c_void_p, C.c_int]),
    ("sageicp_map_reference_order", C.c_int, [C.c_void_p]),
    ("sageicp_map_clone", C.c_void_p, [C.c_void_p]),
    ("sageicp_map_clear", C.c_int, [C.c_void_p]),
    ("sageicp_map_empty", C.c_int, [C.c_void_p]),
    ("sageicp_map_size", C.c_uint64, [C.c_void_p]),
    ("sageicp_map_num_voxels", C.c_uint64, [C.c_void_p]),
    ("sageicp_map_add_points", C.c_int, [C.c_void_p, _dp, C.c_uint64]),
    ("sageicp_map_remove_far", C.c_int, [C.c_void_p, _dp]),
    ("sageicp_map_update", C.c_int, [C.c_void_p, _dp, C.c_uint64, _dp]),
    ("sageicp_map_update_pose", C.c_int, [C.c_void_p, _dp, C.c_uint64, _dp]),
    ("sageicp_map_update_pose_device", C.c_int, [C.c_void_p, _dp, C.c_uint64, _dp]),
    ("sageicp_map_pointcloud", C.c_uint64, [C.c_void_p, _dp, C.c_uint64]),
    ("sageicp_map_resident", C.c_int, [C.c_void_p]),
    ("sageicp_map_point_slots", C.c_uint64, [C.c_void_p]),
    ("sageicp_voxel_hash", C.c_uint32, [C.c_int32, C.c_int32, C.c_int32]),
    ("sageicp_map_table_stats", C.c_int, [C.c_void_p, _u64p]),
    ("sageicp_map_sync", C.c_int, [C.c_void_p]),
    ("sageicp_get_correspondences", C.c_int,
     [C.c_void_p, _dp, C.c_uint64, C.c_double, C.c_double, _dp, _dp, _u64p, _i64p]),
    ("sageicp_get_correspondences_device", C.c_int,
     [C.c_void_p, C.POINTER(DeviceFrame), _dp, C.c_double, C.c_double, C.POINTER(DevicePoints), C.POINTER(DevicePoints),
      C.c_void_p, C.c_uint64, C.c_void_p, _u64p]),
    ("sageicp_registration_quality", C.c_int,
     [C.c_void_p, _dp, C.c_uint64, _dp, C.c_double, C.c_double, C.c_double, C.POINTER(Quality)]),
    ("sageicp_registration_quality_device", C.c_int,
     [C.c_void_p, C.POINTER(DeviceFrame), _dp, C.c_double, C.c_double, C.c_double, C.c_void_p, C.POINTER(Quality)]),
    ("sageicp_pipeline_set_quality", C.c_int, [C.c_void_p, C.c_int]),
    ("sageicp_pipeline_quality", C.c_int, [C.c_void_p, C.POINTER(Quality)]),
    ("sageicp_score_poses", C.c_int,
     [C.c_void_p, _dp, C.c_uint64, _dp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    ("sageicp_score_poses_device", C.c_int,
     [C.c_void_p, C.POINTER(DeviceFrame), _dp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    ("sageicp_relocalize_candidates", C.c_int, [_dp, C.POINTER(RelocalizeParams), _dp, C.c_uint64, _u64p]),
    ("sageicp_relocalize", C.c_int,
     [C.c_void_p, _dp, C.c_uint64, _dp, C.POINTER(RelocalizeParams), _dp, C.POINTER(Quality), C.POINTER(RelocalizeInfo)]),
    ("sageicp_relocalize_device", C.c_int,
     [C.c_void_p, C.POINTER(DeviceFrame), _dp, C.POINTER(RelocalizeParams), C.c_void_p, _dp, C.POINTER(Quality),
      C.POINTER(RelocalizeInfo)]),
    ("sageicp_align_clouds", C.c_int, [_dp, _dp, C.c_uint64, C.c_double, _dp, _dp, _dp, C.c_int]),
    ("sageicp_transform_points", C.c_int, [_dp, _dp, C.c_uint64, C.c_int]),
    ("sageicp_register_frame", C.c_int,
     [C.c_void_p, _dp, C.c_uint64, _dp, C.c_double, C.c_double, C.c_double, _dp,
      C.POINTER(Stats)]),
    ("sageicp_frame_upload", C.c_void_p, [C.c_void_p, _dp, C.c_uint64]),
    ("sageicp_frame_destroy", None, [C.c_void_p]),
    ("sageicp_register_frame_resident", C.c_int,
     [C.c_void_p, C.c_void_p, _dp, C.c_double, C.c_double, C.c_double, C.c_void_p, _dp,
      C.POINTER(Stats)]),
    ("sageicp_comm_unique_id", C.c_int, [_u8p]),
    ("sageicp_comm_create", C.c_void_p, [_u8p, C.c_int, C.c_int, C.c_int]),
    ("sageicp_comm_create_local", C.c_void_p, [C.c_int, C.c_int, C.c_int]),
    ("sageicp_comm_p2p_export", C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    ("sageicp_comm_p2p_connect", C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    ("sageicp_comm_p2p_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("sageicp_comm_p2p_enabled", C.c_int, [C.c_void_p]),
    ("sageicp_comm_describe", C.c_int, [C.c_void_p, C.POINTER(CommInfo)]),
    ("sageicp_comm_destroy", None, [C.c_void_p]),
    ("sageicp_preprocess", C.c_int,
     [_dp, C.c_uint64, C.c_double, C.c_double, C.c_double, _dp, _u64p, C.c_int]),
    ("sageicp_voxel_downsample", C.c_int,
     [_dp, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
      C.c_double, _dp, _u64p, C.c_int]),
    ("sageicp_preprocess_dynamic", C.c_int,
     [_dp, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int), C.c_int,
      C.POINTER(C.c_int), C.c_int, _dp, _u64p, C.POINTER(DynFilterInfo), C.c_int]),
    ("sageicp_cluster_emission_order", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    ("sageicp_pipeline_set_dynamic_vehicle_filter", C.c_int,
     [C.c_void_p, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int), C.c_int]),
    ("sageicp_pipeline_dynamic_filter_info", C.c_int, [C.c_void_p, C.POINTER(DynFilterInfo)]),
    ("sageicp_deskew_scan", C.c_int, [_dp, _dp, C.c_uint64, _dp, _dp, _dp, C.c_int]),
    ("sageicp_pipeline_set_deskew", C.c_int, [C.c_void_p, C.c_int]),
    ("sageicp_pipeline_register_frame_timestamps", C.c_int,
     [C.c_void_p, _dp, _dp, C.c_uint64, _dp, _dp, _dp, _u64p, C.POINTER(Stats)]),
    ("sageicp_pipeline_deskew_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int), _dp]),
    ("sageicp_pipeline_register_frame_device", C.c_int,
     [C.c_void_p, C.POINTER(DeviceFrame), C.c_void_p, C.c_void_p, _dp, _dp, _dp, _u64p, C.POINTER(Stats)]),
    ("sageicp_frame_from_device", C.c_void_p, [C.c_void_p, C.POINTER(DeviceFrame), C.c_void_p]),
    ("sageicp_pipeline_source", C.c_int, [C.c_void_p, _dp, C.c_uint64, _u64p]),
    ("sageicp_pipeline_source_device", C.c_int, [C.c_void_p, C.POINTER(DevicePoints), C.c_void_p, _u64p]),
    ("sageicp_map_pointcloud_device", C.c_int, [C.c_void_p, C.POINTER(DevicePoints), C.c_void_p, _u64p]),
    ("sageicp_pipeline_set_key_frames", C.c_int, [C.c_void_p, C.c_int, C.POINTER(OccupancyParams)]),
    ("sageicp_pipeline_key_frame_reset", C.c_int, [C.c_void_p]),
    ("sageicp_pipeline_key_frame_info", C.c_int, [C.c_void_p, C.POINTER(KeyFrameInfo)]),
    ("sageicp_pipeline_key_frame_grid", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    ("sageicp_pipeline_key_frame_grid_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("sageicp_occupancy_grid", C.c_int, [_dp, C.c_uint64, _dp, C.POINTER(OccupancyParams), C.c_void_p, C.c_int]),
    ("sageicp_occupancy_grid_device", C.c_int,
     [C.POINTER(DeviceFrame), _dp, C.POINTER(OccupancyParams), C.c_void_p, C.c_void_p]),
    ("sageicp_pipeline_register_frame_msg", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(MsgLayout), _dp, _dp, _dp, _u64p, C.POINTER(Stats)]),
    ("sageicp_pipeline_register_frame_msg_device", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(MsgLayout), C.c_void_p, _dp, _dp, _dp, _u64p,
      C.POINTER(Stats)]),
    ("sageicp_msg_output_fields", C.c_uint32, [C.POINTER(MsgField), C.c_uint32]),
    ("sageicp_pipeline_source_msg", C.c_int, [C.c_void_p, C.POINTER(MsgColors), C.c_void_p, C.c_uint64, _u64p]),
    ("sageicp_pipeline_source_msg_device", C.c_int,
     [C.c_void_p, C.POINTER(MsgColors), C.c_void_p, C.c_uint64, C.c_void_p, _u64p]),
    ("sageicp_map_pointcloud_msg", C.c_int, [C.c_void_p, C.POINTER(MsgColors), C.c_void_p, C.c_uint64, _u64p]),
    ("sageicp_map_pointcloud_msg_device", C.c_int,
     [C.c_void_p, C.POINTER(MsgColors), C.c_void_p, C.c_uint64, C.c_void_p, _u64p]),
    ("sageicp_map_set_archive", C.c_int, [C.c_void_p, C.c_int, C.c_uint64]),
    ("sageicp_map_archive_info", C.c_int, [C.c_void_p, C.POINTER(ArchiveInfo)]),
    ("sageicp_map_archive_clear", C.c_int, [C.c_void_p]),
    ("sageicp_map_archive_voxels", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p]),
    ("sageicp_map_archive_rows", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, _dp, C.c_uint64, _u64p]),
    ("sageicp_map_archive_rows_device", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(DevicePoints), C.c_void_p, _u64p]),
    ("sageicp_map_archive_msg", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(MsgColors), C.c_void_p, C.c_uint64, _u64p]),
    ("sageicp_map_archive_msg_device", C.c_int,
     [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(MsgColors), C.c_void_p, C.c_uint64, C.c_void_p, _u64p]),
    ("sageicp_pipeline_set_archive", C.c_int, [C.c_void_p, C.c_int, C.c_uint64]),
    ("sageicp_map_recall", C.c_int, [C.c_void_p, _dp, C.c_double, C.c_void_p, C.POINTER(RecallInfo)]),
    ("sageicp_pipeline_recall", C.c_int, [C.c_void_p, _dp, C.c_double, C.c_void_p, C.POINTER(RecallInfo)]),
    ("sageicp_closure_corrections", C.c_int, [_dp, C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, _dp, C.POINTER(ClosureInfo)]),
    ("sageicp_map_session_stays", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, _dp, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint64, _u64p]),
    ("sageicp_map_session_corrected", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, _dp, _dp, C.c_uint64, _dp, C.c_uint64, _u64p]),
    ("sageicp_map_session_corrected_device", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, _dp, _dp, C.c_uint64,
                                                       C.POINTER(DevicePoints), C.c_void_p, _u64p]),
    ("sageicp_pipeline_closure", C.c_int, [C.c_void_p, C.c_uint64, _dp, _dp, _dp, C.POINTER(ClosureInfo)]),
    ("sageicp_pipeline_session_corrected", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, _dp, C.c_uint64, _dp, C.c_uint64, _u64p]),
    ("sageicp_pipeline_session_corrected_device", C.c_int, [C.c_void_p, C.c_int, C.c_uint64, _dp, C.c_uint64,
                                                            C.POINTER(DevicePoints), C.c_void_p, _u64p]),
    ("sageicp_map_session_rebuild", C.c_int, [C.c_void_p, C.c_int, _dp, _dp, C.c_uint64, _dp, C.c_double, C.c_void_p,
                                              C.POINTER(RebuildInfo)]),
    ("sageicp_pipeline_session_rebuild", C.c_int, [C.c_void_p, C.c_int, _dp, C.c_uint64, _dp, C.c_double, C.c_void_p,
                                                   C.POINTER(RebuildInfo)]),
    ("sageicp_graph_params_default", None, [C.POINTER(GraphParams)]),
    ("sageicp_graph_edge_from_closed", C.c_int, [_dp, C.c_uint64, C.c_uint64, C.c_uint64, _dp, _dp, C.POINTER(GraphEdge)]),
    ("sageicp_graph_cost", C.c_int, [_dp, C.c_uint64, _dp, C.c_uint32, C.POINTER(GraphEdge), C.c_uint32, _dp, _dp, _dp]),
    ("sageicp_graph_optimize", C.c_int, [_dp, C.c_uint64, _dp, C.c_uint32, C.POINTER(GraphEdge), C.c_uint32, _dp,
                                         C.POINTER(GraphParams), _dp, _dp, C.POINTER(GraphInfo)]),
    ("sageicp_pipeline_graph_optimize", C.c_int, [C.c_void_p, _dp, C.c_uint32, C.POINTER(GraphEdge), C.c_uint32,
                                                  C.POINTER(GraphParams), _dp, _dp, C.POINTER(GraphInfo)]),
    ("sageicp_graph_robust_default", None, [C.POINTER(GraphRobust)]),
    ("sageicp_graph_optimize_robust", C.c_int, [_dp, C.c_uint64, _dp, C.c_uint32, C.POINTER(GraphEdge), C.c_uint32, _dp,
                                                C.POINTER(GraphParams), _dp, _dp, C.POINTER(GraphInfo), C.POINTER(GraphRobust),
                                                _dp, _dp, C.POINTER(GraphRobustInfo)]),
    ("sageicp_pipeline_graph_optimize_robust", C.c_int, [C.c_void_p, _dp, C.c_uint32, C.POINTER(GraphEdge), C.c_uint32,
                                                         C.POINTER(GraphParams), _dp, _dp, C.POINTER(GraphInfo),
                                                         C.POINTER(GraphRobust), _dp, _dp, C.POINTER(GraphRobustInfo)]),
    ("sageicp_graph_info_from_quality", C.c_int, [C.POINTER(Quality), _dp, C.c_double, _dp]),
    ("sageicp_place_tables", C.c_int, [C.POINTER(PlaceParams), _dp, _dp]),
    ("sageicp_place_describe", C.c_int, [_dp, C.c_uint64, C.POINTER(PlaceParams), C.c_void_p, C.c_int]),
    ("sageicp_place_describe_device", C.c_int, [C.POINTER(DeviceFrame), C.POINTER(PlaceParams), C.c_void_p, C.c_void_p]),
    ("sageicp_place_db_create", C.c_void_p, [C.POINTER(PlaceParams), C.c_int]),
    ("sageicp_place_db_destroy", None, [C.c_void_p]),
    ("sageicp_place_db_size", C.c_uint64, [C.c_void_p]),
    ("sageicp_place_db_clear", C.c_int, [C.c_void_p]),
    ("sageicp_place_db_add", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, _dp, _u64p]),
    ("sageicp_place_db_read", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("sageicp_place_db_match", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PlaceQuery), C.c_void_p, C.POINTER(C.c_uint32)]),
    ("sageicp_place_prior", C.c_int, [_dp, C.c_uint32, C.c_int32, _dp, _dp]),
    ("sageicp_pipeline_set_places", C.c_int, [C.c_void_p, C.c_int, C.POINTER(PlaceParams), C.POINTER(PlaceQuery)]),
    ("sageicp_pipeline_place_info", C.c_int, [C.c_void_p, C.POINTER(PlaceInfo)]),
    ("sageicp_pipeline_place_db", C.c_void_p, [C.c_void_p]),
    ("sageicp_pipeline_place_reset", C.c_int, [C.c_void_p]),
    ("sageicp_pipeline_create", C.c_void_p, [C.POINTER(PipelineConfig)]),
    ("sageicp_pipeline_destroy", None, [C.c_void_p]),
    ("sageicp_pipeline_register_frame", C.c_int,
     [C.c_void_p, _dp, C.c_uint64, _dp, _dp, _dp, _u64p, C.POINTER(Stats)]),
    ("sageicp_pipeline_prefetch", C.c_int, [C.c_void_p, _dp, C.c_uint64]),
    ("sageicp_pipeline_prefetch_cancel", C.c_int, [C.c_void_p]),
    ("sageicp_pipeline_prefetch_wait", C.c_int, [C.c_void_p]),
    ("sageicp_pipeline_reinitialize", C.c_int, [C.c_void_p]),
    ("sageicp_pipeline_num_poses", C.c_uint64, [C.c_void_p]),
    ("sageicp_pipeline_pose", C.c_int, [C.c_void_p, C.c_uint64, _dp]),
    ("sageicp_pipeline_local_map", C.c_void_p, [C.c_void_p]),
    ("sageicp_metrics_seq_error", C.c_int, [_dp, _dp, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    ("sageicp_metrics_absolute_trajectory_error", C.c_int,
     [_dp, _dp, C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
]

EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]

_lib = None

# The library reads its SAGEICP_* knobs from the environment once (sageicp_reload_env() makes it look again).  Tests and
# probes flip knobs between calls through os.environ: every change of a SAGEICP_* name marks the cache stale, and the next
# call through lib() reloads.
_env_stale = [False]
_Environ = type(os.environ)
if not getattr(_Environ, "_sageicp_hooked", False):
    _set0, _del0 = _Environ.__setitem__, _Environ.__delitem__

    def _set1(self, k, v):
        _set0(self, k, v)
        if str(k).startswith("SAGEICP_"):
            _env_stale[0] = True

    def _del1(self, k):
        _del0(self, k)
        if str(k).startswith("SAGEICP_"):
            _env_stale[0] = True

    _Environ.__setitem__, _Environ.__delitem__, _Environ._sageicp_hooked = _set1, _del1, True


class LoopStatus(C.Structure):
    _fields_ = [("calls_single_launch", C.c_uint64), ("calls_per_iteration", C.c_uint64), ("calls_chained", C.c_uint64), ("timeouts", C.c_uint32),
                ("cooldown_calls", C.c_uint32), ("derate_workgroups", C.c_uint32), ("last_fallback", C.c_int32)]


def lib():
    """Load libsageicp_hip.so.  Raises (loudly) if it has not been built — no fallback."""
    global _lib
    if _lib is not None and _env_stale[0]:
        _env_stale[0] = False
        _lib.sageicp_reload_env()
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        L.sageicp_abi_version.restype = C.c_int
        if L.sageicp_abi_version() != ABI_VERSION:      # struct layouts are part of the ABI
            raise ImportError("%s speaks ABI version %d, this binding %d: rebuild it"
                              % (LIB_PATH, L.sageicp_abi_version(), ABI_VERSION))
        for name, res, args in _SIGNATURES:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise SageIcpError(rc, (lib().sageicp_last_error() or b"").decode())


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def device_count():
    return int(lib().sageicp_device_count())


def voxel_hash(x, y, z):
    """the hash the map's slot table is keyed by (sageicp_voxel_hash; for tests)"""
    return int(lib().sageicp_voxel_hash(int(x), int(y), int(z)))


# ---- frames that are torch tensors on a GPU (sageicp_device_frame) ------------------------------------------------------
# torch is never imported here: a tensor can only exist once its caller has imported it.
_XYZ_DTYPES = {"torch.float32": DTYPE_FLOAT32, "torch.float64": DTYPE_FLOAT64}
_LABEL_DTYPES = {"torch.uint8": DTYPE_UINT8, "torch.int32": DTYPE_INT32, "torch.int64": DTYPE_INT64}


def _is_tensor(x):
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


def _is_device_tensor(x):
    """a torch tensor that is not in host memory: it takes the device path (a CPU tensor keeps the host path)"""
    return _is_tensor(x) and x.device.type != "cpu"


_one_runtime = [False]


def _hip_runtimes():
    """the distinct libamdhip64 files mapped into this process: {(device, inode): path}"""
    found = {}
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith("libamdhip64"):
                found.setdefault((parts[3], parts[4]), parts[5].strip())
    return found


def _check_one_hip_runtime():
    """Pointers and streams of a tensor mean something to this library only if torch and the library share one HIP
    runtime.  Some torch wheels bundle their own libamdhip64 with the ROCm one's soname: imported first, torch's is
    the one the library binds to; loaded after the library, it is a second runtime beside it."""
    if _one_runtime[0]:
        return
    paths = sorted(set(_hip_runtimes().values()))
    if len(paths) > 1:
        raise SageIcpError(ERR_INVALID, "two HIP runtimes are loaded in this process (%s): a torch tensor's memory and "
                                        "stream mean nothing to the library's; import torch before the first "
                                        "sage_icp_amd call" % " and ".join(paths))
    _one_runtime[0] = True       # (torch loads its runtime when it is imported, before any tensor exists)


def _current_stream(device):
    """the handle of torch's current stream on `device`: the library's work on torch tensors is ordered behind it"""
    return sys.modules["torch"].cuda.current_stream(device).cuda_stream


# the wording of _device_rows' messages for a frame that is read and for a destination that is written
_FRAME_WORDS = {
    "shape": "a device frame is a 2-D tensor with stride(1) == 1 and at least %d columns, not shape %s strides %s",
    "dtype": "a device frame is float32 or float64, not %s",
    "labels": "labels of a device frame are a tensor on the same device",
    "labels_shape": "labels: a 1-D tensor of %d elements, not shape %s",
    "labels_dtype": "labels are uint8, int32 or int64, not %s",
    "labels_device": "labels on %s, points on %s",
    "device": "the frame is on %s, the pipeline / map on GPU %d",
}
_OUT_WORDS = {
    "shape": "out= is a 2-D tensor with stride(1) == 1, rows that do not overlap and at least %d columns, not shape %s "
             "strides %s",
    "dtype": "out= is float32 or float64, not %s",
    "labels": "labels_out= is a tensor on the same device as out=",
    "labels_shape": "labels_out: a 1-D tensor of %d elements, not shape %s",
    "labels_dtype": "labels_out is uint8, int32 or int64, not %s",
    "labels_device": "labels_out on %s, out on %s",
    "device": "out= is on %s, the pipeline / map on GPU %d",
}


def _device_rows(struct, pts, labels, device, words, distinct=False):
    """(struct, stream) for rows that are a torch tensor on a GPU and their optional 1-D labels: a frame (DeviceFrame) or
    a destination (DevicePoints, distinct: its rows must not overlap).  Everything that can be wrong with the arguments
    raises ValueError here, before any call into the library; `words` are the messages."""
    cols = 3 if labels is not None else 4
    if pts.dim() != 2 or pts.shape[1] < cols or pts.stride(1) != 1 or \
            (distinct and pts.shape[0] > 1 and pts.stride(0) < cols):
        raise ValueError(words["shape"] % (cols, tuple(pts.shape), tuple(pts.stride())))
    xd = _XYZ_DTYPES.get(str(pts.dtype))
    if xd is None:
        raise ValueError(words["dtype"] % pts.dtype)
    if labels is not None:
        if not _is_device_tensor(labels):
            raise ValueError(words["labels"])
        if labels.dim() != 1 or labels.shape[0] != pts.shape[0] or \
                (distinct and labels.shape[0] > 1 and labels.stride(0) < 1):
            raise ValueError(words["labels_shape"] % (pts.shape[0], tuple(labels.shape)))
        if str(labels.dtype) not in _LABEL_DTYPES:
            raise ValueError(words["labels_dtype"] % labels.dtype)
        if labels.device != pts.device:
            raise ValueError(words["labels_device"] % (labels.device, pts.device))
    if pts.device.type != "cuda" or pts.device.index != device:
        raise ValueError(words["device"] % (pts.device, device))
    _check_one_hip_runtime()
    # (a destination of one row may have any row stride: it is described as rows that do not overlap)
    min_xyz, min_label = (cols, 1) if distinct else (0, 0)
    r = struct(pts.data_ptr() or None, max(pts.stride(0), min_xyz) * pts.element_size(), xd, 0, None, 0, pts.shape[0])
    if labels is not None:
        r.label, r.label_stride = labels.data_ptr() or None, max(labels.stride(0), min_label) * labels.element_size()
        r.label_dtype = _LABEL_DTYPES[str(labels.dtype)]
    return r, _current_stream(pts.device)


def _rows_out(device_index, count, host_rows, device_call, device, dtype, out, labels_out, first=0):
    """SageICP.source / SageICP.LocalMap / VoxelHashMap.Pointcloud: numpy (n, 4) float64 host rows (host_rows(n)); with
    device=True a fresh (n, 4) tensor on the GPU (float64, or dtype=torch.float32); with out= (and labels_out=) the
    caller's tensors, returned as the filled views out[:n] (and labels_out[:n]); an out= of fewer rows than there are
    gets its first len(out) rows (the C entries' cap).  device_call(DevicePoints, stream, n_out) is the C entry;
    count() the rows there are."""
    if labels_out is not None and out is None:
        raise ValueError("labels_out= goes with out=")
    if out is None and not device:
        if dtype is not None:
            raise ValueError("dtype= is for device=True or out= (the host rows are float64)")
        return host_rows(count())
    if out is not None:
        if dtype is not None and dtype != out.dtype:
            raise ValueError("dtype=%s but out= is %s" % (dtype, out.dtype))
        if not _is_device_tensor(out):
            raise ValueError("out= is a torch tensor on the GPU, not %s" % ("a tensor on %s" % out.device if _is_tensor(out)
                                                                              else type(out).__name__))
    else:
        import torch
        dt = torch.float64 if dtype is None else dtype
        if dt not in (torch.float32, torch.float64):
            raise ValueError("dtype= is torch.float32 or torch.float64, not %s" % (dt,))
        _check_one_hip_runtime()
        out = torch.empty((count(), 4), dtype=dt, device=torch.device("cuda", device_index))
    d, stream = _device_rows(DevicePoints, out, labels_out, device_index, _OUT_WORDS, distinct=True)
    n = C.c_uint64(0)
    _check(device_call(C.byref(d), stream, C.byref(n)))
    k = min(max(0, n.value - first), out.shape[0])      # (first: the entry skipped that many of the n rows there are)
    return out[:k] if labels_out is None else (out[:k], labels_out[:k])


# ---- sensor_msgs/PointCloud2 (sageicp_msg_layout) ---------------------------------------------------------
class PointField:
    """sensor_msgs/PointField: a plain container with the message's attribute names and datatype codes"""
    INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = 1, 2, 3, 4, 5, 6, 7, 8

    def __init__(self, name, offset, datatype, count=1):
        self.name, self.offset, self.datatype, self.count = name, int(offset), int(datatype), int(count)

    def __repr__(self):
        return "PointField(%r, %d, %d, %d)" % (self.name, self.offset, self.datatype, self.count)


class PointCloud2:
    """sensor_msgs/PointCloud2 without ROS: a plain container, for tests and callers that have no rclpy.  Anything with
    these attributes (rclpy's message among them) is taken wherever this is.  data: bytes, a bytearray, an array('B'), a
    numpy uint8 array, or a 1-D uint8 torch tensor on the pipeline's GPU."""

    def __init__(self, fields, point_step, data, width=None, height=1, is_bigendian=False, row_step=None, header=None):
        self.header = header
        self.fields = list(fields)
        self.point_step = int(point_step)
        self.height = int(height)
        self.width = int(width) if width is not None else (len(data) // self.point_step if self.point_step else 0)
        self.row_step = int(row_step) if row_step is not None else self.width * self.point_step
        self.is_bigendian = bool(is_bigendian)
        self.is_dense = True
        self.data = data


_FIELD_TYPE_NAMES = {1: "INT8", 2: "UINT8", 3: "INT16", 4: "UINT16", 5: "INT32", 6: "UINT32", 7: "FLOAT32", 8: "FLOAT64"}
NO_TIME_FIELD = "Field 't', 'timestamp', or 'time'  does not exist"      # GetTimestampField's text, ros/ros2/Utils.hpp:63


def _is_message(x):
    return hasattr(x, "fields") and hasattr(x, "point_step") and hasattr(x, "data")


def _field_as(field, datatype, why=""):
    if int(field.datatype) != datatype:
        raise ValueError("field '%s' is declared %s; it is read as %s%s (the reference would reinterpret its bytes)"
                         % (field.name, _FIELD_TYPE_NAMES.get(int(field.datatype), "datatype %d" % field.datatype),
                            _FIELD_TYPE_NAMES[datatype], why))
    return int(field.offset)


def pointcloud2_layout(msg, want_time):
    """The MsgLayout of a PointCloud2 by the reference's field-name rules: x, y, z and label by name (the
    first of a name, as sensor_msgs' iterators take it), FLOAT32 each, the label UINT8 when the message has exactly five
    fields; with want_time the LAST field named t, timestamp (UINT32) or time (FLOAT64).  ValueError names what does
    not fit; a big-endian message is refused."""
    if getattr(msg, "is_bigendian", False):
        raise ValueError("a big-endian PointCloud2 is not supported")
    fields = list(msg.fields)

    def named(name):
        for f in fields:
            if f.name == name:
                return f
        raise ValueError("Field %s does not exist" % name)

    lay = MsgLayout()
    lay.point_step = int(msg.point_step)
    lay.x_offset = _field_as(named("x"), PointField.FLOAT32)
    lay.y_offset = _field_as(named("y"), PointField.FLOAT32)
    lay.z_offset = _field_as(named("z"), PointField.FLOAT32)
    if len(fields) == 5:            # the fields.size() == 5 switch of PointCloud2ToEigen, Utils.hpp:167
        lay.label_offset = _field_as(named("label"), PointField.UINT8, " in a message of exactly five fields")
        lay.label_dtype = DTYPE_UINT8
    else:
        lay.label_offset = _field_as(named("label"), PointField.FLOAT32, " in a message of %d fields" % len(fields))
        lay.label_dtype = DTYPE_FLOAT32
    lay.time_kind, lay.time_offset = 0, 0
    if want_time:
        tf = None
        for f in fields:
            if f.name in ("t", "timestamp", "time"):
                tf = f
        if tf is None or not int(getattr(tf, "count", 1)):
            raise ValueError(NO_TIME_FIELD)
        if tf.name == "time":
            lay.time_offset, lay.time_kind = _field_as(tf, PointField.FLOAT64), 2
        else:
            lay.time_offset, lay.time_kind = _field_as(tf, PointField.UINT32), 1
    return lay


def _message_data(data, device_index):
    """(address, bytes, keep-alive, stream or None) of a message's data; stream is not None for a device tensor"""
    if _is_tensor(data):
        if str(data.dtype) != "torch.uint8" or data.dim() != 1 or (data.shape[0] > 1 and data.stride(0) != 1):
            raise ValueError("message data as a tensor is a contiguous 1-D uint8 tensor, not %s shape %s"
                             % (data.dtype, tuple(data.shape)))
        if data.device.type == "cpu":
            data = data.numpy()
        else:
            if data.device.type != "cuda" or data.device.index != device_index:
                raise ValueError("the message data is on %s, the pipeline on GPU %d" % (data.device, device_index))
            _check_one_hip_runtime()
            return data.data_ptr() or None, int(data.shape[0]), data, _current_stream(data.device)
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8 or data.ndim != 1:
            raise ValueError("message data as an array is 1-D uint8, not %s shape %s" % (data.dtype, data.shape))
        a = np.ascontiguousarray(data)
    else:
        a = np.frombuffer(data, dtype=np.uint8)
    return (a.ctypes.data or None) if a.size else None, int(a.size), a, None


def msg_output_fields():
    """the field table of the outgoing 21-byte record (sageicp_msg_output_fields) as PointFields"""
    buf = (MsgField * 8)()
    k = lib().sageicp_msg_output_fields(buf, 8)
    return [PointField(buf[i].name.decode(), buf[i].offset, buf[i].datatype, buf[i].count) for i in range(k)]


def output_pointcloud2(records, header=None):
    """a PointCloud2 around (n, 21) records (source_msg / LocalMapMsg / PointcloudMsg), as CreatePointCloud2Msg lays
    it out: the five fields, point_step 21, height 1, width n"""
    n = int(records.shape[0])
    return PointCloud2(msg_output_fields(), MSG_POINT_STEP, records.reshape(-1), width=n, height=1, header=header)


def _msg_colors(colors):
    """MsgColors of a {label: colour} mapping or (label, colour) pairs; None: an empty table"""
    pairs = list(colors.items()) if hasattr(colors, "items") else list(colors or ())
    n = len(pairs)
    keys = (C.c_int32 * max(n, 1))(*[int(k) for k, _ in pairs])
    vals = (C.c_int32 * max(n, 1))(*[int(v) for _, v in pairs])
    c = MsgColors(keys, vals, n)
    c._keep = (keys, vals)
    return c


def _records_out(device_index, count, host_call, device_call, colors, device, out, first=0):
    """source_msg / LocalMapMsg / PointcloudMsg: the rows as (n, 21) uint8 records — numpy, with device=True a fresh
    tensor on the GPU, with out= the caller's buffer (a C-contiguous uint8 numpy array or a contiguous uint8 tensor on
    the GPU, 1-D or (k, 21), any base alignment): its first min(rows that fit, n) records are written and returned as a
    view.  host_call(colors, ptr, cap, n_out) / device_call(colors, ptr, cap, stream, n_out) are the C entries."""
    c = _msg_colors(colors)
    n = C.c_uint64(0)
    if out is None and not device:
        a = np.empty((count(), MSG_POINT_STEP), dtype=np.uint8)
        _check(host_call(C.byref(c), a.ctypes.data_as(C.c_void_p) if a.size else None, a.shape[0], C.byref(n)))
        return a[:min(max(0, n.value - first), a.shape[0])]
    if out is None:
        import torch
        _check_one_hip_runtime()
        out = torch.empty((count(), MSG_POINT_STEP), dtype=torch.uint8, device=torch.device("cuda", device_index))
    if isinstance(out, np.ndarray):
        if out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError("out= as an array is writable C-contiguous uint8")
        if out.ndim == 2 and out.shape[1] != MSG_POINT_STEP or out.ndim not in (1, 2):
            raise ValueError("out= is 1-D or (k, %d)" % MSG_POINT_STEP)
        cap = out.size // MSG_POINT_STEP
        _check(host_call(C.byref(c), out.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n)))
        k = min(max(0, n.value - first), cap)
        return out.reshape(-1)[:k * MSG_POINT_STEP].reshape(k, MSG_POINT_STEP)
    if not _is_device_tensor(out):
        raise ValueError("out= is a uint8 numpy array or a uint8 torch tensor on the GPU")
    if str(out.dtype) != "torch.uint8" or not out.is_contiguous() or out.dim() not in (1, 2) or \
            (out.dim() == 2 and out.shape[1] != MSG_POINT_STEP):
        raise ValueError("out= as a tensor is contiguous uint8, 1-D or (k, %d)" % MSG_POINT_STEP)
    if out.device.type != "cuda" or out.device.index != device_index:
        raise ValueError("out= is on %s, the pipeline / map on GPU %d" % (out.device, device_index))
    _check_one_hip_runtime()
    cap = out.numel() // MSG_POINT_STEP
    _check(device_call(C.byref(c), (out.data_ptr() or None) if cap else None, cap, _current_stream(out.device), C.byref(n)))
    k = min(max(0, n.value - first), cap)
    return out.reshape(-1)[:k * MSG_POINT_STEP].view(k, MSG_POINT_STEP)


def robin_sweep(vox, far, listed):
    """sageicp_robin_sweep: (erased voxels in erasure order, iteration order of the rest)"""
    v = np.ascontiguousarray(vox, dtype=np.int32).reshape(-1, 3)
    f = np.ascontiguousarray(far, dtype=np.uint8)
    n = len(v)
    er, af = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
    ne, na = C.c_uint64(0), C.c_uint64(0)
    _check(lib().sageicp_robin_sweep(v.ctypes.data_as(C.c_void_p), n, f.ctypes.data_as(C.c_void_p), 1 if listed else 0,
                                     er.ctypes.data_as(C.c_void_p), C.byref(ne), af.ctypes.data_as(C.c_void_p), C.byref(na)))
    return er[:ne.value].copy(), af[:na.value].copy()


def set_downsample_order(reference_order=True):
    """True (default): VoxelDownsample emits in the reference's robin_map bucket order; False: arrival order"""
    lib().sageicp_set_downsample_order(1 if reference_order else 0)


def set_profiling(level):
    """0 off; 1 (or True) HIP events around k_icp in one iteration out of 8 (what bench.py times
    with); 2 around every kernel of every iteration"""
    lib().sageicp_set_profiling(int(level))


def set_counting(on):
    """True (default): calls that return statistics count candidates and evaluated pairs (sum_candidates,
    pairs_evaluated); False: those two stay zero and the search runs as it does for a caller without statistics"""
    lib().sageicp_set_counting(1 if on else 0)


class Frame:
    """A scan resident in HBM (sageicp_frame).  `pts`: (n,4) host rows, or a torch tensor on the map's GPU (float32 /
    float64, x y z in its first three columns; the label in column 3 or, given, `labels`: 1-D uint8 / int32 / int64 on
    the same device), built on the device in the current torch stream's order."""

    def __init__(self, vmap, pts, labels=None):
        if _is_device_tensor(pts):
            f, stream = _device_rows(DeviceFrame, pts, labels, vmap.device, _FRAME_WORDS)
            self.n = int(f.n)
            self._h = lib().sageicp_frame_from_device(vmap._h, C.byref(f), stream)
            if not self._h:
                raise SageIcpError(ERR_INVALID, (lib().sageicp_last_error() or b"").decode())
            return
        if labels is not None:
            raise ValueError("labels= is for a frame that is a torch tensor on a GPU")
        pts, pp = _d(pts)
        self.n = pts.reshape(-1, 4).shape[0]
        self._h = lib().sageicp_frame_upload(vmap._h, pp, self.n)
        if not self._h:
            raise SageIcpError(ERR_HIP, (lib().sageicp_last_error() or b"").decode())

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:       # (None: interpreter shutdown)
            lib().sageicp_frame_destroy(self._h)
            self._h = None


class Comm:
    """Communicator for query-sharded registration (one process per GPU): RCCL all-reduce, or the
    direct exchange over xGMI once p2p_connect() has been called."""

    def __init__(self, unique_id, rank, nranks, device):
        self.rank, self.nranks = rank, nranks
        if unique_id is None:                       # no RCCL side: direct exchange only
            self._h = lib().sageicp_comm_create_local(rank, nranks, device)
        else:
            buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
            self._h = lib().sageicp_comm_create(buf, rank, nranks, device)
        if not self._h:
            raise SageIcpError(ERR_RCCL, (lib().sageicp_last_error() or b"").decode())

    def p2p_export(self):
        buf = (C.c_uint8 * P2P_HANDLE_BYTES)()
        _check(lib().sageicp_comm_p2p_export(self._h, buf))
        return bytes(buf)

    def p2p_connect(self, handles):
        """handles: the p2p_export() of every rank, in rank order"""
        assert len(handles) == self.nranks
        flat = b"".join(bytes(h) for h in handles)
        buf = (C.c_uint8 * len(flat)).from_buffer_copy(flat)
        _check(lib().sageicp_comm_p2p_connect(self._h, buf))

    def p2p_enable(self, on=True):
        _check(lib().sageicp_comm_p2p_enable(self._h, 1 if on else 0))

    @property
    def p2p_enabled(self):
        return bool(lib().sageicp_comm_p2p_enabled(self._h))

    def describe(self):
        """dict: the ranks as created, the ranks RCCL itself reports (-1 without an RCCL side), the
        state of the direct exchange"""
        info = CommInfo()
        _check(lib().sageicp_comm_describe(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in CommInfo._fields_ if k != "reserved"}

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        _check(lib().sageicp_comm_unique_id(buf))
        return bytes(buf)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:       # (None: interpreter shutdown)
            lib().sageicp_comm_destroy(self._h)
            self._h = None


class VoxelHashMap:
    """sage_icp::VoxelHashMap (core/VoxelHashMap.hpp:35-107) over the C ABI."""

    def __init__(self, voxel_size, max_distance, basic_points_per_voxel=20,
                 critical_points_per_voxel=20, basic_parts_labels=(40, 44, 48, 49, 50, 70, 72),
                 device=0, _handle=None):
        self.voxel_size_ = voxel_size
        self.max_distance_ = max_distance
        self.basic_points_per_voxel_ = basic_points_per_voxel
        self.critical_points_per_voxel_ = critical_points_per_voxel
        self.basic_parts_labels_ = list(basic_parts_labels)
        self.device = device
        if _handle is not None:
            self._h = _handle
            return
        labels = (C.c_int * len(self.basic_parts_labels_))(*self.basic_parts_labels_)
        self._h = lib().sageicp_map_create(voxel_size, max_distance, basic_points_per_voxel,
                                           critical_points_per_voxel, labels,
                                           len(self.basic_parts_labels_), device)
        if not self._h:
            raise SageIcpError(ERR_INVALID, (lib().sageicp_last_error() or b"").decode())

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:       # (None: interpreter shutdown)
            lib().sageicp_map_destroy(self._h)
            self._h = None

    def clone(self):
        h = lib().sageicp_map_clone(self._h)
        return VoxelHashMap(self.voxel_size_, self.max_distance_, self.basic_points_per_voxel_,
                            self.critical_points_per_voxel_, self.basic_parts_labels_,
                            self.device, _handle=h)

    def set_reference_order(self, on=True):
        """Reference-order mode (include/sageicp.h): the far-voxel sweep erases while iterating the
        reference's robin_map bucket array and Pointcloud() lists the voxels in bucket order.  The map
        must be empty."""
        _check(lib().sageicp_map_set_reference_order(self._h, 1 if on else 0))
        return self

    def reference_order(self):
        """0 off, 1 on, -1 on but beyond what the emulation models"""
        return int(lib().sageicp_map_reference_order(self._h))

    def set_devices(self, devices):
        """single-process multi-GPU mode: the map spans these devices, RegisterFrame shards over them"""
        arr = (C.c_int * len(devices))(*devices)
        _check(lib().sageicp_map_set_devices(self._h, arr, len(devices)))

    def num_devices(self):
        return int(lib().sageicp_map_num_devices(self._h))

    # names follow the reference's members
    def Clear(self):
        _check(lib().sageicp_map_clear(self._h))

    def Empty(self):
        return bool(lib().sageicp_map_empty(self._h))

    def size(self):
        return int(lib().sageicp_map_size(self._h))

    def num_voxels(self):
        return int(lib().sageicp_map_num_voxels(self._h))

    def AddPoints(self, pts):
        pts, pp = _d(pts)
        _check(lib().sageicp_map_add_points(self._h, pp, pts.reshape(-1, 4).shape[0]))

    def RemovePointsFarFromLocation(self, origin):
        o, op = _d(origin)
        _check(lib().sageicp_map_remove_far(self._h, op))

    def UpdateOnDevice(self, pts, pose):
        """Update(points, pose) executed on the GPU against the HBM-resident map (row f-2)."""
        pts, pp = _d(pts)
        x, xp = _d(pose)
        assert x.size == 7
        _check(lib().sageicp_map_update_pose_device(self._h, pp, pts.reshape(-1, 4).shape[0], xp))

    def Update(self, pts, pose_or_origin):
        pts, pp = _d(pts)
        x, xp = _d(pose_or_origin)
        n = pts.reshape(-1, 4).shape[0]
        if x.size == 7:
            _check(lib().sageicp_map_update_pose(self._h, pp, n, xp))
        elif x.size == 3:
            _check(lib().sageicp_map_update(self._h, pp, n, xp))
        else:
            raise ValueError("Update takes a pose[7] or an origin[3]")

    def Pointcloud(self, device=False, dtype=None, out=None, labels_out=None):
        """Pointcloud(): the host rows, numpy (n, 4) float64.  device=True: a fresh (n, 4) torch tensor on the map's GPU
        (float64, or dtype=torch.float32); out= (and a 1-D uint8 / int32 / int64 labels_out=): the caller's tensors on
        that GPU, filled with the first rows that fit and returned as out[:n] (labels_out[:n]).  An out= shorter than
        size() gets only its first len(out) rows, as the C entry writes them: compare the returned length with size(),
        or size the tensor from it.  Same rows in the same order either way (sageicp_map_pointcloud_device), written in
        the order of the device's current torch stream; synchronous."""
        if not device and dtype is None and out is None and labels_out is None:
            n = self.size()
            out = np.empty((n, 4))
            lib().sageicp_map_pointcloud(self._h, out.ctypes.data_as(_dp), n)
            return out
        return _map_rows(lambda: self._h, self.device, device, dtype, out, labels_out)

    def PointcloudMsg(self, colors, device=False, out=None):
        """Pointcloud()'s rows, in its order, as the (n, 21) uint8 records EigenToPointCloud2 writes
        (sageicp_map_pointcloud_msg[_device]; colors: {label: colour}): numpy, a fresh tensor with device=True, or the
        caller's out= (see _records_out).  A label outside [0, 255] or without a colour raises (ERR_INVALID)."""
        return _records_out(self.device, self.size,
                            lambda c, o, cap, n: lib().sageicp_map_pointcloud_msg(self._h, c, o, cap, n),
                            lambda c, o, cap, s, n: lib().sageicp_map_pointcloud_msg_device(self._h, c, o, cap, s, n),
                            colors, device, out)

    # ---- the archive: what the map evicts, and the session's map (include/sageicp.h) ----
    def set_archive(self, enable=True, max_rows=0):
        """Keep every voxel the map evicts from now on (off by default); max_rows bounds the log (0: no limit)"""
        _check(lib().sageicp_map_set_archive(self._h, 1 if enable else 0, int(max_rows)))
        return self

    def archive_info(self):
        return _archive_info(self._h)

    def archive_voxels(self):
        """the log's records, one per evicted voxel: a numpy record array (ARCHIVE_VOXEL_DTYPE)"""
        return _archive_voxels(self._h)

    def archive_clear(self):
        _check(lib().sageicp_map_archive_clear(self._h))

    def ArchivedPointcloud(self, which="all", first=0, device=False, dtype=None, out=None, labels_out=None):
        """The rows of a selection from row `first` on: "all" the log as recorded, "latest" the last generation of every
        key the live map does not hold, "session" those followed by Pointcloud().  The keywords as Pointcloud()."""
        return _archive_rows(lambda: self._h, self.device, which, first, device, dtype, out, labels_out)

    def ArchivedPointcloudMsg(self, colors, which="all", first=0, device=False, out=None):
        """ArchivedPointcloud()'s rows as (n, 21) uint8 records; the arguments as PointcloudMsg"""
        return _archive_msg(lambda: self._h, self.device, colors, which, first, device, out)

    def Recall(self, center, radius, into=None):
        """The voxels of the session's map (the archive's latest generations, then the live map: what
        ArchivedPointcloud("session") exports) whose first row lies within `radius` of `center`, put into the map `into`
        on the device (sageicp_map_recall).  `into` is cleared first and ends resident; None: a new map
        with this map's parameters on its device, max_distance = radius.  Returns (into, info dict)."""
        return _recall(lib().sageicp_map_recall, self._h, self, center, radius, into)

    # ---- loop closure: the pose every voxel belongs to, the session's map re-posed ----
    def SessionStays(self, positions, which="session", first=0):
        """One uint32 per voxel of the selection, in its order (the records of "all" / "latest", then for "session" the
        live voxels in Pointcloud() order): the index into `positions` (n, 3) — the sensor position of the call with
        serial s — of the pose the voxel is tied to (sageicp_map_session_stays)."""
        w, first = _archive_which(which), int(first)
        pos = _positions(positions)
        # room for an upper bound that costs no device work (every record, and for "session" every live voxel): the
        # selection is then computed once, by the call that writes, and the result trimmed to what it reported
        room = max(0, self.archive_info()["voxels"] + (self.num_voxels() if w == SESSION else 0) - first)
        out = np.zeros(room, dtype=np.uint32)
        n = C.c_uint64(0)
        _check(lib().sageicp_map_session_stays(self._h, w, first, _p(pos), pos.shape[0],
                                               out.ctypes.data_as(C.POINTER(C.c_uint32)) if room else None, room, C.byref(n)))
        return out[:min(max(0, n.value - first), room)]

    def CorrectedPointcloud(self, which="session", positions=None, corrections=None, first=0, device=False, dtype=None, out=None,
                            labels_out=None):
        """ArchivedPointcloud(which)'s rows, each moved by corrections[stay of its voxel] (closure_corrections; the stays
        as SessionStays takes them against `positions`), label untouched (sageicp_map_session_corrected[_device]).  The
        other keywords as Pointcloud()."""
        pos, corr = _positions(positions), _corrections(corrections, positions)
        w, first, n = _archive_which(which), int(first), pos.shape[0]
        return _corrected_rows(lambda: self._h, self.device, w, first, device, dtype, out, labels_out,
                               lambda a, cap, k: lib().sageicp_map_session_corrected(self._h, w, first, _p(pos), _p(corr), n, a, cap, k),
                               lambda d, st, k: lib().sageicp_map_session_corrected_device(self._h, w, first, _p(pos), _p(corr), n,
                                                                                           d, st, k))

    def RebuildSession(self, positions, corrections, which="session", center=None, radius=math.inf, into=None):
        """CorrectedPointcloud(which)'s rows voxelised again under the map's retention policy, on the device, into the map
        `into`: what a fresh map holds after AddPoints of those rows and, with a `center`, RemovePointsFarFromLocation
        at max_distance = radius (sageicp_map_session_rebuild).  `into` is cleared first and ends
        resident; None: a new map with this map's parameters on its device.  Returns (into, info dict)."""
        pos, corr = _positions(positions), _corrections(corrections, positions)
        w, n = _archive_which(which), pos.shape[0]
        return _rebuild(lambda c, r, h, i: lib().sageicp_map_session_rebuild(self._h, w, _p(pos), _p(corr), n, c, r, h, i),
                        self, center, radius, into)

    def resident(self):
        """True while the HBM copy of the map is the authority (after a device-side update)"""
        return bool(lib().sageicp_map_resident(self._h))

    def point_slots(self):
        """32-B point slots the voxel storage occupies (size-classed regions, free ones included)"""
        return int(lib().sageicp_map_point_slots(self._h))

    def table_stats(self):
        """(capacity, used slots, live voxels) of the slot table of whichever copy is the authority (for tests)"""
        out = (C.c_uint64 * 3)()
        _check(lib().sageicp_map_table_stats(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def sync(self):
        _check(lib().sageicp_map_sync(self._h))

    def loop_status(self):
        """sageicp_map_loop_status: which form of the ICP loop this handle's calls took, and why"""
        st = LoopStatus()
        _check(lib().sageicp_map_loop_status(self._h, C.byref(st)))
        return st

    def GetCorrespondences(self, pts, max_correspondance_distance, th, with_index=False, labels=None, pose=None,
                           dtype=None):
        """GetCorrespondences (core/VoxelHashMap.cpp:48-130): (src, tgt[, idx]), the accepted pairs in query order.
        `pts` as numpy (n, 4) rows or a CPU tensor: numpy (k, 4) float64 arrays and an int64 idx
        (sageicp_get_correspondences; the target rows are read from the host copy, so a resident map is handed back to
        the host).  `pts` as a torch tensor on the map's GPU, in the layouts RegisterFrame takes (`labels` as there):
        tensors on that GPU — (k, 4) float64, or dtype=torch.float32, and an int64 idx — allocated at n rows and
        returned as [:k] views (sageicp_get_correspondences_device); with pose= (qx, qy, qz, qw, tx, ty, tz) the rows
        are first moved as transform_points moves them, and src holds the moved rows.  The map stays where it is: a
        resident map stays resident.  Ordered on the device's current torch stream; synchronous."""
        if _is_device_tensor(pts):
            return self._correspondences_device(pts, max_correspondance_distance, th, with_index, labels, pose, dtype)
        for name, v in (("labels", labels), ("pose", pose), ("dtype", dtype)):
            if v is not None:
                raise ValueError("%s= is for a frame that is a torch tensor on a GPU" % name)
        pts, pp = _d(pts)
        n = pts.reshape(-1, 4).shape[0]
        src = np.empty((n, 4))
        tgt = np.empty((n, 4))
        idx = np.empty(n, dtype=np.int64)
        nout = C.c_uint64(0)
        _check(lib().sageicp_get_correspondences(
            self._h, pp, n, max_correspondance_distance, th, src.ctypes.data_as(_dp),
            tgt.ctypes.data_as(_dp), C.byref(nout), idx.ctypes.data_as(_i64p)))
        k = nout.value
        if with_index:
            return src[:k].copy(), tgt[:k].copy(), idx[:k].copy()
        return src[:k].copy(), tgt[:k].copy()

    def RegistrationQuality(self, pts, max_correspondance_distance, kernel, th, pose=None, labels=None):
        """The quality report (Quality) of `pts` at `pose` against this map: fitness, rmse, the Gauss-Newton system over
        the pairs GetCorrespondences accepts for the same arguments, the step still left, covariances, class tables.
        `pts` as numpy (n, 4) rows (sageicp_registration_quality) or a torch tensor on the map's GPU in the layouts
        RegisterFrame takes, `labels` as there (sageicp_registration_quality_device; ordered on the device's current
        torch stream).  With pose= (qx, qy, qz, qw, tx, ty, tz) the rows are first moved as transform_points moves
        them.  Synchronous; a resident map stays resident."""
        pp = None
        if pose is not None:
            pose_a, pp = _d(pose)
            if pose_a.size != 7:
                raise ValueError("a pose is (qx, qy, qz, qw, tx, ty, tz)")
        q = Quality()
        if _is_device_tensor(pts):
            f, stream = _device_rows(DeviceFrame, pts, labels, self.device, _FRAME_WORDS)
            _check(lib().sageicp_registration_quality_device(self._h, C.byref(f), pp, max_correspondance_distance, kernel,
                                                             th, stream, C.byref(q)))
            return q
        if labels is not None:
            raise ValueError("labels= is for a frame that is a torch tensor on a GPU")
        pts, fp = _d(pts)
        _check(lib().sageicp_registration_quality(self._h, fp, pts.reshape(-1, 4).shape[0], pp,
                                                  max_correspondance_distance, kernel, th, C.byref(q)))
        return q

    def ScorePoses(self, pts, poses, max_correspondance_distance, kernel, th, labels=None):
        """A batch of candidate poses scored in one pass (sageicp_score_poses[_device]): a numpy record array
        (POSE_SCORE_DTYPE) with one PoseScore per row of `poses` ((k, 7): qx, qy, qz, qw, tx, ty, tz), each bit for bit
        the same-named fields of RegistrationQuality(pts, ..., pose=poses[c]).  `pts` as numpy (n, 4) rows or a torch
        tensor on the map's GPU in the layouts RegisterFrame takes, `labels` as there.  Synchronous; a resident map
        stays resident.  The work buffers stay reserved on the map (SAGEICP_SCORE_CHUNK_ROWS rows at most per chunk)."""
        poses_a, pp = _d(poses)
        if poses_a.size % 7:
            raise ValueError("poses is (k, 7): qx, qy, qz, qw, tx, ty, tz per row")
        k = poses_a.size // 7
        out = np.zeros(k, dtype=POSE_SCORE_DTYPE)
        if _is_device_tensor(pts):
            f, stream = _device_rows(DeviceFrame, pts, labels, self.device, _FRAME_WORDS)
            _check(lib().sageicp_score_poses_device(self._h, C.byref(f), pp, k, max_correspondance_distance, kernel, th,
                                                    stream, out.ctypes.data))
            return out
        if labels is not None:
            raise ValueError("labels= is for a frame that is a torch tensor on a GPU")
        pts, fp = _d(pts)
        _check(lib().sageicp_score_poses(self._h, fp, pts.reshape(-1, 4).shape[0], pp, k, max_correspondance_distance,
                                         kernel, th, out.ctypes.data))
        return out

    def Relocalize(self, pts, prior, max_correspondance_distance, kernel, th, xy=(0, 0), z=(0, 0), yaw=(0, 0),
                   refine_top=3, labels=None):
        """Recover a frame whose guess lies outside the basin of the ICP (sageicp_relocalize[_device]): the grid of
        relocalize_candidates(prior, xy, z, yaw) scored in one batch, the best `refine_top` refined by RegisterFrame, the
        result with the largest sum_w returned as (pose, Quality at that pose, info dict).  Each of xy, z, yaw is
        (extent, step): metres along the world axes, radians about world z.  The map is kept, unlike the node's
        reinit."""
        prior_a, pr = _d(prior)
        if prior_a.size != 7:
            raise ValueError("a pose is (qx, qy, qz, qw, tx, ty, tz)")
        params = _relocalize_params(xy, z, yaw, refine_top, max_correspondance_distance, kernel, th)
        pose, q, info = np.empty(7), Quality(), RelocalizeInfo()
        if _is_device_tensor(pts):
            f, stream = _device_rows(DeviceFrame, pts, labels, self.device, _FRAME_WORDS)
            _check(lib().sageicp_relocalize_device(self._h, C.byref(f), pr, C.byref(params), stream,
                                                   pose.ctypes.data_as(_dp), C.byref(q), C.byref(info)))
            return pose, q, info.as_dict()
        if labels is not None:
            raise ValueError("labels= is for a frame that is a torch tensor on a GPU")
        pts, fp = _d(pts)
        _check(lib().sageicp_relocalize(self._h, fp, pts.reshape(-1, 4).shape[0], pr, C.byref(params),
                                        pose.ctypes.data_as(_dp), C.byref(q), C.byref(info)))
        return pose, q, info.as_dict()

    def _correspondences_device(self, pts, max_dist, th, with_index, labels, pose, dtype):
        # everything that can be wrong with the arguments raises ValueError before any call into the library
        f, stream = _device_rows(DeviceFrame, pts, labels, self.device, _FRAME_WORDS)
        pp = None
        if pose is not None:
            pose_a, pp = _d(pose)
            if pose_a.size != 7:
                raise ValueError("a pose is (qx, qy, qz, qw, tx, ty, tz)")
        import torch
        dt = torch.float64 if dtype is None else dtype
        if dt not in (torch.float32, torch.float64):
            raise ValueError("dtype= is torch.float32 or torch.float64, not %s" % (dt,))
        n = int(f.n)
        src = torch.empty((n, 4), dtype=dt, device=pts.device)
        tgt = torch.empty((n, 4), dtype=dt, device=pts.device)
        idx = torch.empty(n, dtype=torch.int64, device=pts.device) if with_index else None
        ds, _ = _device_rows(DevicePoints, src, None, self.device, _OUT_WORDS, distinct=True)
        dg, _ = _device_rows(DevicePoints, tgt, None, self.device, _OUT_WORDS, distinct=True)
        nout = C.c_uint64(0)
        _check(lib().sageicp_get_correspondences_device(
            self._h, C.byref(f), pp, max_dist, th, C.byref(ds), C.byref(dg),
            (idx.data_ptr() or None) if with_index else None, n, stream, C.byref(nout)))
        k = nout.value
        return (src[:k], tgt[:k], idx[:k]) if with_index else (src[:k], tgt[:k])


def _relocalize_params(xy, z, yaw, refine_top=0, max_correspondence_distance=0.0, kernel=1.0, sem_th=0.0):
    p = RelocalizeParams()
    (p.xy_extent, p.xy_step), (p.z_extent, p.z_step), (p.yaw_extent, p.yaw_step) = xy, z, yaw
    p.refine_top = refine_top
    p.max_correspondence_distance, p.kernel, p.sem_th = max_correspondence_distance, kernel, sem_th
    return p


def relocalize_candidates(prior, xy=(0, 0), z=(0, 0), yaw=(0, 0), cap=None):
    """The candidate poses of Relocalize around `prior` (sageicp_relocalize_candidates; the bits are the library's): a
    (K, 7) array, yaw outermost, then x, then y, z innermost, each index ascending from -m to +m.  Each of xy, z, yaw is
    (extent, step).  cap=: at most that many rows are written and (rows, K) is returned."""
    prior_a, pr = _d(prior)
    if prior_a.size != 7:
        raise ValueError("a pose is (qx, qy, qz, qw, tx, ty, tz)")
    params = _relocalize_params(xy, z, yaw)
    k = C.c_uint64(0)
    if cap is None:
        _check(lib().sageicp_relocalize_candidates(pr, C.byref(params), None, 0, C.byref(k)))
    rows = k.value if cap is None else int(cap)
    out = np.empty((rows, 7))
    _check(lib().sageicp_relocalize_candidates(pr, C.byref(params), out.ctypes.data_as(_dp), rows, C.byref(k)))
    return out if cap is None else (out[:min(rows, k.value)], k.value)


def register_frame(frame, voxel_map, initial_guess, max_correspondence_distance, kernel, sem_th,
                   comm=None, return_stats=False):
    """sage_icp::RegisterFrame (core/Registration.cpp:113-141).  `frame` is an (n,4) array or a
    resident Frame; with `comm` the call is one rank of a query-sharded registration."""
    init, ip = _d(initial_guess)
    out = np.empty(7)
    st = Stats()
    if isinstance(frame, Frame):
        _check(lib().sageicp_register_frame_resident(
            voxel_map._h, frame._h, ip, max_correspondence_distance, kernel, sem_th,
            comm._h if comm is not None else None, out.ctypes.data_as(_dp), C.byref(st)))
    else:
        if comm is not None:
            raise ValueError("sharded registration needs a resident Frame")
        pts, pp = _d(frame)
        _check(lib().sageicp_register_frame(
            voxel_map._h, pp, pts.reshape(-1, 4).shape[0], ip, max_correspondence_distance,
            kernel, sem_th, out.ctypes.data_as(_dp), C.byref(st)))
    return (out, st) if return_stats else out


def transform_points(pose, pts, device=0):
    T, tp = _d(pose)
    out = np.array(pts, dtype=np.float64, order="C", copy=True).reshape(-1, 4)
    _check(lib().sageicp_transform_points(tp, out.ctypes.data_as(_dp), out.shape[0], device))
    return out


def occupancy_grid(frame, bounds=KEY_FRAME_BOUNDS, occ_size=KEY_FRAME_OCC_SIZE, pose=None, device=0, labels=None):
    """The key-frame selection's bird's-eye grid of a frame (EigenToGridMap, ros/ros2/Utils.hpp:221-242), moved by
    `pose` first if given: (H, W) uint8 numpy, 0 / 1.  `frame` is numpy (n, 4) rows (sageicp_occupancy_grid, on GPU
    `device`) or a torch tensor on a GPU in the layouts RegisterFrame takes (sageicp_occupancy_grid_device, on the
    tensor's GPU; `labels` as there)."""
    params = occupancy_params(bounds, occ_size, 0.0)
    out = np.zeros((params.occ_h, params.occ_w), dtype=np.uint8)
    pp = None
    if pose is not None:
        pose_a, pp = _d(pose)
        if pose_a.size != 7:
            raise ValueError("a pose is (qx, qy, qz, qw, tx, ty, tz)")
    if _is_device_tensor(frame):
        f, stream = _device_rows(DeviceFrame, frame, labels, frame.device.index, _FRAME_WORDS)
        _check(lib().sageicp_occupancy_grid_device(C.byref(f), pp, C.byref(params), out.ctypes.data_as(C.c_void_p),
                                                   stream))
        return out
    if labels is not None:
        raise ValueError("labels= is for a frame that is a torch tensor on a GPU")
    pts, fp = _d(frame)
    _check(lib().sageicp_occupancy_grid(fp, pts.reshape(-1, 4).shape[0], pp, C.byref(params),
                                        out.ctypes.data_as(C.c_void_p), device))
    return out


def place_tables(params):
    """(edge2[R + 1], dir[S, 2]): the two host-made tables every decision of a place descriptor reads
    (sageicp_place_tables) — the squared ring edges and the sectors' directions (cos, sin)"""
    edge2 = np.empty(max(int(params.rings), 0) + 1)
    dirs = np.empty((max(int(params.sectors), 0), 2))
    _check(lib().sageicp_place_tables(C.byref(params), edge2.ctypes.data_as(_dp), dirs.ctypes.data_as(_dp)))
    return edge2, dirs


def place_prior(pose, shift, sectors):
    """(yaw, prior[7]) of a match at `shift` with an entry at `pose` (sageicp_place_prior; host code)"""
    pose_a, pp = _d(pose)
    if pose_a.size != 7:
        raise ValueError("a pose is (qx, qy, qz, qw, tx, ty, tz)")
    yaw, prior = C.c_double(0), np.empty(7)
    _check(lib().sageicp_place_prior(pp, int(shift), int(sectors), C.byref(yaw), prior.ctypes.data_as(_dp)))
    return yaw.value, prior


def _place_bytes(params, device=0, labels=None, frame=None):
    out = np.zeros(2 * max(int(params.rings), 0) * max(int(params.sectors), 0), dtype=np.uint8)
    if _is_device_tensor(frame):
        f, stream = _device_rows(DeviceFrame, frame, labels, frame.device.index, _FRAME_WORDS)
        _check(lib().sageicp_place_describe_device(C.byref(f), C.byref(params), out.ctypes.data_as(C.c_void_p), stream))
        return out
    if labels is not None:
        raise ValueError("labels= is for a frame that is a torch tensor on a GPU")
    pts, fp = _d(frame)
    _check(lib().sageicp_place_describe(fp, pts.reshape(-1, 4).shape[0], C.byref(params), out.ctypes.data_as(C.c_void_p),
                                        device))
    return out


def place_describe(frame, params, device=0, labels=None):
    """The place descriptor of a frame (sageicp_place_describe[_device]): (heights, classes), two (R, S) uint8 arrays —
    per cell of the polar grid the highest return as a byte (0: empty) and the class of highest rank.  `frame` is numpy
    (n, 4) rows (on GPU `device`) or a torch tensor on a GPU in the layouts RegisterFrame takes (`labels` as there)."""
    out = _place_bytes(params, device, labels, frame).reshape(2, params.rings, params.sectors)
    return out[0], out[1]


def _place_desc(desc, params):
    """a descriptor in any of its forms — (heights, classes), (2, R, S), flat bytes — as 2 * R * S contiguous bytes"""
    a = np.ascontiguousarray(np.stack(desc) if isinstance(desc, tuple) else desc, dtype=np.uint8).reshape(-1)
    if a.size != 2 * params.rings * params.sectors:
        raise ValueError("a descriptor of these params holds 2 * %d * %d bytes" % (params.rings, params.sectors))
    return a


def _place_match(handle, desc, query):
    out = np.zeros(16, dtype=PLACE_MATCH_DTYPE)
    n = C.c_uint32(0)
    _check(lib().sageicp_place_db_match(handle, desc.ctypes.data_as(C.c_void_p), C.byref(query),
                                        out.ctypes.data_as(C.c_void_p), C.byref(n)))
    return out[:n.value].copy()


class PlaceDB:
    """sageicp_place_db: place descriptors of one parameter set on GPU `device`, each with a tag and a pose, and the
    brute-force matcher over them.  PlaceDB(params) owns a new database; a pipeline's (SageICP.places()) is borrowed."""

    def __init__(self, params, device=0, _borrowed=None, _owner=None):
        self.params = params
        self._owner = _owner
        self._own = _borrowed is None
        self._h = _borrowed if _borrowed is not None else lib().sageicp_place_db_create(C.byref(params), device)
        if not self._h:
            raise SageIcpError(ERR_INVALID, (lib().sageicp_last_error() or b"").decode())

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_own", False) and lib is not None:
            lib().sageicp_place_db_destroy(self._h)
            self._h = None

    def __len__(self):
        return int(lib().sageicp_place_db_size(self._h))

    def clear(self):
        _check(lib().sageicp_place_db_clear(self._h))

    def add(self, desc, tag=0, pose=None):
        """appends a descriptor ((heights, classes), (2, R, S) or flat bytes); returns its index"""
        a = _place_desc(desc, self.params)
        pp = None
        if pose is not None:
            pose_a, pp = _d(pose)
            if pose_a.size != 7:
                raise ValueError("a pose is (qx, qy, qz, qw, tx, ty, tz)")
        idx = C.c_uint64(0)
        _check(lib().sageicp_place_db_add(self._h, a.ctypes.data_as(C.c_void_p), int(tag), pp, C.byref(idx)))
        return idx.value

    def match(self, desc, top_k=1, h_tol=0, exclude_last=0, min_similarity=0.0, query=None):
        """the best entries for `desc` as a numpy record array (PLACE_MATCH_DTYPE), best first (sageicp_place_db_match)"""
        q = query if query is not None else place_query(top_k, h_tol, exclude_last, min_similarity)
        return _place_match(self._h, _place_desc(desc, self.params), q)

    def read(self, first=0, count=None):
        """(descriptors (count, 2, R, S) uint8, tags (count,) uint64, poses (count, 7)) as they were added"""
        count = len(self) - first if count is None else count
        desc = np.zeros((max(count, 0), 2, self.params.rings, self.params.sectors), dtype=np.uint8)
        tags = np.zeros(max(count, 0), dtype=np.uint64)
        poses = np.zeros((max(count, 0), 7))
        _check(lib().sageicp_place_db_read(self._h, first, count, desc.ctypes.data_as(C.c_void_p),
                                           tags.ctypes.data_as(C.c_void_p), poses.ctypes.data_as(C.c_void_p)))
        return desc, tags, poses


def align_clouds(src, tgt, kernel, device=0):
    src, sp = _d(src)
    tgt, gp = _d(tgt)
    T = np.empty(7)
    JTJ = np.empty(36)
    JTr = np.empty(6)
    _check(lib().sageicp_align_clouds(sp, gp, src.reshape(-1, 4).shape[0], kernel,
                                      T.ctypes.data_as(_dp), JTJ.ctypes.data_as(_dp),
                                      JTr.ctypes.data_as(_dp), device))
    return T, JTJ.reshape(6, 6), JTr


class SageICP:
    """sage_icp::pipeline::sageICP (pipeline/sageICP.hpp:67-109) over the C ABI."""

    def __init__(self, config=None, **kw):
        self.config = config if config is not None else make_pipeline_config(**kw)
        self._h = lib().sageicp_pipeline_create(C.byref(self.config))
        if not self._h:
            raise SageIcpError(ERR_INVALID, (lib().sageicp_last_error() or b"").decode())
        self._deskew_on = False
        dyn = getattr(self.config, "_dynamic", None)
        if dyn and dyn["enable"]:
            self.set_dynamic_vehicle_filter(True, dyn["dy_th"], dyn["voxid"], dyn["landmarks"])
        if getattr(self.config, "_deskew", False):
            self.set_deskew(True)

    def set_deskew(self, enable=True):
        """sageConfig::deskew (sageicp_pipeline_set_deskew): RegisterFrame(frame, timestamps) deskews from the third
        pose on.  Drops a prepared or announced frame; prefetch() is refused while it is on."""
        _check(lib().sageicp_pipeline_set_deskew(self._h, 1 if enable else 0))
        self._deskew_on = bool(enable)
        if enable:
            self._announced = ()

    def deskew_info(self):
        """(applied, delta[6]): whether the last frame registered was deskewed, and the tangent it used (zeros if not)"""
        applied = C.c_int(0)
        delta = np.zeros(6)
        _check(lib().sageicp_pipeline_deskew_info(self._h, C.byref(applied), delta.ctypes.data_as(_dp)))
        return bool(applied.value), delta

    def set_dynamic_vehicle_filter(self, enable=True, dy_th=0.5, voxid=5, landmark_labels=(44, 48)):
        """Preprocess()'s dynamic vehicle filter for every frame (sageicp_pipeline_set_dynamic_vehicle_filter):
        dynamic labels = the config's label group `voxid`"""
        lm = (C.c_int * max(len(landmark_labels), 1))(*landmark_labels)
        _check(lib().sageicp_pipeline_set_dynamic_vehicle_filter(self._h, 1 if enable else 0, dy_th, voxid, lm,
                                                                 len(landmark_labels)))

    def set_quality(self, enable=True):
        """sageicp_pipeline_set_quality: every RegisterFrame evaluates the quality report of its source cloud at the new
        pose against the map before the update (quality()).  Off by default."""
        _check(lib().sageicp_pipeline_set_quality(self._h, 1 if enable else 0))

    def quality(self):
        """the last RegisterFrame's Quality (valid == 0: none — quality off, the first frame, an empty or failed call)"""
        q = Quality()
        _check(lib().sageicp_pipeline_quality(self._h, C.byref(q)))
        return q

    def set_key_frames(self, enable=True, bounds=KEY_FRAME_BOUNDS, occ_size=KEY_FRAME_OCC_SIZE, overlap=KEY_FRAME_OVERLAP):
        """Key-frame selection by occupancy overlap for every frame registered (sageicp_pipeline_set_key_frames; the
        odometry node's publish_key_frame block): bounds ((x_lo, x_hi), (y_lo, y_hi), (z_lo, z_hi)), occ_size (H, W),
        overlap the key_frame_overlap threshold — the launch files' values by default.  Starts from "no key frame";
        drops a prepared frame."""
        params = occupancy_params(bounds, occ_size, overlap) if enable else None
        _check(lib().sageicp_pipeline_set_key_frames(self._h, 1 if enable else 0,
                                                     C.byref(params) if params is not None else None))
        self._occ_size = (params.occ_h, params.occ_w) if enable else None
        self._place_params = None          # (a new selection starts with places off)

    def key_frame_info(self):
        """dict: enabled, is_key_frame (of the last frame), overlap (NaN on a first key frame or an empty key grid),
        key_frame_index (into poses()), key_frames (since set_key_frames / key_frame_reset), key_occupied, intersect,
        key_pose[7]"""
        info = KeyFrameInfo()
        _check(lib().sageicp_pipeline_key_frame_info(self._h, C.byref(info)))
        return info.as_dict()

    def key_frame_reset(self):
        """back to "no key frame" (reinitialize() keeps the key frame, as the node's ReinitService does)"""
        _check(lib().sageicp_pipeline_key_frame_reset(self._h))

    def key_frame_grid(self, device=False):
        """the key frame's grid, (H, W) uint8 (0 / 1; zeros while there is none): numpy, or with device=True a torch
        tensor on the pipeline's GPU"""
        h, w = getattr(self, "_occ_size", None) or (0, 0)
        if not device:
            out = np.zeros((h, w), dtype=np.uint8)
            _check(lib().sageicp_pipeline_key_frame_grid(self._h, out.ctypes.data_as(C.c_void_p), out.size))
            return out
        import torch
        _check_one_hip_runtime()
        dev = torch.device("cuda", self.config.device)
        out = torch.empty((h, w), dtype=torch.uint8, device=dev)
        stream = _current_stream(dev)
        _check(lib().sageicp_pipeline_key_frame_grid_device(self._h, out.data_ptr() or None, out.numel(), stream))
        return out

    def set_places(self, enable=True, params=None, top_k=1, h_tol=0, exclude_last=0, min_similarity=0.0, query=None):
        """Place recognition for every key frame (sageicp_pipeline_set_places): the raw frame described, matched against
        the places before it (place_info()), then added with tag = its index in poses() and its pose.  Needs key-frame
        selection on; starts from an empty database.  Off by default."""
        self._place_params = None
        if not enable:
            _check(lib().sageicp_pipeline_set_places(self._h, 0, None, None))
            return
        params = params if params is not None else place_params()
        q = query if query is not None else place_query(top_k, h_tol, exclude_last, min_similarity)
        _check(lib().sageicp_pipeline_set_places(self._h, 1, C.byref(params), C.byref(q)))
        self._place_params = params

    def place_info(self):
        """dict: enabled, described (the last frame registered was a key frame and was described), entries, matches (a
        numpy record array, PLACE_MATCH_DTYPE, best first)"""
        info = PlaceInfo()
        _check(lib().sageicp_pipeline_place_info(self._h, C.byref(info)))
        matches = np.frombuffer(bytes(info)[:16 * PLACE_MATCH_BYTES], dtype=PLACE_MATCH_DTYPE)[:info.n_matches].copy()
        return {"enabled": bool(info.enabled), "described": bool(info.described), "entries": int(info.entries),
                "matches": matches}

    def places(self):
        """the pipeline's place database (a borrowed PlaceDB: valid while places stay on), or None"""
        h = lib().sageicp_pipeline_place_db(self._h)
        params = getattr(self, "_place_params", None)
        return PlaceDB(params, _borrowed=h, _owner=self) if h and params is not None else None

    def place_reset(self):
        """empties the place database (key_frame_reset() does too; reinitialize() keeps it)"""
        _check(lib().sageicp_pipeline_place_reset(self._h))

    def dynamic_filter_info(self):
        """dict: what the filter did to the last frame registered (zeros when it was off)"""
        info = DynFilterInfo()
        _check(lib().sageicp_pipeline_dynamic_filter_info(self._h, C.byref(info)))
        return info.as_dict()

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:       # (None: interpreter shutdown)
            lib().sageicp_pipeline_destroy(self._h)
            self._h = None

    def RegisterFrame(self, frame, timestamps=None, labels=None):
        """returns (pose[7], icp_seconds, total_seconds, n_source, stats).  With `timestamps` (one per point, in [0, 1)
        for a scan — see normalize_timestamps) this is RegisterFrame(frame, timestamps), which deskews when deskew is
        on; without, the one-argument RegisterFrame(frame), which never does.
        `frame` may be a torch tensor on the pipeline's GPU (float32 / float64, stride(1) == 1, x y z in columns 0-2 and
        the label in column 3, or `labels`: a 1-D uint8 / int32 / int64 tensor on the same device, column 3 then
        ignored); `timestamps` are then a tensor on that device too.  The frame is read in the order of the device's
        current torch stream, and not any more once the call has returned.
        `frame` may also be a sensor_msgs/PointCloud2 (sage.PointCloud2, rclpy's, anything with their attributes): its
        fields are read by the reference's rules (pointcloud2_layout), the stamps exactly when deskew is on, and its
        data goes to the device as it is (host bytes) or is read in place (a uint8 tensor on the pipeline's GPU)."""
        if _is_message(frame):
            if timestamps is not None or labels is not None:
                raise ValueError("a PointCloud2 carries its own labels and stamps: timestamps= and labels= do not apply")
            return self._register_msg(frame)
        if _is_device_tensor(frame):
            return self._register_device(frame, timestamps, labels)
        if labels is not None:
            raise ValueError("labels= is for a frame that is a torch tensor on a GPU")
        pts, pp = _d(frame)
        n = pts.reshape(-1, 4).shape[0]
        out = np.empty(7)
        icp, tot, ns = C.c_double(0), C.c_double(0), C.c_uint64(0)
        st = Stats()
        if timestamps is None:
            _check(lib().sageicp_pipeline_register_frame(self._h, pp, n, out.ctypes.data_as(_dp), C.byref(icp),
                                                         C.byref(tot), C.byref(ns), C.byref(st)))
        else:
            ts, tp = _d(timestamps)
            if ts.size != n:
                raise ValueError("%d timestamps for %d points" % (ts.size, n))
            _check(lib().sageicp_pipeline_register_frame_timestamps(self._h, pp, tp, n, out.ctypes.data_as(_dp),
                                                                    C.byref(icp), C.byref(tot), C.byref(ns),
                                                                    C.byref(st)))
        return out, icp.value, tot.value, ns.value, st

    def _register_msg(self, msg):
        lay = pointcloud2_layout(msg, self._deskew_on)
        # (the reference's iterators ignore row_step; so does this)
        return self.RegisterFrameBytes(msg.data, int(msg.height) * int(msg.width), lay)

    def RegisterFrameBytes(self, data, n, layout):
        """RegisterFrame of n records described by a MsgLayout (sageicp_pipeline_register_frame_msg[_device]) — what
        RegisterFrame(msg) calls once the field-name rules have given the layout; `data` as PointCloud2.data"""
        lay = layout
        ptr, nbytes, keep, stream = _message_data(data, self.config.device)
        out = np.empty(7)
        icp, tot, ns = C.c_double(0), C.c_double(0), C.c_uint64(0)
        st = Stats()
        if stream is None:
            _check(lib().sageicp_pipeline_register_frame_msg(self._h, ptr, nbytes, n, C.byref(lay),
                                                             out.ctypes.data_as(_dp), C.byref(icp), C.byref(tot),
                                                             C.byref(ns), C.byref(st)))
        else:
            _check(lib().sageicp_pipeline_register_frame_msg_device(self._h, ptr, nbytes, n, C.byref(lay), stream,
                                                                    out.ctypes.data_as(_dp), C.byref(icp), C.byref(tot),
                                                                    C.byref(ns), C.byref(st)))
        del keep
        return out, icp.value, tot.value, ns.value, st

    def _register_device(self, frame, timestamps, labels):
        if timestamps is not None:
            if not _is_device_tensor(timestamps) or timestamps.device != frame.device:
                raise ValueError("timestamps of a device frame are a tensor on the same device")
            if str(timestamps.dtype) != "torch.float64" or timestamps.dim() != 1 or \
                    timestamps.shape[0] != frame.shape[0] or timestamps.stride(0) != 1:
                raise ValueError("timestamps: a contiguous 1-D float64 tensor of %d elements" % frame.shape[0])
        f, stream = _device_rows(DeviceFrame, frame, labels, self.config.device, _FRAME_WORDS)
        out = np.empty(7)
        icp, tot, ns = C.c_double(0), C.c_double(0), C.c_uint64(0)
        st = Stats()
        tp = (timestamps.data_ptr() or None) if timestamps is not None else None
        _check(lib().sageicp_pipeline_register_frame_device(self._h, C.byref(f), tp, stream, out.ctypes.data_as(_dp),
                                                            C.byref(icp), C.byref(tot), C.byref(ns), C.byref(st)))
        return out, icp.value, tot.value, ns.value, st

    def prefetch(self, next_frame):
        """Announce the frame after the next one registered: its Preprocess() + Voxelize() then run
        under that frame's ICP loop (sageicp_pipeline_prefetch).  Returns the array to pass to
        RegisterFrame() later (the same buffer: it is matched by address) — keep it alive."""
        pts, pp = _d(next_frame)
        # keep the buffer alive until it has been registered (the one announced before it may
        # still be waiting for its RegisterFrame)
        self._announced = (getattr(self, "_announced", ()) + ((pts, pp),))[-2:]
        _check(lib().sageicp_pipeline_prefetch(self._h, pp, pts.reshape(-1, 4).shape[0]))
        return pts

    def prefetch_wait(self):
        """wait for the helper thread; what it prepared is kept"""
        _check(lib().sageicp_pipeline_prefetch_wait(self._h))

    def prefetch_cancel(self):
        """drop an announced / prepared frame and wait for the helper thread"""
        _check(lib().sageicp_pipeline_prefetch_cancel(self._h))
        self._announced = ()

    def reinitialize(self):
        _check(lib().sageicp_pipeline_reinitialize(self._h))

    def poses(self):
        n = int(lib().sageicp_pipeline_num_poses(self._h))
        out = np.empty((n, 7))
        for i in range(n):
            _check(lib().sageicp_pipeline_pose(self._h, i, out[i].ctypes.data_as(_dp)))
        return out

    def LocalMap(self, device=False, dtype=None, out=None, labels_out=None):
        """LocalMap(): the map's rows on the host, numpy (n, 4) float64; the keywords as VoxelHashMap.Pointcloud (an
        out= shorter than local_map_size() gets its first len(out) rows)"""
        if not device and dtype is None and out is None and labels_out is None:
            h = lib().sageicp_pipeline_local_map(self._h)
            n = int(lib().sageicp_map_size(h))
            out = np.empty((n, 4))
            lib().sageicp_map_pointcloud(h, out.ctypes.data_as(_dp), n)
            return out
        return _map_rows(lambda: lib().sageicp_pipeline_local_map(self._h), self.config.device, device, dtype, out,
                         labels_out)

    def source(self, device=False, dtype=None, out=None, labels_out=None):
        """RegisterFrame's `source` (pipeline/sageICP.cpp:94): the cloud the last successful RegisterFrame registered,
        n_source rows; none before the first frame, after a failed call and after reinitialize().  Valid until the
        next RegisterFrame.  The order is the pipeline's: arrival order within each label group (a permutation of the
        reference's), the reference's under SAGEICP_SOURCE_REFERENCE_ORDER=1.  The keywords as
        VoxelHashMap.Pointcloud (an out= shorter than source_size() gets its first len(out) rows)."""
        return _rows_out(self.config.device, self.source_size, self._source_host,
                         lambda d, s, n: lib().sageicp_pipeline_source_device(self._h, d, s, n),
                         device, dtype, out, labels_out)

    def source_msg(self, colors, device=False, out=None):
        """source()'s rows, in its order, as the (n, 21) uint8 records the node publishes for the frame
        (sageicp_pipeline_source_msg[_device]); the arguments as VoxelHashMap.PointcloudMsg"""
        return _records_out(self.config.device, self.source_size,
                            lambda c, o, cap, n: lib().sageicp_pipeline_source_msg(self._h, c, o, cap, n),
                            lambda c, o, cap, s, n: lib().sageicp_pipeline_source_msg_device(self._h, c, o, cap, s, n),
                            colors, device, out)

    def LocalMapMsg(self, colors, device=False, out=None):
        """LocalMap()'s rows, in its order, as (n, 21) uint8 records; the arguments as VoxelHashMap.PointcloudMsg"""
        h = lambda: lib().sageicp_pipeline_local_map(self._h)
        return _records_out(self.config.device, self.local_map_size,
                            lambda c, o, cap, n: lib().sageicp_map_pointcloud_msg(h(), c, o, cap, n),
                            lambda c, o, cap, s, n: lib().sageicp_map_pointcloud_msg_device(h(), c, o, cap, s, n),
                            colors, device, out)

    def set_archive(self, enable=True, max_rows=0):
        """the local map's archive (VoxelHashMap.set_archive): keep what the per-frame update evicts"""
        _check(lib().sageicp_pipeline_set_archive(self._h, 1 if enable else 0, int(max_rows)))
        return self

    def archive_info(self):
        return _archive_info(lib().sageicp_pipeline_local_map(self._h))

    def Recall(self, center, radius, into=None):
        """VoxelHashMap.Recall on the pipeline's local map (sageicp_pipeline_recall): returns (into, info dict)"""
        c = self.config
        like = VoxelHashMap(c.voxel_size_map, float(radius), c.basic_points_per_voxel, c.critical_points_per_voxel,
                            [c.basic_parts_labels[i] for i in range(c.n_basic_parts_labels)], device=c.device, _handle=0)
        return _recall(lib().sageicp_pipeline_recall, self._h, like, center, radius, into)

    def archive_voxels(self):
        return _archive_voxels(lib().sageicp_pipeline_local_map(self._h))

    def SessionMap(self, which="session", first=0, device=False, dtype=None, out=None, labels_out=None):
        """The map of what the session drove through: the latest generation of every evicted voxel the local map does
        not hold, then LocalMap() (VoxelHashMap.ArchivedPointcloud; which= "all" / "latest" give the log alone)"""
        return _archive_rows(lambda: lib().sageicp_pipeline_local_map(self._h), self.config.device, which, first, device, dtype,
                             out, labels_out)

    def Closure(self, i, closed):
        """A loop closure between pose i and the last pose: `closed` is where the last pose really is in pose i's frame
        of the world (what Relocalize returns against a map recalled around pose i).  Returns (corrections (n, 7),
        corrected poses (n, 7), info dict) — info["delta"] is the map->odom transform (sageicp_pipeline_closure).  The
        pipeline itself is not touched.  Needs the archive on from the first frame."""
        n = int(lib().sageicp_pipeline_num_poses(self._h))
        corr, poses, info = np.empty((n, 7)), np.empty((n, 7)), ClosureInfo()
        c = np.ascontiguousarray(closed, dtype=np.float64).reshape(-1)
        if c.size != 7:
            raise ValueError("Closure takes closed[7]")
        _check(lib().sageicp_pipeline_closure(self._h, int(i), _p(c), _p(corr), _p(poses), C.byref(info)))
        return corr, poses, info.as_dict()

    def OptimizeGraph(self, closures, odom_info, anchor=0, max_iterations=None, max_halvings=None, step_tol=None, where="auto",
                      robust=None):
        """The pipeline's poses optimised under all `closures` at once (graph_edge() records; sageicp_pipeline_graph_optimize,
        DESIGN.md D19).  Returns (corrections (n, 7), corrected poses (n, 7), info dict), as Closure does; the corrections go
        into CorrectedSessionMap.  The pipeline itself is not touched.  robust: as graph_optimize's."""
        n = int(lib().sageicp_pipeline_num_poses(self._h))
        corr, poses, info = np.empty((n, 7)), np.empty((n, 7)), GraphInfo()
        arr, c = _graph_edges(closures)
        O, stride = _graph_odom_info(odom_info, n)
        prm = _graph_params(anchor, max_iterations, max_halvings, step_tol, where)
        if robust is None:
            _check(lib().sageicp_pipeline_graph_optimize(self._h, _p(O), stride, arr, c, C.byref(prm), _p(corr), _p(poses), C.byref(info)))
            return corr, poses, info.as_dict()
        rb, chi2, weight, ri = _graph_robust(robust), np.empty(c), np.empty(c), GraphRobustInfo()
        _check(lib().sageicp_pipeline_graph_optimize_robust(self._h, _p(O), stride, arr, c, C.byref(prm), _p(corr), _p(poses), C.byref(info),
                                                            C.byref(rb), _p(chi2), _p(weight), C.byref(ri)))
        return corr, poses, _graph_robust_dict(info, chi2, weight, ri)

    def CorrectedSessionMap(self, corrections, which="session", first=0, device=False, dtype=None, out=None, labels_out=None):
        """SessionMap(which)'s rows re-posed by `corrections` (n, 7), one per pose of the pipeline, as Closure returns
        them (sageicp_pipeline_session_corrected[_device]; VoxelHashMap.CorrectedPointcloud)"""
        corr = np.ascontiguousarray(corrections, dtype=np.float64)
        if corr.ndim != 2 or corr.shape[1] != 7:
            raise ValueError("corrections is (n, 7)")
        w, first, n = _archive_which(which), int(first), corr.shape[0]
        handle = lambda: lib().sageicp_pipeline_local_map(self._h)
        return _corrected_rows(handle, self.config.device, w, first, device, dtype, out, labels_out,
                               lambda a, cap, k: lib().sageicp_pipeline_session_corrected(self._h, w, first, _p(corr), n, a, cap, k),
                               lambda d, st, k: lib().sageicp_pipeline_session_corrected_device(self._h, w, first, _p(corr), n, d, st, k))

    def RebuildSessionMap(self, corrections, which="session", center=None, radius=math.inf, into=None):
        """CorrectedSessionMap(corrections, which)'s rows voxelised again into the map `into` (None: a new map with the
        local map's parameters): VoxelHashMap.RebuildSession with the pipeline's positions
        (sageicp_pipeline_session_rebuild).  Returns (into, info dict).  The pipeline itself is not touched."""
        corr = np.ascontiguousarray(corrections, dtype=np.float64)
        if corr.ndim != 2 or corr.shape[1] != 7:
            raise ValueError("corrections is (n, 7)")
        w, n, c = _archive_which(which), corr.shape[0], self.config
        like = VoxelHashMap(c.voxel_size_map, c.local_map_range, c.basic_points_per_voxel, c.critical_points_per_voxel,
                            [c.basic_parts_labels[i] for i in range(c.n_basic_parts_labels)], device=c.device, _handle=0)
        return _rebuild(lambda ctr, r, h, i: lib().sageicp_pipeline_session_rebuild(self._h, w, _p(corr), n, ctr, r, h, i),
                        like, center, radius, into)

    def SessionMapMsg(self, colors, which="session", first=0, device=False, out=None):
        return _archive_msg(lambda: lib().sageicp_pipeline_local_map(self._h), self.config.device, colors, which, first, device,
                            out)

    def source_size(self):
        """rows of source(): n_source of the last successful RegisterFrame, 0 if there is none"""
        n = C.c_uint64(0)
        _check(lib().sageicp_pipeline_source(self._h, None, 0, C.byref(n)))
        return n.value

    def local_map_size(self):
        """rows of LocalMap()"""
        return int(lib().sageicp_map_size(lib().sageicp_pipeline_local_map(self._h)))

    def _source_host(self, n):
        a = np.empty((n, 4))
        k = C.c_uint64(0)
        _check(lib().sageicp_pipeline_source(self._h, a.ctypes.data_as(_dp), n, C.byref(k)))
        return a


def _recall(entry, handle, like, center, radius, into):
    """`like`: the VoxelHashMap (or its parameters) a fresh destination is created from"""
    c = np.ascontiguousarray(center, dtype=np.float64).reshape(-1)
    if c.size != 3:
        raise ValueError("Recall takes a centre[3]")
    if into is None:
        into = VoxelHashMap(like.voxel_size_, float(radius), like.basic_points_per_voxel_, like.critical_points_per_voxel_,
                            like.basic_parts_labels_, device=like.device)
    info = RecallInfo()
    _check(entry(handle, c.ctypes.data_as(_dp), float(radius), into._h, C.byref(info)))
    return into, info.as_dict()


def _rebuild(entry, like, center, radius, into):
    """`like`: the VoxelHashMap (or its parameters) a fresh destination is created from; entry(center, radius, dst, info)"""
    c = None
    if center is not None:
        c = np.ascontiguousarray(center, dtype=np.float64).reshape(-1)
        if c.size != 3:
            raise ValueError("RebuildSession takes a centre[3]")
    if into is None:
        into = VoxelHashMap(like.voxel_size_, like.max_distance_, like.basic_points_per_voxel_, like.critical_points_per_voxel_,
                            like.basic_parts_labels_, device=like.device)
    info = RebuildInfo()
    _check(entry(c.ctypes.data_as(_dp) if c is not None else None, float(radius), into._h, C.byref(info)))
    return into, info.as_dict()


def _archive_info(h):
    i = ArchiveInfo()
    _check(lib().sageicp_map_archive_info(h, C.byref(i)))
    return i.as_dict()


def _archive_voxels(h):
    n = C.c_uint64(0)
    _check(lib().sageicp_map_archive_voxels(h, 0, None, 0, C.byref(n)))
    a = np.zeros(n.value, dtype=ARCHIVE_VOXEL_DTYPE)
    if n.value:
        _check(lib().sageicp_map_archive_voxels(h, 0, a.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    return a.view(np.recarray)


def _archive_which(which):
    return ARCHIVE_WHICH[which] if isinstance(which, str) else int(which)


def _archive_room(handle, w, first):
    """rows to make room for: what selection w has from row `first` on ("all"), or an upper bound of it that costs no
    device work ("latest": every archived row; "session": those and the map's) — the selection itself is then computed
    once, by the call that writes the rows, and the result trimmed to what it reported"""
    i = _archive_info(handle())
    n = i["rows"] + (int(lib().sageicp_map_size(handle())) if w == SESSION else 0)
    return max(0, n - first)


def _archive_rows(handle, device_index, which, first, device, dtype, out, labels_out):
    w, first = _archive_which(which), int(first)

    def host_rows(n):
        a = np.empty((n, 4))
        k = C.c_uint64(0)
        _check(lib().sageicp_map_archive_rows(handle(), w, first, a.ctypes.data_as(_dp) if n else None, n, C.byref(k)))
        return a[:min(max(0, k.value - first), n)]

    return _rows_out(device_index, lambda: _archive_room(handle, w, first), host_rows,
                     lambda d, s, n: lib().sageicp_map_archive_rows_device(handle(), w, first, d, s, n),
                     device, dtype, out, labels_out, first=first)


def _p(a):
    """the address of a C-contiguous float64 array (the caller keeps it alive)"""
    return a.ctypes.data_as(_dp)


def _positions(positions):
    pos = np.ascontiguousarray(positions, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
        raise ValueError("positions is (n, 3), n >= 1")
    return pos


def _corrections(corrections, positions):
    corr = np.ascontiguousarray(corrections, dtype=np.float64)
    if corr.ndim != 2 or corr.shape[1] != 7 or corr.shape[0] != len(positions):
        raise ValueError("corrections is (n, 7), one per position")
    return corr


def _corrected_rows(handle, device_index, w, first, device, dtype, out, labels_out, host_call, device_call):
    """the re-posed export of a selection: host_call(rows, cap, n_out) / device_call(DevicePoints, stream, n_out)"""
    def host_rows(n):
        a = np.empty((n, 4))
        k = C.c_uint64(0)
        _check(host_call(a.ctypes.data_as(_dp) if n else None, n, C.byref(k)))
        return a[:min(max(0, k.value - first), n)]

    return _rows_out(device_index, lambda: _archive_room(handle, w, first), host_rows, device_call, device, dtype, out, labels_out,
                     first=first)


def closure_corrections(poses, i, j, closed, return_info=False):
    """The corrections C_k (n, 7) that spread the closure "pose j really is at `closed`, in pose i's frame of the world"
    over poses i..j by path length, and the corrected poses C_k * poses[k] (sageicp_closure_corrections).
    Host arithmetic, no device.  return_info=True adds the info dict (delta, angle, shift, path, i, j)."""
    P = np.ascontiguousarray(poses, dtype=np.float64)
    c = np.ascontiguousarray(closed, dtype=np.float64).reshape(-1)
    if P.ndim != 2 or P.shape[1] != 7 or c.size != 7:
        raise ValueError("closure_corrections takes poses (n, 7) and closed[7]")
    corr, out, info = np.empty_like(P), np.empty_like(P), ClosureInfo()
    _check(lib().sageicp_closure_corrections(_p(P), P.shape[0], int(i), int(j), _p(c), _p(corr), _p(out), C.byref(info)))
    return (corr, out, info.as_dict()) if return_info else (corr, out)


def _graph_edges(closures):
    closures = list(closures) if closures is not None else []
    arr = (GraphEdge * max(1, len(closures)))()
    for k, e in enumerate(closures):
        if not isinstance(e, GraphEdge):
            raise ValueError("closures are GraphEdge records (graph_edge())")
        arr[k] = e
    return arr, len(closures)


def _graph_odom_info(odom_info, n):
    """(array, stride): one 6x6 for all odometry edges, or (n - 1, 6, 6) / (n - 1, 36), one per edge"""
    O = np.ascontiguousarray(odom_info, dtype=np.float64)
    if O.size == 36:
        return O.reshape(36), 0
    if n >= 2 and O.size == 36 * (n - 1):
        return O.reshape(-1), 36
    raise ValueError("odom_info is one 6x6, or one per odometry edge (n - 1 of them)")


def _graph_params(anchor, max_iterations, max_halvings, step_tol, where):
    prm = GraphParams()
    lib().sageicp_graph_params_default(C.byref(prm))
    prm.anchor = int(anchor)
    if max_iterations is not None:
        prm.max_iterations = int(max_iterations)
    if max_halvings is not None:
        prm.max_halvings = int(max_halvings)
    if step_tol is not None:
        prm.step_tol = float(step_tol)
    prm.where = GRAPH_WHERE[where] if isinstance(where, str) else int(where)
    return prm


def _graph_robust(robust):
    """sageicp_graph_robust from a dict or a tuple (kernel, scale, anneal, anneal_factor, stage_iterations); absent: the defaults"""
    names = ("kernel", "scale", "anneal", "anneal_factor", "stage_iterations")
    if isinstance(robust, str):
        robust = dict(kernel=robust)
    elif not isinstance(robust, dict):
        robust = dict(zip(names, tuple(robust)))
    unknown = set(robust) - set(names)
    if unknown or "kernel" not in robust:
        raise ValueError("robust takes kernel, scale, anneal, anneal_factor, stage_iterations")
    rb = GraphRobust()
    lib().sageicp_graph_robust_default(C.byref(rb))
    k = robust["kernel"]
    if isinstance(k, str) and k not in GRAPH_KERNEL:
        raise ValueError('robust kernel is "huber", "cauchy" or "gm"')
    rb.kernel = GRAPH_KERNEL[k] if isinstance(k, str) else int(k)
    if robust.get("scale") is not None:
        rb.scale = float(robust["scale"])
    if robust.get("anneal") is not None:
        rb.anneal = int(robust["anneal"])
    if robust.get("anneal_factor") is not None:
        rb.anneal_factor = float(robust["anneal_factor"])
    if robust.get("stage_iterations") is not None:
        rb.stage_iterations = int(robust["stage_iterations"])
    return rb


def _graph_robust_dict(info, chi2, weight, ri):
    d = info.as_dict()
    d.update(closure_chi2=chi2, closure_weight=weight, stages=int(ri.stages), outliers=int(ri.outliers), scale2_first=ri.scale2_first)
    return d


def graph_edge_info(quality, closed, gain=1.0):
    """The 6x6 information of the closure edge graph_edge() makes of `closed`, from the Quality report at `closed` (what
    Relocalize returns): gain * Ad(closed)^T (JTJ / s2) Ad(closed), symmetric to the bit (sageicp_graph_info_from_quality;
    DESIGN.md D20).  gain is the caller's noise model: ICP covariances are overconfident."""
    if not isinstance(quality, Quality):
        raise ValueError("graph_edge_info takes the Quality record of Relocalize / registration_quality")
    c = np.ascontiguousarray(closed, dtype=np.float64).reshape(-1)
    if c.size != 7:
        raise ValueError("closed is (qx, qy, qz, qw, tx, ty, tz)")
    out = np.empty((6, 6))
    _check(lib().sageicp_graph_info_from_quality(C.byref(quality), _p(c), float(gain), _p(out)))
    return out


def graph_edge(poses, i, j, closed, info):
    """The closure edge of "pose j really is at `closed`, in pose i's frame of the world" (closure_corrections' argument):
    a GraphEdge with a = i, b = j, z = poses[i]^-1 * closed and the 6x6 information `info` (sageicp_graph_edge_from_closed)"""
    P = np.ascontiguousarray(poses, dtype=np.float64)
    c = np.ascontiguousarray(closed, dtype=np.float64).reshape(-1)
    O = np.ascontiguousarray(info, dtype=np.float64).reshape(-1)
    if P.ndim != 2 or P.shape[1] != 7 or c.size != 7 or O.size != 36:
        raise ValueError("graph_edge takes poses (n, 7), closed[7] and info 6x6")
    e = GraphEdge()
    _check(lib().sageicp_graph_edge_from_closed(_p(P), P.shape[0], int(i), int(j), _p(c), _p(O), C.byref(e)))
    return e


def graph_cost(poses, closures, odom_info, at=None, per_edge=False):
    """F(at) of the pose graph of `poses` and `closures` (at=None: at poses), host fp64 (sageicp_graph_cost);
    per_edge=True adds each edge's term, odometry edges first"""
    P = np.ascontiguousarray(poses, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 7:
        raise ValueError("graph_cost takes poses (n, 7)")
    A = P if at is None else np.ascontiguousarray(at, dtype=np.float64)
    if A.shape != P.shape:
        raise ValueError("at has the shape of poses")
    arr, c = _graph_edges(closures)
    O, stride = _graph_odom_info(odom_info, P.shape[0])
    cost, pe = C.c_double(0.0), np.empty(max(0, P.shape[0] - 1) + c)
    _check(lib().sageicp_graph_cost(_p(P), P.shape[0], _p(O), stride, arr, c, _p(A), C.byref(cost), _p(pe)))
    return (cost.value, pe) if per_edge else cost.value


def graph_optimize(poses, closures, odom_info, initial=None, anchor=0, max_iterations=None, max_halvings=None, step_tol=None,
                   where="auto", return_info=False, robust=None):
    """`poses` (n, 7) optimised under its own odometry (information `odom_info`) and all `closures` (graph_edge()) at once:
    Gauss-Newton on SE(3) with exact Jacobians, pose `anchor` fixed (sageicp_graph_optimize).  Returns
    (corrections (n, 7), optimised poses (n, 7)); the corrections are closure_corrections' kind.  where: "auto", "host" or
    "device".  return_info=True adds the info dict (cost_initial, cost_final, grad_max, step_last, max_shift, iterations,
    halvings, status, where).  robust: a robust kernel on the closures (sageicp_graph_optimize_robust), a
    dict or tuple of kernel="huber"|"cauchy"|"gm", scale, anneal, anneal_factor, stage_iterations; the info dict then gains
    closure_chi2, closure_weight (below 0.5: drop the match), stages, outliers and scale2_first."""
    P = np.ascontiguousarray(poses, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != 7:
        raise ValueError("graph_optimize takes poses (n, 7)")
    X0 = None if initial is None else np.ascontiguousarray(initial, dtype=np.float64)
    if X0 is not None and X0.shape != P.shape:
        raise ValueError("initial has the shape of poses")
    arr, c = _graph_edges(closures)
    O, stride = _graph_odom_info(odom_info, P.shape[0])
    prm = _graph_params(anchor, max_iterations, max_halvings, step_tol, where)
    corr, out, info = np.empty_like(P), np.empty_like(P), GraphInfo()
    if robust is not None:
        rb, chi2, weight, ri = _graph_robust(robust), np.empty(c), np.empty(c), GraphRobustInfo()
        _check(lib().sageicp_graph_optimize_robust(_p(P), P.shape[0], _p(O), stride, arr, c, None if X0 is None else _p(X0), C.byref(prm),
                                                   _p(out), _p(corr), C.byref(info), C.byref(rb), _p(chi2), _p(weight), C.byref(ri)))
        return (corr, out, _graph_robust_dict(info, chi2, weight, ri)) if return_info else (corr, out)
    _check(lib().sageicp_graph_optimize(_p(P), P.shape[0], _p(O), stride, arr, c, None if X0 is None else _p(X0), C.byref(prm),
                                        _p(out), _p(corr), C.byref(info)))
    return (corr, out, info.as_dict()) if return_info else (corr, out)


def _archive_msg(handle, device_index, colors, which, first, device, out):
    w, first = _archive_which(which), int(first)
    return _records_out(device_index, lambda: _archive_room(handle, w, first),
                        lambda c, o, cap, n: lib().sageicp_map_archive_msg(handle(), w, first, c, o, cap, n),
                        lambda c, o, cap, s, n: lib().sageicp_map_archive_msg_device(handle(), w, first, c, o, cap, s, n),
                        colors, device, out, first=first)


def _map_rows(handle, device_index, device, dtype, out, labels_out):
    """the map's rows on the device (VoxelHashMap.Pointcloud, SageICP.LocalMap); handle() gives the map's handle"""
    return _rows_out(device_index, lambda: int(lib().sageicp_map_size(handle())), None,
                     lambda d, s, n: lib().sageicp_map_pointcloud_device(handle(), d, s, n), device, dtype, out,
                     labels_out)


def preprocess(frame, max_range, min_range, label_max_range, device=0, dynamic_vehicle_filter=False, dy_th=0.5,
               dynamic_labels=(), landmark_labels=(44, 48), return_info=False):
    """sage_icp::Preprocess (core/Preprocessing.cpp:86-187); with dynamic_vehicle_filter the PCL clustering branch
    (:95-172, sageicp_preprocess_dynamic).  return_info: also the filter's DynFilterInfo as a dict."""
    pts, pp = _d(frame)
    n = pts.reshape(-1, 4).shape[0]
    out = np.empty((n, 4))
    k = C.c_uint64(0)
    info = DynFilterInfo()
    if dynamic_vehicle_filter:
        dl = (C.c_int * max(len(dynamic_labels), 1))(*dynamic_labels)
        ll = (C.c_int * max(len(landmark_labels), 1))(*landmark_labels)
        _check(lib().sageicp_preprocess_dynamic(pp, n, max_range, min_range, label_max_range, dy_th, dl,
                                                len(dynamic_labels), ll, len(landmark_labels),
                                                out.ctypes.data_as(_dp), C.byref(k), C.byref(info), device))
    else:
        _check(lib().sageicp_preprocess(pp, n, max_range, min_range, label_max_range,
                                        out.ctypes.data_as(_dp), C.byref(k), device))
    res = out[:k.value].copy()
    return (res, info.as_dict()) if return_info else res


def deskew_scan(frame, timestamps, start_pose, finish_pose, device=0):
    """sage_icp::DeSkewScan (core/Deskew.cpp:31-50) on the device: every point moved by exp((t - 0.5) * delta),
    delta = (start.inverse() * finish).log(); labels and row order kept"""
    pts, pp = _d(frame)
    n = pts.reshape(-1, 4).shape[0]
    ts, tp = _d(timestamps)
    if ts.size != n:
        raise ValueError("%d timestamps for %d points" % (ts.size, n))
    a, ap = _d(start_pose)
    b, bp = _d(finish_pose)
    if a.size != 7 or b.size != 7:
        raise ValueError("poses are (qx, qy, qz, qw, tx, ty, tz)")
    out = np.empty((n, 4))
    _check(lib().sageicp_deskew_scan(pp, tp, n, ap, bp, out.ctypes.data_as(_dp), device))
    return out


def normalize_timestamps(timestamps):
    """NormalizeTimestamps (ros/ros2/Utils.hpp:68-77): the stamps unchanged if their maximum is below 1, else divided
    by it — for integer per-point stamps (the reference's node does this before RegisterFrame(frame, timestamps))"""
    t = np.asarray(timestamps, dtype=np.float64)
    if t.size == 0:
        return t.copy()
    m = t.max()
    return t.copy() if m < 1.0 else t / m


def cluster_emission_order(sizes):
    """sageicp_cluster_emission_order: PCL's cluster order (std::sort(rbegin, rend) by size) for clusters found with
    these sizes; element j = index of the j-th cluster emitted"""
    s = np.ascontiguousarray(sizes, dtype=np.uint32)
    out = np.zeros(max(len(s), 1), dtype=np.uint32)
    _check(lib().sageicp_cluster_emission_order(s.ctypes.data_as(C.c_void_p), len(s), out.ctypes.data_as(C.c_void_p)))
    return out[:len(s)].copy()


def voxel_downsample(frame, voxel_labels, voxel_size, vox_scale, device=0):
    """sage_icp::VoxelDownsample (core/Preprocessing.cpp:44-84)"""
    pts, pp = _d(frame)
    n = pts.reshape(-1, 4).shape[0]
    counts = (C.c_int * len(voxel_labels))(*[len(g) for g in voxel_labels])
    flat = [l for g in voxel_labels for l in g]
    labels = (C.c_int * max(len(flat), 1))(*flat)
    sizes = (C.c_double * len(voxel_size))(*voxel_size)
    out = np.empty((n, 4))
    k = C.c_uint64(0)
    _check(lib().sageicp_voxel_downsample(pp, n, len(voxel_labels), counts, labels, sizes, vox_scale,
                                          out.ctypes.data_as(_dp), C.byref(k), device))
    return out[:k.value].copy()


def _poses44(p):
    a = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 4, 4)
    return a, a.ctypes.data_as(_dp)


def seq_error(poses_gt, poses_result):
    """sage_icp::metrics::SeqError (metrics/Metrics.cpp:140-155): (avg translation error %,
    avg rotation error deg/100 m) over the KITTI devkit segments; poses are (n, 4, 4)"""
    g, gp = _poses44(poses_gt)
    r, rp = _poses44(poses_result)
    assert g.shape == r.shape
    t, o = C.c_float(0), C.c_float(0)
    _check(lib().sageicp_metrics_seq_error(gp, rp, g.shape[0], C.byref(t), C.byref(o)))
    return t.value, o.value


def absolute_trajectory_error(poses_gt, poses_result):
    """sage_icp::metrics::AbsoluteTrajectoryError (metrics/Metrics.cpp:157-191): (ATE rotation
    [rad], ATE translation [m]) after a rigid Umeyama alignment; poses are (n, 4, 4)"""
    g, gp = _poses44(poses_gt)
    r, rp = _poses44(poses_result)
    assert g.shape == r.shape
    a, b = C.c_float(0), C.c_float(0)
    _check(lib().sageicp_metrics_absolute_trajectory_error(gp, rp, g.shape[0], C.byref(a), C.byref(b)))
    return a.value, b.value
