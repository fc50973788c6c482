"""The session rebuild restated (include/sageicp.h "session rebuild"), for the tests only: the selection, the
stays and the move of tests/closureref.py, then tests/mapref.py's sequential add_points into a fresh map and, with a
centre, its remove_far at max_distance = radius.  Nothing of the closed form is in here."""
import math

import numpy as np

import closureref
import mapref

INFO_FIELDS = ("voxels", "rows", "session_voxels", "session_rows", "built_voxels", "built_rows", "cropped_voxels", "cropped_rows")


def moved_rows(m, which, positions, corrections, voxel_size):
    """the rows sageicp_map_session_corrected(m, which, 0, ..) returns, and the voxels of the selection"""
    rows, counts, updates = closureref.session_voxels(m, which, voxel_size)
    stay = closureref.stays(closureref.first_rows(rows, counts), updates, positions, m.max_distance_)
    return closureref.move(rows, counts, stay, corrections), len(counts)


def rebuild_rows(moved, params, center=None, radius=math.inf, session_voxels=None):
    """(Pointcloud() of the rebuilt map, its info dict) from the moved rows; params: voxel_size, basic, critical, basic_labels"""
    ref = mapref.MapRef(params["voxel_size"], radius if center is not None else 1.0, params["basic"], params["critical"],
                        params["basic_labels"])
    ref.add_points(np.asarray(moved, dtype=np.float64).reshape(-1, 4))
    built = (ref.num_voxels(), ref.size())
    if center is not None:
        ref.remove_far(center)
    cloud = ref.pointcloud()
    info = dict(voxels=ref.num_voxels(), rows=ref.size(), session_rows=len(moved), built_voxels=built[0], built_rows=built[1],
                cropped_voxels=built[0] - ref.num_voxels(), cropped_rows=built[1] - ref.size())
    if session_voxels is not None:
        info["session_voxels"] = session_voxels
    return cloud, info


def rebuild(m, which, positions, corrections, params, center=None, radius=math.inf):
    moved, voxels = moved_rows(m, which, positions, corrections, params["voxel_size"])
    return rebuild_rows(moved, params, center, radius, session_voxels=voxels)
