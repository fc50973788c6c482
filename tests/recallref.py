"""Plain Python restatement of recall (include/sageicp.h "recall"), for the tests only, written from the
definition:

  * the session's voxels are the groups of consecutive SESSION rows that share a voxel key (every key appears once there,
    with all its rows together: the LATEST records in log order, then Pointcloud());
  * a voxel is kept iff its FIRST row is not far from the centre — mapref.MapRef.remove_far's expression, with the
    association SQNORM3_ORDER selects, against radius * radius formed once;
  * what lands in the destination is the kept groups concatenated, in session order."""
import numpy as np

import archiveref
import mapref


def groups(session_rows, voxel_size):
    """[(key, rows)] of consecutive rows with one voxel key"""
    rows = np.asarray(session_rows, dtype=np.float64).reshape(-1, 4)
    out = []
    for key, p in zip(archiveref.keys_of(rows, voxel_size), rows):
        if out and out[-1][0] == key:
            out[-1][1].append(p)
        else:
            out.append((key, [p]))
    return out


def is_far(p, center, radius):
    cx, cy, cz = (float(v) for v in center)
    dx, dy, dz = float(p[0]) - cx, float(p[1]) - cy, float(p[2]) - cz
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    d2 = xx + (yy + zz) if mapref.SQNORM3_ORDER == 0 else (xx + yy) + zz
    return d2 > float(radius) * float(radius)


def recall(session_rows, voxel_size, center, radius):
    """(rows the destination's Pointcloud() must equal, number of kept voxels)"""
    kept = [g for g in groups(session_rows, voxel_size) if not is_far(g[1][0], center, radius)]
    rows = [p for _, g in kept for p in g]
    return np.array(rows, dtype=np.float64).reshape(-1, 4), len(kept)


def info(session_rows, n_archive_rows, voxel_size, center, radius):
    """sageicp_recall_info from the SESSION rows, the first n_archive_rows of which are the LATEST part"""
    rows = np.asarray(session_rows, dtype=np.float64).reshape(-1, 4)
    parts = (rows[:n_archive_rows], rows[n_archive_rows:])
    kept = [recall(p, voxel_size, center, radius) for p in parts]
    return {"voxels": kept[0][1] + kept[1][1], "rows": len(kept[0][0]) + len(kept[1][0]),
            "archive_voxels": kept[0][1], "archive_rows": len(kept[0][0]),
            "map_voxels": kept[1][1], "map_rows": len(kept[1][0]),
            "session_voxels": len(groups(parts[0], voxel_size)) + len(groups(parts[1], voxel_size)),
            "session_rows": len(rows)}
