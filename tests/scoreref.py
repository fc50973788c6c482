"""The batch score of candidate poses and Relocalize (sageicp_score_poses, sageicp_relocalize*, include/sageicp.h; DESIGN.md
D14) restated in plain numpy: what tests/test_score_poses_host.py and tests/test_score_poses_gpu.py compare with.

  candidates(prior, xy, z, yaw)   the candidate grid of sageicp_relocalize_candidates, operation for operation (math.sin
                                  and math.cos are libm's, as the library's)
  score(map, rows, poses, ...)    every candidate's sum_w and n_pairs in fp64 over the ORACLE's pairs of the moved rows
  the scene                       a frame whose prior lies outside the basin of the ICP: the map, the scan, T_GT, the grid
"""
import math

import numpy as np

# ---- the scene ----------------------------------------------------------------------------------------------------------
MAP_SEED, MAP_POINTS, HALF, VOXEL = 0xC1, 35000, 60.0, 0.8
SCAN_SEED, SCAN_POINTS = 5, 2000
MD, KERNEL, TH = 6.0, 2.0 / 3.0, 0.4           # the cold parameters: 3 sigma, sigma / 3 of the initial threshold 2.0
PRIOR = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
GRID = dict(xy=(6.0, 2.0), z=(0.0, 0.0), yaw=(math.radians(30.0), math.radians(5.0)))
GRID_CANDIDATES = 13 * 7 * 7


def t_gt():
    from sage_icp_amd import synthetic as syn
    return syn.pose_from_rpy_t([0.0, 0.0, 25.0], [4.0, -3.0, 0.0])


def map_points():
    from sage_icp_amd import synthetic as syn
    return syn.sample_surfaces(np.random.default_rng(MAP_SEED), MAP_POINTS, HALF)


def scan():
    from sage_icp_amd import synthetic as syn
    return syn.make_scan(np.random.default_rng(SCAN_SEED), SCAN_POINTS, HALF, t_gt())


def pose_error(a, b):
    """(metres, radians) between two poses (qx, qy, qz, qw, tx, ty, tz)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = abs(float(np.dot(a[:4], b[:4]))) / (np.linalg.norm(a[:4]) * np.linalg.norm(b[:4]))
    return float(np.linalg.norm(a[4:] - b[4:])), 2.0 * math.acos(min(1.0, d))


# ---- the candidate grid ---------------------------------------------------------------------------------------------------
def axis_steps(extent, step):
    """the largest integer m >= 0 with m * step <= extent in fp64; 0 when step <= 0 or extent < step"""
    if not step > 0.0 or extent < step:
        return 0
    m = int(extent / step)
    while (m + 1) * step <= extent:
        m += 1
    while m > 0 and m * step > extent:
        m -= 1
    return m


def candidates(prior, xy=(0.0, 0.0), z=(0.0, 0.0), yaw=(0.0, 0.0)):
    """(K, 7): yaw outermost, then x, then y, z innermost, each index ascending from -m to +m"""
    prior = [float(v) for v in prior]
    my, mx, mz = axis_steps(*yaw), axis_steps(*xy), axis_steps(*z)
    out = []
    for a in range(-my, my + 1):
        q = prior[:4]
        if a:
            th = float(a) * yaw[1]
            s, c = math.sin(th / 2.0), math.cos(th / 2.0)
            q = [c * prior[0] - s * prior[1], c * prior[1] + s * prior[0], c * prior[2] + s * prior[3],
                 c * prior[3] - s * prior[2]]
        for i in range(-mx, mx + 1):
            for j in range(-mx, mx + 1):
                for l in range(-mz, mz + 1):
                    out.append(q + [prior[4] + float(i) * xy[1] if i else prior[4],
                                    prior[5] + float(j) * xy[1] if j else prior[5],
                                    prior[6] + float(l) * z[1] if l else prior[6]])
    return np.array(out, dtype=np.float64).reshape(-1, 7)


# ---- the score --------------------------------------------------------------------------------------------------------------
def quat_to_mat(q):
    """csrc/se3_math.h's quat_to_mat, operation for operation"""
    x, y, z, w = (float(v) for v in q)
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
            2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]


def move(pose, rows):
    """the rows moved as k_tf moves them: R[0] x + R[1] y + R[2] z + t, left to right, the label kept"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    R, t = quat_to_mat(pose[:4]), [float(v) for v in pose[4:7]]
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    out = rows.copy()
    out[:, 0] = R[0] * x + R[1] * y + R[2] * z + t[0]
    out[:, 1] = R[3] * x + R[4] * y + R[5] * z + t[1]
    out[:, 2] = R[6] * x + R[7] * y + R[8] * z + t[2]
    return out


def score(oracle_map, rows, poses, md, kernel, th):
    """(sum_w [K], n_pairs [K]) over the oracle's pairs of the rows moved by each pose: w = k^2 / (k + |r|^2)^2, fp64"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    sum_w, pairs = np.zeros(len(poses)), np.zeros(len(poses), dtype=np.int64)
    for c, pose in enumerate(poses):
        src, tgt = oracle_map.get_correspondences(move(pose, rows), md, th)
        r = src[:, :3] - tgt[:, :3]
        e = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        den = kernel + e
        sum_w[c] = float(np.sum(kernel * kernel / (den * den)))
        pairs[c] = len(src)
    return sum_w, pairs


def ranking(scores):
    """indices by score, descending, ties to the lower index"""
    return np.lexsort((np.arange(len(scores)), -np.asarray(scores)))
