"""An independent restatement of key-frame selection by occupancy overlap — the odometry node's block at
ros/ros2/OdometryServer.cpp:222-243 with EigenToGridMap and compute_occ_overlap of ros/ros2/Utils.hpp:221-260 — in
plain float64 operations in the reference's order (numpy evaluates no fused multiply-add).

    grid        a point is skipped if x < bx_lo || x > bx_hi || y < by_lo || y > by_hi || z < bz_lo || z > bz_hi;
                occ_x = int((x + bx_hi) / x_res), occ_y = int((y + by_hi) / y_res) with x_res = (bx_hi - bx_lo) / W,
                y_res = (by_hi - by_lo) / H — the UPPER bound as the offset, the cast truncating toward zero — and the
                cell is set if 0 <= occ_x < W and 0 <= occ_y < H (tested on the double: v > -1 and v < W)
    overlap     |key & cur| / |key| as a double of the exact counts; NaN when |key| = 0
    replay      the node's state machine over (raw frame, pose) pairs
"""
import math

import numpy as np


def grid(points, bounds, occ_size):
    """(H, W) uint8: EigenToGridMap of (n, 4) rows"""
    H, W = int(occ_size[0]), int(occ_size[1])
    (xl, xh), (yl, yh), (zl, zh) = [(float(a), float(b)) for a, b in bounds]
    x_res = (xh - xl) / W
    y_res = (yh - yl) / H
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    g = np.zeros((H, W), dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        skip = (x < xl) | (x > xh) | (y < yl) | (y > yh) | (z < zl) | (z > zh)
        vx = (x + xh) / x_res
        vy = (y + yh) / y_res
        ok = ~skip & (vx > -1.0) & (vx < float(W)) & (vy > -1.0) & (vy < float(H))
    g[np.trunc(vy[ok]).astype(np.int64), np.trunc(vx[ok]).astype(np.int64)] = 1
    return g


def overlap(key, cur):
    """compute_occ_overlap(key, cur): (|key & cur| / |key|, |key & cur|, |key|)"""
    inter = int(np.count_nonzero((key == 1) & (cur == 1)))
    total = int(np.count_nonzero(key == 1))
    with np.errstate(invalid="ignore"):
        ov = float(np.float64(inter) / np.float64(total))
    return ov, inter, total


# ---- the SE(3) operations of the library's se3_math.h (the Sophus restatement), in Python floats ----------------------
def quat_to_mat(q):
    x, y, z, w = (float(v) for v in q[:4])
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
            2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
            2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]


def _apply(R, t, p):
    return [R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0],
            R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1],
            R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2]]


def se3_mul(A, B):
    ax, ay, az, aw = (float(v) for v in A[:4])
    bx, by, bz, bw = (float(v) for v in B[:4])
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by - ax * bz + ay * bw + az * bx
    z = aw * bz + ax * by - ay * bx + az * bw
    w = aw * bw - ax * bx - ay * by - az * bz
    inv = 1.0 / math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x * inv, y * inv, z * inv, w * inv
    t = _apply(quat_to_mat(A), [float(v) for v in A[4:7]], [float(v) for v in B[4:7]])
    return np.array([x, y, z, w] + t, dtype=np.float64)


def se3_inv(A):
    qi = [-float(A[0]), -float(A[1]), -float(A[2]), float(A[3])]
    t = _apply(quat_to_mat(qi), [0.0, 0.0, 0.0], [float(v) for v in A[4:7]])
    return np.array(qi + [-t[0], -t[1], -t[2]], dtype=np.float64)


def transform(pose, points):
    """TransformPoints (the library's k_tf): R p + t, each row's sum in the order R0 x + R1 y + R2 z + t"""
    R = quat_to_mat(pose)
    t = [float(v) for v in pose[4:7]]
    p = np.array(points, dtype=np.float64, copy=True).reshape(-1, 4)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    p[:, 0] = R[0] * x + R[1] * y + R[2] * z + t[0]
    p[:, 1] = R[3] * x + R[4] * y + R[5] * z + t[1]
    p[:, 2] = R[6] * x + R[7] * y + R[8] * z + t[2]
    return p


class Replay:
    """The node's key-frame state machine (OdometryServer.cpp:222-243) over registered frames."""

    def __init__(self, bounds, occ_size, th):
        self.bounds, self.occ_size, self.th = bounds, occ_size, float(th)
        self.key_pose = None
        self.key_grid = None
        self.key_index = None
        self.key_frames = 0

    def step(self, points, pose, index):
        """one registered frame: dict(is_key_frame, overlap, key_occupied, intersect, key_pose, key_grid, ...)"""
        pose = np.asarray(pose, dtype=np.float64)
        if self.key_grid is None:
            take, ov, inter, total = True, float("nan"), 0, 0
        else:
            rel = se3_mul(se3_inv(self.key_pose), pose)
            cur = grid(transform(rel, points), self.bounds, self.occ_size)
            ov, inter, total = overlap(self.key_grid, cur)
            take = ov < self.th
        if take:
            self.key_pose = pose.copy()
            self.key_grid = grid(points, self.bounds, self.occ_size)     # the untransformed frame
            self.key_index = index
            self.key_frames += 1
        return dict(is_key_frame=take, overlap=ov, key_occupied=total, intersect=inter, key_pose=self.key_pose.copy(),
                    key_grid=self.key_grid.copy(), key_frame_index=self.key_index, key_frames=self.key_frames)
