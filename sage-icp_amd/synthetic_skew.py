"""Skewed scans of a spinning sensor: the input the reference's deskew (core/Deskew.cpp, pipeline/sageICP.cpp:36-52) is
for, with a known answer.

Frame k is taken at the nominal pose P_k = exp(k xi) of a constant-velocity trajectory (xi: the motion per frame, a
twist, translation first).  The ring scan of synthetic.make_ring_scan at P_k gives every return x in the sensor frame
of P_k; its timestamp is its azimuth as a fraction of a turn, t in [0, 1), as a sensor that spins once per frame would
stamp it.  The sensor that saw the return at time t was at P_k exp((t - 0.5) xi), so the point it reports is
    p = exp((t - 0.5) xi)^-1 x.
Deskewing p with the true poses (delta = log(P_{k-1}^-1 P_k) = xi) gives x back: the unskewed ring scan."""
import numpy as np

from . import synthetic as syn


def _exp(a):
    """SE(3) exponential of tangents a (m, 6) -> (R (m, 3, 3), t (m, 3)); closed forms, Taylor below 1e-4 rad"""
    a = np.atleast_2d(np.asarray(a, dtype=np.float64))
    u, w = a[:, :3], a[:, 3:]
    th2 = np.einsum("ij,ij->i", w, w)
    th = np.sqrt(th2)
    small = th < 1e-4
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)                        # sin / th
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / ths ** 2)          # (1 - cos) / th^2
    C = np.where(small, 1.0 / 6.0 - th2 / 120.0, (ths - np.sin(ths)) / ths ** 3)   # (th - sin) / th^3
    W = np.zeros((len(a), 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    W[:, 1, 0], W[:, 2, 0], W[:, 2, 1] = w[:, 2], -w[:, 1], w[:, 0]
    W2 = W @ W
    I = np.eye(3)[None]
    R = I + A[:, None, None] * W + B[:, None, None] * W2
    V = I + B[:, None, None] * W + C[:, None, None] * W2
    return R, np.einsum("mij,mj->mi", V, u)


def _mat_to_quat(R):
    """unit quaternion (x, y, z, w) of a rotation matrix (Shepperd's method, w >= 0 branch first)"""
    tr = np.trace(R)
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[i] = 0.25 * s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
        q[3] = (R[k, j] - R[j, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def pose_of(a):
    """pose[7] = exp(a) for one tangent a[6]"""
    R, t = _exp(a)
    return np.concatenate([_mat_to_quat(R[0]), t[0]])


def azimuth_timestamps(pts):
    """t in [0, 1): the azimuth of every point in its sensor frame as a fraction of a counter-clockwise turn from +x"""
    az = np.arctan2(pts[:, 1], pts[:, 0])
    t = np.mod(az, 2.0 * np.pi) / (2.0 * np.pi)
    return np.where(t >= 1.0, 0.0, t)


def skew_scan(scan, timestamps, xi):
    """the points a sensor moving by xi per turn reports for the returns `scan` (sensor frame of the mid-scan pose)"""
    s = np.asarray(timestamps, dtype=np.float64) - 0.5
    R, t = _exp(s[:, None] * np.asarray(xi, dtype=np.float64)[None, :])
    out = np.array(scan, dtype=np.float64, copy=True)
    out[:, :3] = np.einsum("mji,mj->mi", R, scan[:, :3] - t)              # R^T (x - t)
    return out


DEFAULT_XI = (1.5, 0.0, 0.0, 0.0, 0.0, np.deg2rad(1.5))      # 1.5 m forward and 1.5 degrees of yaw per frame


def make_skewed_stream(seed=0x5E, n_frames=12, xi=DEFAULT_XI, az_steps=2048, **ring_kw):
    """dict(frames, timestamps, unskewed, poses, xi): n_frames skewed ring scans (131k points each at the default
    2048 azimuth steps), their per-point timestamps, the unskewed scans (the known answer of deskewing with the true
    poses), the true poses P_k = exp(k xi) as (n_frames, 7) and xi"""
    rng = np.random.default_rng(seed)
    xi = np.asarray(xi, dtype=np.float64)
    frames, stamps, unskewed, poses = [], [], [], []
    for k in range(n_frames):
        P = pose_of(k * xi)
        scan = syn.make_ring_scan(rng, P, az_steps=az_steps, **ring_kw)
        t = azimuth_timestamps(scan)
        frames.append(np.ascontiguousarray(skew_scan(scan, t, xi)))
        stamps.append(t)
        unskewed.append(scan)
        poses.append(P)
    return dict(frames=frames, timestamps=stamps, unskewed=unskewed, poses=np.array(poses), xi=xi)
