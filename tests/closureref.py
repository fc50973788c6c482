"""Plain numpy restatement of the loop closure (include/sageicp.h "loop closure"), for the tests only, written
from the definitions:

  * corrections(): delta, the pivot, the shares of path length, C_k and the corrected poses, with the SE(3) arithmetic in
    the operation order of csrc/se3_math.h, in any numpy float type (np.float64: what the library is held to;
    np.longdouble: what both are measured against, as tests/gnref.py does for the Gauss-Newton step);
  * session_voxels(): the voxels of a selection enumerated from archive_voxels(), the plain exports and Pointcloud();
  * stays(): the stay rule — walk back from hi while the position is not far from the voxel's first row, keep the nearest,
    the later on a tie — with mapref.MapRef.remove_far's far test in the association SQNORM3_ORDER selects;
  * move(): every row moved by the correction of its voxel's stay, in the operation order of quat_to_mat / mat_apply.
nearest_pose() is the rule the stay rule is NOT: the nearest position over all poses."""
import numpy as np

import archiveref
import mapref
import recallref


# ---- SE(3): (qx, qy, qz, qw, tx, ty, tz), csrc/se3_math.h --------------------------------------------------------------
def quat_to_mat(q):
    x, y, z, w = q[0], q[1], q[2], q[3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    xx, yy, zz = x * x, y * y, z * z
    xy, xz, yz = x * y, x * z, y * z
    wx, wy, wz = w * x, w * y, w * z
    return np.array([one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
                     two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
                     two * (xz - wy), two * (yz + wx), one - two * (xx + yy)], dtype=q.dtype)


def mat_apply(R, t, p):
    return np.array([R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + t[0],
                     R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + t[1],
                     R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + t[2]], dtype=R.dtype)


def se3_mul(A, B):
    ax, ay, az, aw = A[:4]
    bx, by, bz, bw = B[:4]
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by - ax * bz + ay * bw + az * bx
    z = aw * bz + ax * by - ay * bx + az * bw
    w = aw * bw - ax * bx - ay * by - az * bz
    inv = A.dtype.type(1) / np.sqrt(x * x + y * y + z * z + w * w)
    t = mat_apply(quat_to_mat(A), A[4:], B[4:])
    return np.array([x * inv, y * inv, z * inv, w * inv, t[0], t[1], t[2]], dtype=A.dtype)


def se3_inv(A):
    qi = np.array([-A[0], -A[1], -A[2], A[3]], dtype=A.dtype)
    t = mat_apply(quat_to_mat(qi), np.zeros(3, dtype=A.dtype), A[4:])
    return np.array([qi[0], qi[1], qi[2], qi[3], -t[0], -t[1], -t[2]], dtype=A.dtype)


def _cross(w, u):
    return np.array([w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]], dtype=w.dtype)


def se3_log(T):
    f = T.dtype.type
    n2 = T[0] * T[0] + T[1] * T[1] + T[2] * T[2]
    qw = T[3]
    if n2 < 1e-20:
        k = f(2) / qw - (f(2) / f(3)) * n2 / (qw * qw * qw)
        th = f(2) * n2 / qw
    else:
        n = np.sqrt(n2)
        at = np.arctan2(-n, -qw) if qw < 0 else np.arctan2(n, qw)
        k = f(2) * at / n
        th = k * n
    w = np.array([k * T[0], k * T[1], k * T[2]], dtype=T.dtype)
    if abs(th) < 1e-10:
        c = f(1) / f(12)
    else:
        half = f(0.5) * th
        c = (f(1) - th * np.cos(half) / (f(2) * np.sin(half))) / (th * th)
    t = T[4:]
    cr = _cross(w, t)
    ccr = _cross(w, cr)
    return np.array([t[0] - f(0.5) * cr[0] + c * ccr[0], t[1] - f(0.5) * cr[1] + c * ccr[1], t[2] - f(0.5) * cr[2] + c * ccr[2],
                     w[0], w[1], w[2]], dtype=T.dtype)


def se3_exp(a):
    f = a.dtype.type
    w = a[3:]
    th2 = a[3] * a[3] + a[4] * a[4] + a[5] * a[5]
    th = np.sqrt(th2)
    if th < 1e-10:
        th4 = th2 * th2
        imag = f(0.5) - th2 / f(48) + th4 / f(3840)
        real = f(1) - th2 / f(8) + th4 / f(384)
        A = f(0.5) - th2 / f(24)
        B = f(1) / f(6) - th2 / f(120)
    else:
        half = f(0.5) * th
        imag = np.sin(half) / th
        real = np.cos(half)
        A = (f(1) - np.cos(th)) / th2
        B = (th - np.sin(th)) / (th2 * th)
    u = a[:3]
    cr = _cross(w, u)
    ccr = _cross(w, cr)
    return np.array([imag * w[0], imag * w[1], imag * w[2], real,
                     u[0] + A * cr[0] + B * ccr[0], u[1] + A * cr[1] + B * ccr[1], u[2] + A * cr[2] + B * ccr[2]], dtype=a.dtype)


def _dist3(a, b):
    d = a - b
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def corrections(poses, i, j, closed, dtype=np.float64):
    """dict: C (n, 7), poses_out (n, 7), alpha (n,), delta, angle, shift, path — all in `dtype`"""
    P = np.asarray(poses, dtype=np.float64).astype(dtype)
    closed = np.asarray(closed, dtype=np.float64).astype(dtype)
    f = P.dtype.type
    n = len(P)
    c = P[j, 4:]
    delta = se3_mul(closed, se3_inv(P[j]))
    u = mat_apply(quat_to_mat(delta), delta[4:], c)
    D = np.concatenate([delta[:4], u - c])
    a = se3_log(D)
    steps = np.array([_dist3(P[m, 4:], P[m - 1, 4:]) for m in range(i + 1, j + 1)], dtype=dtype)
    path = f(0)
    for s in steps:
        path = path + s
    C, out, alpha = np.zeros((n, 7), dtype=dtype), np.zeros((n, 7), dtype=dtype), np.zeros(n, dtype=dtype)
    run = f(0)
    for k in range(n):
        if k <= i:
            C[k] = np.array([0, 0, 0, 1, 0, 0, 0], dtype=dtype)
            out[k] = P[k]
            continue
        if k >= j:
            alpha[k] = f(1)
            C[k] = delta
        else:
            run = run + steps[k - i - 1]
            alpha[k] = run / path if path > 0 else f(k - i) / f(j - i)
            E = se3_exp(alpha[k] * a)
            v = mat_apply(quat_to_mat(E), E[4:], -c)
            C[k] = np.concatenate([E[:4], v + c])
        out[k] = se3_mul(C[k], P[k])
    return dict(C=C, poses_out=out, alpha=alpha, delta=delta, angle=np.sqrt((a[3] * a[3] + a[4] * a[4]) + a[5] * a[5]),
                shift=np.sqrt((D[4] * D[4] + D[5] * D[5]) + D[6] * D[6]), path=path)


# ---- the session's voxels ---------------------------------------------------------------------------------------------
def session_voxels(m, which, voxel_size):
    """The voxels of selection `which` ("all", "latest", "session") of map m in selection order, from archive_voxels(), the
    ALL export and Pointcloud(): (rows (r, 4), counts (v,), updates (v,): the serial of a record, -1 for a live voxel).
    The rows are asserted to be the plain export's."""
    rec = m.archive_voxels()
    log = m.ArchivedPointcloud("all")
    cloud = m.Pointcloud() if which == "session" else np.zeros((0, 4))
    keep = np.ones(len(rec), dtype=bool)
    if which != "all":
        live = set(archiveref.keys_of(m.Pointcloud(), voxel_size))
        keys = [(int(r.x), int(r.y), int(r.z)) for r in rec]
        later = set()
        for idx in range(len(rec) - 1, -1, -1):
            keep[idx] = keys[idx] not in live and keys[idx] not in later
            later.add(keys[idx])
    parts, counts, updates = [], [], []
    for r in rec[keep]:
        parts.append(log[int(r.first_row):int(r.first_row) + int(r.count)])
        counts.append(int(r.count))
        updates.append(int(r.update))
    for _, g in recallref.groups(cloud, voxel_size):
        parts.append(np.array(g, dtype=np.float64).reshape(-1, 4))
        counts.append(len(g))
        updates.append(-1)
    rows = np.concatenate(parts) if parts else np.zeros((0, 4))
    assert rows.tobytes() == m.ArchivedPointcloud(which).tobytes(), "the enumeration is not the plain export"
    return rows, np.array(counts, dtype=np.int64), np.array(updates, dtype=np.int64)


def first_rows(rows, counts):
    return rows[np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)] if len(counts) else np.zeros((0, 4))


def _sqdist(p, c):
    dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    return xx + (yy + zz) if mapref.SQNORM3_ORDER == 0 else (xx + yy) + zz


def stays(first, updates, positions, max_distance):
    """the stay of every voxel: first (v, >= 3) its first row, updates (v,) as session_voxels gives them"""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    n, v = len(pos), len(first)
    hi = np.where(updates < 0, n, np.minimum(updates, n)) - 1
    best = np.maximum(hi, 0)
    best_d = np.full(v, np.inf)
    walking = hi >= 0
    max2 = float(max_distance) * float(max_distance)
    k = int(hi.max()) if v else -1
    while k >= 0 and walking.any():
        at = np.flatnonzero(walking & (hi >= k))
        d = _sqdist(first[at], pos[k])
        far = d > max2
        walking[at[far]] = False
        better = ~far & (d < best_d[at])
        best_d[at[better]] = d[better]
        best[at[better]] = k
        k -= 1
    return best.astype(np.uint32)


def stay_lengths(first, updates, positions, max_distance):
    """how many positions each voxel's walk accepted"""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    out = np.zeros(len(first), dtype=np.int64)
    for v in range(len(first)):
        k = (n if updates[v] < 0 else min(int(updates[v]), n)) - 1
        while k >= 0 and not _sqdist(first[v:v + 1], pos[k])[0] > float(max_distance) * float(max_distance):
            out[v] += 1
            k -= 1
    return out


def nearest_pose(first, positions):
    """NOT the rule: the nearest position over all poses, the later on a tie"""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    d = np.stack([_sqdist(first, c) for c in pos], axis=1)
    return (len(pos) - 1 - np.argmin(d[:, ::-1], axis=1)).astype(np.uint32)


def move(rows, counts, stay, corrections):
    """every row by corrections[stay of its voxel]: R from quat_to_mat, ((R0 x + R1 y) + R2 z) + t; the label untouched"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    C = np.asarray(corrections, dtype=np.float64)[np.repeat(np.asarray(stay, dtype=np.int64), counts)]
    x, y, z, w = C[:, 0], C[:, 1], C[:, 2], C[:, 3]
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    R = [1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
         2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
         2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)]
    p = rows[:, :3]
    out = rows.copy()
    for r in range(3):
        out[:, r] = ((R[3 * r] * p[:, 0] + R[3 * r + 1] * p[:, 1]) + R[3 * r + 2] * p[:, 2]) + C[:, 4 + r]
    return out
