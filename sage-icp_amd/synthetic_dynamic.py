"""Synthetic street scans for the dynamic vehicle filter (core/Preprocessing.cpp:95-172).

A straight street along x, seen from a sensor 1.73 m above the ground: road (40) for |y| < 6, parking (44) for
6 <= |y| < 9, sidewalk (48) for 9 <= |y| < 11, terrain (72) to the building (50) walls at |y| = 14, poles (80) and
vegetation (70) beside them, ~2 % unlabelled (0).  Planted vehicles:

  parked   cars on the parking strips (labels 10 / 18), with dense parking ground under and around them: their points
           see far more landmark (44 / 48) points within 0.5 m than any dy_th in [0, 1] asks for -> kept
  moving   cars on the road (|y| <= 3.9), more than 2 m from any landmark point -> removed
  kerb     cars on the road whose outer side is near the parking strip's ordinary (sparse) ground: what they see
           of it decides — kept for a low dy_th, removed for a high one
  fragments  groups of 1-4 vehicle points (on the road and on the parking strip) -> removed (clusters need 5)
  far      cars beyond label_max_range (50 m): their labels are zeroed, they are ordinary points -> kept

Every car is the same 284-point grid on the top and the four sides of a 4.2 x 1.8 x 1.5 m box (0.3 m pitch, 4 cm
jitter: each car is one connected cluster, no two cars touch), so a scan holds more than 16 clusters of equal size
and the kept ones leave PCL's unstable sort in an order only an exact replay reproduces.  Points are shuffled
(the cluster order follows the smallest frame index), rounded to fp32 and widened.  `make_dynamic_scan` is one
scan; `make_dynamic_stream` moves the sensor along the street (and the moving cars faster) frame by frame.
"""
import numpy as np

GROUND_Z = -1.73
VEHICLE_LABELS = (10, 11, 13, 15, 16, 18, 20)      # voxel_labels[5] of the SemanticKITTI launches
LANDMARK_LABELS = (44, 48)
CAR_DIMS = (4.2, 1.8, 1.5)
CAR_POINTS = 284
PARKED_X = tuple(-27.0 + 6.0 * k for k in range(10))                 # both sides: 20 parked cars
MOVING = ((12.0, -3.0), (20.0, 3.0), (30.0, -3.0), (-15.0, 3.0), (-25.0, -3.0), (40.0, 3.0))
KERB = ((35.0, 5.3), (-35.0, -5.3), (40.0, -5.3), (-40.0, 5.2))   # on the road, one side by the parking strip
FAR = ((62.0, 7.5), (71.0, -7.5), (-66.0, 7.5), (82.0, -7.5))
FRAGMENTS = ((-40.0, -2.0, 1), (-43.0, 2.0, 2), (-46.0, 0.0, 3), (-37.0, 4.0, 4),
             (34.0, 7.5, 2), (37.0, -7.5, 4), (44.0, 7.5, 3), (47.0, -7.5, 1))


def _ground_label(y):
    a = np.abs(y)
    return np.select([a < 6.0, a < 9.0, a < 11.0], [40.0, 44.0, 48.0], 72.0)


def _car(rng, cx, cy, label):
    """the 284-point box grid of one car centred at (cx, cy), its floor 0.1 m above the ground"""
    L, W, H = CAR_DIMS
    s = 0.3
    xs = -L / 2 + s / 2 + s * np.arange(round(L / s))
    ys = -W / 2 + s / 2 + s * np.arange(round(W / s))
    zs = s / 2 + s * np.arange(round(H / s))
    faces = []
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    faces.append(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, H)], 1))                    # top
    for side in (-W / 2, W / 2):
        gx, gz = np.meshgrid(xs, zs, indexing="ij")
        faces.append(np.stack([gx.ravel(), np.full(gx.size, side), gz.ravel()], 1))
    for end in (-L / 2, L / 2):
        gy, gz = np.meshgrid(ys, zs, indexing="ij")
        faces.append(np.stack([np.full(gy.size, end), gy.ravel(), gz.ravel()], 1))
    p = np.concatenate(faces)
    assert len(p) == CAR_POINTS
    p = p + rng.uniform(-0.04, 0.04, size=p.shape)
    p[:, 0] += cx
    p[:, 1] += cy
    p[:, 2] += GROUND_Z + 0.1
    return np.column_stack([p, np.full(len(p), float(label))])


def _ground_patch(rng, cx, cy, n):
    """dense parking / sidewalk ground under and around a parked car"""
    L, W, _ = CAR_DIMS
    x = cx + rng.uniform(-L / 2 - 0.6, L / 2 + 0.6, n)
    y = cy + rng.uniform(-W / 2 - 0.6, W / 2 + 0.6, n)
    z = GROUND_Z + rng.normal(0, 0.02, n)
    lab = np.where(np.abs(y) < 9.0, 44.0, 48.0)
    return np.column_stack([x, y, z, lab])


def _background(rng, n, sx):
    """n points of ground, walls, poles and vegetation around a sensor at x = sx (range-weighted density)"""
    kind = rng.choice(4, size=n, p=[0.62, 0.25, 0.03, 0.10])
    out = np.empty((n, 4))
    # ground: range uniform in (3, 100) -> density ~ 1 / r, like a spinning sensor's rings; kept off the walls
    g = kind == 0
    r = rng.uniform(3.0, 100.0, g.sum())
    a = rng.uniform(0, 2 * np.pi, g.sum())
    y = np.clip(r * np.sin(a), -13.9, 13.9)
    out[g] = np.column_stack([sx + r * np.cos(a), y, GROUND_Z + rng.normal(0, 0.02, g.sum()), _ground_label(y)])
    w = kind == 1
    k = w.sum()
    out[w] = np.column_stack([sx + rng.uniform(-95, 95, k), rng.choice([-14.0, 14.0], k) + rng.normal(0, 0.02, k),
                              rng.uniform(GROUND_Z, 6.0, k), np.full(k, 50.0)])
    pl = kind == 2
    k = pl.sum()
    px = np.floor((sx + rng.uniform(-95, 95, k)) / 10.0) * 10.0 + 5.0           # a pole every 10 m on both sides
    out[pl] = np.column_stack([px + rng.normal(0, 0.05, k), rng.choice([-12.0, 12.0], k) + rng.normal(0, 0.05, k),
                               rng.uniform(GROUND_Z, 3.0, k), np.full(k, 80.0)])
    v = kind == 3
    k = v.sum()
    vx = np.floor((sx + rng.uniform(-95, 95, k)) / 14.0) * 14.0 + 7.0           # crowns between the poles
    out[v] = np.column_stack([vx + rng.normal(0, 1.0, k), rng.choice([-12.5, 12.5], k) + rng.normal(0, 0.6, k),
                              2.5 + rng.normal(0, 0.8, k), np.full(k, 70.0)])
    out[rng.uniform(size=n) < 0.02, 3] = 0.0
    return out


def _scene(rng, n, sx, t):
    """(frame in the sensor frame, {part: index array}) for a sensor at x = sx: the parked and far cars and the
    fragments stay where the street has them, the moving cars keep their place relative to the sensor + 1.5 t m"""
    parts, chunks = {}, []

    def add(name, pts):
        start = sum(len(c) for c in chunks)
        chunks.append(pts)
        parts.setdefault(name, []).extend(range(start, start + len(pts)))

    for side in (-7.5, 7.5):
        for k, x in enumerate(PARKED_X):
            add("parked", _car(rng, x, side, 10 if k % 3 else 18))
            add("patch", _ground_patch(rng, x, side, 300))
    for k, (x, y) in enumerate(MOVING):
        add("moving", _car(rng, sx + x + 1.5 * t, y, (10, 18, 13)[k % 3]))
    for x, y in KERB:
        add("kerb", _car(rng, x, y, 10))
    for k, (x, y) in enumerate(FAR):
        add("far", _car(rng, x, y, 10))
    for x, y, m in FRAGMENTS:
        p = np.column_stack([x + 0.2 * np.arange(m), np.full(m, y), np.full(m, GROUND_Z + 0.5), np.full(m, 11.0)])
        add("fragment", p)
    have = sum(len(c) for c in chunks)
    assert n > have, "n too small for the planted vehicles"
    add("background", _background(rng, n - have, sx))
    pts = np.concatenate(chunks)
    perm = rng.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    frame = pts[perm]
    frame[:, 0] -= sx
    frame[:, :3] = frame[:, :3].astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(frame), {k: np.sort(inv[np.asarray(v, dtype=np.int64)]) for k, v in parts.items()}


def make_dynamic_scan(seed, n=120000, return_parts=False):
    """One labelled scan of n points in the sensor frame.  With return_parts: (frame, {"parked", "moving", "kerb", "far",
    "fragment", "patch", "background": frame indices of those points})."""
    frame, parts = _scene(np.random.default_rng(seed), n, 0.0, 0)
    return (frame, parts) if return_parts else frame


def make_dynamic_stream(seed, n_frames, n=40000, step=1.0):
    """n_frames scans of a sensor advancing `step` m per frame along the street (the moving cars 1.5 m per frame
    faster); returns (frames, true poses as (qx, qy, qz, qw, tx, ty, tz))."""
    rng = np.random.default_rng(seed)
    frames, poses = [], []
    x0 = -0.5 * n_frames * step
    for k in range(n_frames):
        sx = x0 + k * step
        frames.append(_scene(rng, n, sx, k)[0])
        poses.append(np.array([0.0, 0.0, 0.0, 1.0, sx, 0.0, 0.0]))
    return frames, poses
