"""Adversarial scenes for the dynamic vehicle filter (csrc/dyn_filter.hip; core/Preprocessing.cpp:95-172), for the
tests only.  synthetic_dynamic.py plants 284-point cars with a few neighbours per point; these families aim at what
it leaves out: long union-find chains, cells holding hundreds of points, components of thousands of points, points on
the 0.5 m cell faces and pairs at d2 == 0.25f, and frame sizes around the kernels' block and table boundaries.

Every generator is deterministic from its seed; coordinates are rounded to fp32 and widened, and every scene lies
inside the default crop (5-100 m) unless it says otherwise, vehicles and landmarks within label_max_range (50 m).  Vehicles carry KITTI vehicle labels (10, 18, 20),
landmarks 44 / 48, everything else 40 (road)."""
import numpy as np

VEH = (10, 11, 13, 15, 16, 18, 20)
ORDERS = ("path", "reversed", "bitrev", "random")


def _f32(p):
    p = np.array(p, dtype=np.float64).reshape(-1, 4)
    p[:, :3] = p[:, :3].astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(p)


def _rows(xyz, label):
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    return np.column_stack([xyz, np.full(len(xyz), float(label))])


def _road(rng, n, x=(20.0, 40.0), y=(-30.0, -20.0), z=-1.7):
    """ordinary points well away from every planted vehicle"""
    return _rows(np.column_stack([rng.uniform(*x, n), rng.uniform(*y, n), z + rng.normal(0, 0.02, n)]), 40.0)


def order(n, kind, rng):
    """a permutation of range(n): along the path, reversed, bit-reversed interleave, or random"""
    if kind == "path":
        return np.arange(n)
    if kind == "reversed":
        return np.arange(n)[::-1].copy()
    if kind == "bitrev":
        bits = max(1, int(np.ceil(np.log2(max(n, 2)))))
        k = np.arange(1 << bits, dtype=np.int64)
        r = np.zeros_like(k)
        for b in range(bits):
            r |= ((k >> b) & 1) << (bits - 1 - b)
        return r[r < n]
    if kind == "random":
        return rng.permutation(n)
    raise ValueError(kind)


def serpentine_path(n):
    """n points 0.4 m apart along a 3-D serpentine: rows along x of 60 points, rows 0.6 m apart in y, layers of 20
    rows 0.6 m apart in z.  Consecutive rows (and layers) are joined by one point 0.42 m from both row ends, so the
    vehicle points form one path graph: no two points but consecutive ones are within 0.5 m."""
    per_row, rows_per_layer = 60, 20
    pts = []
    row = layer = 0
    forward = True
    y_up = True
    while len(pts) < n:
        y = 0.6 * (row if y_up else rows_per_layer - 1 - row)
        z = 0.6 * layer
        xs = 10.0 + 0.4 * np.arange(per_row)
        if not forward:
            xs = xs[::-1]
        for x in xs:
            pts.append((x, y, z))
        end_x = xs[-1] + (0.3 if forward else -0.3)
        if row + 1 < rows_per_layer:       # turn to the next row of this layer
            pts.append((end_x, y + (0.3 if y_up else -0.3), z))
            row += 1
        else:                               # climb to the next layer, rows run back the other way in y
            pts.append((end_x, y, z + 0.3))
            row = 0
            layer += 1
            y_up = not y_up
        forward = not forward
    return np.array(pts[:n]) + np.array([0.0, 5.0, -1.0])


def serpentine(seed, n=30000, kind="path", lm_rows=3):
    """one path-graph component of n vehicle points in frame order `kind`, landmarks 0.35 m under the first lm_rows
    rows of the path (one per point), a few road points; returns (frame, number of landmark points)"""
    rng = np.random.default_rng(seed)
    path = serpentine_path(n)
    veh = _rows(path, 20.0)[order(n, kind, rng)]
    m = min(n, 61 * lm_rows)
    lm = _rows(path[:m] - np.array([0.0, 0.0, 0.35]), 44.0)
    road = _road(rng, 777)
    return _f32(np.concatenate([road[:400], lm, veh, road[400:]])), m


def dense_blob(seed, n=20000, repeat=1, centre=(30.0, 10.0, -1.0), shuffle=True):
    """n vehicle points uniform in a 2 x 2 x 1.5 m box (cells of 0.5 m hold hundreds of points) over a landmark layer
    0.2 m under its floor on a 0.1 m grid; with repeat > 1 every vehicle point appears that many times (d2 == 0)"""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre)
    v = c + rng.uniform([-1.0, -1.0, 0.0], [1.0, 1.0, 1.5], size=(n, 3))
    v = np.repeat(v, repeat, axis=0)
    g = np.arange(-1.0, 1.0001, 0.1)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    lm = np.column_stack([c[0] + gx.ravel(), c[1] + gy.ravel(), np.full(gx.size, c[2] - 0.2)])
    f = np.concatenate([_rows(v, 10.0), _rows(lm, 48.0), _road(rng, 1500)])
    if shuffle:
        f = f[rng.permutation(len(f))]
    return _f32(f)


def _grid_box(lo, dims, pitch=0.25):
    """the surface points of a box on a grid of `pitch` (exact in fp32 for pitch 0.25 and lo on that grid)"""
    nx, ny, nz = dims
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    s = (i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1) | (k == 0) | (k == nz - 1)
    return np.asarray(lo) + pitch * np.column_stack([i[s], j[s], k[s]]).astype(np.float64)


def bumper_rows(seed, n_cars=(30, 24)):
    """Row A: n_cars[0] grid cars 0.25 m apart bumper to bumper — one component of thousands of points.  Row B, 3 m
    away: n_cars[1] cars exactly 0.5 m apart (exact in fp32: d2 == 0.25f, no neighbours), so they stay separate; some
    lose one point, so the sizes are equal or differ by one and only an exact replay of PCL's unstable sort orders
    them.  Landmarks lie under part of row A and under every other car of row B.  Returns (frame, {"a": size of row
    A, "b": sizes of row B's cars})."""
    rng = np.random.default_rng(seed)
    dims = (9, 5, 4)                                    # 2.0 x 1.0 x 0.75 m, 138 surface points
    L = 0.25 * (dims[0] - 1)
    parts, lms, sizes_b = [], [], []
    row_a = [_grid_box((-30.0 + k * (L + 0.25), 6.0, -1.0), dims) for k in range(n_cars[0])]
    parts.append(_rows(np.concatenate(row_a), 10.0))
    for k in range(0, n_cars[0] // 3):                  # landmarks under the first third of row A
        lms.append(_grid_box((-30.0 + k * (L + 0.25), 6.0, -1.375), (dims[0], dims[1], 1)))
    for k in range(n_cars[1]):
        car = _grid_box((-30.0 + k * (L + 0.5), 10.0, -1.0), dims)
        if rng.uniform() < 0.5:
            car = np.delete(car, int(rng.integers(len(car))), axis=0)
        sizes_b.append(len(car))
        parts.append(_rows(car, 18.0))
        if k % 2 == 0:
            lms.append(_grid_box((-30.0 + k * (L + 0.5), 10.0, -1.375), (dims[0], dims[1], 1)))
    f = np.concatenate(parts + [_rows(np.concatenate(lms), 44.0), _road(rng, 2000)])
    f = f[rng.permutation(len(f))]
    return _f32(f), {"a": len(row_a) * len(row_a[0]), "b": sizes_b}


def ulp_steps(x, k):
    """x moved by k fp32 ulps"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return float(x)


def d2_f32(a, b):
    """FLANN's L2_Simple on fp32 copies: (dx*dx + dy*dy) + dz*dz in float, no FMA"""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32)
    d = (a - b).astype(np.float32)
    return np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + np.float32(d[2] * d[2]))


QUARTER = np.float32(0.25)
BELOW_QUARTER = np.nextafter(np.float32(0.25), np.float32(0), dtype=np.float32)


def edge_pair(rng, a, target):
    """a point b near a + 0.5 u (u random) whose fp32 d2 to a is exactly `target` (0.25f or the float below), or
    None"""
    for _ in range(200):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        b0 = (np.asarray(a) + 0.5 * u).astype(np.float32)
        for dx in range(-3, 4):
            for dy in range(-3, 4):
                for dz in range(-3, 4):
                    b = [ulp_steps(b0[0], dx), ulp_steps(b0[1], dy), ulp_steps(b0[2], dz)]
                    if d2_f32(a, b) == target:
                        return b
    return None


def cell_faces(seed, n_pairs=24):
    """Points on the 0.5 m cell faces and one ulp either side, negative and straddling 0 included: vehicle and
    landmark points on the lattice k * 0.5 (k ranges chosen so x and z straddle 0, y negative or far), and isolated
    probes — a 5-point vehicle clump with one partner at fp32 d2 exactly 0.25f or the float below it, the partner a
    vehicle clump (linked or not) or a landmark (counted or not)."""
    rng = np.random.default_rng(seed)
    rows = []
    # lattice blocks: every point on k * 0.5 moved by -1, 0 or +1 ulp per axis
    for (x0, y0, z0, nx, ny, nz) in ((-1.5, -12.0, -1.0, 7, 3, 5), (6.0, 7.0, -0.5, 4, 4, 3), (-9.0, 3.0, 0.0, 3, 5, 2)):
        for i in range(nx):
            for j in range(ny):
                for k in range(nz):
                    base = (x0 + 0.5 * i, y0 + 0.5 * j, z0 + 0.5 * k)
                    for _ in range(int(rng.integers(1, 4))):
                        p = [ulp_steps(c, int(rng.integers(-1, 2))) for c in base]
                        lab = 10.0 if rng.uniform() < 0.7 else 44.0
                        rows.append(p + [lab])
    # probes: 4 extra points on the far side of a keep each clump at 5 points and away from its partner
    for t in range(n_pairs):
        a = np.array([-40.0 + 3.0 * (t % 12), 20.0 + 3.0 * (t // 12), -1.0 + 0.5 * (t % 3)], dtype=np.float32)
        a = a.astype(np.float64)
        target = QUARTER if t % 2 == 0 else BELOW_QUARTER
        b = edge_pair(rng, a, target)
        assert b is not None
        b = np.asarray(b)
        u = (b - a) / np.linalg.norm(b - a)
        clump_a = [a] + [a - 0.05 * (m + 1) * u for m in range(4)]
        rows += [list(p) + [10.0] for p in clump_a]
        if (t // 2) % 2 == 0:                      # partner: another vehicle clump
            rows += [list(p) + [18.0] for p in [b] + [b + 0.05 * (m + 1) * u for m in range(4)]]
        else:                                      # partner: one landmark point
            rows.append(list(b) + [48.0])
    f = np.array(rows, dtype=np.float64)
    f = np.concatenate([f, _road(rng, 300)])
    # the probes' exact d2 is a property of the fp32 points as stored: the rows are not rounded again
    f[:, :3] = f[:, :3].astype(np.float32).astype(np.float64)
    return np.ascontiguousarray(f[rng.permutation(len(f))])


def with_vehicle_count(seed, nv, n):
    """n points (nv of them vehicles, in clumps and chains) for the size boundaries of the kernels and tables"""
    rng = np.random.default_rng(seed)
    assert n >= nv
    k = np.arange(nv)
    # vehicle points on a 0.3 m lattice of 16 x 16 x z, broken into blocks by 1 m gaps: many components
    ix, iy, iz = k % 16, (k // 16) % 16, k // 256
    veh = np.column_stack([10.0 + 0.3 * ix + (ix // 4) * 0.7, -8.0 + 0.3 * iy + (iy // 8) * 0.7, -1.0 + 0.3 * (iz % 40)])
    veh[:, 0] += 5.0 * (iz // 40)
    veh = veh + rng.uniform(-0.02, 0.02, size=veh.shape)
    lm = veh[:: 7] - np.array([0.0, 0.0, 0.2])
    m = min(len(lm), n - nv)
    parts = [_rows(veh, 20.0), _rows(lm[:m], 44.0), _road(rng, n - nv - m, x=(30.0, 90.0), y=(20.0, 40.0))]
    f = np.concatenate(parts)
    return _f32(f[rng.permutation(len(f))])


def _chain(x0, y, z, m, step, label):
    return [[x0 + step * k, y, z, label] for k in range(m)]


# ---- known-answer scenes for the label and threshold edges (ranges of dynref.KAT_RANGES) ----------------------------
def label_kat_scenes():
    """{name: (frame, kwargs of preprocess, expected filtered frame)} — answers derived by hand from the reference:
    labels are static_cast<uint32_t>(static_cast<long long>(l)) as x86-64 computes it, lists compare as unsigned"""
    S = {}
    road = [[8.0, 3.0, 0.0, 40.0]]
    six = _chain(20.0, 0.0, 0.0, 6, 0.3, 10.0)
    beside = [[20.0 + 0.3 * k, 0.45, 0.0, 44.0] for k in range(6)]         # one landmark neighbour per point

    # a label in both lists: every vehicle point counts itself and its chain neighbours (2 + 3 * 4 + 2 = 16)
    for th, kept in ((2.0, True), (3.0, False)):            # thresholds 12 and 18
        f = np.array(road + six)
        exp = road + (six if kept else [])
        S["both_lists_dy_%g" % th] = (f, dict(dy_th=th, dynamic_labels=(10,), landmark_labels=(10,)), np.array(exp))
    # label -1.0 listed as -1: 0xFFFFFFFF on both sides — as a vehicle and as a landmark
    v = _chain(20.0, 0.0, 0.0, 6, 0.3, -1.0)
    f = np.array(v + beside + road)
    S["minus_one_vehicle"] = (f, dict(dy_th=0.5, dynamic_labels=(-1,), landmark_labels=(44,)), np.array(beside + road + v))
    lmm = [[20.0 + 0.3 * k, 0.45, 0.0, -1.0] for k in range(6)]
    f = np.array(six + lmm + road)
    S["minus_one_landmark"] = (f, dict(dy_th=0.5, dynamic_labels=(10,), landmark_labels=(-1,)), np.array(lmm + road + six))
    # fractional labels truncate toward zero: 10.9 -> 10 (vehicle), -0.5 -> 0 (landmark with 0 listed)
    v = _chain(20.0, 0.0, 0.0, 6, 0.3, 10.9)
    lmh = [[20.0 + 0.3 * k, 0.45, 0.0, -0.5] for k in range(6)]
    f = np.array(v + lmh + road)
    S["fractional"] = (f, dict(dy_th=0.5, dynamic_labels=(10,), landmark_labels=(0,)), np.array(lmh + road + v))
    # 2^32 + 10 acts as 10: a vehicle cluster with no landmark -> dropped
    v = _chain(20.0, 0.0, 0.0, 6, 0.3, 4294967306.0)
    f = np.array(v + road)
    S["two_pow_32_plus_10"] = (f, dict(dy_th=0.5, dynamic_labels=(10,), landmark_labels=(44,)), np.array(road))
    # |l| >= 2^63 converts to INT64_MIN (cvttsd2si), whose low 32 bits are 0
    v = [[20.0 + 0.3 * k, 0.0, 0.0, 1e19 if k % 2 else -1e19] for k in range(6)]
    f = np.array(v + road)
    S["pm_1e19_dynamic_0"] = (f, dict(dy_th=0.5, dynamic_labels=(0,), landmark_labels=(44,)), np.array(road))
    lmb = [[20.0 + 0.3 * k, 0.45, 0.0, 1e19 if k % 2 else -1e19] for k in range(6)]
    f = np.array(six + lmb + road)
    S["pm_1e19_landmark_0"] = (f, dict(dy_th=0.5, dynamic_labels=(10,), landmark_labels=(0,)), np.array(lmb + road + six))
    S["pm_1e19_landmark_0_none"] = (f, dict(dy_th=0.5, dynamic_labels=(10,), landmark_labels=(44,)), np.array(lmb + road))
    # beyond label_max_range (50 m) a label is zeroed first: 0 listed as dynamic turns a far car into a vehicle cluster
    far = _chain(60.0, 0.0, 0.0, 6, 0.3, 10.0)
    far0 = [[r[0], r[1], r[2], 0.0] for r in far]
    f = np.array(far + road)
    S["far_zeroed_dynamic_0"] = (f, dict(dy_th=0.5, dynamic_labels=(10, 0), landmark_labels=(44,)), np.array(road))
    S["far_zeroed_not_listed"] = (f, dict(dy_th=0.5, dynamic_labels=(10,), landmark_labels=(44,)), np.array(far0 + road))
    # ... and 0 listed as a landmark: zeroed points beyond 50 m count for vehicles just inside it.  Vehicles at
    # 49.42 .. 49.92, zeroed landmarks at 50.1, 50.2, 50.3: 4 + 3 + 2 = 9 pairs within 0.5 m (the farthest 0.48 m)
    veh = [[49.42 + 0.1 * k, 0.0, 0.0, 10.0] for k in range(6)]
    lz = [[50.1 + 0.1 * k, 0.0, 0.0, 10.0] for k in range(3)]
    lz0 = [[r[0], r[1], r[2], 0.0] for r in lz]
    f = np.array(veh + lz + road)
    for th, kept in ((1.0, True), (1.5, False)):              # thresholds 6 and 9
        S["far_zeroed_landmark_0_dy_%g" % th] = (f, dict(dy_th=th, dynamic_labels=(10,), landmark_labels=(0,)),
                                                 np.array(lz0 + road + (veh if kept else [])))
    return {k: (_f32(a), kw, _f32(e)) for k, (a, kw, e) in S.items()}


def threshold_kat_scenes():
    """{name: (frame, kwargs, expected)}: a cluster of 8 points with 6 landmark neighbours, one of 7 with none,
    clusters of exactly 5 and exactly 4 with landmarks beside every point, over the dy_th edges.  The reference's
    threshold is static_cast<int>(dy_th * size): INT_MIN once the product leaves the int range (x86-64)."""
    road = [[8.0, 3.0, 0.0, 40.0]]
    c8 = _chain(20.0, 0.0, 0.0, 8, 0.3, 10.0)
    l8 = [[20.0 + 0.3 * k, 0.45, 0.0, 44.0] for k in range(6)]
    c7 = _chain(20.0, 10.0, 0.0, 7, 0.3, 10.0)
    c5 = _chain(20.0, -10.0, 0.0, 5, 0.3, 10.0)
    l5 = [[20.0 + 0.3 * k, -9.55, 0.0, 44.0] for k in range(5)]
    c4 = _chain(30.0, -10.0, 0.0, 4, 0.3, 10.0)
    l4 = [[30.0 + 0.3 * k, -9.55, 0.0, 44.0] for k in range(4)]
    f = np.array(c8 + l8 + c7 + road + c5 + l5 + c4 + l4)
    inl = l8 + road + l5 + l4
    two31_8 = 2.0 ** 28                       # 2^31 / 8: the size-8 cluster's product reaches 2^31 exactly
    below = float(np.nextafter(two31_8, 0.0))
    above = float(np.nextafter(two31_8, np.inf))
    # (dy_th, kept c8, kept c5): c8 has count 6, c5 count 5; c7 (count 0) and c4 (too small) never stay
    cases = [(-1.0, True, True), (0.0, True, True), (0.5, True, True), (0.75, False, True), (1.0, False, False),
             (below, False, False), (two31_8, True, False), (above, True, False), (1e10, True, True),
             (1e300, True, True)]
    S = {}
    for th, k8, k5 in cases:
        # emission order: the larger cluster first
        exp = inl + (c8 if k8 else []) + (c5 if k5 else [])
        S["dy_th_%r" % th] = (f, dict(dy_th=th, dynamic_labels=(10,), landmark_labels=(44,)), np.array(exp))
    return {k: (_f32(a), kw, _f32(e)) for k, (a, kw, e) in S.items()}
