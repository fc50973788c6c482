"""Scenes at the far end of the voxel domain, for tests/test_far_scenes_host.py (which asserts that they decide) and
tests/test_far_coordinates_gpu.py (which holds the search to the oracle on them).  numpy only, deterministic seeds.

The map takes any point whose voxel index lies in (-LIM, LIM), LIM = 2^20.  Three parts of the search carry a term that
grows with the coordinate: the fp32 filter's slack (icp_body.h, FILT), the face gaps' slack (icp_body.h, axis_gaps) and
the guard of the reciprocal voxel index (kernels.hip, voxel_index).  Behind them sit the i32 voxel keys of the slot table,
the home-voxel words of a row, the row shift and the 21-bit packed keys of the device update.

  corner         the near-tie scene of test_gpu_parity.py, in voxels, its centre at index LIM - 6 on every axis
  edge           the same, centred at LIM - 3: the map ends at the domain's edge, the queries go on beyond it
  face_deciders  queries on voxel faces whose home voxel x * fl(1 / vs) gets wrong, one map point each that only the
                 right home voxel reaches
  slack_deciders two candidates per query, the nearer one scanned last and one fp32 ulp further away than it is on every
                 axis: the corner scene's neighbours are a third of a voxel away, and a filter slack 256 times too small
                 still passes it (measured) — here the size of the slack decides
  resident_updates  corner's map built and changed by device updates that evict
  planted_frame  a frame of corner's map moved off its place, for RegisterFrame"""
import numpy as np

LIM = 1 << 20

VOXELS = (0.1, 0.8, 1.0, 100.0)
OCTANTS = ((1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1))
LABEL_VARIANTS = ("int", "exotic")
SEM_THS = (0.4, 1.0, 2.5, 0.0)
MAX_DIST_VOXELS = 3.0              # GetCorrespondences' acceptance radius in every scene here, in voxels

DECIDER_VOXELS = (0.1, 0.8)        # (for 0.3, 1.0 and 3.0 the product and the quotient never truncate differently)
FRAME_VOXELS = (0.8, 1.0)
FRAME_POINTS = 2000
FRAME_TWIST_T = (1.0, -1.0, 0.5)   # the planted motion: 1.5 voxels ...
FRAME_TWIST_W = (0.012, -0.0096, 0.0128)                    # ... and 0.02 rad, about the scene's centre


def octant_id(octant):
    return "".join("+" if s > 0 else "-" for s in octant)


def centre_of(vs, octant, back):
    """the voxel-aligned centre `back` voxels inside the domain's corner of this octant"""
    return np.array(octant, dtype=np.float64) * ((LIM - back) * vs)


def voxel_of(p, vs):
    """trunc(fl(p / vs)): the reference's voxel index (int64, so that an index beyond the domain stays what it is)"""
    return np.trunc(np.asarray(p, dtype=np.float64)[..., :3] / vs).astype(np.int64)


def _local(vs, labels):
    """the near-tie scene about the origin, in units of the voxel size: 6000 map points in a box of +-4 voxels, 40 probe
    positions each with a shell of 12 points at radius 0.3 vs (1 +- 1e-9) and 3 exact duplicates of label 40; the
    queries are the probes and 3000 uniform points -> (map (6600, 4), queries (3040, 4))"""
    rng = np.random.default_rng(15)
    mp = rng.uniform(-4, 4, size=(6000, 4))
    mp[:, 3] = rng.choice([0, 40, 50, 70], size=len(mp))
    probes = rng.uniform(-3, 3, size=(40, 3))
    extra = []
    for c in probes:
        dirs = rng.normal(size=(12, 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        r = 0.3 * (1.0 + rng.uniform(-1e-9, 1e-9, size=12))
        pts = c + dirs * r[:, None]
        extra.append(np.c_[pts, rng.choice([0, 40, 50], size=12)])
        extra.append(np.c_[pts[:3], [40, 40, 40]])                 # exact duplicates
    mp = np.vstack([mp] + extra)
    q = np.c_[probes, rng.choice([0, 40, 50], size=len(probes))]
    q = np.vstack([q, np.c_[rng.uniform(-4, 4, size=(3000, 3)), rng.choice([0, 40, 50, 70], size=3000)]])
    mp[:, :3] *= vs
    q[:, :3] *= vs
    if labels == "exotic":                                        # fractional, huge and negative labels
        mp[::7, 3] = 40.5
        mp[::11, 3] = 3.0e9
        q[::5, 3] = 0.25
        q[::13, 3] = -7.0
    else:
        assert labels == "int"
    return mp, q


def _placed(vs, octant, labels, back):
    mp, q = _local(vs, labels)
    c = centre_of(vs, octant, back)
    mp[:, :3] += c
    q[:, :3] += c
    return np.ascontiguousarray(mp), np.ascontiguousarray(q), c


def corner(vs, octant, labels="int"):
    """-> map points, queries, centre: every voxel index within LIM - 6 +- 4 in magnitude"""
    return _placed(vs, octant, labels, 6)


def edge(vs, octant, labels="int"):
    """-> map points (those inside the domain), queries (all of them: home indices up to LIM + 1), centre, the number
    of map points dropped"""
    mp, q, c = _placed(vs, octant, labels, 3)
    inside = (np.abs(mp[:, :3] / vs) < LIM).all(axis=1)
    return np.ascontiguousarray(mp[inside]), q, c, int((~inside).sum())


def face_deciders(vs, sign):
    """-> dict(map (n, 4), queries (n, 4), h, hp, planted (n,), ky (n,), max_dist): x on or one ulp beside a voxel face
    near sign * LIM where h = trunc(fl(x / vs)) and hp = trunc(x * fl(1 / vs)) differ.  Every decider has a row of its own
    (a voxel index ky of its own on y, four apart, near -sign * LIM; z in voxel 5) and one map point at the centre of
    voxel 2h - hp on x: inside the 27 voxels around h, 1.5 voxels from x, and two voxels away from hp."""
    rng = np.random.default_rng(3600 + int(round(vs * 10)) + (0 if sign > 0 else 1))
    k = sign * rng.integers(LIM - 3000, LIM - 4, size=400)
    x0 = k * vs
    x = np.concatenate([np.nextafter(x0, -np.inf), x0, np.nextafter(x0, np.inf)])
    inv = 1.0 / vs
    h = np.trunc(x / vs).astype(np.int64)
    hp = np.trunc(x * inv).astype(np.int64)
    keep = h != hp
    x, h, hp = x[keep], h[keep], hp[keep]
    n = len(x)
    ky = -sign * (LIM - 8 - 4 * np.arange(n))
    y = (ky + 0.5 * np.sign(ky)) * vs                               # (truncation toward zero: voxel ky < 0 is ((ky - 1) vs, ky vs])
    z = np.full(n, 5.5 * vs)
    planted = 2 * h - hp
    px = (planted + 0.5 * np.sign(planted)) * vs
    lab = np.full(n, 40.0)
    return dict(map=np.ascontiguousarray(np.c_[px, y, z, lab]), queries=np.ascontiguousarray(np.c_[x, y, z, lab]),
                h=h, hp=hp, planted=planted, ky=ky, max_dist=MAX_DIST_VOXELS * vs)


SLACK_VOXEL = 0.51                 # (2^20 - 400 .. 2^20) * 0.51 m lies just above 2^19 m: fp32 rounds by up to 2^-24 |x| there
SLACK_DECIDERS = 64
U32 = 2.0 ** -24


def _beside_a_midpoint(x, up):
    """the fp64 number next to x that lies just beyond the midpoint of two neighbouring fp32 numbers, on the side that
    rounds up (`up`) or down in value: the fp32 rounding error is all but half an ulp, of the sign asked for"""
    g = np.float32(x)
    lo = g if np.float64(g) <= x else np.nextafter(g, np.float32(-np.inf))
    hi = np.nextafter(lo, np.float32(np.inf))
    mid = 0.5 * (np.float64(lo) + np.float64(hi))
    off = (np.float64(hi) - np.float64(lo)) * 1e-3
    return mid + off if up else mid - off


def slack_deciders(octant, vs=SLACK_VOXEL):
    """Queries on which the size of the fp32 filter's slack decides -> dict(map (2n, 4), queries (n, 4), winner (n,) rows of
    `map`, first (n,) rows of `map`, max_dist).  Every query sits in the middle of an empty home voxel h near the corner
    of the domain, in a row of its own, with two map points of its label on the diagonal through it: A in voxel h - 1 (on
    every axis: the first of the enumeration), B in voxel h + 1 (the last), c = 1.25 - 1.35 voxels from the query per axis;
    B is the nearer one in fp64, by 1e-6 of the distance.  The query's coordinates lie just below midpoints of the fp32
    grid and B's just above: in fp32 B is one ulp further away on every axis, 2 c ulp + ulp^2 further in the square.  A
    lane that has evaluated A holds b = |A - q|^2 and fetches B only if the fp32 distance passes its threshold
    b (1 + 2^-10) + slack: with E = 2^-22 (|q_a| + 4 vs) per axis the bound asks for a slack of |E|^2 (1 + 2^10) — and
    anything below 3 (2 c ulp + ulp^2) - b 2^-10, about 5 |E|^2 here, drops the true neighbour."""
    rng = np.random.default_rng(3650 + OCTANTS.index(tuple(octant)))
    sgn = np.array(octant, dtype=np.float64)
    mp, qs = [], []
    for i in range(SLACK_DECIDERS):
        h = sgn * np.array([LIM - 10, LIM - 10 - 6 * i, LIM - 10])        # the home voxel's index
        centre = (h + 0.5 * sgn) * vs
        c = rng.uniform(1.25, 1.35) * vs
        q = np.array([_beside_a_midpoint(x, False) for x in centre])
        b = np.array([_beside_a_midpoint(x, True) for x in q + c])
        a = q - (b - q) * (1.0 + 1e-6)
        qs.append(np.r_[q, 40.0])
        mp += [np.r_[a, 40.0], np.r_[b, 40.0]]
    n = SLACK_DECIDERS
    return dict(map=np.ascontiguousarray(mp), queries=np.ascontiguousarray(qs), first=2 * np.arange(n),
                winner=2 * np.arange(n) + 1, max_dist=MAX_DIST_VOXELS * vs)


def filter_margin(q, a, b, vs, slack_factor=1.0):
    """the threshold of the fp32 filter of a lane that holds candidate a, minus the fp32 squared distance of candidate b
    (rows (n, 3), unscaled distances, real arithmetic on the fp32 roundings of the coordinates): negative where b is
    dropped.  slack_factor scales the slack |E|^2 (1 + 2^10) (1 + 1e-6) of icp_body.h."""
    q, a, b = (np.asarray(x, dtype=np.float64)[:, :3] for x in (q, a, b))
    d32 = ((b.astype(np.float32).astype(np.float64) - q.astype(np.float32).astype(np.float64)) ** 2).sum(axis=1)
    held = ((a - q) ** 2).sum(axis=1)
    e2 = ((4.0 * U32 * (np.abs(q) + 4.0 * vs)) ** 2).sum(axis=1)
    k = 1.0 + 1e-6
    return held * (1.0 + 2.0 ** -10) * k + slack_factor * e2 * (1.0 + 2.0 ** 10) * k - d32


RESIDENT_CASES = [(1.0, OCTANTS[0]), (1.0, OCTANTS[1]), (0.8, OCTANTS[2]), (0.8, OCTANTS[3])]
RESIDENT_KEEPS = ("whole", "half")


def resident_updates(vs, octant, keep):
    """Two map updates whose sensor origins lie at the world's origin and three voxels along x, away from the scene —
    1.8e6 voxels from the map they build.  -> max_distance, [(frame, pose, the frame in the world)] x 2
      1  corner's map points under the identity;
      2  corner's queries as a frame relative to the second origin, the pose a pure translation by it (the world points
         are fl(f + t): one rounding).
    keep = "whole": max_distance is the distance of the furthest map point, so update 1 keeps the whole map and update 2,
    from 1.7 voxels further away, evicts the voxels of the far corner; "half": the distance from the second origin to the
    scene's centre, so update 1 evicts a quarter of the voxels, update 2 fills them again and evicts half."""
    mp, q, c = corner(vs, octant)
    o2 = np.array([-octant[0] * 3.0 * vs, 0.0, 0.0])
    if keep == "whole":
        far = np.sqrt((mp[:, :3] ** 2).sum(axis=1)).max()
        md = np.nextafter(far, np.inf) * (1.0 + 1e-12)              # (RemovePointsFarFromLocation drops d^2 > max^2)
    else:
        assert keep == "half"
        md = float(np.linalg.norm(c - o2))
    f2 = q.copy()
    f2[:, :3] -= o2
    w2 = f2.copy()
    w2[:, :3] += o2
    ident = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    return md, [(mp, ident, mp), (np.ascontiguousarray(f2), np.r_[ident[:4], o2], np.ascontiguousarray(w2))]


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * W @ W


def planted_frame(vs, octant):
    """-> frame (2000, 4), guess (the identity), centre: 2000 points of corner's map with N(0, 0.03 vs) noise, moved by the
    inverse of the motion x -> R (x - c) + c + t about the scene's centre c, |t| = 1.5 voxels, |w| = 0.02 rad"""
    mp, _ = _local(vs, "int")
    rng = np.random.default_rng(36)
    pick = rng.choice(len(mp), size=FRAME_POINTS, replace=False)
    local = mp[pick, :3] + rng.normal(size=(FRAME_POINTS, 3)) * (0.03 * vs)
    R, t = rodrigues(FRAME_TWIST_W), np.array(FRAME_TWIST_T) * vs
    c = centre_of(vs, octant, 6)
    frame = np.c_[(local - t) @ R + c, mp[pick, 3]]                 # (row-wise R^T (x - t))
    return np.ascontiguousarray(frame), np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), c


# ---- plain restatements of the search (numpy; the host test holds them against the oracle) ---------------------------
def _sqnorm3(xx, yy, zz, order):
    """the association of the oracle's 3-term squared norm (oracle.SQNORM3_ORDER: 0 x + (y + z), 2 (x + y) + z)"""
    return xx + (yy + zz) if order == 0 else (xx + yy) + zz


def _int_of(l):
    """(int) of a label as the reference's build casts it: a value beyond int range becomes INT_MIN"""
    l = np.asarray(l, dtype=np.float64)
    inside = np.abs(l) < 2147483648.0
    return np.where(inside, np.trunc(np.where(inside, l, 0.0)), -2147483648.0).astype(np.int64)


def brute_force(stored, queries, vs, th, max_dist, dtype=np.float64, order=2, homes=None):
    """The reference's search, restated: for every query the stored points of the 27 voxels around its home voxel
    (`homes`, or trunc(fl(q / vs))) in the order of enumeration — x outermost, z innermost, a voxel's points as stored —,
    the squared distance, scaled by th where (int)l_a == (int)l_b or (int)(l_a l_b) == 0, the first minimum wins; accepted
    where the unscaled distance is below max_dist.  `dtype`: the type of the coordinates and of every distance.
    -> winner (n,) row of `stored` or -1, accepted (n,) bool"""
    stored = np.asarray(stored, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.float64)
    vox = voxel_of(stored, vs)
    cells = {}
    for i, v in enumerate(map(tuple, vox)):
        cells.setdefault(v, []).append(i)
    homes = voxel_of(queries, vs) if homes is None else np.asarray(homes, dtype=np.int64)
    P = stored[:, :3].astype(dtype)
    li = _int_of(stored[:, 3])
    win = np.full(len(queries), -1, dtype=np.int64)
    acc = np.zeros(len(queries), dtype=bool)
    thd = dtype(th)
    for qi, (q, hv) in enumerate(zip(queries, homes)):
        cand = []
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                for k in (-1, 0, 1):
                    cand.extend(cells.get((hv[0] + i, hv[1] + j, hv[2] + k), ()))
        if not cand:
            continue
        cand = np.array(cand)
        d = P[cand] - q[:3].astype(dtype)
        d2 = _sqnorm3(d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2], order)
        same = (li[cand] == _int_of(q[3])) | (_int_of(stored[cand, 3] * q[3]) == 0)
        w = int(np.argmin(np.where(same, d2 * thd, d2)))            # (argmin: the first of equal minima)
        win[qi] = cand[w]
        acc[qi] = np.sqrt(d2[w]) < dtype(max_dist)
    return win, acc
