"""Adversarial scenes for the device-side VoxelHashMap::Update (csrc/map_update.hip), for the tests only.

test_map_update_device.py feeds the update uniformly random clouds; these families aim at what that leaves to chance:
runs of equal voxels placed against the 256-position LDS stage of k_up_heads / k_up_insert, counts that land exactly on
the size-class boundaries, hash chains with tombstones in them that wrap around the table, a table rebuilt because of
tombstones alone, and the edges of the key and label domain.

Every scene is deterministic, voxel_size = 1.  A scene is a dict:
  name, params (voxel_size, max_distance, basic, critical), passes [(points, pose, refused)],
  check(pass index, Pointcloud()) -> asserts what the scene rests on from the PRODUCT's map (optional),
  table {pass index: "same" | "grown"}, tombstones [pass indices after which the device table must hold some],
  queries {pass index: (n, 4) rows} for the searches of scene c, extra: rows for a closing AddPoints(),
  new_voxels [voxels each pass opens] (scene d), chain (keys of box 1, of box 2, held back) (scene c).

Points sit at voxel centres in x and y; in z the centre carries a tag (pass * 701 + position in the run) / 16384, exact
in binary and below half a voxel, so that every point of a voxel is distinguishable and a wrong replacement or a wrong
order inside a block shows in the bytes."""
import functools
from collections import Counter

import numpy as np

import mapref

U, B1, B2, C1, C2, C3 = 0.0, 40.0, 44.0, 71.0, 80.0, 99.0      # unlabelled, basic-part (default list), critical
IDENTITY_Q = (0.0, 0.0, 0.0, 1.0)


def pose_at(x, y=0.0, z=0.0):
    return np.array(IDENTITY_Q + (float(x), float(y), float(z)))


def _centre(v):
    return v + 0.5 if v >= 0 else v - 0.5


def frame_from_runs(runs, origin=(0.0, 0.0, 0.0), pno=0, seed=1):
    """runs: [(voxel, labels of its points in arrival order)].  The points of different voxels are interleaved by a
    fixed permutation, each voxel's own points keep their order (the device's sort must be stable); the rows are in
    the sensor frame of a pose that is the translation `origin`."""
    runs = [r for r in runs if len(r[1])]
    ids = np.repeat(np.arange(len(runs)), [len(l) for _, l in runs])
    ids = ids[np.random.default_rng(seed).permutation(len(ids))]
    nxt = [0] * len(runs)
    rows = []
    for r in ids.tolist():
        (vx, vy, vz), labels = runs[r]
        j = nxt[r]
        nxt[r] += 1
        assert j <= 700 and pno <= 10
        tag = (pno * 701 + j) / 16384.0
        z = _centre(vz) + (tag if vz >= 0 else -tag)
        rows.append((_centre(vx) - origin[0], _centre(vy) - origin[1], z - origin[2], labels[j]))
    return np.array(rows, dtype=np.float64).reshape(-1, 4)


def make_map(sage, s):
    """the product's map with the scene's parameters"""
    p = s["params"]
    return sage.VoxelHashMap(p["voxel_size"], p["max_distance"], basic_points_per_voxel=p["basic"],
                             critical_points_per_voxel=p["critical"])


def voxels_of(cloud):
    """voxel of every row of a map's Pointcloud() (voxel_size 1: truncation toward zero)"""
    return [tuple(int(v) for v in row[:3]) for row in np.asarray(cloud).reshape(-1, 4).tolist()]


def sorted_run_lengths(points, pose):
    """the run lengths the device sees after its stable sort by (x, y, z) of the voxel"""
    keys = [(int(p[0]), int(p[1]), int(p[2])) for p in mapref.transform(pose, points)]
    out, last = [], None
    for k in sorted(keys):
        if k == last:
            out[-1] += 1
        else:
            out.append(1)
            last = k
    return out


def _scene(name, md, basic, critical, passes, **more):
    s = dict(name=name, params=dict(voxel_size=1.0, max_distance=float(md), basic=basic, critical=critical),
             passes=[(np.ascontiguousarray(p[0]), np.asarray(p[1], dtype=np.float64), bool(p[2]) if len(p) > 2 else False)
                     for p in passes],
             check=None, table={}, tombstones=[], queries={}, extra=None)
    s.update(more)
    assert len(s["passes"]) <= 25 and all(len(p[0]) <= 20000 for p in s["passes"])
    return s


# ---- a. runs against the 256-position stage ---------------------------------------------------------------------------
LAYOUTS = ([255, 1, 1, 255], [255, 2], [200, 100, 212], [256, 256], [1, 600, 1], [513], [1], [255], [256])
STAGE_CAPS = ((20, 20), (3, 2))
_TAIL = (C1, B1, C2, U, B2, C3, C1, C2)


def stage_scene(layout, basic, critical):
    """voxels along +x, so the sorted layout is the list itself.  A run that crosses a multiple of 256 is unlabelled
    up to it — the part its head finds staged in LDS — and carries the critical and basic-part labels behind it: the
    head's final count (k_up_heads) and every insert / replace decision (k_up_insert) then rest on labels read from
    memory.  Three passes: the fresh path, the same geometry with each run's labels rotated by a third (existing
    voxels: moves and replacements), and the first labels again."""
    runs, start = [], 0
    for r, n in enumerate(layout):
        boundary = (start // 256 + 1) * 256
        crosses = start + n > boundary
        labels = [U if (crosses and start + j < boundary) else _TAIL[(j + r) % len(_TAIL)] for j in range(n)]
        runs.append(((10 + r, 3, 3), labels))
        start += n
    rot = [(v, l[len(l) // 3:] + l[:len(l) // 3]) for v, l in runs]
    origins = ((0.0, 0.0, 0.0), (2.0, -1.0, 0.0), (0.0, 0.0, 0.0))
    passes = [(frame_from_runs(rr, o, pno, seed=7 + pno), pose_at(*o))
              for pno, (rr, o) in enumerate(zip((runs, rot, runs), origins))]
    for pts, pose in passes:
        assert sorted_run_lengths(pts, pose) == list(layout) and len(pts) == sum(layout)
    name = "a_%s_%d_%d" % ("_".join(map(str, layout)), basic, critical)
    return _scene(name, 1e4, basic, critical, passes)


# ---- b. size-class boundaries -----------------------------------------------------------------------------------------
CLASS_CAPS = ((20, 20), (10, 7), (8, 8), (2, 2), (1, 0), (0, 4), (200, 55))


def class_sizes(cap):
    """HostMap::configure: 4 / 8 / 16 below the capacity, then the capacity rounded up to whole units"""
    return [s for s in (4, 8, 16) if s < cap] + [(cap + 3) // 4 * 4]


def class_of(count, sizes):
    return next(k for k, s in enumerate(sizes) if count <= s)


def labels_to(c_from, c_to, basic, critical, salt=0):
    """labels that take a voxel from c_from points (0: a new voxel) to exactly c_to, with points that must NOT be
    appended mixed in wherever the policy has any: below `basic` every point is taken; from there on only a critical
    label appends, unlabelled points are dropped and basic-part labels replace"""
    cap, out, c, k = basic + critical, [], c_from, salt
    mix = (U, B1, C1, B2, C2, U, C3)
    while c < c_to:
        if c == 0 or c < basic:
            out.append(mix[k % 7])
        else:
            if k % 3 == 0:
                out.append(U)
            elif k % 3 == 1:
                out.append(B1)
            out.append((C1, C2, C3)[k % 3])
        k += 1
        c += 1
    if c > 0 and c >= basic:
        out += [U, B2]
        if c == cap:
            out.append(C2)          # a full voxel: a critical label replaces too
    return out


def class_scene(basic, critical):
    cap = basic + critical
    sizes = class_sizes(cap)
    S = sorted({v for v in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, cap - 1, cap) if 1 <= v <= cap})
    at_basic = max(basic, 1)
    # (labels of pass 1, labels of pass 2, count after 1, count after 2)
    vox = [(labels_to(0, a, basic, critical, i), labels_to(a, b, basic, critical, i + 3), a, b)
           for i, (a, b) in enumerate((a, b) for a in S for b in S if a <= b)]
    vox.append((labels_to(0, at_basic, basic, critical), [U, U, U], at_basic, at_basic))          # appends nothing
    vox.append(([U] * at_basic, [B1, B2, B1], at_basic, at_basic))                                   # only replaces
    vox.append(([U] * at_basic + [C1] * (cap - at_basic), [C2, B1, C3, U], cap, cap))                # ... at the capacity
    # two clusters, alternately; B goes in pass 3
    key = lambda p: ((0 if p % 2 == 0 else 1000) + (p // 2) % 16, (p // 2) // 16, 1)
    mid, home = (508.0, 0.0, 0.0), (8.0, 0.0, 0.0)
    expected = []
    count = {}
    p1 = [(key(p), v[0]) for p, v in enumerate(vox)]
    count.update({key(p): v[2] for p, v in enumerate(vox)})
    expected.append(dict(count))
    p2 = [(key(p), v[1]) for p, v in enumerate(vox)]
    count.update({key(p): v[3] for p, v in enumerate(vox)})
    expected.append(dict(count))
    # pass 3: two new voxels next to A; the origin moves onto A and cluster B is evicted
    p3 = [((0, 40, 1), [U]), ((1, 40, 1), [C1])]
    ever = Counter()                 # regions of class k that can lie on its free stack by pass 4, at most
    for v in vox:
        for k in {class_of(v[2], sizes), class_of(v[3], sizes)}:
            ever[k] += 1
    count = {k: c for k, c in count.items() if k[0] < 500}
    count.update({(0, 40, 1): 1, (1, 40, 1): 1})
    expected.append(dict(count))
    # pass 4: more new voxels of every class than its stack can hold, at the class's first and last count, plus every
    # surviving voxel grown into the next class (its region is released by the move)
    p4, i = [], 0
    for k, s in enumerate(sizes):
        lo, hi = (sizes[k - 1] + 1 if k else 1), min(s, cap)
        for j in range(ever[k] + 2):
            c = hi if (j % 8 == 7 if k == len(sizes) - 1 and hi > 40 else j % 2) else lo
            kk = (i % 16, 50 + i // 16, 1)
            p4.append((kk, labels_to(0, c, basic, critical, i)))
            count[kk] = c
            i += 1
    for kk, c in sorted(count.items()):
        if kk[1] < 50 and c < cap:
            k = class_of(c, sizes)
            t = min(cap, sizes[k] + 1) if k + 1 < len(sizes) else cap
            p4.append((kk, labels_to(c, t, basic, critical, c)))
            count[kk] = t
    expected.append(dict(count))
    # pass 5: new voxels of the classes the moves of pass 4 released
    p5 = []
    for k, s in enumerate(sizes):
        lo, hi = (sizes[k - 1] + 1 if k else 1), min(s, cap)
        for j, c in enumerate((lo, hi, (lo + hi) // 2)):
            kk = (3 * k + j, 90, 1)
            p5.append((kk, labels_to(0, c, basic, critical, j)))
            count[kk] = c
    expected.append(dict(count))
    passes = [(frame_from_runs(r, o, pno, seed=20 + pno), pose_at(*o))
              for pno, (r, o) in enumerate(((p1, mid), (p2, mid), (p3, home), (p4, home), (p5, home)))]

    def check(k, cloud):
        got = Counter(voxels_of(cloud))
        assert dict(got) == expected[k], "pass %d: the counts the scene aims at were not reached" % (k + 1)

    extra = frame_from_runs([((j, 2 * j % 7, 1), [C1, U, B1]) for j in range(0, 16)] + [((j, 95, 2), [U, C2]) for j in range(40)],
                            pno=6, seed=3)
    return _scene("b_%d_%d" % (basic, critical), 700.0, basic, critical, passes, check=check, extra=extra)


# ---- c. hash chains ---------------------------------------------------------------------------------------------------
BOXES = ((1, 200), (3001, 3200))
_COLLIDING = {}


def colliding_keys(sage):
    """{low 16 bits: (keys of box 1, keys of box 2)} for 0xFFFF and 0xFFFE, the hash read from the product
    (sageicp_voxel_hash).  A key whose hash ends in sixteen ones has the LAST slot as its home in every table of up to
    65,536 slots, so these keys form one probe chain that wraps to slot 0; the 0xFFFE keys start one slot earlier and
    run into it."""
    if not _COLLIDING:
        h = sage.lib().sageicp_voxel_hash
        found = {0xFFFF: ([], []), 0xFFFE: ([], [])}
        for b, (x0, x1) in enumerate(BOXES):
            for x in range(x0, x1 + 1):
                for y in range(1, 201):
                    for z in range(1, 51):
                        low = h(x, y, z) & 0xFFFF
                        if low >= 0xFFFE:
                            found[low][b].append((x, y, z))
        _COLLIDING.update(found)
    return _COLLIDING


def chain_scene(sage, lows):
    ck = colliding_keys(sage)
    box1, box2 = [], []
    for low in lows:
        a, b = ck[low]
        assert len(a) >= 12 and len(b) >= 12, "fewer than 12 keys ending in %#x per box: %d, %d" % (low, len(a), len(b))
        assert all(sage.voxel_hash(*k) & 0xFFFF == low for k in a + b)
        box1 += a
        box2 += b
    held = box1[-2:] + box2[-2:]                 # opened in pass 3 only: they claim a slot behind tombstones
    box1, box2 = box1[:-2], box2[:-2]
    inter = [k for pair in zip(box1, box2) for k in pair] + box1[len(box2):] + box2[len(box1):]
    mid, near1 = (1600.0, 100.0, 25.0), (-600.0, 100.0, 25.0)
    more = 1 if len(lows) > 1 else 3             # (pass 3 must stay below the load that rebuilds the table)
    lab = (U, C1, B1, U, C2, U, B2)
    p1 = [(k, [lab[i % 7]]) for i, k in enumerate(inter)]
    p2 = [((5, 5, 5), [U])]                      # origin beyond box 1: box 2, every second link, is out of range
    back = box2[:2]
    p3 = [(k, [lab[(i + j) % 7] for j in range(more)]) for i, k in enumerate(box1)] + \
         [(k, [C1, U]) for k in held] + [(k, [B1]) for k in back]
    fill = [((1600 + i % 20, 300 + i // 20, 5), [lab[i % 7]]) for i in range(250)]
    p5 = [(k, [C2, U, C3][:1 + i % 3]) for i, k in enumerate(box1 + held + back)]
    p6 = [((6, 5, 5), [C1])]
    p7 = [(k, [C3, B2]) for k in box1 + held[:2]] + [(k, [U]) for k in box2[2:6]]
    plan = ((p1, mid), (p2, near1), (p3, mid), (fill, mid), (p5, mid), (p6, near1), (p7, mid))
    passes = [(frame_from_runs(r, o, pno, seed=40 + pno), pose_at(*o)) for pno, (r, o) in enumerate(plan)]
    assert len(p1) * 4 <= 1024 and (len(p1) + sum(len(l) for _, l in p3) + 1) * 4 <= 1024
    n_live = len(inter) + 1 + len(held) + len(back) + len(fill)
    assert n_live + max(len(p[0]) for p in passes) < 16384

    # queries in and around the chain voxels: the 27 positions 0.9 of a voxel around each centre
    allk = box1 + box2 + held
    offs = [(dx, dy, dz) for dx in (-0.9, 0.0, 0.9) for dy in (-0.9, 0.0, 0.9) for dz in (-0.9, 0.0, 0.9)]
    q = [(k[0] + 0.5 + o[0], k[1] + 0.5 + o[1], k[2] + 0.55 + o[2], (U, C1, B1, C2)[(i + j) % 4])
         for i, k in enumerate(allk) for j, o in enumerate(offs)]
    q = np.array(q[:2000], dtype=np.float64)
    return _scene("c_" + "_".join("%x" % l for l in lows), 2500.0, 3, 2, passes,
                  table={0: "same", 1: "same", 2: "same", 3: "grown"}, tombstones=[1, 2], queries={1: q, 2: q, 3: q, 6: q}, chain=(box1, box2, held),
                  extra=frame_from_runs([(k, [C1, B1]) for k in box1[:8] + box2[6:12]], pno=8, seed=5))


# ---- d. a table rebuilt because of tombstones alone -------------------------------------------------------------------
def tombstone_scene():
    """twenty passes of 300 new one-point voxels, 40 voxels further along x each time, the eviction radius such that a
    pass evicts about what it inserts: ~300 live voxels while the used slots climb by 300 a pass"""
    lab = (U, C1, B1, U, C2)
    passes = []
    for k in range(20):
        runs = [((40 * k + i % 40, i // 40, 0), [lab[(i + k) % 5]]) for i in range(300)]
        if k % 3 == 2:      # ... and points for voxels of the pass before that are still in range
            runs += [((40 * (k - 1) + 35 + i % 5, i // 5, 0), [C1, lab[i % 5]]) for i in range(35)]
        o = (40.0 * k + 20.0, 0.0, 0.0)
        passes.append((frame_from_runs(runs, o, pno=k % 6, seed=60 + k), pose_at(*o)))
    extra = frame_from_runs([((40 * 19 + i, 9, 0), [C1, U]) for i in range(60)], pno=6, seed=9)
    return _scene("d_tombstones", 30.0, 3, 2, passes, extra=extra, new_voxels=[300] * 20)


# ---- e. edges of the key and label domain -----------------------------------------------------------------------------
EDGE = 1048575.5                   # voxel index 2^20 - 1, exact in fp64


def key_edge_scene():
    ok = [(sx * EDGE if a == 0 else 0.5, sx * EDGE if a == 1 else 0.5, sx * EDGE if a == 2 else 0.5, C1)
          for a in range(3) for sx in (1.0, -1.0)] + [(EDGE, -EDGE, EDGE, U), (-EDGE, -EDGE, -EDGE, B1)]
    ok = np.array(ok + ok[:3])                                            # (three of them take a second point)
    bad = [np.array([(0.5, 0.5, 0.5, C1), tuple(s * 1048576.0 if a == j else 0.5 for j in range(3)) + (C2,)])
           for a in range(3) for s in (1.0, -1.0)]
    passes = [(ok, pose_at(0, 0, 0))] + [(b, pose_at(0, 0, 0), True) for b in bad] + \
             [(np.array([(2.5, 0.5, 0.5, U)]), pose_at(0, 0, 0))]

    def check(k, cloud):
        if k == 0:
            v = set(voxels_of(cloud))
            lim = (1 << 20) - 1
            assert {(lim, 0, 0), (-lim, 0, 0), (0, lim, 0), (0, -lim, 0), (0, 0, lim), (0, 0, -lim)} <= v

    return _scene("e_key_edges", 1e7, 3, 2, passes, check=check)


def voxel_zero_scene():
    """400 points in (-1, 1)^3: truncation toward zero makes voxel (0, 0, 0) two voxels wide on every axis"""
    rng = np.random.default_rng(70)
    p = rng.uniform(-1.0, 1.0, size=(400, 4))
    p[:, :3] = np.round(p[:, :3] * 4096) / 4096
    p[np.abs(p[:, :3]).max(axis=1) >= 1.0, :3] = 0.25
    p[::50, 0] = -0.0
    p[1::50, 1] = -0.0
    p[2::50, :3] = (-0.0, -0.0, -0.0)
    p[:, 3] = np.array(_TAIL + (U, U, U))[np.arange(400) % 11]
    assert sorted_run_lengths(p, pose_at(0, 0, 0)) == [400]
    return _scene("e_voxel_zero", 100.0, 20, 20, [(p, pose_at(0, 0, 0)), (p[::-1].copy(), pose_at(0, 0, 0))])


ODD_LABELS = (0.5, -0.7, 40.9, -3.0, 296.0, 2147483647.0)


def odd_label_scene():
    """labels that are fractional (0.5 and -0.7 truncate to 0: unlabelled; 40.9 to 40: a basic part), negative or
    beyond a byte (critical), into voxels that are full or filling: the cast to int is made in three places on the
    device (the staged code, the label read from memory, the search for the first unlabelled point)"""
    runs = []
    for v in range(12):
        fill = [U] * (3 + v % 3)                       # at `basic` or beyond it, all unlabelled
        odd = [ODD_LABELS[(v + j) % 6] for j in range(9)]
        runs.append(((v, 2, 2), fill + odd))
    long = [ODD_LABELS[j % 6] if j % 5 else U for j in range(300)]      # crosses the stage with such labels behind it
    runs.append(((40, 2, 2), long))
    o = (3.0, 0.0, 0.0)
    again = [(v, l[::-1]) for v, l in runs]
    passes = [(frame_from_runs(runs, o, 0, seed=80), pose_at(*o)), (frame_from_runs(again, o, 1, seed=81), pose_at(*o))]
    return _scene("e_odd_labels", 1e4, 3, 2, passes)


def face_scene():
    """a rotation with nine non-zero entries and 2,000 points p = R^T (f - t), f on integer voxel faces: the
    transformed points land within an ulp of the faces, where the voxel is decided by the last bit of R p + t"""
    rng = np.random.default_rng(90)
    q = np.array([0.31, -0.47, 0.22, 0.79])
    q /= np.linalg.norm(q)
    t = np.array([3.25, -7.5, 1.125])
    R = np.array(mapref.quat_to_mat(q)).reshape(3, 3)
    assert np.all(R != 0.0)
    f = rng.uniform(-12, 12, size=(2000, 3))
    on = rng.integers(0, 7, size=2000)                 # which axes sit on a face: one, two or all three
    for a in range(3):
        m = ((on + 1) >> a) & 1 == 1
        f[m, a] = np.round(f[m, a])
    p = np.column_stack([(f - t) @ R, np.array((U, C1, B1, C2, U))[np.arange(2000) % 5]])
    pose = np.concatenate([q, t])
    w = np.array(mapref.transform(pose, p))[:, :3]
    near = np.abs(w - np.round(w)) < 1e-12
    assert near.any(axis=1).sum() >= 1500              # the points did land on (or an ulp off) the faces
    return _scene("e_faces", 1e4, 3, 2, [(p, pose), (p[::-1].copy(), pose)])


# ---- registry ---------------------------------------------------------------------------------------------------------
def _lname(layout):
    return "_".join(map(str, layout))


STAGE_NAMES = ["a_%s_%d_%d" % (_lname(l), b, c) for l in LAYOUTS for b, c in STAGE_CAPS]
CLASS_NAMES = ["b_%d_%d" % bc for bc in CLASS_CAPS]
CHAIN_NAMES = ["c_ffff", "c_fffe_ffff"]
EDGE_NAMES = ["e_key_edges", "e_voxel_zero", "e_odd_labels", "e_faces"]
ALL_NAMES = STAGE_NAMES + CLASS_NAMES + CHAIN_NAMES + ["d_tombstones"] + EDGE_NAMES


@functools.lru_cache(maxsize=None)
def _build(name, sage):
    if name.startswith("a_"):
        for l in LAYOUTS:
            for b, c in STAGE_CAPS:
                if name == "a_%s_%d_%d" % (_lname(l), b, c):
                    return stage_scene(l, b, c)
    if name.startswith("b_"):
        b, c = (int(v) for v in name.split("_")[1:])
        return class_scene(b, c)
    if name == "c_ffff":
        return chain_scene(sage, (0xFFFF,))
    if name == "c_fffe_ffff":
        return chain_scene(sage, (0xFFFE, 0xFFFF))
    return dict(d_tombstones=tombstone_scene, e_key_edges=key_edge_scene, e_voxel_zero=voxel_zero_scene,
                e_odd_labels=odd_label_scene, e_faces=face_scene)[name]()


def scene(name, sage):
    """the scene (built once per session; `sage`: the product package, whose hash scene c reads)"""
    return _build(name, sage)


@functools.lru_cache(maxsize=None)
def reference(name, sage):
    """tests/mapref.py run over the scene, once: per pass (Pointcloud() rows, size, voxels, refused).  Shared by the
    host and the device tests; the arrays are read-only."""
    s = scene(name, sage)
    m = mapref.MapRef(**s["params"])
    out = []
    for pts, pose, refused in s["passes"]:
        try:
            m.update(pts, pose)
            was = False
        except mapref.RefusedUpdate:
            was = True
        assert was == refused, "the restatement and the scene disagree on whether this frame is refused"
        cloud = m.pointcloud()
        cloud.setflags(write=False)
        out.append((cloud, m.size(), m.num_voxels(), was))
    return tuple(out)
