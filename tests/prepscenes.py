"""Scenes for the device Preprocess / VoxelDownsample tests (csrc/preprocess.hip, csrc/prep.hip): inputs on which one wrong
keep/drop changes the output.  Every builder is seeded and returns the frame with its parameters (a Crop or a Vds), and
every builder checks on the CPU, against tests/prepref.py alone, that the wrong evaluation it targets (prepref's
variant=) gives a different output on at least MIN_DECIDING rows, or on every planted row where fewer are planted.  A
scene that cannot tell the wrong kernel from the right one is a bug here.  REPORT collects the counts
(tests/test_preprocess_host.py prints them).

crop_scenes() and vds_scenes() are the stand-alone scenes by name; refusal_scenes(), fallback(), pipeline_frames() and
hash_chain() have their own shapes."""
import functools
import itertools
from collections import namedtuple

import numpy as np

import prepref

Crop = namedtuple("Crop", "frame max_range min_range label_max_range")
Vds = namedtuple("Vds", "frame labels sizes scale")

MIN_DECIDING = 8
REPORT = {}         # scene name -> {variant or property: deciding rows}

KITTI_LABELS = [[40, 44, 48, 49], [50, 51, 52], [70, 72], [60, 71, 80, 81, 99], [0], [10, 11, 13, 15, 16, 18, 20]]
KITTI_SIZES = [0.6, 1.0, 0.9, 0.8, 1.0, 0.6]
RANGES = (100.0, 5.0, 50.0)         # max_range, min_range, label_max_range of the pipeline's defaults
UNLISTED = 77.0                     # a label of no group


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 4)


def crop_deciding(case, variant):
    """rows of the scene on which Preprocess under `variant` differs: kept by one only, or kept with another label"""
    a, ia = prepref.preprocess(*case, return_index=True)
    b, ib = prepref.preprocess(*case, variant=variant, return_index=True)
    both = np.intersect1d(ia, ib)
    la = a[np.searchsorted(ia, both), 3]
    lb = b[np.searchsorted(ib, both), 3]
    return len(np.setxor1d(ia, ib)) + int(np.count_nonzero(la != lb))


def vds_deciding(case, variant):
    """rows of the scene that survive under exactly one of VoxelDownsample and its `variant`"""
    _, ia = prepref.voxel_downsample(*case, return_index=True)
    _, ib = prepref.voxel_downsample(*case, variant=variant, return_index=True)
    return len(np.setxor1d(ia, ib))


def _record(name, what, count, minimum=MIN_DECIDING):
    assert count >= minimum, "%s does not decide %s: %d rows, %d needed" % (name, what, count, minimum)
    REPORT.setdefault(name, {})[what] = int(count)


# ---- threshold deciders -------------------------------------------------------------------------------------------------
def _signed_permutations(a, b, c, label):
    rows = set()
    for p in itertools.permutations((a, b, c)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            rows.add(tuple(s[k] * p[k] + 0.0 for k in range(3)))       # (+ 0.0: -0.0 and 0.0 are one row)
    return [list(r) + [label] for r in sorted(rows)]


def fixed_threshold_rows():
    """(3, 4, 0) -> 5, (30, 40, 0) -> 50, (60, 80, 0) -> 100 over the axes and signs: exactly ON the default thresholds in
    either association (the squares and their sums are small integers), so the strict comparisons drop them / keep
    their labels; plus rows whose squares overflow: their norm is Inf, they are dropped and not refused"""
    rows = _signed_permutations(3.0, 4.0, 0.0, 40.0) + _signed_permutations(30.0, 40.0, 0.0, 44.0) + \
        _signed_permutations(60.0, 80.0, 0.0, 50.0)
    rows += [[1e200, 1.0, 1.0, 40.0], [1.0, -1e200, 1.0, 40.0], [1.0, 1.0, 1e200, 40.0], [-1e200, 1e200, 1e200, 40.0],
             [1e155, 1e155, 0.0, 40.0]]
    return _c(rows)


def _street_points(rng, n):
    p = rng.normal(size=(n, 3)) * [30.0, 30.0, 2.0]
    return np.column_stack([p, rng.choice([40.0, 44.0, 50.0, 70.0, 10.0, 81.0], size=n)])


@functools.lru_cache(maxsize=None)
def crop_scenes(seed=101, calls_per_case=2):
    """Targets: the other association ("assoc"), the two FMA-contracted norms ("fma_full", "fma_outer"), and <= / >= at
    the three thresholds ("max_le", "min_ge", "label_ge").

    <variant>/<threshold>/<j>: a street-like row whose norm under the variant differs from the right one, in all eight
    sign combinations (the squares, hence every evaluation, are the same), with the threshold under test set to the
    row's RIGHT norm: the strict comparison then falls on the other side for the variant.  Around them the rows on the
    fixed thresholds, the overflowing rows and some ordinary rows.  A few rows per call, several calls.
    fixed: the default thresholds, deciding the three non-strict comparisons."""
    rng = np.random.default_rng(seed)
    cand = _street_points(rng, 4000)
    ref = prepref.crop_norm(cand)
    scenes = {}
    fixed = fixed_threshold_rows()
    case = Crop(np.ascontiguousarray(np.concatenate([fixed, _street_points(rng, 60)])[rng.permutation(len(fixed) + 60)]),
                *RANGES)
    for v in ("max_le", "min_ge", "label_ge"):
        _record("crop/fixed", v, crop_deciding(case, v))
    out = prepref.preprocess(*case)
    assert not np.any(np.abs(out[:, :3]) > 1e100), "an overflowing row was kept"
    scenes["crop/fixed"] = case
    signs = np.array(list(itertools.product((1.0, -1.0), repeat=3)))
    for variant in ("assoc", "fma_full", "fma_outer"):
        bad = prepref.crop_norm(cand, variant)
        ok = (ref > 8.0) & (ref < 90.0)
        lower, higher = np.flatnonzero(ok & (bad < ref)), np.flatnonzero(ok & (bad > ref))
        for which, pool in (("max", lower), ("min", higher), ("label_max", higher)):
            assert len(pool) >= calls_per_case, (variant, which, len(pool))
            for j in range(calls_per_case):
                i = pool[(7 * j + len(which)) % len(pool)]
                planted = np.column_stack([cand[i, :3] * signs, np.full(8, 40.0)])
                f = np.concatenate([planted, fixed, _street_points(rng, 40)])
                f = np.ascontiguousarray(f[rng.permutation(len(f))])
                r = float(ref[i])
                th = {"max": (r, RANGES[1], RANGES[2]), "min": (RANGES[0], r, RANGES[2]),
                      "label_max": (RANGES[0], RANGES[1], r)}[which]
                name = "crop/%s/%s/%d" % (variant, which, j)
                scenes[name] = Crop(f, *th)
                _record(name, variant, crop_deciding(scenes[name], variant))
    return scenes


# ---- voxel faces --------------------------------------------------------------------------------------------------------
def faces(seed, labels, sizes, scale, per_axis=100, k_max=3000):
    """Targets: "recip" (p * (1/vs)), "fp32" and "floor" voxel indices.

    Per label group and axis: rows at fl(k * vs), one ulp up and one ulp down, vs = size * scale, for k = 0, +-1, +-2,
    +-k_max and per_axis random k in +-[0, k_max]; +-0.0, denormals and +-(vs - ulp), all of cell 0 (which is two voxels
    wide); the other two coordinates sit inside cell 0.  A third of the rows have their mirror image -p in the same frame
    (another voxel unless k = 0).  Rows of one voxel collide, so an index that is off by one changes who survives."""
    rng = np.random.default_rng(seed)
    rows = []
    for ls, size in zip(labels, sizes):
        vs = size * scale
        for axis in range(3):
            ks = np.unique(np.concatenate([[0, 1, -1, 2, -2, k_max, -k_max], rng.integers(-k_max, k_max + 1, size=per_axis)]))
            x = ks.astype(np.float64) * vs
            tiny, small = 5e-324, 2.2250738585072014e-308
            vals = np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf),
                                   [0.0, -0.0, tiny, -tiny, small, -small, np.nextafter(vs, 0.0), -np.nextafter(vs, 0.0)]])
            p = np.empty((len(vals), 3))
            p[:] = [0.37 * vs, -0.21 * vs, 0.63 * vs]
            p[:, axis] = vals
            rows.append(np.column_stack([p, rng.choice(np.asarray(ls, dtype=np.float64), size=len(vals))]))
    f = np.concatenate(rows)
    mirrored = f[rng.random(len(f)) < 1.0 / 3.0].copy()
    mirrored[:, :3] *= -1.0
    f = np.concatenate([f, mirrored])
    return Vds(np.ascontiguousarray(f[rng.permutation(len(f))]), labels, sizes, scale)


def _cells(cells, vs, jitter=0.5):
    """a point well inside each voxel (ix, iy, iz) of a grid of size vs; cell 0 from its positive half"""
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    return (c + np.where(c < 0, -jitter, jitter)) * vs


# ---- labels -------------------------------------------------------------------------------------------------------------
def label_scenes(seed=303):
    """Targets: "label_round" (labels/trunc), and the group rules by construction (checked here by count)."""
    rng = np.random.default_rng(seed)
    scenes = {}
    # 40.99 -> 40, -0.9 -> 0, -40.5 -> -40, 39.999999999999 -> 39 (listed nowhere: dropped; rounded it would be 40)
    labs = [40.99, -0.9, -40.5, 39.999999999999, 40.0, 0.0, -40.0, float(2 ** 30), float(-2 ** 30), 2.0 ** 30 - 0.5]
    rows = [[*_cells([[i, j, 0]], 0.8)[0], l] for j, l in enumerate(labs) for i in range(4)]
    case = Vds(_c(rows)[rng.permutation(len(rows))], [[40, 2 ** 30], [0], [-40, -2 ** 30, 2 ** 30 - 1]], [0.8, 0.8, 0.8], 1.0)
    _record("labels/trunc", "label_round", vds_deciding(case, "label_round"))
    assert len(prepref.voxel_downsample(*case)) == 4 * 9        # all but the 39.99... rows
    scenes["labels/trunc"] = case
    # a label listed in two groups with different sizes: the first group wins (1.0: rows 0.3 apart collide; 0.1: none would)
    rows = [[0.05 + 0.3 * i, 0.05, 0.05, 40.0] for i in range(40)] + [[0.05 + 0.3 * i, 0.05, 0.05, 50.0] for i in range(40)]
    case = Vds(_c(rows), [[40], [50, 40], [50]], [1.0, 0.1, 1.0], 1.0)
    out = prepref.voxel_downsample(*case)
    assert np.count_nonzero(out[:, 3] == 40.0) == 12 and np.count_nonzero(out[:, 3] == 50.0) == 40
    _record("labels/first_group", "rows the second listing would keep", 40 - 12)
    scenes["labels/first_group"] = case
    # the same voxel coordinates occupied in all 8 groups, every row twice: 8 survivors, the first of each
    rows = [[1.25 + 0.01 * r, -2.25, 3.25, 100.0 + g] for r in range(2) for g in range(8)]
    case = Vds(_c(rows), [[100 + g] for g in range(8)], [1.0] * 8, 1.0)
    out = prepref.voxel_downsample(*case)
    assert len(out) == 8 and np.all(out[:, 0] == 1.25)
    _record("labels/eight_groups", "survivors", 8)
    scenes["labels/eight_groups"] = case
    # no groups: everything is dropped
    case = Vds(_c(_street_points(rng, 300)), [], [], 1.0)
    assert len(prepref.voxel_downsample(*case)) == 0
    scenes["labels/no_groups"] = case
    # one group with 64 labels, eight groups with one label each: listed and unlisted labels mixed
    many = list(range(200, 264))
    f = _street_points(rng, 600)
    f[:, 3] = rng.choice(many + [199, 264, 0], size=len(f))
    scenes["labels/sixty_four"] = Vds(_c(f), [many], [0.7], 1.0)
    f = _street_points(rng, 600)
    f[:, 3] = rng.choice(many[:10], size=len(f))
    scenes["labels/eight_single"] = Vds(_c(f), [[l] for l in many[:8]], [0.3 + 0.1 * g for g in range(8)], 0.5)
    for name in ("labels/sixty_four", "labels/eight_single"):
        out = prepref.voxel_downsample(*scenes[name])
        assert 0 < len(out) < 600
    return scenes


# ---- key range ----------------------------------------------------------------------------------------------------------
def _key_range_rows():
    edge = {-2 ** 19: -524288.0, 0: 0.25, 2 ** 19 - 1: 524287.5}
    rows = []
    for g in range(8):
        for ix, iy, iz in itertools.product(edge, repeat=3):
            for r in range(2):      # every row twice; the copy differs in the label's fraction (truncated away)
                rows.append([edge[ix], edge[iy], edge[iz], 100.0 + g + 0.25 * r])
    return rows


def key_range(seed=404):
    """Targets: a key whose 20-bit fields alias at +-2^19.  vs = 1, all 27 combinations of the voxel indices -2^19, 0 and
    2^19 - 1 in each of 8 groups, every row twice: 216 survivors, the first of each pair."""
    rng = np.random.default_rng(seed)
    rows = _c(_key_range_rows())
    order = rng.permutation(len(rows))
    case = Vds(np.ascontiguousarray(rows[order]), [[100 + g] for g in range(8)], [1.0] * 8, 1.0)
    assert len(prepref.voxel_downsample(*case)) == 216
    _record("range/edges", "survivors", 216)
    _record("range/edges", "last_wins", vds_deciding(case, "last_wins"))
    return case


def refusal_scenes():
    """[(name, refused Vds, error name, clean Vds)]: one more row at voxel index 2^19 on each axis in turn refuses the whole
    call; the same call without that row is correct"""
    clean = key_range()
    out = []
    for axis in range(3):
        row = [0.25, 0.25, 0.25, 103.0]
        row[axis] = 524288.0
        bad = Vds(np.ascontiguousarray(np.concatenate([clean.frame[:200], _c(row), clean.frame[200:]])), *clean[1:])
        try:
            prepref.voxel_downsample(*bad)
            raise AssertionError("index 2^19 on axis %d is not refused" % axis)
        except prepref.Refused as e:
            assert e.code == "ERR_CAPACITY"
        out.append(("range/beyond/%d" % axis, bad, "ERR_CAPACITY", clean))
    return out


# ---- contention ---------------------------------------------------------------------------------------------------------
def contention(n=200000, layout="late", seed=505):
    """Targets: "last_wins" — a winner that is the last writer, or any writer but the lowest index.

    All contended rows fall into 3 voxels of 2 groups; the other rows carry a label of no group.
    late: the first three quarters of the frame are such rows, so each voxel's lowest index sits at a position >= 3n/4,
      among shuffled rows of all three voxels (on the device: in workgroups that start late).
    first_and_last: voxel A's survivor is row 0, everything else of the three voxels is in the last workgroup (256 rows)."""
    rng = np.random.default_rng(seed)
    labels, sizes = [[40], [50]], [1.0, 2.0]
    corners = np.array([[3.0, 0.0, 0.0], [-3.0, 1.0, 0.0], [0.0, 0.0, 2.0]])       # voxel A, B (group 0), C (group 1)
    spans = np.array([[1.0, 1.0, 1.0], [-1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
    lab = np.array([40.0, 40.0, 50.0])
    m = n - (3 * n) // 4 if layout == "late" else min(n - 1, 256 if n % 256 == 0 else n % 256)
    which = rng.integers(0, 3, size=m)
    which[:3] = rng.permutation(3)
    hot = np.column_stack([corners[which] + spans[which] * rng.uniform(0.05, 0.95, size=(m, 3)), lab[which]])
    fill = np.column_stack([rng.normal(size=(n - m, 3)) * 20.0, np.full(n - m, UNLISTED)])
    if layout == "late":
        f = np.concatenate([fill, hot])
        assert len(fill) == (3 * n) // 4
    else:
        first = np.array([[3.5, 0.5, 0.5, 40.0]])
        f = np.concatenate([first, fill[: n - m - 1], hot])
    case = Vds(np.ascontiguousarray(f), labels, sizes, 1.0)
    out, idx = prepref.voxel_downsample(*case, return_index=True)
    assert len(out) == 3
    if layout == "late":
        assert idx.min() >= (3 * n) // 4
    else:
        assert idx[0] == 0 and np.all(idx[1:] >= n - m)
    name = "contention/%s/%d" % (layout, n)
    _record(name, "last_wins", vds_deciding(case, "last_wins") // 2, minimum=3)     # every planted voxel decides
    return case


def sizes_scene(n, keep, seed=606):
    """n rows around the 256-row workgroup and the 65,536 boundary, with all rows kept (each in a voxel of its own), none
    kept (no label listed) or only the last row kept: the survivor count (k_vds_count) at its edges"""
    rng = np.random.default_rng(seed + n)
    i = np.arange(n)
    cells = np.column_stack([i % 61 - 30, (i // 61) % 61 - 30, i // 3721 - 9])
    f = np.column_stack([_cells(cells, 1.0, jitter=0.25) + rng.uniform(0.0, 0.5, size=(n, 3)) * np.where(cells < 0, -1.0, 1.0),
                         np.full(n, 40.0)])
    f = f[rng.permutation(n)]
    if keep == "none":
        f[:, 3] = UNLISTED
    elif keep == "last":
        f[:-1, 3] = UNLISTED
    case = Vds(np.ascontiguousarray(f), [[40]], [1.0], 1.0)
    assert len(prepref.voxel_downsample(*case)) == {"all": n, "none": 0, "last": 1}[keep]
    return case


SIZES = (1, 255, 256, 257, 65537)
KEEPS = ("all", "none", "last")


# ---- hash chains in the device table ------------------------------------------------------------------------------------
def mix64(k):
    """csrc/preprocess.hip mix64, restated: the low 32 bits of the finalised key"""
    k = np.asarray(k, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    return k & np.uint64(0xFFFFFFFF)


def table_size(n):
    """csrc/prep.hip Prep::reserve, restated: c = n + n/4 + 1024 rows; the smallest power of two >= 1024 that is >= 2c"""
    c = n + n // 4 + 1024
    t = 1024
    while t < 2 * c:
        t <<= 1
    return t


def device_key(group, cells):
    c = np.asarray(cells, dtype=np.int64) + (1 << 19)
    return (np.uint64(group) << np.uint64(60)) | (c[:, 0].astype(np.uint64) << np.uint64(40)) | \
        (c[:, 1].astype(np.uint64) << np.uint64(20)) | c[:, 2].astype(np.uint64)


def hash_chain(n=1000, seed=707, want=300):
    """Targets: a probe that does not wrap at the end of the device table, and a claim that loses a key on a long chain.

    THIS PINS TODAY'S HASH AND SIZING (mix64 and Prep::reserve, restated above; a stand-alone call owns a fresh Prep, so
    the mask is a function of n).  >= `want` distinct voxels whose home slot is mask - 2, each offered twice, shuffled,
    padded to n rows with rows of no group: the chain runs over the last slot and wraps to slot 0.  One survivor per
    voxel, the first.  If the product changes its hash or its sizing, the self-check below fails — not the product: the
    device result is compared with prepref either way.  Returns (Vds, chain length)."""
    rng = np.random.default_rng(seed)
    mask = table_size(n) - 1
    found = np.zeros((0, 3), dtype=np.int64)
    for _ in range(12):
        cells = np.column_stack([rng.integers(-2000, 2000, size=1 << 20), rng.integers(-2000, 2000, size=1 << 20),
                                 rng.integers(-50, 50, size=1 << 20)])
        home = mix64(device_key(0, cells)) & np.uint64(mask)
        found = np.unique(np.concatenate([found, cells[home == np.uint64(mask - 2)]]), axis=0)
        if len(found) >= min(n // 2, want + 100):
            break
    found = found[rng.permutation(len(found))[: n // 2]]
    k = len(found)
    assert k >= want, "only %d voxels home at mask - 2" % k
    assert np.all(mix64(device_key(0, found)) & np.uint64(mask) == np.uint64(mask - 2)), "the restated hash disagrees with itself"
    assert k > 3, "the chain does not reach past the last slot"
    twice = np.concatenate([found, found])
    p = _cells(twice, 1.0, jitter=0.25) + rng.uniform(0.0, 0.5, size=(2 * k, 3)) * np.where(twice < 0, -1.0, 1.0)
    rows = np.column_stack([p, np.full(2 * k, 40.0)])
    fill = np.column_stack([rng.normal(size=(n - 2 * k, 3)) * 20.0, np.full(n - 2 * k, UNLISTED)])
    f = np.concatenate([rows, fill])
    case = Vds(np.ascontiguousarray(f[rng.permutation(n)]), [[40]], [1.0], 1.0)
    assert len(case.frame) == n and len(prepref.voxel_downsample(*case)) == k
    _record("chain/%d" % n, "chain length (slots %d..%d, then 0..%d)" % (mask - 2, mask, k - 4), k, minimum=want)
    _record("chain/%d" % n, "last_wins", vds_deciding(case, "last_wins"))
    return case, k


# ---- the order replay's fall-back ---------------------------------------------------------------------------------------
def reference_voxel_hash(cells):
    """core/VoxelHashMap.hpp:72-77, restated: 20 bits of the three products' xor (uint32 arithmetic)"""
    c = np.asarray(cells, dtype=np.int64) & 0xFFFFFFFF
    h = (c[:, 0] * 73856093) ^ (c[:, 1] * 19349663) ^ (c[:, 2] * 83492791)
    return h & ((1 << 20) - 1)


def fallback(seed=808, n_a=300, n_b=3000, target=0x5A5A5):
    """Targets: the arrival-order fall-back of the emission-order replay (include/sageicp.h, sageicp_robin_iteration_order:
    a probe distance of 128 is not modelled).  Group A (label 40, vs = 0.01): n_a voxels with ONE 20-bit VoxelHash —
    vz = 0, vx random, vy solved from vy * 19349663 = target ^ vx * 73856093 (mod 2^20) with the modular inverse and
    mapped into [-2^19, 2^19); a third of them offered twice.  Group B (label 50, vs = 0.6): an ordinary cloud of ~2,000
    voxels.  Returns (Vds, mask of group A's rows)."""
    rng = np.random.default_rng(seed)
    m = 1 << 20
    vx = rng.choice(np.arange(-(1 << 19), 1 << 19), size=n_a, replace=False).astype(np.int64)
    vy = ((target ^ ((vx * 73856093) & (m - 1))) * pow(19349663, -1, m)) & (m - 1)
    vy = np.where(vy >= (1 << 19), vy - m, vy)
    cells = np.column_stack([vx, vy, np.zeros(n_a, dtype=np.int64)])
    assert np.all(reference_voxel_hash(cells) == target) and len(np.unique(cells, axis=0)) == n_a
    again = cells[rng.random(n_a) < 1.0 / 3.0]
    a = np.column_stack([np.concatenate([_cells(cells, 0.01), _cells(again, 0.01, jitter=0.25)]),
                         np.full(n_a + len(again), 40.0)])
    b = np.column_stack([rng.normal(size=(n_b, 3)) * [12.0, 12.0, 1.0], np.full(n_b, 50.0)])
    # the two groups interleaved at random, each in its own order (group A's first offers stay ahead of their repeats)
    f = np.empty((len(a) + len(b), 4))
    slots = rng.permutation(len(f))
    sa, sb = np.sort(slots[: len(a)]), slots[len(a):]
    f[sa], f[sb] = a, b
    is_a = np.zeros(len(f), dtype=bool)
    is_a[sa] = True
    case = Vds(np.ascontiguousarray(f), [[40], [50]], [0.01, 0.6], 1.0)
    out = prepref.voxel_downsample(*case)
    assert np.count_nonzero(out[:, 3] == 40.0) == n_a and 1500 < np.count_nonzero(out[:, 3] == 50.0) < n_b
    assert np.all(np.abs(f[:, :3]) < 5300.0)
    _record("fallback", "voxels of one VoxelHash", n_a, minimum=129)
    return case, is_a


# ---- the stand-alone scenes by name -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vds_scenes(contention_n=200000):
    scenes = {}
    for name, args in (("faces/0.5", (201, KITTI_LABELS, KITTI_SIZES, 0.5)), ("faces/1.5", (202, KITTI_LABELS, KITTI_SIZES, 1.5)),
                       ("faces/awkward", (203, [[40], [50]], [1.0 / 3.0, 0.7], 1.0))):
        scenes[name] = faces(*args)
        for v in ("recip", "fp32", "floor"):
            _record(name, v, vds_deciding(scenes[name], v))
    scenes.update(label_scenes())
    scenes["range/edges"] = key_range()
    for layout in ("late", "first_and_last"):
        scenes["contention/" + layout] = contention(contention_n, layout)
    for n in SIZES:
        for keep in KEEPS:
            scenes["sizes/%d/%s" % (n, keep)] = sizes_scene(n, keep)
    scenes["chain"] = hash_chain()[0]
    scenes["fallback"] = fallback()[0]
    return scenes


# scenes that also run in the reference's emission order (faces, labels, range)
REFERENCE_ORDER_SCENES = ("faces/0.5", "faces/1.5", "faces/awkward", "labels/trunc", "labels/first_group",
                          "labels/eight_groups", "labels/no_groups", "labels/sixty_four", "labels/eight_single", "range/edges")


# ---- the pipeline's fused first level -----------------------------------------------------------------------------------
def _pipeline_plants(rng, full, on_thresholds=True):
    """rows for a street frame (all above it, z >= 6 m, so that only planted rows share their voxels):
      * the rows exactly on 5 / 50 / 100 m (fixed_threshold_rows, without the overflowing ones);
      * face rows of the six KITTI groups at both levels' voxel sizes, inside 5..45 m (labels kept);
      * pairs beyond 50 m: a row of label 0 and, later, a row of label 40 in the same 0.5 m voxel.  Zeroed, the second is of
        group [0] and loses to the first; looked up by its label before zeroing it would be of group [40, ...] (0.3 m
        voxels), survive level 0 ahead of the first (group-major emission) and take the first's place in the source."""
    rows = [r for r in fixed_threshold_rows().tolist() if max(abs(v) for v in r[:3]) < 1e100] if on_thresholds else []
    n_k, n_pairs = (12, 12) if full else (1, 2)
    for g, (ls, size) in enumerate(zip(KITTI_LABELS, KITTI_SIZES)):
        for scale in (0.5, 1.5):
            vs = size * scale
            ks = rng.integers(int(8.0 / vs) + 1, int(40.0 / vs), size=n_k)
            for k in ks.tolist():
                x = float(k) * vs
                for v in (x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)):
                    rows.append([v, 0.2 * vs, 6.0 + g + 0.1 * vs, float(ls[0])])
                    rows.append([0.2 * vs, -v, 6.0 + g + 0.1 * vs, float(ls[-1])])
    for j in range(n_pairs):
        x = 60.05 + 2.0 * j
        rows.append([x, 3.05, 14.05, 0.0])
        rows.append([x + 0.35, 3.05, 14.05, 40.0])        # another 0.3 m voxel, the same 0.5 m voxel
    return _c(rows)


@functools.lru_cache(maxsize=None)
def pipeline_frames(seed=909, sizes=(30000, 300, 45000, 2000)):
    """Targets (through the pipeline's fused crop + level 0, then level 1): "max_le", "min_ge", "label_ge", "recip", "fp32"
    and "stale_label".  Consecutive street frames of one synthetic stream (so that registration converges), cut to
    `sizes` rows, each with planted rows inserted at random positions in their order; then the first frame again.
    Returns (frames, ranges, labels, sizes).  The two big frames carry the full set of planted rows and must decide."""
    from sage_icp_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    stream, _ = syn.make_stream(seed, len(sizes), points_per_frame=max(sizes))
    frames = []
    for k, (f, n) in enumerate(zip(stream, sizes)):
        full = n >= 30000
        plants = _pipeline_plants(rng, full, on_thresholds=n >= 1000)      # (the 300-row frame stays mostly street)
        body = np.asarray(f, dtype=np.float64)[np.sort(rng.choice(len(f), size=n - len(plants), replace=False))]
        out = np.empty((n, 4))
        at = np.sort(rng.choice(n, size=len(plants), replace=False))
        rest = np.ones(n, dtype=bool)
        rest[at] = False
        out[at], out[rest] = plants, body
        frames.append(np.ascontiguousarray(out))
        if full:
            name = "pipeline/%d" % k
            ref = prepref.chain(out, *RANGES, KITTI_LABELS, KITTI_SIZES)
            assert len(ref) > 100
            for v in ("max_le", "min_ge", "label_ge", "recip", "fp32", "stale_label"):
                bad = prepref.chain(out, *RANGES, KITTI_LABELS, KITTI_SIZES, variant=v)
                a = {r.tobytes() for r in ref}
                b = {r.tobytes() for r in bad}
                _record(name, v, len(a ^ b))
    for f in frames:
        assert len(prepref.chain(f, *RANGES, KITTI_LABELS, KITTI_SIZES)) > 0, "a frame whose source would be empty"
    frames.append(frames[0])
    return frames, RANGES, KITTI_LABELS, KITTI_SIZES
