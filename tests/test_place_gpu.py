"""Place recognition on the device (sageicp_place_*, csrc/place.hip).  Needs a real MI355X:
python -m pytest tests -m gpu

Everything is compared as bytes with the independent restatement (tests/placeref.py), which reads the library's two
tables and decides every edge case itself: the descriptor at shapes that leave a partial last word and wave, at every
ring edge and sector boundary, at the z and class edges; the matcher against three nested loops with Python integers;
recognition on the periodic street scene; the loop closed through Relocalize; and the pipeline against a host replay."""
import math

import numpy as np
import pytest
import torch

import placeref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LARGEST = (64, 256)          # rings * sectors == 16384, the most the library takes
SHAPES = [(1, 3), (20, 60), (7, 61), (45, 360), LARGEST]
# the street scene's ranks: 0 for unlabelled and moving classes, ground and everything else 1, then what tells places apart
STREET_RANK = {c: 1 for c in range(1, 256)}
STREET_RANK.update({10: 0, 70: 2, 51: 3, 50: 4, 71: 5, 80: 6, 81: 6})
LABELS = np.array([0, 10, 40, 44, 48, 72, 70, 51, 50, 71, 80, 81, 99, 255])


def _params(sage, R=20, S=60, rank=None, **kw):
    return sage.place_params(rings=R, sectors=S, rank=STREET_RANK if rank is None else rank, **kw)


def _cloud(rng, n, reach=55.0):
    f = np.empty((n, 4))
    r = rng.uniform(0.0, reach, n)
    a = rng.uniform(-np.pi, np.pi, n)
    f[:, 0], f[:, 1] = r * np.cos(a), r * np.sin(a)
    f[:, 2] = rng.uniform(-5.0, 9.0, n)
    f[:, 3] = rng.choice(LABELS, n)
    return f


def _same_planes(sage, rows, params, tables=None):
    tables = tables if tables is not None else sage.place_tables(params)
    ref = placeref.describe(rows, params, tables)
    got = sage.place_describe(rows, params)
    assert got[0].dtype == np.uint8 and got[0].shape == (params.rings, params.sectors)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    return ref


# ---- the descriptor ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", SHAPES)
def test_descriptor_matches_the_restatement(gpu_sage, R, S):
    p = _params(gpu_sage, R, S)
    tables = gpu_sage.place_tables(p)
    rng = np.random.default_rng(R * 1000 + S)
    for n in (0, 1, 63, 64, 65, 5000):
        ref = _same_planes(gpu_sage, _cloud(rng, n), p, tables)
        if n == 0:
            assert not ref[0].any() and not ref[1].any()
    assert ref[0].any() and (ref[1][ref[0] > 0] > 0).all()
    if R * S >= 1200:
        assert (ref[0][-1] > 0).any() and (ref[0][:, -1] > 0).any()        # the last ring and the last sector are drawn


def test_a_frame_of_many_workgroups_merges_through_memory(gpu_sage):
    p = _params(gpu_sage, 20, 60)
    rows = _cloud(np.random.default_rng(5), 300000)
    ref = _same_planes(gpu_sage, rows, p)
    assert (ref[0] > 0).all()
    # any order of the rows gives the same bytes
    again = gpu_sage.place_describe(rows[::-1].copy(), p)
    assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])


def ring_edge_rows(edge2, e_of_k, ks):
    """rows whose x * x + y * y lies one ulp below, at and one ulp above edge2[k]: x is the edge (or the double below it),
    y * y a few ulps of edge2[k]"""
    rows, wanted = [], []
    for k in ks:
        e, t = e_of_k[k], edge2[k]
        ulp = np.spacing(t)
        for x in (np.nextafter(e, 0.0), e):
            for j in range(0, 12):
                y = np.sqrt(j * ulp)
                rows.append([x, y, 0.0, 40.0])
                rows.append([-y, -x, 0.0, 40.0])
        wanted.append((k, np.nextafter(t, 0.0), t, np.nextafter(t, np.inf)))
    return np.array(rows), wanted


@pytest.mark.parametrize("R,S,lo,hi", [(20, 60, 3.0, 50.0), (7, 61, 0.7, 33.1), (1, 3, 3.0, 50.0)])
def test_ring_edges(gpu_sage, R, S, lo, hi):
    p = _params(gpu_sage, R, S, min_range=lo, max_range=hi)
    tables = gpu_sage.place_tables(p)
    edge2 = tables[0]
    e_of_k = np.float64(lo) + np.arange(R + 1, dtype=np.float64) * ((np.float64(hi) - np.float64(lo)) / np.float64(R))
    assert np.array_equal(e_of_k * e_of_k, edge2)
    ks = sorted({0, 1, R // 2, R - 1, R} & set(range(R + 1)))
    rows, wanted = ring_edge_rows(edge2, e_of_k, ks)
    r2 = rows[:, 0] * rows[:, 0] + rows[:, 1] * rows[:, 1]
    # one row per descriptor: the restatement decides, and the device must agree row by row
    _, _, kept, ring, _ = placeref.describe(rows, p, tables, return_kept=True)
    ring_of = dict(zip(kept.tolist(), ring.tolist()))
    for k, below, at, above in wanted:
        for v, inside in ((below, k - 1), (at, k), (above, k)):
            hit = np.flatnonzero(r2 == v)
            assert len(hit), "no row lands on this side of edge %d" % k
            for i in hit:
                want = inside if 0 <= inside < R else None       # below the first edge and from the last on: ignored
                assert ring_of.get(int(i)) == want
    _same_planes(gpu_sage, rows, p, tables)
    for i in np.flatnonzero(np.isin(r2, [v for w in wanted for v in w[1:]])):
        h, _ = gpu_sage.place_describe(rows[i:i + 1], p)
        got = np.flatnonzero(h.any(axis=1))
        assert got.tolist() == ([ring_of[int(i)]] if int(i) in ring_of else [])


def sector_boundary_rows(dirs, scale=8.0):
    rows = []
    for s in range(len(dirs)):
        x, y = dirs[s, 0] * scale, dirs[s, 1] * scale
        for yy in (y, np.nextafter(y, -np.inf), np.nextafter(y, np.inf)):
            rows.append([x, yy, 1.0, 40.0])
        for xx in (np.nextafter(x, -np.inf), np.nextafter(x, np.inf)):
            rows.append([xx, y, 1.0, 40.0])
    return np.array(rows)


@pytest.mark.parametrize("S", [3, 4, 60, 61, 360])
def test_sector_boundaries_and_axes(gpu_sage, S):
    p = _params(gpu_sage, 2, S)
    tables = gpu_sage.place_tables(p)
    rows = sector_boundary_rows(tables[1])
    axes = np.array([[10.0, 0.0, 0.0, 40.0], [-10.0, 0.0, 0.0, 40.0], [0.0, 10.0, 0.0, 40.0], [0.0, -10.0, 0.0, 40.0],
                     [10.0, -0.0, 0.0, 40.0], [-10.0, -0.0, 0.0, 40.0], [-0.0, 10.0, 0.0, 40.0]])
    rows = np.concatenate([rows, axes])
    _, _, kept, _, sector = placeref.describe(rows, p, tables, return_kept=True)
    assert len(kept) == len(rows)
    # a row on dir[s] lies in sector s; one ulp to the side it falls into s - 1 for some rows: both sides are populated
    on = sector[0:5 * S:5]
    assert np.array_equal(on, np.arange(S))
    moved = sector[:5 * S].reshape(S, 5)
    assert ((moved == np.arange(S)[:, None]).sum(axis=1) >= 2).all()
    assert ((moved == ((np.arange(S) - 1) % S)[:, None]).sum(axis=1) >= 1).all()
    assert sector[5 * S] == 0 and sector[5 * S + 4] == 0
    _same_planes(gpu_sage, rows, p, tables)
    for i in range(0, len(rows), max(1, len(rows) // 300)):      # row by row: a cell shared with a neighbour hides nothing
        h, _ = gpu_sage.place_describe(rows[i:i + 1], p)
        assert np.flatnonzero(h.any(axis=0)).tolist() == [int(sector[i])]


def test_heights_classes_and_ranks(gpu_sage):
    rank = {0: 2, 3: 1, 40: 1, 44: 1, 80: 6, 255: 5}
    p = _params(gpu_sage, 4, 16, rank=rank, z_lo=-3.0, z_hi=7.0)
    tables = gpu_sage.place_tables(p)

    def at(sector, ring=1, r=None):
        a = (sector + 0.5) * 2 * np.pi / 16
        r = r if r is not None else 3.0 + (ring + 0.5) * (47.0 / 4)
        return [r * np.cos(a), r * np.sin(a)]

    zs = [-4.0, -3.0, np.nextafter(-3.0, -np.inf), np.nextafter(-3.0, np.inf), 2.0, np.nextafter(7.0, 0.0), 7.0,
          np.nextafter(7.0, np.inf), 8.0, -3.0 + 10.0 / 254, np.nextafter(-3.0 + 10.0 / 254, -np.inf)]
    rows = [at(s) + [z, 40.0] for s, z in enumerate(zs)]
    h, c = _same_planes(gpu_sage, np.array(rows), p, tables)
    assert h[1, 0] == 1 and h[1, 1] == 1 and h[1, 2] == 1 and h[1, 6] == 255 and h[1, 7] == 255 and h[1, 8] == 255
    assert h[1, 4] == 1 + math.floor(0.5 * 254.0) and (c[1, :len(zs)] == 40).all()
    # labels: truncated toward zero; outside 0 .. 255 and rank 0 are ignored
    labels = [255.0, 256.0, -1.0, 3.9, -0.5, -0.999, 255.9, 1.0, 41.0, float("nan"), float("inf"), 1e300, -1e300]
    rows = [at(s, ring=2) + [0.0, l] for s, l in enumerate(labels)]
    h, c = _same_planes(gpu_sage, np.array(rows), p, tables)
    assert c[2, :13].tolist() == [255, 0, 0, 3, 0, 0, 255, 0, 0, 0, 0, 0, 0]
    assert (h[2, :13] > 0).tolist() == [True, False, False, True, True, True, True] + [False] * 6
    # two classes of equal rank in one cell: the higher class number; a higher rank at a lower height: both planes keep
    # their own maximum
    rows = [at(0, ring=3) + [0.0, 40.0], at(0, ring=3) + [0.0, 44.0], at(0, ring=3) + [0.0, 40.0],
            at(1, ring=3) + [-2.0, 80.0], at(1, ring=3) + [5.0, 40.0],
            at(2, ring=3) + [5.0, 0.0], at(2, ring=3) + [1.0, 3.0]]
    h, c = _same_planes(gpu_sage, np.array(rows), p, tables)
    assert c[3, 0] == 44 and c[3, 1] == 80 and c[3, 2] == 0
    assert h[3, 1] == 1 + math.floor((8.0 / 10.0) * 254.0) and h[3, 2] == h[3, 1]


def test_forms_of_a_frame_give_the_same_bytes(gpu_sage):
    p = _params(gpu_sage, 7, 61)
    f = _cloud(np.random.default_rng(23), 40000)
    f[:, :3] = f[:, :3].astype(np.float32).astype(np.float64)
    want = _same_planes(gpu_sage, f, p)
    t32 = torch.from_numpy(f.astype(np.float32)).to(DEV)
    got = gpu_sage.place_describe(t32, p)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    wide = torch.zeros((len(f), 6), dtype=torch.float64, device=DEV)       # strided rows, labels apart
    wide[:, :3] = torch.from_numpy(f[:, :3]).to(DEV)
    wide[:, 3] = 99.0
    for dt in (np.int32, np.int64, np.uint8):
        lab = torch.from_numpy(f[:, 3].astype(dt)).to(DEV)
        got = gpu_sage.place_describe(wide, p, labels=lab)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    empty = gpu_sage.place_describe(t32[:0], p)
    assert not empty[0].any() and not empty[1].any()
    torch.cuda.synchronize()


def test_non_finite_coordinates_are_refused(gpu_sage):
    p = _params(gpu_sage)
    f = _cloud(np.random.default_rng(29), 3000)
    for bad, col in ((np.nan, 0), (np.inf, 1), (-np.inf, 2)):
        g = f.copy()
        g[1500, col] = bad
        for frame in (g, torch.from_numpy(g).to(DEV), torch.from_numpy(g.astype(np.float32)).to(DEV)):
            with pytest.raises(gpu_sage.SageIcpError) as e:
                gpu_sage.place_describe(frame, p)
            assert e.value.code == gpu_sage.ERR_INVALID
    _same_planes(gpu_sage, f, p)


# ---- the matcher -------------------------------------------------------------------------------------------------------
def _random_desc(rng, R, S, fill=0.5):
    h = rng.integers(1, 256, size=(R, S)).astype(np.uint8)
    h[rng.random((R, S)) >= fill] = 0
    c = rng.choice(np.array([40, 44, 50, 70, 71, 80], dtype=np.uint8), size=(R, S))
    return h, c


def _roll(desc, k):
    """the descriptor a sensor turned so that it sees the entry's sector s + k in its own sector s"""
    return np.roll(desc[0], -k, axis=1), np.roll(desc[1], -k, axis=1)


def _db(sage, params, entries, tags=None, poses=None):
    db = sage.PlaceDB(params)
    for i, e in enumerate(entries):
        assert db.add(e, tag=tags[i] if tags is not None else 0, pose=poses[i] if poses is not None else None) == i
    assert len(db) == len(entries)
    return db


def _both(db, entries, desc, tags=None, poses=None, **q):
    got = db.match(desc, **q)
    ref = placeref.match(entries, desc, tags=tags, poses=poses, **q)
    placeref.same(got, ref)
    return got


@pytest.mark.parametrize("R,S,N", [(20, 60, 1), (20, 60, 63), (20, 60, 65), (20, 60, 1000), (7, 61, 1), (7, 61, 63),
                                   (7, 61, 65), (45, 360, 5), (64, 256, 3)])
def test_a_rolled_copy_finds_its_entry(gpu_sage, R, S, N):
    p = _params(gpu_sage, R, S)
    rng = np.random.default_rng(N * 7 + S)
    entries = [_random_desc(rng, R, S) for _ in range(N)]
    tags = [1000 + 3 * i for i in range(N)]
    poses = [np.concatenate([[0, 0, math.sin(0.1 * i), math.cos(0.1 * i)], rng.uniform(-9, 9, 3)]) for i in range(N)]
    db = _db(gpu_sage, p, entries, tags, poses)
    planted, roll = N // 2, (7 if S < 100 else 201)
    query = _roll(entries[planted], roll)
    got = _both(db, entries, query, tags, poses, top_k=16 if N == 1000 else 5, h_tol=3)
    assert got[0]["index"] == planted and got[0]["tag"] == tags[planted]
    assert got[0]["agree"] == got[0]["n_query"] == got[0]["n_entry"] and got[0]["similarity"] == 1.0
    assert got[0]["shift"] == roll != S - roll          # the direction: the entry's sector s + shift is the query's sector s
    assert np.array_equal(query[0][:, 0], entries[planted][0][:, roll])
    assert len(got) == min(16 if N == 1000 else 5, N)
    if N > 1:
        assert got[1]["similarity"] < 0.5
    # the other direction is another answer
    back = db.match(_roll(entries[planted], -roll), top_k=1, h_tol=3)
    assert back[0]["index"] == planted and back[0]["shift"] == S - roll


def test_ties_constant_descriptors_and_tolerance(gpu_sage):
    R, S = 20, 60
    p = _params(gpu_sage, R, S)
    rng = np.random.default_rng(31)
    twin = _random_desc(rng, R, S)
    entries = [_random_desc(rng, R, S), twin, _random_desc(rng, R, S), twin]
    db = _db(gpu_sage, p, entries)
    got = _both(db, entries, _roll(twin, 11), top_k=4)
    assert got["index"].tolist()[:2] == [1, 3] and got["shift"].tolist()[:2] == [11, 11]
    # constant along the sectors: every shift agrees alike, the smallest is reported
    ring = (np.repeat(np.arange(1, R + 1, dtype=np.uint8)[:, None] * 9, S, axis=1), np.full((R, S), 50, dtype=np.uint8))
    entries = [ring]
    db = _db(gpu_sage, p, entries)
    got = _both(db, entries, ring, top_k=1)
    assert got[0]["shift"] == 0 and got[0]["agree"] == R * S
    # a height difference of exactly h_tol agrees, of h_tol + 1 does not
    base = (np.full((R, S), 100, dtype=np.uint8), np.full((R, S), 40, dtype=np.uint8))
    q = (base[0].copy(), base[1].copy())
    q[0][:, :30] = 117                                   # + 17
    q[0][:, 30:] = 82                                    # - 18
    db = _db(gpu_sage, p, [base])
    for tol, agree in ((16, 0), (17, R * 30), (18, R * S), (255, R * S), (0, 0)):
        got = _both(db, [base], q, top_k=1, h_tol=tol)
        assert got[0]["agree"] == agree
    # near the ends of the byte: 1 against 255 differ by 254
    lo = (np.full((R, S), 1, dtype=np.uint8), base[1])
    hi = (np.full((R, S), 255, dtype=np.uint8), base[1])
    db = _db(gpu_sage, p, [hi])
    assert _both(db, [hi], lo, h_tol=253)[0]["agree"] == 0 and _both(db, [hi], lo, h_tol=254)[0]["agree"] == R * S
    # the class must be equal even where the heights are
    other = (base[0], np.full((R, S), 41, dtype=np.uint8))
    assert _both(_db(gpu_sage, p, [base]), [base], other, h_tol=255)[0]["agree"] == 0


def test_empty_descriptors_exclusion_top_k_and_threshold(gpu_sage):
    R, S = 7, 61
    p = _params(gpu_sage, R, S)
    rng = np.random.default_rng(37)
    N = 9
    entries = [_random_desc(rng, R, S, fill=0.1 + 0.1 * i) for i in range(N)]
    empty = (np.zeros((R, S), dtype=np.uint8), np.full((R, S), 40, dtype=np.uint8))
    entries[N - 1] = empty
    db = _db(gpu_sage, p, entries)
    # an empty query: every similarity is 0 (0 / 0 counts as 0 for the empty entry), the order is the index
    got = _both(db, entries, empty, top_k=16)
    assert len(got) == N and got["index"].tolist() == list(range(N)) and not got["similarity"].any()
    # an empty entry among the others comes last
    query = _roll(entries[6], 5)
    got = _both(db, entries, query, top_k=16, h_tol=2)
    assert len(got) == N and got[0]["index"] == 6 and got[-1]["index"] == N - 1 and got[-1]["n_entry"] == 0
    for ex, n in ((0, N), (2, N - 2), (3, N - 3), (N - 1, 1), (N, 0), (N + 5, 0)):
        got = _both(db, entries, query, top_k=16, h_tol=2, exclude_last=ex)
        assert len(got) == n and (n == 0 or got["index"].max() == N - ex - 1)
        assert (len(got) > 0 and got[0]["index"] == 6) == (ex <= 2)
    assert len(_both(db, entries, query, top_k=1, h_tol=2)) == 1
    assert len(_both(db, entries, query, top_k=3, h_tol=2)) == 3
    # min_similarity cuts the list in the middle
    full = db.match(query, top_k=16, h_tol=2)
    cut = float(full[3]["similarity"])
    assert full[2]["similarity"] > cut or full[4]["similarity"] < cut
    got = _both(db, entries, query, top_k=16, h_tol=2, min_similarity=cut)
    assert 0 < len(got) < N and (got["similarity"] >= cut).all() and len(got) == int((full["similarity"] >= cut).sum())
    assert len(_both(db, entries, query, top_k=16, h_tol=2, min_similarity=np.nextafter(1.0, 2.0))) == 0
    for bad in (dict(top_k=0), dict(top_k=17), dict(h_tol=256), dict(min_similarity=float("nan"))):
        with pytest.raises(gpu_sage.SageIcpError) as e:
            db.match(query, **bad)
        assert e.value.code == gpu_sage.ERR_INVALID


def test_the_ratio_ranks_not_the_count(gpu_sage):
    R, S = 20, 60
    p = _params(gpu_sage, R, S)
    steps = (1 + 4 * np.arange(S)).astype(np.uint8)      # distinct along a ring: only shift 0 agrees

    def desc(cells_per_ring, cls):
        h, c = np.zeros((R, S), dtype=np.uint8), np.zeros((R, S), dtype=np.uint8)
        for r, (n, k) in enumerate(zip(cells_per_ring, cls)):
            h[r, :n] = steps[:n]
            c[r, :n] = k
        return h, c

    query = desc([40], [5])
    a = desc([40, 35, 25], [5, 9, 9])                    # 100 cells, 30 of them the query's
    a[1][0, 30:40] = 6
    b = desc([40], [5])                                  # 40 cells, 20 of them the query's
    b[1][0, 20:40] = 6
    entries = [a, b]
    got = _both(_db(gpu_sage, p, entries), entries, query, top_k=2)
    assert got["agree"].tolist() == [20, 30] and got["index"].tolist() == [1, 0]
    assert (got["n_entry"].tolist(), got["n_query"].tolist()) == ([40, 100], [40, 40])
    assert got["similarity"].tolist() == [20 / 40, 30 / 100]


def test_growth_read_and_a_round_trip(gpu_sage):
    R, S = 7, 61
    p = _params(gpu_sage, R, S)
    rng = np.random.default_rng(41)
    N = 150                                              # across the first two doublings of 64 entries
    entries = [_random_desc(rng, R, S) for _ in range(N)]
    tags = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    poses = rng.normal(size=(N, 7))
    db = gpu_sage.PlaceDB(p)
    for i, e in enumerate(entries):
        db.add(e, tag=int(tags[i]), pose=poses[i])
        if i in (63, 64, 65, 127, 128, 149):
            d, t, ps = db.read()
            assert len(d) == i + 1 and np.array_equal(d, np.array(entries[:i + 1]))
            assert np.array_equal(t, tags[:i + 1]) and ps.tobytes() == poses[:i + 1].tobytes()
    d, t, ps = db.read(60, 10)
    assert np.array_equal(d, np.array(entries[60:70])) and np.array_equal(t, tags[60:70])
    with pytest.raises(gpu_sage.SageIcpError):
        db.read(100, 51)
    # save and load: a second database built from what read() gave answers alike
    loaded = gpu_sage.PlaceDB(p)
    d, t, ps = db.read()
    for i in range(N):
        loaded.add(d[i], tag=int(t[i]), pose=ps[i])
    for k in (0, 70, 149):
        query = _roll(entries[k], 13)
        a, b = db.match(query, top_k=16, h_tol=4), loaded.match(query, top_k=16, h_tol=4)
        assert a.tobytes() == b.tobytes() and a[0]["index"] == k and a[0]["tag"] == tags[k]
        assert np.array_equal(a[0]["pose"], poses[k])
    placeref.same(db.match(_roll(entries[70], 13), top_k=3), placeref.match(entries, _roll(entries[70], 13), top_k=3,
                                                                         tags=tags, poses=poses))
    db.clear()
    assert len(db) == 0 and len(db.match(query, top_k=16)) == 0
    db.add(entries[3])
    assert len(db) == 1 and db.match(_roll(entries[3], 2))[0]["shift"] == 2


@pytest.mark.parametrize("R,S", [(20, 60), (7, 61), (3, 130)])
def test_both_entry_layouts_give_the_same_answers(gpu_sage, monkeypatch, R, S):
    """the scoring pass holds an entry once in LDS and wraps the sector index (the default) or holds it twice along S
    (SAGEICP_PLACE_DOUBLED=1): the same records, and the restatement's"""
    p = _params(gpu_sage, R, S)
    rng = np.random.default_rng(S)
    entries = [_random_desc(rng, R, S) for _ in range(20)]
    db = _db(gpu_sage, p, entries)
    query = _roll(entries[11], S - 1)
    got = {}
    for doubled in ("0", "1"):
        monkeypatch.setenv("SAGEICP_PLACE_DOUBLED", doubled)
        got[doubled] = _both(db, entries, query, top_k=16, h_tol=9)
        assert got[doubled][0]["index"] == 11 and got[doubled][0]["shift"] == S - 1
    assert got["0"].tobytes() == got["1"].tobytes()


# ---- recognition on the street scene -----------------------------------------------------------------------------------
class Street:
    """17 places along the periodic street, and queries at a place seen before (turned) and at places never seen"""
    H_TOL = 40
    PLACES = [(-64.0 + 8.0 * i, 1.0) for i in range(17)]
    REVISITS = [((8.3, 0.8), 90.0, (0.4, -0.3)), ((7.8, 1.3), 137.0, (-0.5, 0.6))]       # xy, yaw, (roll, pitch) in degrees
    UNVISITED = [(8.0, 41.0), (30.0, -95.0)]

    def __init__(self, sage):
        from sage_icp_amd import synthetic as syn
        self.syn = syn
        self.p = _params(sage)
        self.tables = sage.place_tables(self.p)
        rng = np.random.default_rng(2024)
        self.poses = [syn.pose_from_rpy_t([0, 0, 0], [x, y, 0.0]) for x, y in self.PLACES]
        self.scans = [syn.make_scan(rng, 8000, 120.0, T) for T in self.poses]
        self.entries = [placeref.describe(s, self.p, self.tables) for s in self.scans]
        self.q_poses = [syn.pose_from_rpy_t([rp[0], rp[1], yaw], [xy[0], xy[1], 0.0]) for xy, yaw, rp in self.REVISITS]
        self.q_poses += [syn.pose_from_rpy_t([0, 0, 30.0], [x, y, 0.0]) for x, y in self.UNVISITED]
        self.q_scans = [syn.make_scan(rng, 8000, 120.0, T) for T in self.q_poses]
        self.queries = [placeref.describe(s, self.p, self.tables) for s in self.q_scans]
        self.ref = [placeref.match(self.entries, q, top_k=3, h_tol=self.H_TOL, tags=list(range(17)), poses=self.poses)
                    for q in self.queries]


@pytest.fixture(scope="module")
def street(gpu_sage):
    return Street(gpu_sage)


def test_a_revisit_is_recognised_and_a_new_place_is_not(gpu_sage, street):
    s = street
    w = 360.0 / s.p.sectors
    for (xy, yaw, _), ref in zip(s.REVISITS, s.ref[:2]):
        print("revisit yaw %.0f: top %d sim %.3f runner-up %.3f shift %d" %
              (yaw, ref[0]["index"], ref[0]["similarity"], ref[1]["similarity"], ref[0]["shift"]))
        assert ref[0]["index"] == 9                      # (8, 1)
        assert ref[0]["similarity"] - ref[1]["similarity"] >= 0.03
        assert abs(ref[0]["shift"] * w - yaw) <= w       # within one sector of the true yaw
    for xy, ref in zip(s.UNVISITED, s.ref[2:]):
        print("unvisited %s: best sim %.3f" % (xy, ref[0]["similarity"]))
        assert ref[0]["similarity"] < 0.4
    assert min(r[0]["similarity"] for r in s.ref[:2]) > 0.4
    # the device: descriptors byte for byte, answers exactly
    db = gpu_sage.PlaceDB(s.p)
    for i, (scan, e) in enumerate(zip(s.scans, s.entries)):
        d = gpu_sage.place_describe(scan, s.p)
        assert np.array_equal(d[0], e[0]) and np.array_equal(d[1], e[1])
        db.add(d, tag=i, pose=s.poses[i])
    for scan, q, ref in zip(s.q_scans, s.queries, s.ref):
        d = gpu_sage.place_describe(torch.from_numpy(scan).to(DEV), s.p)
        assert np.array_equal(d[0], q[0]) and np.array_equal(d[1], q[1])
        placeref.same(db.match(d, top_k=3, h_tol=s.H_TOL), ref)


def _yaw_of(q):
    return math.atan2(2.0 * (q[3] * q[2] + q[0] * q[1]), 1.0 - 2.0 * (q[1] * q[1] + q[2] * q[2]))


def _errors(pose, truth):
    dyaw = (_yaw_of(pose) - _yaw_of(truth) + math.pi) % (2 * math.pi) - math.pi
    return float(np.linalg.norm(pose[4:6] - truth[4:6])), abs(math.degrees(dyaw))


def test_closing_the_loop_through_relocalize(gpu_sage, street):
    s = street
    db = gpu_sage.PlaceDB(s.p)
    for i, e in enumerate(s.entries):
        db.add(e, tag=i, pose=s.poses[i])
    # (the revisit at 137 degrees: no multiple of a sector, so the prior's yaw is off as well as its position)
    truth = s.q_poses[1]
    m = db.match(s.queries[1], top_k=1, h_tol=s.H_TOL)[0]
    assert m["index"] == 9
    # the map of the matched place: a dense scan taken there, moved by its true pose
    rng = np.random.default_rng(77)
    T = s.poses[9]
    vmap = gpu_sage.VoxelHashMap(1.0, 100.0)
    vmap.AddPoints(s.syn.apply_pose(T, s.syn.make_scan(rng, 30000, 120.0, T)))
    ring_width = (s.p.max_range - s.p.min_range) / s.p.rings
    sector = 2.0 * math.pi / s.p.sectors
    pose, q, info = vmap.Relocalize(s.q_scans[1], m["prior"], 2.0, 0.5, 0.05, xy=(ring_width, ring_width / 2),
                                    yaw=(sector, sector / 2), refine_top=3)
    before, after = _errors(m["prior"], truth), _errors(pose, truth)
    print("prior off by %.2f m %.2f deg; relocalised off by %.3f m %.3f deg" % (before + after))
    assert after[0] < before[0] and after[1] < before[1]
    assert after[0] < 0.5 and after[1] < 3.0             # half the map's voxel, half a sector


# ---- the pipeline ------------------------------------------------------------------------------------------------------
NEAR = ((-20.0, 20.0), (-20.0, 20.0), (-4.0, 2.4))
NEAR_OCC = (64, 64)
QUERY = dict(top_k=4, h_tol=40, exclude_last=1, min_similarity=0.05)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _frames(n_frames=24, n=10000):
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(43, n_frames, points_per_frame=n, step=(1.5, 0.0, 0.0), yaw_step_deg=3.0)
    return [np.ascontiguousarray(f, dtype=np.float64) for f in frames]


def _key_threshold(frames, poses, takes=3):
    """the first threshold (of a fixed list) under which the selection's restatement (tests/keyframe_ref.py) takes at
    least `takes` key frames after the first and rejects as many: both branches of the place step run"""
    import keyframe_ref as kr
    for th in np.round(np.arange(0.02, 1.0, 0.01), 2):
        r = kr.Replay(NEAR, NEAR_OCC, th)
        taken = sum(r.step(f, p, i)["is_key_frame"] for i, (f, p) in enumerate(zip(frames, poses))) - 1
        if taken >= takes and len(frames) - 1 - taken >= takes:
            return float(th)
    raise AssertionError("no threshold gives both branches on this stream")


def _run(sage, frames, mode, th, places=True, cfg=None, timestamps=None, params=None):
    p = sage.SageICP(cfg if cfg is not None else sage.make_pipeline_config())
    p.set_key_frames(True, NEAR, NEAR_OCC, th)
    if places:
        p.set_places(True, params, **QUERY)
    infos, keys, nxt = [], [], None
    for k, f in enumerate(frames):
        if mode == "prefetch":
            cur = nxt if nxt is not None else f
            nxt = p.prefetch(frames[k + 1]) if k + 1 < len(frames) else None
            p.RegisterFrame(cur)
        elif mode == "device":
            p.RegisterFrame(torch.from_numpy(f).to(DEV))
        elif mode == "timestamps":
            p.RegisterFrame(f, timestamps[k])
        else:
            p.RegisterFrame(f)
        keys.append(p.key_frame_info())
        infos.append(p.place_info() if places else None)
    return p, infos, keys


def _check_against_replay(sage, p, frames, infos, keys, params, takes=4):
    """place_info after every frame is PlaceDB.match, then add, of the raw key frames, replayed on the host side"""
    replay = sage.PlaceDB(params)
    poses = p.poses()
    taken = 0
    for k, (info, key) in enumerate(zip(infos, keys)):
        assert info["enabled"]
        if not key["is_key_frame"]:
            assert not info["described"] and len(info["matches"]) == 0 and info["entries"] == taken
            continue
        d = sage.place_describe(frames[k], params)
        want = replay.match(d, **QUERY)
        replay.add(d, tag=k, pose=poses[k])
        taken += 1
        assert info["described"] and info["entries"] == taken
        assert info["matches"].tobytes() == want.tobytes(), k
    assert taken >= takes and taken < len(frames)
    assert any(len(i["matches"]) for i in infos)
    got, want = p.places().read(), replay.read()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
    assert np.array_equal(got[1], np.array([k for k, key in enumerate(keys) if key["is_key_frame"]], dtype=np.uint64))
    return replay


@pytest.fixture(scope="module")
def stream(gpu_sage):
    frames = _frames()
    first, _, _ = _run(gpu_sage, frames, "host", 0.5, places=False)        # (the selection changes no pose)
    th = _key_threshold(frames, first.poses())
    off, _, keys = _run(gpu_sage, frames, "host", th, places=False)
    return frames, off.poses(), keys, th


@pytest.mark.parametrize("mode", ["host", "device", "prefetch"])
def test_pipeline_places_match_the_replay(gpu_sage, stream, mode):
    frames, poses_off, keys_off, th = stream
    params = _params(gpu_sage)
    p, infos, keys = _run(gpu_sage, frames, mode, th, params=params)
    assert np.array_equal(_bits(p.poses()), _bits(poses_off))             # places change nothing of the registration
    assert [k["is_key_frame"] for k in keys] == [k["is_key_frame"] for k in keys_off]
    _check_against_replay(gpu_sage, p, frames, infos, keys, params)


def test_pipeline_places_under_deskew_and_the_dynamic_filter(gpu_sage):
    from sage_icp_amd import synthetic_skew as sk
    S = sk.make_skewed_stream(seed=0x6B, n_frames=12, az_steps=512)
    frames, stamps = S["frames"], S["timestamps"]
    params = _params(gpu_sage, 7, 61)
    mk = lambda: gpu_sage.make_pipeline_config(deskew=True, dynamic_vehicle_filter=True)
    off, _, _ = _run(gpu_sage, frames, "timestamps", 0.5, places=False, cfg=mk(), timestamps=stamps)
    th = _key_threshold(frames, off.poses(), takes=2)
    p, infos, keys = _run(gpu_sage, frames, "timestamps", th, cfg=mk(), timestamps=stamps, params=params)
    assert p.deskew_info()[0]
    assert np.array_equal(_bits(p.poses()), _bits(off.poses()))
    _check_against_replay(gpu_sage, p, frames, infos, keys, params, takes=3)


def test_pipeline_reinitialize_resets_failures_and_refusals(gpu_sage, stream):
    frames, th = stream[0], stream[3]
    params = _params(gpu_sage)
    p = gpu_sage.SageICP()
    with pytest.raises(gpu_sage.SageIcpError) as e:
        p.set_places(True, params)                       # key frames are off
    assert e.value.code == gpu_sage.ERR_INVALID and p.places() is None
    p.set_key_frames(True, NEAR, NEAR_OCC, th)
    p.set_places(True, params, **QUERY)
    for f in frames[:12]:
        p.RegisterFrame(f)
    n = len(p.places())
    before = p.places().read()
    assert n >= 2 and p.place_info()["entries"] == n
    # a register call that fails changes nothing in the database
    bad = frames[12].copy()
    bad[10, 1] = np.nan
    with pytest.raises(gpu_sage.SageIcpError):
        p.RegisterFrame(bad)
    info = p.place_info()
    assert len(p.places()) == n and not info["described"] and len(info["matches"]) == 0 and info["entries"] == n
    # reinitialize keeps the database (tags refer to the earlier trajectory) ...
    p.reinitialize()
    assert len(p.places()) == n and np.array_equal(p.places().read()[0], before[0])
    p.key_frame_reset()
    p.RegisterFrame(frames[12])                          # a first key frame again: matched against nothing, then added
    info = p.place_info()
    assert info["described"] and info["entries"] == 1 and len(info["matches"]) == 0
    assert p.places().read()[1].tolist() == [len(p.poses()) - 1] == [0]
    # ... the two resets clear it
    p.RegisterFrame(frames[13])
    p.place_reset()
    assert len(p.places()) == 0 and p.place_info()["entries"] == 0 and p.key_frame_info()["key_frames"] >= 1
    # switching key frames off switches places off
    p.set_key_frames(False)
    assert p.places() is None and not p.place_info()["enabled"]
    p.RegisterFrame(frames[14])
    assert not p.place_info()["described"]
