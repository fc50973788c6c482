"""Scenes that take the place matcher and the descriptor beyond one pass of their loops, for
tests/test_place_scenes_host.py (which asserts with tests/placeref.py alone that they decide) and
tests/test_place_beyond_one_pass_gpu.py (which holds the device to them).  numpy only; every builder is a pure function of
its arguments and a fixed seed.

The loops (csrc/place.hip): k_place_score strides the entries by its 2048 workgroups and rezeroes its LDS words per
entry, k_place_select strides them by its 1024 threads and drops what earlier rounds took, the shift loop of the scoring
pass strides the sectors by 64, k_place_draw deals the rows of a frame to its workgroups 256 at a time.

Building blocks (h_tol = 0 wherever a closed form is claimed):
  base_plane   every cell occupied, of a class of Q_CLASSES, the heights distinct along each ring: a rolled copy agrees
               with it at exactly one shift, cell by cell
  planted      the query rolled by s, all but `a` of its cells moved to a class no query holds or emptied until `n_entry`
               are occupied: its record is (a, s, n_entry), and no other shift agrees anywhere
  fillers      occupied cells only of classes no query holds: (0, 0, n_entry) — they rank by index behind everything that
               agrees, unless the device hands one another entry's state

  A  scene_a(order)        (3, 7), 6145 entries = 3 * 2048 + 1: 16 planted entries at every residue of both strides
  B  scene_b_*             (4, 6): ties at 1023 .. 3073 entries, equal ratios from different operands, exclude_last
  C  scene_c(R, S)         (2, 130) and (1, 360), 2049 entries: shifts on both sides of every multiple of 64 on an entry
                           that a workgroup scores second; random fillers that agree, the expected records from
                           placeref.scores
  D  scene_d()             (5, 9), 16 entries: heights at both ends of the byte, every tolerance that saturates a window,
                           arbitrary class bytes under empty cells
  E  scene_e(R, S)         rows of a frame for grids of 8192 .. 16384 cells, 3 R S + 1 of them"""
import numpy as np

Q_CLASSES = np.array([50, 71], dtype=np.uint8)        # the classes a query of scenes A and B holds
OTHER = np.array([7, 9], dtype=np.uint8)              # classes no such query holds
TOP = 16

SCORE_STRIDE = 2048                                   # launch_place_score: min(n, 2048) workgroups
SELECT_STRIDE = 1024                                  # k_place_select: one workgroup of 1024 threads
SHIFT_STRIDE = 64                                     # the scoring pass: a lane per shift, 64 at a time
DRAW_ROWS = 256                                       # k_place_draw: threads of a workgroup
DRAW_MAX_BLOCKS = 512


def _tags(n):
    return (1000 + 3 * np.arange(n)).astype(np.uint64)


def base_plane(R, S, rng):
    assert S <= 255
    h = np.stack([1 + rng.choice(255, size=S, replace=False) for _ in range(R)]).astype(np.uint8)
    c = rng.choice(Q_CLASSES, size=(R, S))
    return h, c


def planted(query, s, a, n_entry, rng):
    """(2, R, S): the entry that a query sees with `a` agreeing cells at shift s and nowhere else, n_entry cells occupied.
    The cells that do not agree keep the query's height under a class of OTHER, the empty ones the query's class byte"""
    qh, qc = (np.asarray(x).reshape(-1) for x in query)
    R, S = np.asarray(query[0]).shape
    occ = np.flatnonzero(qh > 0)
    assert 0 <= a <= len(occ) and a <= n_entry <= R * S
    keep = rng.choice(occ, size=a, replace=False)
    rest = np.setdiff1d(np.arange(R * S), keep)
    moved = rng.choice(rest, size=n_entry - a, replace=False)
    h, c = np.zeros(R * S, dtype=np.uint8), qc.copy()
    h[keep] = qh[keep]
    h[moved] = np.where(qh[moved] > 0, qh[moved], rng.integers(1, 256, size=len(moved)))
    c[moved] = rng.choice(OTHER, size=len(moved))
    e = np.stack([h.reshape(R, S), c.reshape(R, S)])
    return np.roll(e, s, axis=2)                       # e[r, j] = q[r, j - s]: the query's sector j lies at j + s


def fillers(n, R, S, rng, fill=0.7):
    """(n, 2, R, S) and their records' n_entry"""
    h = rng.integers(1, 256, size=(n, R, S)).astype(np.uint8)
    h[rng.random((n, R, S)) >= fill] = 0
    c = rng.choice(OTHER, size=(n, R, S))
    return np.stack([h, c], axis=1), (h > 0).sum(axis=(1, 2))


def _scene(entries, query, closed, n_query, top, exclude_last=0, poses=None):
    """closed: (agree, shift, n_entry) of every entry, by construction; top: the indices of the best 16, by design"""
    return dict(entries=entries, query=query, h_tol=0, closed=tuple(np.asarray(a, dtype=np.int64) for a in closed),
                n_query=n_query, top=list(top), exclude_last=exclude_last, tags=_tags(len(entries)), poses=poses)


def _assemble(n, R, S, query, plants, rng):
    """fillers everywhere but at plants: {index: (a, s, n_entry)}"""
    entries, ne = fillers(n, R, S, rng)
    agree, shift = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for i, (a, s, m) in plants.items():
        entries[i] = planted(query, s, a, m, rng)
        agree[i], shift[i], ne[i] = a, (s if a else 0), m
    return entries, (agree, shift, ne)


# ---- A: every residue of both strides ------------------------------------------------------------------------------------
A_SHAPE = (3, 7)
A_N = 3 * SCORE_STRIDE + 1
A_SINGLES = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 6144)
A_TRIPLE = (700, 700 + SCORE_STRIDE, 700 + 2 * SCORE_STRIDE)           # one workgroup's first, second and third entry
A_PAIR = (300, 300 + SELECT_STRIDE)                                    # one thread's first and second candidate
A_PLANTS = tuple(sorted(A_SINGLES + A_TRIPLE + A_PAIR))
A_ORDERS = ("descending", "ascending", "empty")


def scene_a(order):
    """The query is the base plane (n_query = 21), so the ratio is agree / 21 and sixteen different counts rank strictly.
      descending  the strength falls with the index, the shifts differ along every workgroup's entries: a key left in the
                  maximum word, or sums left in the per-shift words, outrank the later entry's own
      ascending   the strength rises with the index and the entries of one workgroup share a shift: sums left in the
                  per-shift words add up under the later entry's own shift; counts left in the n_entry word add up
      empty       descending, the middle entry of the triple empty (all heights 0, the query's class bytes): whatever it
                  reports but (0, 0, 0) is another entry's; the 16th record is the first filler's
    S = 7 admits 7 shifts, so the 16 records differ pairwise in agree and n_entry and as triples; shifts repeat."""
    assert order in A_ORDERS
    R, S = A_SHAPE
    rng = np.random.default_rng(3801 + A_ORDERS.index(order))
    query = base_plane(R, S, rng)
    plants = {}
    for j, i in enumerate(A_PLANTS):
        a = j + 1 if order == "ascending" else TOP - j
        s = j % S
        if order == "ascending":
            s = 5 if i in A_TRIPLE else 3 if i % SCORE_STRIDE == 0 else s
        plants[i] = (a, s, a + 5)
    if order == "empty":
        plants[A_TRIPLE[1]] = (0, 0, 0)
    entries, closed = _assemble(A_N, R, S, query, plants, rng)
    top = sorted((i for i in A_PLANTS if plants[i][0]), key=lambda i: -plants[i][0])
    if order == "empty":
        top.append(2)                                  # ratio 0: the lowest index that is no planted entry
    poses = rng.normal(size=(A_N, 7))
    return _scene(entries, query, closed, R * S, top, poses=poses)


# ---- B: ties at scale ----------------------------------------------------------------------------------------------------
B_SHAPE = (4, 6)
B_SIZES = (1023, 1024, 1025, 2049, 3073)
B_N = 3073
B_CONSIDERED = (1023, 1024, 1025, 2048, 2049)
B_LADDER = (1022, 1023, 1024, 2047, 2048, 3072)


def scene_b_identical(n):
    """all entries one planted entry: the best 16 are the indices 0 .. 15"""
    R, S = B_SHAPE
    rng = np.random.default_rng(3810)
    query = base_plane(R, S, rng)
    one = planted(query, 2, 9, 14, rng)
    entries = np.repeat(one[None], n, axis=0)
    return _scene(entries, query, (np.full(n, 9), np.full(n, 2), np.full(n, 14)), R * S, range(TOP))


def scene_b_last(n):
    """n - 16 copies of a weak entry, then 16 entries of rising strength: the winner is the last index"""
    R, S = B_SHAPE
    rng = np.random.default_rng(3811)
    query = base_plane(R, S, rng)
    weak = planted(query, 1, 2, 14, rng)
    entries = np.repeat(weak[None], n, axis=0)
    closed = [np.full(n, 2), np.full(n, 1), np.full(n, 14)]
    for j in range(TOP):
        i, a = n - TOP + j, 6 + j
        entries[i] = planted(query, j % S, a, min(R * S, a + 2), rng)
        closed[0][i], closed[1][i], closed[2][i] = a, j % S, min(R * S, a + 2)
    return _scene(entries, query, closed, R * S, range(n - 1, n - TOP - 1, -1))


def scene_b_cross():
    """The query holds half the cells (n_query = 12).  Entries (agree, n_entry) = (3, 12) and (6, 24) have the ratio 1/4
    from different operands, 3 * 24 == 6 * 12 in the cross products: the order among them is the index.  They sit at
    i, i + 1024 and i + 2048, alternating, the rest are fillers"""
    R, S = B_SHAPE
    rng = np.random.default_rng(3812)
    qh, qc = base_plane(R, S, rng)
    drop = rng.choice(R * S, size=R * S // 2, replace=False)
    qh.reshape(-1)[drop] = 0
    nq = R * S // 2
    small, large = (3, nq), (6, 2 * nq)
    plants = {}
    for i, kinds in ((5, (small, large, small)), (1023, (large, small, large))):
        for t, (a, m) in enumerate(kinds):
            plants[i + t * SELECT_STRIDE] = (a, (i + t) % S, m)
    entries, closed = _assemble(B_N, R, S, (qh, qc), plants, rng)
    top = sorted(plants) + [i for i in range(TOP) if i not in plants][:TOP - len(plants)]
    return _scene(entries, (qh, qc), closed, nq, top)


def scene_b_exclude(considered):
    """one database of 3073 entries, fillers and a ladder of rising strength on both sides of each stride's multiples:
    with exclude_last = 3073 - considered the winner is the last rung below `considered`"""
    R, S = B_SHAPE
    rng = np.random.default_rng(3813)
    query = base_plane(R, S, rng)
    plants = {i: (4 + j, j % S, 12 + j) for j, i in enumerate(B_LADDER)}
    entries, closed = _assemble(B_N, R, S, query, plants, rng)
    rungs = [i for i in reversed(B_LADDER) if i < considered]
    top = rungs + [i for i in range(TOP)][:TOP - len(rungs)]
    return _scene(entries, query, closed, R * S, top, exclude_last=B_N - considered)


# ---- C: wide S on a workgroup's second entry -------------------------------------------------------------------------------
C_SHAPES = ((2, 130), (1, 360))
C_N = SCORE_STRIDE + 1
C_PLANTS = {0: 63, SCORE_STRIDE - 1: 64, SCORE_STRIDE: 65}            # index: the roll of the entry against turn 0
C_H_TOL = 1


def c_turns(S):
    """the queries of a shape: the planted shifts are roll + turn — 63 64 65, 127 128 129, S - 1 0 1, S - 3 S - 2 S - 1"""
    return sorted({0, 64, S - 64, S - 66})


def _small(rng, shape, fill=0.8):
    h = rng.integers(1, 7, size=shape).astype(np.uint8)
    h[rng.random(shape) >= fill] = 0
    return h, rng.choice(Q_CLASSES, size=shape)


def scene_c(R, S):
    """Heights of 1 .. 6 and two classes under h_tol = 1: every filler agrees somewhere, at a shift of its own, so the 13
    records behind the planted three are no ties of zeros.  The planted entries are the turn-0 query rolled, a tenth of
    their cells drawn again.  Nothing here is a closed form: the expected records are placeref.scores'."""
    rng = np.random.default_rng(3820 + S)
    q0 = np.stack(_small(rng, (R, S)))
    entries = np.stack(_small(rng, (C_N, R, S)), axis=1)
    for i, k in C_PLANTS.items():
        e = np.roll(q0, k, axis=2)
        again = rng.random((R, S)) < 0.1
        e[:, again] = np.stack(_small(rng, (R, S)))[:, again]
        entries[i] = e
    queries = {t: (np.roll(q0[0], -t, axis=1), np.roll(q0[1], -t, axis=1)) for t in c_turns(S)}
    shifts = {t: {i: (k + t) % S for i, k in C_PLANTS.items()} for t in queries}
    return dict(entries=entries, queries=queries, shifts=shifts, h_tol=C_H_TOL, tags=_tags(C_N))


# ---- D: saturating windows, bytes under empty cells ------------------------------------------------------------------------
D_SHAPE = (5, 9)
D_N = 16
D_HEIGHTS = np.array([1, 2, 3, 4, 252, 253, 254, 255], dtype=np.uint8)
D_TOLS = (0, 1, 2, 3, 251, 252, 253, 254, 255)
D_CLASS = 50
D_UNDER = (D_CLASS, D_CLASS - 1, D_CLASS + 1, 0, 255)


def _d_heights(rng, shape):
    h = np.where(rng.random(shape) < 0.7, rng.choice(D_HEIGHTS, size=shape), rng.integers(1, 256, size=shape))
    return h.astype(np.uint8)


def scene_d():
    """The query: heights at both ends of the byte mixed with uniform ones, the class 50 but for a few cells of 49 and 51.
    The entries: the query rolled, half of the heights drawn again, a fifth of the classes moved by one, cells emptied and
    filled; under every empty cell (of the query too) a class byte no descriptor would carry there: the query's class,
    that class - 1 and + 1, 0, 255 in turn, then any byte"""
    R, S = D_SHAPE
    rng = np.random.default_rng(3830)
    near = np.array([D_CLASS - 1, D_CLASS, D_CLASS + 1], dtype=np.uint8)

    def under(h, c):
        short = len(D_UNDER) + 1 - int((h == 0).sum())                # at least one empty cell over each byte of D_UNDER
        if short > 0:
            h.reshape(-1)[rng.choice(np.flatnonzero(h.reshape(-1)), size=short, replace=False)] = 0
        empty = np.flatnonzero(h.reshape(-1) == 0)
        c.reshape(-1)[empty] = rng.integers(0, 256, size=len(empty))
        k = min(len(empty), 2 * len(D_UNDER))
        c.reshape(-1)[empty[:k]] = np.resize(np.array(D_UNDER, dtype=np.uint8), k)

    qh = _d_heights(rng, (R, S))
    qc = rng.choice(near, size=(R, S), p=[0.1, 0.8, 0.1])
    qh[rng.random((R, S)) < 0.15] = 0
    entries = np.zeros((D_N, 2, R, S), dtype=np.uint8)
    for i in range(D_N):
        h, c = np.roll(qh, i % S, axis=1), np.roll(qc, i % S, axis=1)
        again = rng.random((R, S)) < 0.5
        h[again] = _d_heights(rng, (R, S))[again]
        moved = rng.random((R, S)) < 0.2
        c[moved] = rng.choice(near, size=(R, S))[moved]
        h[rng.random((R, S)) < 0.15] = 0
        under(h, c)
        entries[i] = h, c
    under(qh, qc)
    return dict(entries=entries, query=(qh, qc), tols=D_TOLS, tags=_tags(D_N))


# ---- E: descriptor rows for large grids --------------------------------------------------------------------------------------
E_SHAPES = ((32, 256), (33, 256), (45, 360), (64, 256))       # 8192 cells: 64 KiB of planes, the last below the attribute path
E_LABELS = np.array([0, 10, 40, 44, 48, 72, 70, 51, 50, 71, 80, 81, 99, 255])
E_RANK = {c: 1 for c in range(1, 256)}
E_RANK.update({10: 0, 70: 2, 51: 3, 50: 4, 71: 5, 80: 6, 81: 6})


def scene_e(R, S):
    """3 R S + 1 rows: three per cell on average, so most cells have one row that alone holds their maximum, in either
    plane; some rows fall inside the first ring edge, beyond the last, below z_lo, above z_hi, on classes of rank 0"""
    rng = np.random.default_rng(3840 + R * S)
    n = 3 * R * S + 1
    f = np.empty((n, 4))
    r, a = rng.uniform(0.0, 55.0, n), rng.uniform(-np.pi, np.pi, n)
    f[:, 0], f[:, 1] = r * np.cos(a), r * np.sin(a)
    f[:, 2] = rng.uniform(-5.0, 9.0, n)
    f[:, 3] = rng.choice(E_LABELS, n)
    return f


def draw_blocks(n, cells):
    """launch_place_draw: a workgroup takes at least as many rows as it has cells"""
    per = max(4 * DRAW_ROWS, cells)
    return min((n + per - 1) // per, DRAW_MAX_BLOCKS)


def draw_block_of(i, blocks):
    """k_place_draw: row i = blockIdx.x * 256 + threadIdx.x, then + gridDim.x * 256"""
    return (np.asarray(i) // DRAW_ROWS) % blocks


def row_codes(rows, params):
    """(height byte, rank << 8 | class) of every row by the header's rules, for the rows placeref.describe keeps"""
    z, l = rows[:, 2], rows[:, 3]
    t = (z - params.z_lo) / (params.z_hi - params.z_lo)
    h = 1 + np.floor(np.clip(t, 0.0, 1.0) * 254.0).astype(np.int64)
    c = np.trunc(l).astype(np.int64)
    return h, np.array(params.rank[:], dtype=np.int64)[c] << 8 | c
