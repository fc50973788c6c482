"""The scenes of tests/placescenes.py decide: each holds what makes a wrong second trip of a device loop show, asserted
with tests/placeref.py and numpy alone.  A scene that stops deciding fails here instead of passing silently in
tests/test_place_beyond_one_pass_gpu.py.  Also: placeref.scores is placeref.score, entry by entry.  No GPU."""
import numpy as np
import pytest

import placeref
import placescenes as ps


# ---- the restatement that scales ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("h_tol", [0, 3, 255])
@pytest.mark.parametrize("R,S", [(1, 3), (3, 7), (7, 61), (2, 130)])
def test_scores_is_the_loop_over_score(R, S, h_tol):
    rng = np.random.default_rng(R * 1000 + S + h_tol)
    # few heights and classes, so that agreements are many and maxima tie between shifts
    h = rng.integers(0, 9, size=(50, R, S)).astype(np.uint8)
    tall = rng.random(h.shape) < 0.3
    h[tall] = rng.integers(1, 256, size=int(tall.sum()))
    c = rng.choice(np.array([40, 44, 50], dtype=np.uint8), size=(50, R, S))
    entries = [(h[i], c[i]) for i in range(50)]
    entries[7] = (np.zeros((R, S), dtype=np.uint8), c[7])                    # an empty entry
    entries[9] = (np.roll(h[3], 1, axis=1), np.roll(c[3], 1, axis=1))
    query = (h[3], c[3])
    (agree, shift, ne), nq = placeref.scores(entries, query, h_tol)
    loop = [placeref.score(query[0], query[1], e[0], e[1], h_tol) for e in entries]
    assert [(int(a), int(s), nq, int(m)) for a, s, m in zip(agree, shift, ne)] == loop
    assert agree[7] == 0 and shift[7] == 0 and ne[7] == 0 and agree[3] == nq
    assert len({s for _, s, _, _ in loop}) > 1 or S == 3
    # ranked from the scores or from the loop: the same records
    kw = dict(top_k=16, h_tol=h_tol, exclude_last=3, tags=list(range(50)))
    a, b = placeref.match(entries, query, **kw), placeref.match(entries, query, scores=((agree, shift, ne), nq), **kw)
    assert len(a) == len(b) == 16
    for x, y in zip(a, b):
        assert {k: v for k, v in x.items() if k not in ("pose", "prior")} == {k: v for k, v in y.items() if k not in ("pose", "prior")}
        assert np.array_equal(x["prior"], y["prior"])


# ---- A and B: closed forms ---------------------------------------------------------------------------------------------
def _closed_is_the_restatement(sc):
    (agree, shift, ne), nq = placeref.scores(sc["entries"], sc["query"], sc["h_tol"])
    assert nq == sc["n_query"]
    for got, want in zip((agree, shift, ne), sc["closed"]):
        assert np.array_equal(got, want)


def _ranked(sc):
    return placeref.match(sc["entries"], sc["query"], top_k=ps.TOP, h_tol=sc["h_tol"], exclude_last=sc["exclude_last"],
                          tags=sc["tags"], poses=sc["poses"], scores=(sc["closed"], sc["n_query"]))


@pytest.mark.parametrize("order", ps.A_ORDERS)
def test_scene_a_plants_every_residue_of_both_strides(order):
    sc = ps.scene_a(order)
    assert len(sc["entries"]) == 3 * 2048 + 1 == 6145 and len(ps.A_PLANTS) == len(set(ps.A_PLANTS)) == ps.TOP
    # both ends of each stride's multiples, one workgroup's three entries, one thread's first two candidates
    assert set(ps.A_SINGLES) == {0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 6144}
    e = ps.A_TRIPLE
    assert e[1] - e[0] == e[2] - e[1] == ps.SCORE_STRIDE and ps.A_PAIR[1] - ps.A_PAIR[0] == ps.SELECT_STRIDE
    assert len({i % ps.SCORE_STRIDE for i in e}) == 1 and len({i % ps.SELECT_STRIDE for i in ps.A_PAIR}) == 1
    _closed_is_the_restatement(sc)
    agree, shift, ne = sc["closed"]
    top = _ranked(sc)
    assert [r["index"] for r in top] == sc["top"]
    planted = [i for i in ps.A_PLANTS if agree[i]]
    assert sorted(sc["top"][:len(planted)]) == planted
    ratios = [r["agree"] * 1.0 / r["m"] for r in top[:len(planted)]]
    assert all(a > b for a, b in zip(ratios, ratios[1:])) and ratios[-1] > 0
    recs = [(int(agree[i]), int(shift[i]), int(ne[i])) for i in planted]
    assert len({r[0] for r in recs}) == len({r[2] for r in recs}) == len(set(recs)) == len(planted)
    assert len({r[1] for r in recs}) == ps.A_SHAPE[1]                        # every shift the shape has, 0 among them
    # everything else agrees nowhere
    rest = np.setdiff1d(np.arange(ps.A_N), planted)
    assert not agree[rest].any() and not shift[rest].any()
    along = [int(agree[i]) for i in e]
    if order == "descending":
        assert len(planted) == ps.TOP and along[0] > along[1] > along[2] and len({int(shift[i]) for i in e}) == 3
        assert top[0]["index"] == 0
    elif order == "ascending":
        assert len(planted) == ps.TOP and along[0] < along[1] < along[2] and len({int(shift[i]) for i in e}) == 1
        assert top[0]["index"] == ps.A_N - 1
        assert len({int(shift[i]) for i in (0, 2048, 4096)}) == 1
    else:
        assert len(planted) == ps.TOP - 1 and (along[1], int(ne[e[1]])) == (0, 0) and along[0] and along[2]
        assert not sc["entries"][e[1], 0].any() and np.array_equal(sc["entries"][e[1], 1], sc["query"][1])
        assert top[-1]["index"] == 2 and top[-1]["agree"] == 0 and top[-1]["n_entry"] == ne[2] > 0


def _tie_scene(sc):
    _closed_is_the_restatement(sc)
    top = _ranked(sc)
    assert [r["index"] for r in top] == sc["top"] and len(top) == ps.TOP
    return top


@pytest.mark.parametrize("n", ps.B_SIZES)
def test_scene_b_identical_entries_rank_by_index(n):
    sc = ps.scene_b_identical(n)
    assert len(sc["entries"]) == n and (sc["entries"] == sc["entries"][0]).all()
    top = _tie_scene(sc)
    assert [r["index"] for r in top] == list(range(16)) and {(r["agree"], r["shift"], r["n_entry"]) for r in top} == {(9, 2, 14)}


@pytest.mark.parametrize("n", ps.B_SIZES)
def test_scene_b_the_best_are_the_last(n):
    sc = ps.scene_b_last(n)
    top = _tie_scene(sc)
    assert [r["index"] for r in top] == list(range(n - 1, n - 17, -1))
    ratios = [r["agree"] / r["m"] for r in top]
    assert all(a > b for a, b in zip(ratios, ratios[1:])) and ratios[-1] > 2 / 24
    assert (sc["entries"][:n - 16] == sc["entries"][0]).all() and sc["closed"][0][0] == 2


def test_scene_b_equal_ratios_from_different_operands():
    sc = ps.scene_b_cross()
    R, S = ps.B_SHAPE
    assert sc["n_query"] == R * S // 2 == 12 and len(sc["entries"]) == 3073
    top = _tie_scene(sc)
    tied = top[:6]
    assert [r["index"] for r in tied] == [5, 1023, 5 + 1024, 1023 + 1024, 5 + 2048, 1023 + 2048]
    assert [(r["agree"], r["n_entry"]) for r in tied] == [(3, 12), (6, 24), (6, 24), (3, 12), (3, 12), (6, 24)]
    assert len({r["agree"] * t["m"] for r in tied for t in tied if r["m"] != t["m"]}) == 1       # the cross products: 72
    assert {r["similarity"] for r in tied} == {0.25} and all(r["agree"] == 0 for r in top[6:])
    assert [r["index"] for r in top[6:]] == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]


@pytest.mark.parametrize("considered", ps.B_CONSIDERED)
def test_scene_b_exclude_last_moves_the_winner(considered):
    sc = ps.scene_b_exclude(considered)
    assert len(sc["entries"]) == 3073 and sc["exclude_last"] == 3073 - considered
    top = _tie_scene(sc)
    assert top[0]["index"] == max(i for i in ps.B_LADDER if i < considered)
    assert top[0]["index"] in (considered - 1, considered - 2)
    assert all(r["index"] < considered for r in top)
    # one more entry considered and the winner is another, wherever a rung stands at `considered`
    if considered in ps.B_LADDER:
        assert ps.scene_b_exclude(considered + 1)["top"][0] == considered


# ---- C ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", ps.C_SHAPES)
def test_scene_c_shifts_on_both_sides_of_64_on_a_second_trip(R, S):
    sc = ps.scene_c(R, S)
    assert len(sc["entries"]) == ps.SCORE_STRIDE + 1 and S > ps.SHIFT_STRIDE
    assert set(ps.C_PLANTS) == {0, 2047, 2048}
    seen = set()
    for t, query in sc["queries"].items():
        (agree, shift, ne), nq = placeref.scores(sc["entries"], query, sc["h_tol"])
        top = placeref.match(sc["entries"], query, top_k=ps.TOP, h_tol=sc["h_tol"], scores=((agree, shift, ne), nq))
        assert sorted(r["index"] for r in top[:3]) == [0, 2047, 2048]
        for i, want in sc["shifts"][t].items():
            assert shift[i] == want and agree[i] > 0.8 * nq
            seen.add((i, want))
        # the fillers agree too, at shifts of their own: the other 13 records are no ties of zeros
        rest = [r for r in top[3:]]
        assert all(0 < r["agree"] < 0.8 * nq for r in rest) and len({r["shift"] for r in rest}) >= 6
        assert any(r["shift"] >= ps.SHIFT_STRIDE for r in rest)
    # on the entry a workgroup scores second: the last shift of a pass of 64, the first of the next, and the last of all
    second = {s for i, s in seen if i == 2048}
    assert {65, 129, S - 1} <= second
    assert {63, 127} <= {s for i, s in seen if i == 0} and {64, 128} <= {s for i, s in seen if i == 2047}
    assert {63, 64, 65, 127, 128, 129, S - 1} <= {s for _, s in seen}


# ---- D ------------------------------------------------------------------------------------------------------------------
def _window_scores(entries, query, lo_of, hi_of):
    """agreement as an interval on class * 256 + height, the interval's ends given per query cell: the rule of the header
    when lo_of = max(1, h - tol) and hi_of = min(255, h + tol), and what a window that does not saturate would count"""
    e = entries.astype(np.int64)
    qh, qc = (np.asarray(a).astype(np.int64) for a in query)
    S = qh.shape[1]
    v = np.concatenate([e[:, 1] * 256 + e[:, 0]] * 2, axis=2)
    lo, hi = qc * 256 + lo_of(qh), qc * 256 + hi_of(qh)
    best = np.full(len(e), -1)
    for k in range(S):
        w = v[:, :, k:k + S]
        best = np.maximum(best, ((qh > 0) & (w >= lo) & (w <= hi)).sum(axis=(1, 2)))
    return best


def test_scene_d_reaches_every_branch_of_the_window():
    sc = ps.scene_d()
    entries, (qh, qc) = sc["entries"], sc["query"]
    assert entries.shape == (16, 2, 5, 9) and sc["tols"] == (0, 1, 2, 3, 251, 252, 253, 254, 255)
    h = qh[qh > 0].astype(np.int64)
    assert set(ps.D_HEIGHTS.tolist()) <= set(h.tolist()) and len(set(h.tolist()) - set(ps.D_HEIGHTS.tolist())) >= 5
    branches = dict(low_saturates=0, low_at_one=0, low_free=0, high_254=0, high_255=0, high_saturates=0, high_free=0)
    for tol in sc["tols"]:
        branches["low_saturates"] += int((h <= tol).sum())
        branches["low_at_one"] += int((h == tol + 1).sum())
        branches["low_free"] += int((h > tol + 1).sum())
        branches["high_254"] += int((h + tol == 254).sum())
        branches["high_255"] += int((h + tol == 255).sum())
        branches["high_saturates"] += int((h + tol > 255).sum())
        branches["high_free"] += int((h + tol < 254).sum())
    print(branches)
    assert all(n >= 3 for n in branches.values()), branches
    # under the empty cells: the query's class, its neighbours, 0 and 255 — in the query and in every entry
    for hh, cc in [(qh, qc)] + [(e[0], e[1]) for e in entries]:
        assert set(ps.D_UNDER) <= set(cc[hh == 0].tolist())
    assert {ps.D_CLASS - 1, ps.D_CLASS, ps.D_CLASS + 1} == set(qc[qh > 0].tolist())
    # the records differ from entry to entry and from tolerance to tolerance, and two wrong windows count otherwise:
    # a lower end that reaches 0 takes empty cells over the query's class, an upper end past 255 takes the next class
    seen = set()
    for tol in sc["tols"]:
        (agree, shift, ne), nq = placeref.scores(entries, (qh, qc), tol)
        right = _window_scores(entries, (qh, qc), lambda x: np.maximum(1, x - tol), lambda x: np.minimum(255, x + tol))
        assert np.array_equal(right, agree)
        zero = _window_scores(entries, (qh, qc), lambda x: np.maximum(0, x - tol), lambda x: np.minimum(255, x + tol))
        past = _window_scores(entries, (qh, qc), lambda x: np.maximum(1, x - tol), lambda x: x + tol)
        print("h_tol %3d: agree %s; lower end 0: %d entries differ; upper end unsaturated: %d" %
              (tol, agree.tolist(), (zero != agree).sum(), (past != agree).sum()))
        assert (zero != agree).any() == (tol >= 1)
        if tol != 1:                                     # (at 1 only a query cell of 255 reaches past the byte)
            assert (past != agree).any() == (tol >= 2)
        assert len(set(agree.tolist())) >= 6 and 0 < agree.min() and agree.max() < nq
        seen.add(tuple(agree.tolist()))
    assert len(seen) >= 7


def test_the_window_of_the_header_has_one_form():
    """max(1, h - tol) is h - tol where h > tol + 1 and 1 elsewhere; at h == tol + 1 both give 1, so a comparison with
    tol in place of tol + 1 is the same window: no scene can tell them apart, and none has to"""
    h, tol = np.meshgrid(np.arange(1, 256), np.arange(0, 256), indexing="ij")
    a = np.where(h > tol + 1, h - tol, 1)
    b = np.where(h > tol, h - tol, 1)
    assert np.array_equal(a, b) and np.array_equal(a, np.maximum(1, h - tol))


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", ps.E_SHAPES)
def test_scene_e_every_workgroup_alone_holds_maxima_of_both_planes(sage, R, S):
    cells = R * S
    assert (cells == 8192) == ((R, S) == ps.E_SHAPES[0]) and cells >= 8192
    assert (2 * cells * 4 > 64 * 1024) == ((R, S) != ps.E_SHAPES[0])          # both planes as u32: the dynamic LDS asked for
    params = sage.place_params(rings=R, sectors=S, rank=ps.E_RANK)
    tables = sage.place_tables(params)
    rows = ps.scene_e(R, S)
    n = len(rows)
    assert n == 3 * cells + 1
    blocks = ps.draw_blocks(n, cells)
    assert blocks == 4 and n > cells
    heights, classes, kept, ring, sector = placeref.describe(rows, params, tables, return_kept=True)
    assert 0.5 * n < len(kept) < n
    cell = ring * S + sector
    h, key = ps.row_codes(rows[kept], params)
    for name, plane, code in (("heights", heights, h), ("keys", classes, key)):
        top = np.zeros(cells, dtype=np.int64)
        np.maximum.at(top, cell, code)
        assert np.array_equal(top & 0xFF, plane.reshape(-1))                    # the codes are the restatement's
        at_top = code == top[cell]
        alone = at_top & (np.bincount(cell[at_top], minlength=cells)[cell] == 1)
        for order in (kept, n - 1 - kept):                                      # as given, and the reversed copy
            per_block = np.bincount(ps.draw_block_of(order[alone], blocks), minlength=blocks)
            print("%dx%d %s: rows that alone hold a cell's maximum, per workgroup: %s" % (R, S, name, per_block.tolist()))
            assert (per_block >= 500).all()
    assert (heights > 0).mean() > 0.8 and (heights[-1] > 0).any() and (heights[:, -1] > 0).any()
