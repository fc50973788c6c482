"""The place matcher and the descriptor beyond one pass of their device loops (csrc/place.hip).  Needs a
real MI355X: python -m pytest tests -m gpu

The scenes are tests/placescenes.py's; tests/test_place_scenes_host.py asserts without a GPU that each decides what it
claims.  Here the device is held to them: every record PlaceDB.match returns against the restatement (tests/placeref.py,
placeref.same: integers and doubles exactly), for scenes A and B also against the closed form the scene was built to; the
descriptor's bytes against placeref.describe.  Each database is built once per module."""
import numpy as np
import pytest

import placeref
import placescenes as ps

pytestmark = pytest.mark.gpu


def _db(sage, R, S, sc):
    db = sage.PlaceDB(sage.place_params(rings=R, sectors=S))
    poses = sc.get("poses")
    for i, e in enumerate(sc["entries"]):
        db.add(e, tag=int(sc["tags"][i]), pose=poses[i] if poses is not None else None)
    assert len(db) == len(sc["entries"])
    return db


_BUILT = {}


def _built(sage, name, shape, make, *args):
    """(scene, database), made once"""
    key = (name,) + args
    if key not in _BUILT:
        sc = make(*args)
        _BUILT[key] = (sc, _db(sage, shape[0], shape[1], sc))
    return _BUILT[key]


@pytest.fixture(scope="module", autouse=True)
def _databases_go_with_the_module():
    yield
    _BUILT.clear()


def _held_to_the_closed_form(sc, db):
    """the records against the restatement's scores, then against the scene's own closed form"""
    q = dict(top_k=ps.TOP, h_tol=sc["h_tol"], exclude_last=sc["exclude_last"])
    got = db.match(sc["query"], **q)
    scores = placeref.scores(sc["entries"], sc["query"], sc["h_tol"])
    placeref.same(got, placeref.match(sc["entries"], sc["query"], tags=sc["tags"], poses=sc["poses"], scores=scores, **q))
    agree, shift, ne = sc["closed"]
    assert got["index"].tolist() == sc["top"]
    for field, want in (("agree", agree), ("shift", shift), ("n_entry", ne)):
        assert got[field].tolist() == [int(want[i]) for i in sc["top"]], field
    assert (got["n_query"] == sc["n_query"]).all() and got["tag"].tolist() == [int(sc["tags"][i]) for i in sc["top"]]
    return got


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ps.A_ORDERS)
def test_planted_entries_at_every_residue_of_both_strides(gpu_sage, order):
    sc, db = _built(gpu_sage, "a", ps.A_SHAPE, ps.scene_a, order)
    assert len(db) == 6145
    got = _held_to_the_closed_form(sc, db)
    if order == "empty":
        assert got[-1]["index"] == 2 and got[-1]["agree"] == 0
    # each planted entry as the last one considered: its record again, and the empty one still behind the fillers
    for i in ps.A_PLANTS:
        one = db.match(sc["query"], top_k=ps.TOP, exclude_last=len(db) - i - 1)
        rec = one[one["index"] == i]
        if sc["closed"][0][i]:
            assert len(rec) == 1 and (int(rec[0]["agree"]), int(rec[0]["shift"]), int(rec[0]["n_entry"])) == \
                tuple(int(a[i]) for a in sc["closed"])
        else:
            assert len(rec) == 0


# ---- B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ps.B_SIZES)
def test_identical_entries_rank_by_index(gpu_sage, n):
    sc, db = _built(gpu_sage, "b identical", ps.B_SHAPE, ps.scene_b_identical, n)
    got = _held_to_the_closed_form(sc, db)
    assert got["index"].tolist() == list(range(16))


@pytest.mark.parametrize("n", ps.B_SIZES)
def test_the_best_sixteen_are_the_last_sixteen(gpu_sage, n):
    sc, db = _built(gpu_sage, "b last", ps.B_SHAPE, ps.scene_b_last, n)
    got = _held_to_the_closed_form(sc, db)
    assert got[0]["index"] == n - 1 and got[-1]["index"] == n - 16


def test_equal_ratios_from_different_operands_rank_by_index(gpu_sage):
    sc, db = _built(gpu_sage, "b cross", ps.B_SHAPE, ps.scene_b_cross)
    got = _held_to_the_closed_form(sc, db)
    assert got["index"].tolist()[:6] == [5, 1023, 1029, 2047, 2053, 3071] and (got["similarity"][:6] == 0.25).all()
    assert sorted(set(zip(got["agree"].tolist()[:6], got["n_entry"].tolist()[:6]))) == [(3, 12), (6, 24)]


@pytest.mark.parametrize("considered", ps.B_CONSIDERED)
def test_exclude_last_on_both_sides_of_each_stride(gpu_sage, considered):
    # (the scenes of all `considered` are one database: the seed is the same, only exclude_last and the expected top differ)
    sc = ps.scene_b_exclude(considered)
    first, db = _built(gpu_sage, "b exclude", ps.B_SHAPE, ps.scene_b_exclude, ps.B_CONSIDERED[0])
    assert np.array_equal(first["entries"], sc["entries"]) and len(db) == 3073 and 3073 - sc["exclude_last"] == considered
    got = _held_to_the_closed_form(sc, db)
    assert got[0]["index"] in (considered - 1, considered - 2) and got["index"].max() < considered


# ---- C ------------------------------------------------------------------------------------------------------------------
def _c_cases():
    return [(R, S, t) for R, S in ps.C_SHAPES for t in ps.c_turns(S)]


@pytest.mark.parametrize("R,S,turn", _c_cases())
def test_wide_descriptors_on_a_workgroups_second_entry(gpu_sage, monkeypatch, R, S, turn):
    """both entry layouts of the scoring pass: held once with a wrapped sector index, held twice along S"""
    # the doubled layout is taken where its LDS fits 32 KiB: the head of 360 + 2 words and 4 bytes per cell
    assert 4 * (360 + 2) + 4 * R * S <= 32768
    sc, db = _built(gpu_sage, "c", (R, S), ps.scene_c, R, S)
    assert len(db) == 2049
    query = sc["queries"][turn]
    scores = placeref.scores(sc["entries"], query, sc["h_tol"])
    ref = placeref.match(sc["entries"], query, top_k=ps.TOP, h_tol=sc["h_tol"], tags=sc["tags"], scores=scores)
    got = {}
    for doubled in ("0", "1"):
        monkeypatch.setenv("SAGEICP_PLACE_DOUBLED", doubled)
        got[doubled] = db.match(query, top_k=ps.TOP, h_tol=sc["h_tol"])
        placeref.same(got[doubled], ref)
        for i, shift in sc["shifts"][turn].items():
            rec = got[doubled][got[doubled]["index"] == i]
            assert len(rec) == 1 and rec[0]["shift"] == shift
    assert got["0"].tobytes() == got["1"].tobytes()


# ---- D ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h_tol", ps.D_TOLS)
def test_saturating_windows_and_bytes_under_empty_cells(gpu_sage, h_tol):
    sc, db = _built(gpu_sage, "d", ps.D_SHAPE, ps.scene_d)
    got = db.match(sc["query"], top_k=ps.TOP, h_tol=h_tol)
    assert len(got) == ps.D_N == len(db)                 # every entry's record is compared
    placeref.same(got, placeref.match(sc["entries"], sc["query"], top_k=ps.TOP, h_tol=h_tol, tags=sc["tags"]))
    # the same from the vectorised restatement, and through read(): the bytes under empty cells are kept as given
    scores = placeref.scores(sc["entries"], sc["query"], h_tol)
    placeref.same(got, placeref.match(sc["entries"], sc["query"], top_k=ps.TOP, h_tol=h_tol, tags=sc["tags"], scores=scores))
    assert np.array_equal(db.read()[0], sc["entries"])


# ---- E ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", ps.E_SHAPES)
def test_descriptor_of_a_frame_that_several_workgroups_merge(gpu_sage, R, S):
    params = gpu_sage.place_params(rings=R, sectors=S, rank=ps.E_RANK)
    rows = ps.scene_e(R, S)
    assert ps.draw_blocks(len(rows), R * S) == 4
    want = placeref.describe(rows, params, gpu_sage.place_tables(params))
    for frame in (rows, rows[::-1].copy()):
        got = gpu_sage.place_describe(frame, params)
        assert got[0].dtype == np.uint8 and got[0].shape == (R, S)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
