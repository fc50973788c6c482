"""The device's dynamic vehicle filter (csrc/dyn_filter.hip; core/Preprocessing.cpp:95-172) against the independent
CPU restatement (tests/dynfilter_ref.cpp) on the adversarial scenes of tests/dynscenes.py: path-graph components in
four frame orders (deep union-find trees, contended CAS), dense blobs whose cells hold hundreds of points, bumper-to-
bumper rows, points on the cell faces and pairs at d2 == 0.25f, the size boundaries of the kernels and tables, the
label and threshold edges, the +-2^19 m cell range, buffer reuse inside one pipeline and random mixtures.  Outputs
must be the same rows in the same order, and every info field must match."""
import concurrent.futures

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import dynref
import dynscenes as ds

VEH = dynref.KITTI_VEHICLES


def _dev(sage, f, dy_th=0.5, dynamic_labels=VEH, landmark_labels=(44, 48), max_range=100.0, min_range=5.0,
         label_max_range=50.0):
    return sage.preprocess(f, max_range, min_range, label_max_range, dynamic_vehicle_filter=True, dy_th=dy_th,
                           dynamic_labels=dynamic_labels, landmark_labels=landmark_labels, return_info=True)


def _refs(jobs):
    """dynref.preprocess over [(frame, kwargs)] on a few threads (the restatement is O(|V|^2); ctypes drops the GIL)"""
    dynref.lib()
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda j: dynref.preprocess(j[0], **j[1]), jobs))


def _same(sage, f, ref, what, **kw):
    out, info = _dev(sage, f, **kw)
    rout, rinfo = ref
    assert out.shape == rout.shape and np.array_equal(out, rout), (what, out.shape, rout.shape)
    assert all(info[k] == rinfo[k] for k in rinfo), (what, info, rinfo)
    return info


def _sweep(sage, cases):
    """cases: [(name, frame, kwargs)]; returns the restatement's info per case"""
    refs = _refs([(f, kw) for _, f, kw in cases])
    for (name, f, kw), ref in zip(cases, refs):
        _same(sage, f, ref, name, **kw)
    return [r[1] for r in refs]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ds.ORDERS)
def test_serpentine_path_graph_in_every_order(gpu_sage, kind):
    f, _ = ds.serpentine(11, 20000, kind)
    infos = _sweep(gpu_sage, [((kind, th), f, dict(dy_th=th)) for th in (0.0, 0.005, 0.5)])
    assert all(i["vehicle_points"] == 20000 and i["clusters"] == 1 for i in infos)
    assert [i["clusters_kept"] for i in infos] == [1, 1, 0]          # dy_th decides


@pytest.mark.gpu
@pytest.mark.parametrize("n,repeat", [(20000, 1), (8000, 3)])
def test_dense_blob(gpu_sage, n, repeat):
    f = ds.dense_blob(12, n, repeat)
    infos = _sweep(gpu_sage, [((n, repeat, th), f, dict(dy_th=th)) for th in (0.5, 4.0, 16.0)])
    assert all(i["vehicle_points"] == n * repeat and i["clusters"] == 1 for i in infos)
    assert [i["clusters_kept"] for i in infos] == [1, 1, 0]


@pytest.mark.gpu
def test_bumper_to_bumper_rows(gpu_sage):
    f, sizes = ds.bumper_rows(13)
    assert len(sizes["b"]) > 16 and max(sizes["b"]) - min(sizes["b"]) == 1
    infos = _sweep(gpu_sage, [(("rows", th), f, dict(dy_th=th)) for th in (0.0, 0.5, 2.0)])
    assert all(i["clusters"] == 1 + len(sizes["b"]) for i in infos)
    assert infos[1]["clusters_kept"] > 1 and infos[2]["clusters_kept"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_cell_faces_and_quarter_d2(gpu_sage, seed):
    f = ds.cell_faces(seed)
    cases = [((seed, th), f, dict(dy_th=th)) for th in (-1.0, 0.0, 0.5)]
    cases.append(((seed, "10 a landmark too"), f, dict(dy_th=0.0, landmark_labels=(10, 48))))
    infos = _sweep(gpu_sage, cases)
    assert infos[0]["clusters_kept"] > 0


@pytest.mark.gpu
def test_vehicle_counts_at_the_size_boundaries(gpu_sage):
    sizes = [(0, 1001), (4, 1003), (5, 1237), (6, 777), (255, 2001), (256, 2222), (257, 3333), (65536, 70001),
             (65537, 70003)]
    cases = [((nv, n), ds.with_vehicle_count(nv, nv, n), dict(dy_th=0.5)) for nv, n in sizes]
    infos = _sweep(gpu_sage, cases)
    assert [i["vehicle_points"] for i in infos] == [nv for nv, _ in sizes]
    assert infos[-1]["clusters_kept"] > 0 and infos[-1]["points_removed"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ds.label_kat_scenes()))
def test_label_edges_on_device(gpu_sage, name):
    frame, kw, expected = ds.label_kat_scenes()[name]
    ref = dynref.preprocess(frame, **kw, **dynref.KAT_RANGES)
    assert np.array_equal(ref[0], expected)
    _same(gpu_sage, frame, ref, name, **kw, **dynref.KAT_RANGES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ds.threshold_kat_scenes()))
def test_threshold_edges_on_device(gpu_sage, name):
    frame, kw, expected = ds.threshold_kat_scenes()[name]
    ref = dynref.preprocess(frame, **kw, **dynref.KAT_RANGES)
    assert np.array_equal(ref[0], expected)
    _same(gpu_sage, frame, ref, name, **kw, **dynref.KAT_RANGES)


@pytest.mark.gpu
def test_cell_range_capacity(gpu_sage):
    sage = gpu_sage
    far = dict(max_range=1e7, min_range=5.0, label_max_range=1e7)
    road = [[20.0, 1.0, 0.0, 40.0], [21.0, -1.0, 0.0, 40.0]]
    beyond = np.array(road + [[600000.0 + 0.25 * k, 0.0, 0.0, 10.0] for k in range(6)])
    with pytest.raises(sage.SageIcpError) as e:
        _dev(sage, beyond, **far)
    assert e.value.code == sage.ERR_CAPACITY
    # a landmark beyond is refused as well; an ordinary point is not placed in a cell
    with pytest.raises(sage.SageIcpError) as e:
        _dev(sage, np.array(road + [[-600000.0, 0.0, 0.0, 44.0]]), **far)
    assert e.value.code == sage.ERR_CAPACITY
    # just inside: cells 2^20 - 1 and -2^20, vehicles with landmarks beside
    inside = []
    for x0, s in ((524287.5, -1.0), (-524288.0, 1.0)):
        inside += [[x0 + s * 0.25 * k, 0.0, 0.0, 10.0] for k in range(6)]
        inside += [[x0 + s * 0.25 * k, 0.375, 0.0, 44.0] for k in range(4)]
    f = ds._f32(road + inside + [[600000.0, 3.0, 0.0, 40.0]])
    ref = dynref.preprocess(f, dy_th=0.5, **far)
    info = _same(sage, f, ref, "inside", dy_th=0.5, **far)
    assert info["clusters"] == 2 and info["clusters_kept"] == 2
    ok = ds.dense_blob(14, 2000)                      # the next call is unaffected
    _same(sage, ok, dynref.preprocess(ok), "after")


def _relabel(f, keep):
    """the frame with every vehicle point but the first `keep` relabelled road (40): the geometry is unchanged"""
    g = f.copy()
    veh = np.flatnonzero(np.isin(g[:, 3], VEH) & (np.linalg.norm(g[:, :3], axis=1) < 50.0)
                         & (np.linalg.norm(g[:, :3], axis=1) > 5.0))
    g[veh[keep:], 3] = 40.0
    return g


@pytest.mark.gpu
def test_buffer_reuse_inside_one_pipeline(gpu_sage):
    """one pipeline keeps its filter's buffers across frames: sizes shrink to nothing and grow past the capacity, the
    label table is reallocated twice and shrinks again; each frame against the restatement, and the poses against a
    pipeline fed the restatement's filtered frames"""
    sage = gpu_sage
    from sage_icp_amd import synthetic_dynamic as sd
    frames, _ = sd.make_dynamic_stream(61, 16, n=30000)
    seq = [(sd.make_dynamic_scan(62, n=120000), (44, 48)),
           (_relabel(frames[0], 5), (44, 48)), (_relabel(frames[1], 0), (44, 48)), (_relabel(frames[2], 4), (44, 48)),
           (sd.make_dynamic_scan(63, n=200000), (44, 48))]
    for k, m in enumerate((1, 2, 3, 8, 17, 18, 24, 35, 40, 12, 1)):
        lm = tuple(range(1000, 1000 + m - 2)) + ((44, 48) if m >= 2 else (48,))
        seq.append((frames[3 + k], lm))
    refs = _refs([(f, dict(dy_th=0.5, landmark_labels=lm)) for f, lm in seq])
    a = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
    b = sage.SageICP(sage.make_pipeline_config())
    for k, ((f, lm), (g, rinfo)) in enumerate(zip(seq, refs)):
        a.set_dynamic_vehicle_filter(True, 0.5, 5, lm)
        pa, _, _, ns_a, st_a = a.RegisterFrame(f)
        info = a.dynamic_filter_info()
        assert all(info[key] == rinfo[key] for key in rinfo), (k, info, rinfo)
        pb, _, _, ns_b, st_b = b.RegisterFrame(g)
        assert np.array_equal(pa, pb) and ns_a == ns_b and st_a.iterations == st_b.iterations, k
        if k == 2:      # the standalone entry on an empty frame between two pipeline frames
            empty, einfo = _dev(sage, np.zeros((0, 4)))
            assert len(empty) == 0 and einfo["vehicle_points"] == 0
    assert [r[1]["vehicle_points"] for r in refs[1:4]] == [5, 0, 4]
    assert np.array_equal(a.LocalMap(), b.LocalMap())


@pytest.mark.gpu
def test_pipeline_with_a_dense_blob_equals_pipeline_fed_filtered_frames(gpu_sage):
    sage = gpu_sage
    from sage_icp_amd import synthetic_dynamic as sd
    frames, poses = sd.make_dynamic_stream(71, 4, n=30000)
    rng = np.random.default_rng(72)
    blobbed = []
    for f, p in zip(frames, poses):                 # a dense parked blob, fixed in the world
        blob = ds.dense_blob(73, 12000, centre=(20.0 - p[4], 10.0, -1.63), shuffle=False)
        g = np.concatenate([f, blob])
        blobbed.append(np.ascontiguousarray(g[rng.permutation(len(g))]))
    refs = _refs([(f, dict(dy_th=0.5)) for f in blobbed])
    a = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
    b = sage.SageICP(sage.make_pipeline_config())
    for k, (f, (g, rinfo)) in enumerate(zip(blobbed, refs)):
        pa, _, _, ns_a, st_a = a.RegisterFrame(f)
        info = a.dynamic_filter_info()
        assert all(info[key] == rinfo[key] for key in rinfo), (k, info, rinfo)
        assert info["vehicle_points"] > 12000 and info["clusters_kept"] > 0, k
        pb, _, _, ns_b, st_b = b.RegisterFrame(g)
        assert np.array_equal(pa, pb) and ns_a == ns_b and st_a.iterations == st_b.iterations, k
    assert np.array_equal(a.LocalMap(), b.LocalMap())


def _mixture(seed, blobs, label_sets, dup):
    rng = np.random.default_rng(seed)
    rows = []
    for n, edge, (cx, cy, cz), ulps, lab in blobs:
        c = np.array([ds.ulp_steps(0.5 * cx, ulps), ds.ulp_steps(0.5 * cy, -ulps), ds.ulp_steps(0.5 * cz, ulps)])
        p = c + rng.uniform(-edge / 2, edge / 2, size=(n, 3))
        if edge == 0.0:             # on the cell corner itself, +-1 ulp per axis
            p = np.array([[ds.ulp_steps(v, int(rng.integers(-1, 2))) for v in c] for _ in range(n)])
        labels = rng.choice(label_sets[lab], size=n)
        rows.append(np.column_stack([p, labels]))
    f = np.concatenate(rows)
    if dup > 1:
        f = np.concatenate([f, f[: len(f) * (dup - 1) // 2]])
    f = f[rng.permutation(len(f))]
    return ds._f32(f)


_LABEL_SETS = [(10.0,), (10.0, 44.0), (18.0, 48.0, 40.0), (20.0, 44.0, 44.0, 10.0), (0.0, 10.0, -1.0)]
_blob = st.tuples(st.integers(1, 450), st.sampled_from([0.0, 0.05, 0.4, 1.0, 2.0]),
                  st.tuples(st.integers(20, 60), st.integers(-40, 40), st.integers(-8, 8)), st.integers(-1, 1),
                  st.integers(0, len(_LABEL_SETS) - 1))


@pytest.mark.gpu
@settings(max_examples=150, deadline=None, derandomize=True)
@given(seed=st.integers(0, 2 ** 32 - 1), blobs=st.lists(_blob, min_size=1, max_size=4), dup=st.integers(1, 3),
       dyn=st.sampled_from([VEH, (10,), (10, 0), (-1, 18)]), lm=st.sampled_from([(44, 48), (44,), (), (10, 48), (0,)]),
       dy_th=st.one_of(st.sampled_from([-1.0, 0.0, 0.5, 1.0, 2.0 ** 28, 1e10]), st.floats(-0.5, 4.0)))
def test_random_mixtures_match_the_restatement(gpu_sage, seed, blobs, dup, dyn, lm, dy_th):
    f = _mixture(seed, blobs, _LABEL_SETS, dup)
    assert len(f) <= 3600
    kw = dict(dy_th=dy_th, dynamic_labels=dyn, landmark_labels=lm)
    _same(gpu_sage, f, dynref.preprocess(f, **kw), (seed, dy_th), **kw)
