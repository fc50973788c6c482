"""The device's Preprocess and VoxelDownsample (csrc/preprocess.hip: k_vds_insert, k_vds_flag, k_vds_count, k_vds_gather;
csrc/prep.hip: Prep::downsample, Prep::restore_reference_order) against the fp64 numpy restatement tests/prepref.py on the
scenes of tests/prepscenes.py: rows whose crop norm decides at a threshold under one evaluation only, rows on the voxel
faces, the label cast and the group rules, the +-2^19 key range, 200,000 rows contending for three voxels, the survivor
count at the workgroup boundaries, a probe chain that wraps around the device table, the order replay's fall-back, the
pipeline's fused first level over growing and shrinking frames, random mixtures, and the refusals.

Every comparison is of bits (uint64 views): the same rows in the same order.  tests/test_preprocess_host.py holds prepref
to the oracle and to the literal loops, and each scene to deciding what it claims to decide."""
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import prepref
import prepscenes as ps


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 4).view(np.uint64)


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (what, got.shape, want.shape)


def _sorted(a):
    return a[np.lexsort(a.T)]


@pytest.fixture
def arrival_order(gpu_sage):
    gpu_sage.set_downsample_order(False)
    try:
        yield gpu_sage
    finally:
        gpu_sage.set_downsample_order(True)


@pytest.fixture(scope="module")
def vds_refs():
    """prepref's answer per stand-alone scene, computed once and left unchanged"""
    return {name: prepref.voxel_downsample(*case) for name, case in ps.vds_scenes().items()}


# ---- the crop ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_crop_thresholds_decided_by_one_evaluation_only(gpu_sage):
    scenes = ps.crop_scenes()
    assert len(scenes) == 19
    for name, case in scenes.items():
        want = prepref.preprocess(*case)
        assert 0 < len(want) < len(case.frame), name
        _same(gpu_sage.preprocess(*case), want, name)


# ---- one level of VoxelDownsample ----------------------------------------------------------------------------------------
def _names(*prefixes):
    return sorted(n for n in ps.REFERENCE_ORDER_SCENES + ("contention/late", "contention/first_and_last", "chain")
                  if n.startswith(prefixes))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("faces/", "labels/", "range/", "contention/", "chain"))
def test_arrival_order_matches_the_restatement(arrival_order, vds_refs, name):
    case = ps.vds_scenes()[name]
    _same(arrival_order.voxel_downsample(*case), vds_refs[name], name)


@pytest.mark.gpu
def test_survivor_count_at_the_workgroup_boundaries(arrival_order, vds_refs):
    for n in ps.SIZES:
        for keep in ps.KEEPS:
            name = "sizes/%d/%s" % (n, keep)
            want = vds_refs[name]
            assert len(want) == {"all": n, "none": 0, "last": 1}[keep]
            _same(arrival_order.voxel_downsample(*ps.vds_scenes()[name]), want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ps.REFERENCE_ORDER_SCENES)
def test_reference_order_matches_the_oracle(gpu_sage, oracle, reference_emission_order, vds_refs, name):
    """the default emission order: the oracle's in mode 1 row for row, and prepref's rows as a multiset"""
    case = ps.vds_scenes()[name]
    out = gpu_sage.voxel_downsample(*case)
    _same(out, oracle.voxel_downsample(*case), name)
    _same(_sorted(out), _sorted(vds_refs[name]), name)


@pytest.mark.gpu
def test_replay_fallback_emits_the_group_in_arrival_order(gpu_sage, oracle, reference_emission_order, vds_refs):
    """300 voxels of one 20-bit VoxelHash: the replay does not model their probe distances, so group A comes in arrival
    order; group B, an ordinary group of the same call, still comes in the reference's order"""
    case, is_a = ps.fallback()
    a = prepref.voxel_downsample(case.frame[is_a], *case[1:])
    b = oracle.voxel_downsample(case.frame[~is_a], *case[1:])
    assert len(a) == 300 and len(b) > 1500
    assert not np.array_equal(_bits(b), _bits(prepref.voxel_downsample(case.frame[~is_a], *case[1:])))
    out = gpu_sage.voxel_downsample(*case)
    _same(out, np.concatenate([a, b]), "fallback")
    _same(_sorted(out), _sorted(vds_refs["fallback"]), "fallback, multiset")


# ---- the pipeline's fused first level -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipeline_case():
    frames, ranges, labels, sizes = ps.pipeline_frames()
    chains = [prepref.chain(f, *ranges, labels, sizes) for f in frames[:-1]]
    return frames, ranges, labels, sizes, chains + [chains[0]]


def _config(sage, ranges, labels, sizes):
    return sage.make_pipeline_config(max_range=ranges[0], min_range=ranges[1], label_max_range=ranges[2],
                                     voxel_labels=labels, voxel_size=sizes)


@pytest.mark.gpu
def test_pipeline_source_is_the_chain_in_arrival_order(arrival_order, pipeline_case):
    """crop fused into level 0 (no stand-alone entry runs that), then level 1, in ONE pipeline over frames of 30,000, 300,
    45,000 and 2,000 rows and the first again: buffer growth, a big table under a small frame, reuse"""
    sage = arrival_order
    frames, ranges, labels, sizes, chains = pipeline_case
    p = sage.SageICP(_config(sage, ranges, labels, sizes))
    for k, (f, want) in enumerate(zip(frames, chains)):
        n_source = p.RegisterFrame(f)[3]
        _same(p.source(), want, k)
        assert n_source == len(want) > 0, k
    assert np.array_equal(_bits(chains[0]), _bits(chains[-1]))


@pytest.mark.gpu
def test_pipeline_source_is_the_oracle_chain_in_reference_order(gpu_sage, oracle, reference_emission_order, pipeline_case):
    sage = gpu_sage
    frames, ranges, labels, sizes, chains = pipeline_case
    os.environ["SAGEICP_SOURCE_REFERENCE_ORDER"] = "1"
    try:
        p = sage.SageICP(_config(sage, ranges, labels, sizes))
        for k, (f, arrival) in enumerate(zip(frames, chains)):
            want = prepref.chain(f, *ranges, labels, sizes, ds=oracle.voxel_downsample)
            n_source = p.RegisterFrame(f)[3]
            _same(p.source(), want, k)
            assert n_source == len(want) == len(arrival), k
    finally:
        del os.environ["SAGEICP_SOURCE_REFERENCE_ORDER"]


# ---- random mixtures -------------------------------------------------------------------------------------------------------
_AWKWARD = [0.45, 0.15000000000000002, 1.0 / 3.0, 0.7, 0.3, 0.9]
_LISTED = [0, 10, 40, 44, 50, 70, 81, 99]
_group = st.tuples(st.lists(st.sampled_from(_LISTED), min_size=1, max_size=4), st.sampled_from(_AWKWARD))


def _mixture(seed, n, groups, scale):
    rng = np.random.default_rng(seed)
    labels, sizes = [g[0] for g in groups], [g[1] for g in groups]
    vs = np.asarray(sizes)[rng.integers(0, len(sizes), size=n)] * scale        # a face of SOME group's grid
    p = rng.integers(-400, 401, size=(n, 3)).astype(np.float64) * vs[:, None]
    step = rng.integers(-1, 2, size=(n, 3))
    p = np.where(step > 0, np.nextafter(p, np.inf), np.where(step < 0, np.nextafter(p, -np.inf), p))
    uniform = rng.random(n) < 0.3
    p[uniform] = rng.uniform(-30.0, 30.0, size=(int(uniform.sum()), 3))
    lab = rng.choice(np.asarray(_LISTED + [77, 41, -1], dtype=np.float64), size=n)
    frac = rng.random(n) < 0.3
    lab[frac] += rng.choice([0.99, 0.5, -0.9, 1e-12, -0.000001], size=int(frac.sum()))     # truncated, never rounded
    return np.column_stack([p, lab]), labels, sizes


@pytest.mark.gpu
@settings(max_examples=40, deadline=None, derandomize=True)
@given(seed=st.integers(0, 2 ** 32 - 1), n=st.integers(1, 2000), groups=st.lists(_group, min_size=1, max_size=8),
       scale=st.sampled_from([0.5, 1.0, 1.5]))
def test_random_mixtures_match_the_restatement(gpu_sage, seed, n, groups, scale):
    f, labels, sizes = _mixture(seed, n, groups, scale)
    want = prepref.voxel_downsample(f, labels, sizes, scale)
    gpu_sage.set_downsample_order(False)
    try:
        out = gpu_sage.voxel_downsample(f, labels, sizes, scale)
    finally:
        gpu_sage.set_downsample_order(True)
    _same(out, want, (seed, n, scale))


# ---- the refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_voxel_index_beyond_the_key_range_is_refused_and_the_next_call_is_clean(arrival_order):
    sage = arrival_order
    for name, bad, code, clean in ps.refusal_scenes():
        with pytest.raises(sage.SageIcpError) as e:
            sage.voxel_downsample(*bad)
        assert e.value.code == getattr(sage, code), name
        want = prepref.voxel_downsample(*clean)
        assert len(want) == 216
        _same(sage.voxel_downsample(*clean), want, name)


@pytest.mark.gpu
def test_nan_label_is_refused_on_a_kept_row_only(gpu_sage):
    """include/sageicp.h: a non-finite label of a KEPT point refuses the call; on a row the crop drops it is not looked at"""
    sage = gpu_sage
    clean = ps.crop_scenes()["crop/fixed"]
    want = prepref.preprocess(*clean)
    kept = np.concatenate([clean.frame[:30], [[20.0, 1.0, 0.0, np.nan]], clean.frame[30:]])
    with pytest.raises(sage.SageIcpError) as e:
        sage.preprocess(kept, *clean[1:])
    assert e.value.code == sage.ERR_INVALID
    _same(sage.preprocess(*clean), want, "after the refusal")
    # below min_range, beyond max_range, exactly on max_range, and a norm that overflows: all dropped, the label unread
    dropped = np.concatenate([clean.frame[:30], [[1.0, 1.0, 0.0, np.nan], [150.0, 0.0, 0.0, np.nan], [60.0, 80.0, 0.0, np.inf],
                                                 [1e200, 0.0, 0.0, np.nan]], clean.frame[30:]])
    _same(sage.preprocess(dropped, *clean[1:]), want, "NaN labels on dropped rows")
    _same(sage.preprocess(*clean), want, "after the accepted call")
