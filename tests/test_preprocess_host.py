"""The references and scenes of the device Preprocess / VoxelDownsample tests, checked without a GPU: tests/prepref.py
(vectorised numpy) against the oracle and against the literal per-point loops on every stand-alone scene of
tests/prepscenes.py, every scene's self-check (how many planted rows decide the wrong evaluation it targets), and the
voxel sizes the C entries refuse before they touch a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import prepref
import prepscenes as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP_ROWS = 20000           # the contention scenes are cut to this for the per-point loops


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 4).view(np.uint64)


@pytest.fixture(scope="module")
def scenes():
    return ps.vds_scenes(contention_n=LOOP_ROWS)


def test_every_scene_decides_and_says_how_many_rows():
    ps.REPORT.clear()
    ps.crop_scenes.cache_clear()
    ps.vds_scenes.cache_clear()
    ps.pipeline_frames.cache_clear()
    crop, vds = ps.crop_scenes(), ps.vds_scenes(contention_n=LOOP_ROWS)
    ps.contention(200000, "late")
    ps.contention(200000, "first_and_last")
    ps.refusal_scenes()
    frames = ps.pipeline_frames()[0]
    assert [len(f) for f in frames] == [30000, 300, 45000, 2000, 30000]
    for name in sorted(ps.REPORT):
        print("%-34s %s" % (name, ", ".join("%s: %d" % kv for kv in ps.REPORT[name].items())))
    targeted = {v for d in ps.REPORT.values() for v in d}
    assert set(prepref.VARIANTS) <= targeted, set(prepref.VARIANTS) - targeted
    for name, d in ps.REPORT.items():
        for what, count in d.items():
            if what in prepref.VARIANTS and not name.startswith("contention/"):
                assert count >= ps.MIN_DECIDING, (name, what, count)
    chain = [(k, v) for k, v in ps.REPORT["chain/1000"].items() if k.startswith("chain length")]
    assert chain[0][1] >= 300 and "then 0.." in chain[0][0]          # it wraps past the last slot
    assert len(crop) == 19 and len(vds) == 29


def test_vectorised_voxel_downsample_equals_the_oracle_and_the_loop(oracle, scenes):
    oracle.set_robin_order(0)
    for name, case in scenes.items():
        ref = prepref.voxel_downsample(*case)
        assert np.array_equal(_bits(ref), _bits(oracle.voxel_downsample(*case))), name
        assert np.array_equal(_bits(ref), _bits(prepref.py_voxel_downsample(*case))), name


def test_refused_scenes_are_clean_without_the_offending_row(oracle):
    for name, bad, code, clean in ps.refusal_scenes():
        with pytest.raises(prepref.Refused) as e:
            prepref.voxel_downsample(*bad)
        assert e.value.code == code, name
        assert np.array_equal(_bits(prepref.voxel_downsample(*clean)), _bits(oracle.voxel_downsample(*clean))), name
    for bad in ([[1.0, 2.0, 3.0, np.nan]], [[np.inf, 2.0, 3.0, 40.0]], [[1.0, np.nan, 3.0, 77.0]]):
        with pytest.raises(prepref.Refused) as e:
            prepref.voxel_downsample(bad, [[40]], [1.0], 1.0)
        assert e.value.code == "ERR_INVALID"


_CROP_CODE = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, prepref, prepscenes as ps
assert prepref.SQNORM3_ORDER == int(sys.argv[1])
scenes = ps.crop_scenes()
for name, case in scenes.items():
    a, b = prepref.preprocess(*case), prepref.py_preprocess(*case)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), name
    assert 0 < len(a) < len(case.frame), name
print(prepref.SQNORM3_ORDER, len(scenes), sum(sum(d.values()) for k, d in ps.REPORT.items() if k.startswith("crop/")))
"""


@pytest.mark.parametrize("order", ["2", "0"])
def test_vectorised_preprocess_equals_the_loop_under_both_associations(order):
    """a subprocess per value of SAGE_SQNORM3_ORDER (prepref reads it at import); the scenes are rebuilt under that value,
    so their deciders are the ones of that association"""
    r = subprocess.run([sys.executable, "-c", _CROP_CODE % (ROOT, os.path.join(ROOT, "tests")), order],
                       env=dict(os.environ, SAGE_SQNORM3_ORDER=order), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.split()
    assert got[:2] == [order, "19"] and int(got[2]) >= 19 * ps.MIN_DECIDING


def test_chain_is_crop_then_both_levels():
    frames, ranges, labels, sizes = ps.pipeline_frames()
    f = frames[1]
    fd, src = prepref.chain(f, *ranges, labels, sizes, levels=True)
    cropped = prepref.py_preprocess(f, *ranges)
    assert np.array_equal(_bits(fd), _bits(prepref.py_voxel_downsample(cropped, labels, sizes, 0.5)))
    assert np.array_equal(_bits(src), _bits(prepref.py_voxel_downsample(fd, labels, sizes, 1.5)))
    assert 0 < len(src) < len(fd) < len(f)


def test_fallback_group_is_beyond_what_the_replay_models(sage):
    """group A of the fall-back scene: sageicp_robin_iteration_order itself refuses its voxels (probe distance 128)"""
    case, is_a = ps.fallback()
    out = prepref.voxel_downsample(case.frame[is_a], [[40]], [0.01], 1.0)
    vox = np.ascontiguousarray(np.trunc(out[:, :3] / 0.01), dtype=np.int32)
    assert len(vox) == 300 and len(set(ps.reference_voxel_hash(vox).tolist())) == 1
    order = np.zeros(len(vox), dtype=np.uint32)
    rc = sage.lib().sageicp_robin_iteration_order(vox.ctypes.data_as(C.c_void_p), len(vox), order.ctypes.data_as(C.c_void_p))
    assert rc == sage.ERR_CAPACITY
    rc = sage.lib().sageicp_robin_iteration_order(vox.ctypes.data_as(C.c_void_p), 100, order.ctypes.data_as(C.c_void_p))
    assert rc == 0


@pytest.mark.parametrize("name", ps.REFERENCE_ORDER_SCENES)
def test_reference_order_scenes_stay_within_what_the_replay_models(sage, oracle, scenes, name):
    """what the GPU module expects of the default emission order, put together on the host: prepref's survivors, each
    group's run permuted by sageicp_robin_iteration_order (no probe distance reaches the limit), are the oracle's
    mode-1 rows"""
    case = scenes[name]
    out = prepref.voxel_downsample(*case)
    group = prepref._groups_of(np.trunc(out[:, 3]).astype(np.int64), case.labels)
    parts = []
    for g in range(len(case.labels)):
        run = out[group == g]
        vox = np.ascontiguousarray(np.trunc(run[:, :3] / (case.sizes[g] * case.scale)), dtype=np.int32)
        order = np.zeros(max(len(vox), 1), dtype=np.uint32)
        rc = sage.lib().sageicp_robin_iteration_order(vox.ctypes.data_as(C.c_void_p), len(vox), order.ctypes.data_as(C.c_void_p))
        assert rc == 0, (name, g, len(vox))
        parts.append(run[order[:len(vox)]])
    want = np.concatenate(parts) if parts else out
    oracle.set_robin_order(1)
    try:
        got = oracle.voxel_downsample(*case)
    finally:
        oracle.set_robin_order(0)
    assert np.array_equal(_bits(got), _bits(want)), name


# ---- the voxel sizes the entries refuse ---------------------------------------------------------------------------------
_BAD_SIZES = [float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -0.5]


def _vds_rc(sage, sizes, scale):
    f = np.array([[1.0, 2.0, 3.0, 40.0]])
    out = np.empty((1, 4))
    k = C.c_uint64(0)
    dp = C.POINTER(C.c_double)
    counts = (C.c_int * len(sizes))(*[1] * len(sizes))
    labels = (C.c_int * len(sizes))(*range(40, 40 + len(sizes)))
    rc = sage.lib().sageicp_voxel_downsample(f.ctypes.data_as(dp), 1, len(sizes), counts, labels,
                                             (C.c_double * len(sizes))(*sizes), scale, out.ctypes.data_as(dp), C.byref(k), 0)
    return rc, (sage.lib().sageicp_last_error() or b"").decode()


@pytest.mark.parametrize("bad", _BAD_SIZES)
def test_voxel_downsample_refuses_a_voxel_size_that_is_not_finite_or_not_above_zero(sage, bad):
    """sageicp_voxel_downsample looks at group_voxel_size[g] * vox_scale before it touches a device: ERR_INVALID, whichever
    group carries the size"""
    for sizes in ([bad], [1.0, bad], [0.6, 1.0, bad, 0.8]):
        rc, msg = _vds_rc(sage, sizes, 0.5)
        assert rc == sage.ERR_INVALID and "voxel size" in msg, (sizes, rc, msg)
    # the product of two finite factors that is not: overflow to Inf, underflow to 0
    for sizes, scale in (([1e200], 1e200), ([1e-200], 1e-200)):
        rc, msg = _vds_rc(sage, sizes, scale)
        assert rc == sage.ERR_INVALID and "voxel size" in msg, (sizes, scale, rc, msg)


@pytest.mark.parametrize("bad", _BAD_SIZES)
def test_pipeline_create_refuses_a_voxel_size_that_is_not_finite_or_not_above_zero(sage, bad):
    for sizes in ([bad], [0.6, 1.0, bad]):
        cfg = sage.make_pipeline_config(voxel_labels=[[40 + g] for g in range(len(sizes))], voxel_size=sizes)
        assert not sage.lib().sageicp_pipeline_create(C.byref(cfg))
        assert "voxel size" in (sage.lib().sageicp_last_error() or b"").decode()
        with pytest.raises(sage.SageIcpError) as e:
            sage.SageICP(cfg)
        assert e.value.code == sage.ERR_INVALID
