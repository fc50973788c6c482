"""Place recognition, the part that needs no device (include/sageicp.h, sageicp_place_*): what is refused, the layout of
the structs, the two host-made tables, and yaw and prior of a shift."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import placeref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refused(sage, params):
    edge2, dirs = np.zeros(70), np.zeros((400, 2))
    _dp = C.POINTER(C.c_double)
    L = sage.lib()
    rcs = [L.sageicp_place_tables(C.byref(params), edge2.ctypes.data_as(_dp), dirs.ctypes.data_as(_dp))]
    out = np.zeros(2 * 16384 + 8, dtype=np.uint8)
    row = np.array([[10.0, 0.0, 0.0, 40.0]])
    rcs.append(L.sageicp_place_describe(row.ctypes.data_as(_dp), 1, C.byref(params), out.ctypes.data_as(C.c_void_p), 0))
    assert not L.sageicp_place_db_create(C.byref(params), 0)
    return all(rc == sage.ERR_INVALID for rc in rcs)


@pytest.mark.parametrize("change", [
    dict(min_range=float("nan")), dict(max_range=float("inf")), dict(z_lo=float("-inf")), dict(z_hi=float("nan")),
    dict(min_range=0.0), dict(min_range=-1.0), dict(min_range=50.0), dict(min_range=60.0),
    dict(z_lo=7.0), dict(z_lo=8.0),
    dict(rings=0), dict(rings=65), dict(rings=-3),
    dict(sectors=2), dict(sectors=361), dict(sectors=0),
    dict(rings=64, sectors=360), dict(rings=64, sectors=257), dict(rings=46, sectors=360),
])
def test_parameters_that_are_refused(sage, change):
    assert _refused(sage, sage.place_params(**change))


@pytest.mark.parametrize("change", [dict(), dict(rings=1, sectors=3), dict(rings=64, sectors=256), dict(rings=45, sectors=360),
                                    dict(min_range=1e-3, max_range=1e-3 * (1 + 2.0 ** -40))])
def test_parameters_that_are_taken(sage, change):
    p = sage.place_params(**change)
    edge2, dirs = sage.place_tables(p)
    assert edge2.shape == (p.rings + 1,) and dirs.shape == (p.sectors, 2)
    assert p.rings * p.sectors <= sage.PLACE_MAX_CELLS


def test_null_arguments_and_queries_that_are_refused(sage):
    L = sage.lib()
    p = sage.place_params()
    assert L.sageicp_place_tables(None, None, None) == sage.ERR_INVALID
    assert L.sageicp_place_tables(C.byref(p), None, None) == sage.ERR_INVALID
    assert L.sageicp_place_describe(None, 0, C.byref(p), None, 0) == sage.ERR_INVALID
    assert L.sageicp_place_describe_device(None, C.byref(p), None, None) == sage.ERR_INVALID
    assert L.sageicp_place_db_size(None) == 0
    for entry in (L.sageicp_place_db_clear, L.sageicp_pipeline_place_reset):
        assert entry(None) == sage.ERR_INVALID
    assert L.sageicp_place_db_add(None, None, 0, None, None) == sage.ERR_INVALID
    assert L.sageicp_place_db_read(None, 0, 0, None, None, None) == sage.ERR_INVALID
    assert L.sageicp_place_db_match(None, None, None, None, None) == sage.ERR_INVALID
    assert L.sageicp_pipeline_place_info(None, None) == sage.ERR_INVALID
    assert not L.sageicp_pipeline_place_db(None)
    L.sageicp_place_db_destroy(None)
    # a row that is not finite is refused before a device is asked
    out = np.zeros(2 * 20 * 60, dtype=np.uint8)
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            rows = np.array([[10.0, 1.0, 0.0, 40.0], [10.0, 1.0, 0.0, 40.0]])
            rows[1, col] = bad
            with pytest.raises(sage.SageIcpError) as e:
                sage.place_describe(rows, p)
            assert e.value.code == sage.ERR_INVALID and "not finite" in str(e.value)


def test_places_need_key_frames(sage):
    p = sage.SageICP(sage.make_pipeline_config())
    with pytest.raises(sage.SageIcpError) as e:
        p.set_places(True, sage.place_params())
    assert e.value.code == sage.ERR_INVALID and "key-frame" in str(e.value)
    p.set_places(False)                                  # off is always taken
    info = p.place_info()
    assert not info["enabled"] and not info["described"] and info["entries"] == 0 and len(info["matches"]) == 0
    assert p.places() is None
    p.place_reset()
    if sage.device_count() == 0:
        return
    p.set_key_frames(True)
    for bad in (dict(top_k=0), dict(top_k=17), dict(h_tol=256), dict(min_similarity=float("nan"))):
        with pytest.raises(sage.SageIcpError) as e:
            p.set_places(True, sage.place_params(), **bad)
        assert e.value.code == sage.ERR_INVALID
    with pytest.raises(sage.SageIcpError):
        p.set_places(True, sage.place_params(rings=0))


def test_struct_sizes_match_the_header(sage):
    names = ["sageicp_place_params", "sageicp_place_query", "sageicp_place_match", "sageicp_place_info"]
    structs = [sage.PlaceParams, sage.PlaceQuery, sage.PlaceMatch, sage.PlaceInfo]
    said = [sage.PLACE_PARAMS_BYTES, sage.PLACE_QUERY_BYTES, sage.PLACE_MATCH_BYTES, sage.PLACE_INFO_BYTES]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){'
    for n, s in zip(names, structs):
        src += 'printf("%%zu ", sizeof(%s));' % n
        src += "".join('printf("%%zu ", offsetof(%s, %s));' % (n, f) for f, _ in s._fields_)
    src += 'printf("%d", SAGEICP_ABI_VERSION);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = []
    for s, b in zip(structs, said):
        assert C.sizeof(s) == b
        want += [b] + [getattr(s, f).offset for f, _ in s._fields_]
        # doubles first, no padding: the fields' sizes add up to the struct's
        assert sum(C.sizeof(t) for _, t in s._fields_) == b
    assert got == want + [4]
    header = open(os.path.join(ROOT, "include", "sageicp.h")).read()
    for n, b in zip(names, said):
        assert "} %s;" % n in header and "%d bytes" % b in header.split("} %s;" % n)[1].split("\n")[0]


@pytest.mark.parametrize("lo,hi,R", [(3.0, 50.0, 20), (0.1, 0.7, 7), (5.0, 120.0, 64), (1e-3, 1e3, 1), (2.5, 81.3, 33)])
def test_ring_edges_bit_for_bit(sage, lo, hi, R):
    p = sage.place_params(min_range=lo, max_range=hi, rings=R, sectors=60 if R < 64 else 256)
    edge2, _ = sage.place_tables(p)
    k = np.arange(R + 1, dtype=np.float64)
    e = np.float64(lo) + k * ((np.float64(hi) - np.float64(lo)) / np.float64(R))
    assert np.array_equal(edge2, e * e)
    assert (np.diff(edge2) > 0).all()


@pytest.mark.parametrize("S", [3, 4, 60, 61, 255, 360])
def test_sector_directions_within_one_ulp(sage, S):
    p = sage.place_params(rings=4, sectors=S)
    _, dirs = sage.place_tables(p)
    a = (2.0 * np.pi * np.arange(S, dtype=np.float64)) / np.float64(S)
    for col, fn in ((0, np.cos), (1, np.sin)):
        want = fn(a)
        ulp = np.spacing(np.maximum(np.abs(want), np.abs(dirs[:, col])))
        assert (np.abs(dirs[:, col] - want) <= ulp).all()
    assert dirs[0, 0] == 1.0 and dirs[0, 1] == 0.0
    assert not np.signbit(dirs[0, 1])


def _yaw(shift, S):
    w = 2.0 * math.pi / S
    return shift * w if shift <= S // 2 else (shift - S) * w


@pytest.mark.parametrize("S", [60, 61, 3, 360])
def test_yaw_and_prior_of_a_shift(sage, S):
    rng = np.random.default_rng(S)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    pose = np.concatenate([q, rng.uniform(-50, 50, size=3)])
    half = S // 2
    for shift in sorted({0, 1, half - 1, half, half + 1, S - 1}):
        yaw, prior = sage.place_prior(pose, shift, S)
        assert yaw == _yaw(shift, S)
        assert (yaw > 0) == (0 < shift <= half) and abs(yaw) <= math.pi * (1 + 2.0 ** -50)
        ref_yaw, ref_prior = placeref.prior(pose, shift, S)
        assert yaw == ref_yaw and np.allclose(prior, ref_prior, rtol=0, atol=2.0 ** -52)
        assert np.array_equal(prior[4:], pose[4:])
        # the prior is the entry's orientation turned by yaw about its own z: q_entry (x) q_z(yaw)
        qz = np.array([0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)])
        x1, y1, z1, w1 = pose[:4]
        x2, y2, z2, w2 = qz
        ham = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
        assert np.allclose(prior[:4], ham, rtol=0, atol=1e-15)
        if shift == 0:
            assert prior.tobytes() == pose.tobytes() and yaw == 0.0
    # S even: shift == S / 2 is +pi, not -pi; S odd: (S - 1) / 2 is the last positive one
    assert sage.place_prior(pose, half, S)[0] > 0 and sage.place_prior(pose, half + 1, S)[0] < 0
    if S % 2 == 0:
        assert sage.place_prior(pose, half, S)[0] == half * (2.0 * math.pi / S)
    with pytest.raises(sage.SageIcpError):
        sage.place_prior(pose, S, S)
    with pytest.raises(sage.SageIcpError):
        sage.place_prior(pose, 0, 2)
