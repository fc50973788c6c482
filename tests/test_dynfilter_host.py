"""Host-side tests of Preprocess()'s dynamic vehicle filter (core/Preprocessing.cpp:95-172): the independent CPU
restatement (tests/dynfilter_ref.cpp) against hand-derived answers, the library's replay of PCL's cluster order
against the restatement's, the C ABI additions where no device is needed, and csrc/dyn_rules.h (the label cast and the
static test) compiled for the host against the reference's expressions."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dynref
import dynscenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(dynref.kat_scenes()))
def test_restatement_known_answers(name):
    frame, dy_th, expected = dynref.kat_scenes()[name]
    out, info = dynref.preprocess(frame, dy_th=dy_th, dynamic_labels=(10,), landmark_labels=(44,), **dynref.KAT_RANGES)
    assert np.array_equal(out, expected)
    if name == "chain_0.49_one_cluster":
        assert (info["clusters"], info["clusters_kept"], info["points_removed"]) == (1, 1, 0)
    if name == "exactly_0.5_not_linked":
        assert info["clusters"] == 0 and info["points_removed"] == 6
    if name == "count_5_of_10":
        assert (info["clusters"], info["clusters_kept"]) == (1, 0)
    if name == "no_vehicles":
        assert np.array_equal(out, dynref.crop_only(frame, **dynref.KAT_RANGES))


def test_restatement_without_vehicles_is_the_crop():
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(3, 1, points_per_frame=20000)
    f = frames[0]
    out, info = dynref.preprocess(f, dynamic_labels=(12345,))
    assert info["vehicle_points"] == 0
    assert np.array_equal(out, dynref.crop_only(f))


def test_restatement_refuses_a_non_finite_label():
    f = np.array([[10.0, 0.0, 0.0, np.nan], [11.0, 0.0, 0.0, 10.0]])
    with pytest.raises(ValueError):
        dynref.preprocess(f)
    # ... but not one the crop drops first
    f = np.array([[200.0, 0.0, 0.0, np.nan], [11.0, 0.0, 0.0, 40.0]])
    out, _ = dynref.preprocess(f)
    assert len(out) == 1


def test_synthetic_scene_plants_what_it_says():
    from sage_icp_amd import synthetic_dynamic as sd
    f, parts = sd.make_dynamic_scan(4, return_parts=True)
    assert len(f) == 120000
    assert np.array_equal(f[:, :3], f[:, :3].astype(np.float32).astype(np.float64))
    f2 = sd.make_dynamic_scan(4)
    assert np.array_equal(f, f2)
    out, info = dynref.preprocess(f, dy_th=0.5)
    # 20 parked cars kept, 6 moving cars + 4 kerb cars + fragments removed, far cars are ordinary points
    assert info["clusters_kept"] == 20 and info["clusters"] == 30
    assert info["points_removed"] == len(parts["moving"]) + len(parts["kerb"]) + len(parts["fragment"])
    # the kept clusters have equal sizes, more than 16 of them: the order depends on the unstable sort
    assert len(parts["parked"]) == 20 * sd.CAR_POINTS


def test_cluster_emission_order_matches_the_restatement(sage):
    rng = np.random.default_rng(17)
    for trial in range(300):
        n = int(rng.integers(1, 201))
        hi = int(rng.choice([2, 4, 10, 300]))            # few distinct sizes: many ties
        sizes = rng.integers(5, 5 + hi, size=n).astype(np.uint32)
        got = sage.cluster_emission_order(sizes)
        want = dynref.emission_order(sizes)
        assert np.array_equal(got, want), (trial, n)
        assert sorted(got.tolist()) == list(range(n))
        assert np.all(np.diff(sizes[got].astype(np.int64)) <= 0)
    # more than 16 equal sizes: not the identity (std::sort is not stable there)
    eq = np.full(40, 284, dtype=np.uint32)
    got = sage.cluster_emission_order(eq)
    assert np.array_equal(got, dynref.emission_order(eq)) and not np.array_equal(got, np.arange(40))
    assert len(sage.cluster_emission_order(np.zeros(0, dtype=np.uint32))) == 0


def test_dynamic_entries_need_a_device(sage):
    if sage.device_count() > 0:
        pytest.skip("a HIP device is present")
    f = np.array([[10.0, 0.0, 0.0, 10.0]] * 6)
    with pytest.raises(sage.SageIcpError) as e:
        sage.preprocess(f, 100.0, 5.0, 50.0, dynamic_vehicle_filter=True, dynamic_labels=(10,))
    assert e.value.code == sage.ERR_NO_DEVICE
    p = sage.SageICP(sage.make_pipeline_config(dynamic_vehicle_filter=True))
    with pytest.raises(sage.SageIcpError) as e:
        p.RegisterFrame(f)
    assert e.value.code == sage.ERR_NO_DEVICE


def test_pipeline_dynamic_filter_setter(sage):
    L = sage.lib()
    p = sage.SageICP(sage.make_pipeline_config())
    assert p.dynamic_filter_info()["vehicle_points"] == 0
    with pytest.raises(sage.SageIcpError) as e:
        p.set_dynamic_vehicle_filter(True, 0.5, 6)           # six label groups: voxid 0..5
    assert e.value.code == sage.ERR_INVALID
    with pytest.raises(sage.SageIcpError):
        p.set_dynamic_vehicle_filter(True, 0.5, -1)
    with pytest.raises(sage.SageIcpError):
        p.set_dynamic_vehicle_filter(True, float("nan"), 5)
    p.set_dynamic_vehicle_filter(True, 0.5, 5, (44, 48))
    p.set_dynamic_vehicle_filter(False)
    assert L.sageicp_pipeline_set_dynamic_vehicle_filter(None, 1, 0.5, 5, None, 0) == sage.ERR_INVALID
    assert L.sageicp_pipeline_dynamic_filter_info(p._h, None) == sage.ERR_INVALID
    cfg = sage.make_pipeline_config(dynamic_vehicle_filter=True, dynamic_vehicle_voxid=7)
    with pytest.raises(sage.SageIcpError):
        sage.SageICP(cfg)
    assert L.sageicp_cluster_emission_order(None, 3, None) == sage.ERR_INVALID


def test_dynfilter_info_layout_matches_header(sage):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "sageicp.h"\nint main(void){printf("%zu", sizeof(sageicp_dynfilter_info));' + \
          "".join('printf(" %%zu", offsetof(sageicp_dynfilter_info, %s));' % f for f, _ in sage.DynFilterInfo._fields_) + \
          'printf(" %d", SAGEICP_ABI_VERSION);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[0] == ctypes.sizeof(sage.DynFilterInfo) == 64
    assert got[1:-1] == [getattr(sage.DynFilterInfo, f).offset for f, _ in sage.DynFilterInfo._fields_]
    assert got[-1] == 4 == sage.ABI_VERSION


# ---- the label and threshold edges (tests/dynscenes.py), and dyn_rules.h against the reference's expressions ------
@pytest.mark.parametrize("name", sorted(dynscenes.label_kat_scenes()))
def test_restatement_label_known_answers(name):
    frame, kw, expected = dynscenes.label_kat_scenes()[name]
    out, _ = dynref.preprocess(frame, **kw, **dynref.KAT_RANGES)
    assert np.array_equal(out, expected)


@pytest.mark.parametrize("name", sorted(dynscenes.threshold_kat_scenes()))
def test_restatement_threshold_known_answers(name):
    frame, kw, expected = dynscenes.threshold_kat_scenes()[name]
    out, info = dynref.preprocess(frame, **kw, **dynref.KAT_RANGES)
    assert np.array_equal(out, expected)
    assert info["clusters"] == 3 and info["vehicle_points"] == 24


RULES_SRC = r'''
#include "dyn_rules.h"
extern "C" int dr_static(unsigned long long count, unsigned size, double dy_th) {
    return sageicp::cluster_is_static(count, size, dy_th) ? 1 : 0;
}
extern "C" unsigned dr_label(double l) { return sageicp::label_code(l); }
// the reference's expressions (Preprocessing.cpp:107-111, 141-158), as tests/dynfilter_ref.cpp states them
extern "C" int ref_static(int count, int size, double dy_th) {
    int count_size = 0;
    for (int k = 0; k < count; ++k) {
        ++count_size;
        if (count_size > static_cast<int>(dy_th * static_cast<double>(size))) return 1;
    }
    return 0;
}
extern "C" unsigned ref_label(double l) { return static_cast<uint32_t>(static_cast<long long>(l)); }
'''


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    d = tmp_path_factory.mktemp("dyn_rules")
    src, so = d / "rules.cpp", d / "librules.so"
    src.write_text(RULES_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "sage-icp_amd", "csrc"), str(src), "-o", str(so)])
    L = ctypes.CDLL(str(so))
    L.dr_static.argtypes = [ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_double]
    L.ref_static.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double]
    L.dr_label.argtypes = L.ref_label.argtypes = [ctypes.c_double]
    L.dr_label.restype = L.ref_label.restype = ctypes.c_uint
    return L


def test_cluster_is_static_follows_the_reference_expression(rules):
    counts = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 99, 100, 101, 1000)
    sizes = (5, 6, 7, 8, 10, 100, 1000, 65537)
    ths = [-1e300, -1e10, -2.0 ** 31, -1.0, -0.5, 0.0, 0.1, 0.5, 0.75, 1.0, 2.0, 10.0, 1e10, 1e300, float("nan")]
    for s in sizes:        # either side of the int range of dy_th * size
        for edge in (2.0 ** 31 / s, -(2.0 ** 31) / s, (2.0 ** 31 + 1) / s):
            ths += [float(np.nextafter(edge, -np.inf)), edge, float(np.nextafter(edge, np.inf))]
    for s in sizes:
        for th in ths:
            for c in counts:
                assert rules.dr_static(c, s, th) == rules.ref_static(c, s, th), (c, s, th)
    # the overflow: static_cast<int> gives INT_MIN, so one landmark neighbour keeps any cluster
    assert rules.ref_static(1, 10, 1e10) == 1 and rules.dr_static(1, 10, 1e10) == 1
    assert rules.dr_static(1 << 40, 10, 2.0 ** 31 / 10 * 0.999) == 1 and rules.dr_static(0, 10, 1e10) == 0
    assert rules.dr_static(2 ** 31 - 1, 8, float(np.nextafter(2.0 ** 28, 0))) == 0


def test_label_code_follows_the_reference_cast(rules):
    ls = [0.0, -0.0, 0.5, -0.5, 10.9, -1.0, -1.5, 4294967295.0, 4294967296.0, 4294967306.0, 2.0 ** 53, -(2.0 ** 53),
          2.0 ** 63 - 1024, -(2.0 ** 63), float(np.nextafter(-(2.0 ** 63), -np.inf)), 2.0 ** 63, 1e19, -1e19, 1e300,
          -1e300, 2.0 ** 64 + 2.0 ** 33]
    for l in ls:
        assert rules.dr_label(l) == rules.ref_label(l), l
    assert [rules.dr_label(l) for l in (10.9, -0.5, -1.0, 4294967306.0, 1e19, -1e19)] == [10, 0, 0xFFFFFFFF, 10, 0, 0]
