"""GetCorrespondences on a device frame into device memory (sageicp_get_correspondences_device, csrc/correspond.hip)
against the host entry (sageicp_get_correspondences) and the oracle: idx, src and tgt array_equal — every comparison is
bit for bit, no tolerance anywhere.  Needs a real MI355X:  python -m pytest tests -m gpu

The compaction counts per workgroup of 256 queries and scans the counts in one workgroup, 256 counts per step
(kCorrScanTile, correspond.h): 256 * 257 + 1 queries are 258 counts, a second step of the scan with a carry."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LABELS = [0, 0, 10, 40, 44, 50, 70, 71, 80, 251]
TH = 0.4
MD_ALL, MD_NONE, MD_MIXED = 1e3, 1e-7, 0.25
SENTINEL = -7.25
POSE = np.array([0.02, -0.05, 0.1, 0.99, 0.4, -0.3, 0.05])
POSE[:4] /= np.linalg.norm(POSE[:4])
NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8, torch.int32: np.int32,
         torch.int64: np.int64}


def _map_points(seed=11, n=6000, span=6.0):
    rng = np.random.default_rng(seed)
    mp = rng.uniform(-span, span, size=(n, 4))
    mp[:, 2] *= 0.2
    mp[:, 3] = rng.choice(LABELS, size=n)
    return mp


class Scene:
    """the map of 6 000 random points as the product and the oracle hold it, query sets by size, and the reference
    answers (host entry, checked against the oracle), each computed once"""

    def __init__(self, sage, oracle):
        self.sage, self.oracle = sage, oracle
        self.mp = _map_points()
        self.a = sage.VoxelHashMap(1.0, 100.0)
        self.b = oracle.Map(1.0, 100.0, 20, 20)
        self.a.AddPoints(self.mp)
        self.b.add_points(self.mp)
        self.a.sync()
        self.stored = self.a.Pointcloud()
        self._q, self._ref = {}, {}

    def queries(self, n):
        """n map points (as stored), each moved by up to 0.3 per axis: every query has a neighbour within 0.52"""
        if n not in self._q:
            rng = np.random.default_rng(1000 + n)
            q = self.stored[rng.integers(0, len(self.stored), size=n)].copy()
            q[:, :3] += rng.uniform(-0.3, 0.3, size=(n, 3))
            q[:, 3] = rng.choice(LABELS, size=n)
            self._q[n] = q
        return self._q[n]

    def reference(self, q, md, th=TH, key=None):
        if key is not None and key in self._ref:
            return self._ref[key]
        src, tgt, idx = self.a.GetCorrespondences(q, md, th, with_index=True)
        osrc, otgt, oidx = self.b.get_correspondences(q, md, th, with_index=True)
        assert np.array_equal(idx, oidx) and np.array_equal(src, osrc) and np.array_equal(tgt, otgt)
        if key is not None:
            self._ref[key] = (src, tgt, idx)
        return src, tgt, idx


@pytest.fixture(scope="module")
def scene(gpu_sage, oracle):
    return Scene(gpu_sage, oracle)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if t.numel() == 0:                  # (the copy of an empty tensor comes back with strides of 0)
        return torch.empty(t.shape, dtype=t.dtype if dtype is None else dtype, device="cuda")
    return t.cuda() if dtype is None else t.cuda().to(dtype)


def _same(got, want):
    src, tgt, idx = (x.cpu().numpy() for x in got)
    assert np.array_equal(idx, want[2])
    assert np.array_equal(src, want[0]) and np.array_equal(tgt, want[1])


# ---- the C entry on tensors in any layout ----------------------------------------------------------------------------
def _dtype_code(sage, dt):
    return {torch.float32: sage.DTYPE_FLOAT32, torch.float64: sage.DTYPE_FLOAT64, torch.uint8: sage.DTYPE_UINT8,
            torch.int32: sage.DTYPE_INT32, torch.int64: sage.DTYPE_INT64}[dt]


def _rows_struct(sage, struct, t, labels=None, rows=None):
    """DeviceFrame / DevicePoints of a 2-D tensor (and 1-D labels of any of the five types), `rows` of them"""
    r = struct(t.data_ptr() or None, t.stride(0) * t.element_size(), _dtype_code(sage, t.dtype), 0, None, 0,
               t.shape[0] if rows is None else rows)
    if labels is not None:
        r.label, r.label_stride = labels.data_ptr(), labels.stride(0) * labels.element_size()
        r.label_dtype = _dtype_code(sage, labels.dtype)
    r.keep = (t, labels)                # (the struct holds addresses only: a tensor that goes gives its block to the next one)
    return r


def _entry(sage, vmap, frame, md, th=TH, pose=None, src=None, tgt=None, idx=None, idx_cap=0, stream=None):
    """(rc, n_out): frame / src / tgt are structs or None, idx a tensor or None"""
    n = ctypes.c_uint64(987654321)
    pp = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).ctypes.data_as(
        ctypes.POINTER(ctypes.c_double))
    rc = sage.lib().sageicp_get_correspondences_device(
        vmap._h, ctypes.byref(frame), pp, md, th, None if src is None else ctypes.byref(src),
        None if tgt is None else ctypes.byref(tgt), None if idx is None else idx.data_ptr(), idx_cap,
        torch.cuda.current_stream().cuda_stream if stream is None else stream, ctypes.byref(n))
    return rc, n.value


def _strided(dtype, rows, cols, stride, offset, fill=SENTINEL):
    """(base, view): a (rows, cols) view with row stride `stride` elements, `offset` elements into a 1-D base tensor
    that is filled with the sentinel (torch's allocations are aligned to 512 bytes)"""
    base = torch.full((offset + max(rows, 1) * stride + 8,), fill, dtype=dtype, device="cuda")
    view = base[offset:offset + rows * stride].view(rows, stride)[:, :cols] if rows else base[offset:offset].view(0, cols)
    return base, view


# ---- compaction edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("md", [MD_ALL, MD_NONE, MD_MIXED], ids=["all", "none", "mixed"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, 256 * 257 + 1])
def test_compaction_edges(scene, n, md):
    q = scene.queries(n)
    want = scene.reference(q, md, key=(n, md))
    got = scene.a.GetCorrespondences(_dev(q), md, TH, with_index=True)
    k = len(got[2])
    if md == MD_ALL:
        assert k == n
    elif md == MD_NONE:
        assert k == 0
    elif n >= 63:
        assert 0 < k < n
    assert got[0].shape == (k, 4) and got[1].shape == (k, 4) and got[2].dtype == torch.int64
    _same(got, want)


PATTERNS = {
    "alternating": lambda i: i % 2 == 0,
    "alternating_odd": lambda i: i % 2 == 1,
    "first_of_each_wave": lambda i: i % 64 == 0,
    "last_of_each_wave": lambda i: i % 64 == 63,
    "64_on_64_off": lambda i: (i // 64) % 2 == 0,
    "64_off_64_on": lambda i: (i // 64) % 2 == 1,
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", [256, 300])
def test_hand_made_patterns(scene, pattern, n):
    """queries ON stored map points (distance 0: accepted) or 0.01 beside them (rejected at 1e-3)"""
    on = np.array([PATTERNS[pattern](i) for i in range(n)])
    rng = np.random.default_rng(5)
    pick = rng.choice(len(scene.stored), size=n, replace=False)
    q = scene.stored[pick].copy()
    q[~on, 0] += 0.01
    want = scene.reference(q, 1e-3)
    assert np.array_equal(want[2], np.flatnonzero(on))             # the pattern is what the reference accepts
    assert np.array_equal(want[1], scene.stored[pick][on])         # ... each query's own map point
    _same(scene.a.GetCorrespondences(_dev(q), 1e-3, TH, with_index=True), want)


def test_the_sorted_searchs_permutation_is_undone(scene):
    rng = np.random.default_rng(77)
    q = scene.queries(700)[rng.permutation(700)]
    want = scene.reference(q, MD_MIXED)
    got = scene.a.GetCorrespondences(_dev(q), MD_MIXED, TH, with_index=True)
    idx = got[2].cpu().numpy()
    assert len(idx) > 100 and (np.diff(idx) > 0).all()
    _same(got, want)
    src2, tgt2 = scene.a.GetCorrespondences(_dev(q), MD_MIXED, TH)           # without the index
    assert np.array_equal(src2.cpu().numpy(), want[0]) and np.array_equal(tgt2.cpu().numpy(), want[1])


# ---- capacity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_of_k", [lambda k: 0, lambda k: 1, lambda k: k - 1, lambda k: k, lambda k: k + 1],
                         ids=["0", "1", "k-1", "k", "k+1"])
def test_cap_writes_the_first_pairs_and_nothing_else(scene, cap_of_k):
    sage = scene.sage
    q = scene.queries(513)
    want = scene.reference(q, MD_MIXED, key=(513, MD_MIXED))
    k = len(want[2])
    cap = cap_of_k(k)
    rows = k + 5                                    # the tensors are larger than the cap they are declared with
    src = torch.full((rows, 4), SENTINEL, dtype=torch.float64, device="cuda")
    tgt = torch.full((rows, 4), SENTINEL, dtype=torch.float64, device="cuda")
    idx = torch.full((rows,), -99, dtype=torch.int64, device="cuda")
    f = _rows_struct(sage, sage.DeviceFrame, _dev(q))
    rc, n = _entry(sage, scene.a, f, MD_MIXED, src=_rows_struct(sage, sage.DevicePoints, src, rows=cap),
                   tgt=_rows_struct(sage, sage.DevicePoints, tgt, rows=cap), idx=idx, idx_cap=cap)
    assert rc == 0 and n == k
    w = min(cap, k)
    for got, exp, fill in ((src, want[0], SENTINEL), (tgt, want[1], SENTINEL), (idx, want[2], -99)):
        got = got.cpu().numpy()
        assert np.array_equal(got[:w], exp[:w])
        assert (got[w:] == fill).all()


def test_three_nulls_count_only(scene):
    sage = scene.sage
    q = scene.queries(513)
    want = scene.reference(q, MD_MIXED, key=(513, MD_MIXED))
    f = _rows_struct(sage, sage.DeviceFrame, _dev(q))
    assert _entry(sage, scene.a, f, MD_MIXED) == (0, len(want[2]))
    # ... and each destination alone
    idx = torch.full((513,), -99, dtype=torch.int64, device="cuda")
    assert _entry(sage, scene.a, f, MD_MIXED, idx=idx, idx_cap=513) == (0, len(want[2]))
    assert np.array_equal(idx.cpu().numpy()[:len(want[2])], want[2])
    tgt = torch.full((513, 4), SENTINEL, dtype=torch.float64, device="cuda")
    assert _entry(sage, scene.a, f, MD_MIXED, tgt=_rows_struct(sage, sage.DevicePoints, tgt)) == (0, len(want[2]))
    assert np.array_equal(tgt.cpu().numpy()[:len(want[2])], want[1])


# ---- layouts -----------------------------------------------------------------------------------------------------------
# (frame dtype, frame label dtype or None for column 3, frame offset, frame stride) -> (out dtype, out label dtype or None,
# out offset in elements, out stride in elements): offsets of 1 element are 4 bytes for float32 and 8 for float64, i.e. a
# base that is not 16-B aligned: the element-wise writer; offset 0 / 4 with a stride of 4 or 8: the 16-B one
LAYOUTS = [
    (torch.float64, None, 0, 4, torch.float64, None, 0, 4),
    (torch.float32, None, 0, 4, torch.float32, None, 0, 4),
    (torch.float64, None, 1, 5, torch.float64, None, 1, 4),
    (torch.float32, None, 1, 7, torch.float32, None, 1, 4),
    (torch.float64, torch.uint8, 0, 3, torch.float32, torch.uint8, 0, 3),
    (torch.float32, torch.int32, 0, 4, torch.float64, torch.int32, 0, 4),
    (torch.float32, torch.int64, 1, 3, torch.float64, torch.int64, 1, 3),
    (torch.float64, torch.int64, 0, 8, torch.float64, torch.float32, 0, 8),
    (torch.float64, None, 0, 4, torch.float32, torch.float64, 0, 6),
    (torch.float32, None, 0, 8, torch.float64, None, 0, 6),
    (torch.float64, torch.int32, 2, 6, torch.float32, None, 4, 8),
]


@pytest.mark.parametrize("lay", LAYOUTS, ids=["-".join(str(x).replace("torch.", "") for x in lay) for lay in LAYOUTS])
def test_layouts_in_and_out(scene, lay):
    sage = scene.sage
    fdt, fl, foff, fstride, odt, ol, ooff, ostride = lay
    n = 300
    q = scene.queries(n).astype(NP_OF[fdt]).astype(np.float64)         # what a (double) cast of the frame gives
    want = scene.reference(q, MD_MIXED)
    k = len(want[2])
    assert 0 < k < n
    # the frame
    cols = 4 if fl is None else 3
    _, fv = _strided(fdt, n, cols, max(fstride, cols), foff)
    fv.copy_(_dev(q[:, :cols], fdt))
    flab = None if fl is None else _dev(q[:, 3], fl)
    f = _rows_struct(sage, sage.DeviceFrame, fv, flab)
    # the destinations
    ocols = 4 if ol is None else 3
    outs = []
    for _ in range(2):
        base, view = _strided(odt, n, ocols, max(ostride, ocols), ooff)
        lab = None if ol is None else torch.full((2 * n,), 99, dtype=ol, device="cuda")[::2]     # stride of 2 labels
        outs.append((base, view, lab))
    idx = torch.full((n,), -99, dtype=torch.int64, device="cuda")
    rc, got_k = _entry(sage, scene.a, f, MD_MIXED, src=_rows_struct(sage, sage.DevicePoints, outs[0][1], outs[0][2]),
                       tgt=_rows_struct(sage, sage.DevicePoints, outs[1][1], outs[1][2]), idx=idx, idx_cap=n)
    assert rc == 0, sage.lib().sageicp_last_error()
    assert got_k == k
    assert np.array_equal(idx.cpu().numpy()[:k], want[2]) and (idx.cpu().numpy()[k:] == -99).all()
    for (base, view, lab), exp in zip(outs, want[:2]):
        got = view.cpu().numpy()
        assert np.array_equal(got[:k], exp[:, :ocols].astype(NP_OF[odt]))
        if lab is not None:
            assert np.array_equal(lab.cpu().numpy()[:k], exp[:, 3].astype(NP_OF[ol]))
            assert (lab.cpu().numpy()[k:] == 99).all()
        # nothing but the k rows' own columns was written
        touched = torch.zeros_like(base, dtype=torch.bool)
        touched[ooff:ooff + n * max(ostride, ocols)].view(n, max(ostride, ocols))[:k, :ocols] = True
        assert (base[~touched] == SENTINEL).all()


def test_a_label_that_does_not_fit_uint8_is_refused(scene):
    sage = scene.sage
    q = scene.queries(64).copy()
    q[7, 3] = 259.0
    f = _rows_struct(sage, sage.DeviceFrame, _dev(q))
    src = torch.zeros((64, 3), dtype=torch.float64, device="cuda")
    lab = torch.zeros(64, dtype=torch.uint8, device="cuda")
    rc, n = _entry(sage, scene.a, f, MD_ALL, src=_rows_struct(sage, sage.DevicePoints, src, lab))
    assert rc == sage.ERR_INVALID and n == 987654321
    assert "label" in sage.lib().sageicp_last_error().decode()
    # the same frame into labels that hold it
    lab64 = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert _entry(sage, scene.a, f, MD_ALL, src=_rows_struct(sage, sage.DevicePoints, src, lab64)) == (0, 64)
    assert lab64[7].item() == 259


# ---- pose --------------------------------------------------------------------------------------------------------------
def test_pose_moves_the_queries_as_transform_points_does(scene):
    sage = scene.sage
    inv = scene.oracle.se3_inv(POSE)
    q0 = sage.transform_points(inv, scene.queries(513))              # so that the moved rows land on the map
    moved = sage.transform_points(POSE, q0)
    want = scene.reference(moved, MD_MIXED)
    assert 0 < len(want[2]) < 513
    _same(scene.a.GetCorrespondences(_dev(q0), MD_MIXED, TH, with_index=True, pose=POSE), want)
    # float32 in and out: the (double) cast first, then the pose
    q32 = q0.astype(np.float32)
    want32 = scene.reference(sage.transform_points(POSE, q32.astype(np.float64)), MD_MIXED)
    got = scene.a.GetCorrespondences(_dev(q32), MD_MIXED, TH, with_index=True, pose=POSE, dtype=torch.float32)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32
    _same(got, (want32[0].astype(np.float32), want32[1].astype(np.float32), want32[2]))


def test_no_pose_is_the_identity(scene):
    q = scene.queries(513)
    want = scene.reference(q, MD_MIXED, key=(513, MD_MIXED))
    _same(scene.a.GetCorrespondences(_dev(q), MD_MIXED, TH, with_index=True, pose=[0, 0, 0, 1, 0, 0, 0]), want)
    _same(scene.a.GetCorrespondences(_dev(q), MD_MIXED, TH, with_index=True, pose=None), want)


# ---- map states ----------------------------------------------------------------------------------------------------------
def _status(m):
    st = m.loop_status()
    return tuple(int(getattr(st, f)) for f, _ in st._fields_)


def test_map_states(scene):
    sage, oracle = scene.sage, scene.oracle
    q = scene.queries(513)
    want = scene.reference(q, MD_MIXED, key=(513, MD_MIXED))
    qt = _dev(q)
    # host-built, never searched: the call builds the mirror
    m = sage.VoxelHashMap(1.0, 100.0)
    m.AddPoints(scene.mp)
    assert not m.resident()
    _same(m.GetCorrespondences(qt, MD_MIXED, TH, with_index=True), want)
    assert not m.resident()
    # mirrored after sync(), and after a host-side change behind the mirror
    m.sync()
    _same(m.GetCorrespondences(qt, MD_MIXED, TH, with_index=True), want)
    # a clone of a host map
    _same(m.clone().GetCorrespondences(qt, MD_MIXED, TH, with_index=True), want)
    # after UpdateOnDevice: the HBM copy is the map, and stays it
    extra = _map_points(seed=12, n=2000)
    pose = np.array([0.0, 0.0, 0.0, 1.0, 0.3, -0.2, 0.0])
    twin = sage.VoxelHashMap(1.0, 100.0)
    twin.AddPoints(scene.mp)
    twin.Update(extra, pose)
    otwin = oracle.Map(1.0, 100.0, 20, 20)
    otwin.add_points(scene.mp)
    otwin.update(extra, pose)
    wsrc, wtgt, widx = twin.GetCorrespondences(q, MD_MIXED, TH, with_index=True)
    osrc, otgt, oidx = otwin.get_correspondences(q, MD_MIXED, TH, with_index=True)
    assert np.array_equal(widx, oidx) and np.array_equal(wtgt, otgt) and np.array_equal(wsrc, osrc)
    assert len(widx) != len(want[2]) or not np.array_equal(wtgt, want[1])                # the update changed the answer
    m.UpdateOnDevice(extra, pose)
    assert m.resident()
    before = (m.table_stats(), _status(m), m.size(), m.num_voxels())
    _same(m.GetCorrespondences(qt, MD_MIXED, TH, with_index=True), (wsrc, wtgt, widx))
    assert m.resident()
    assert (m.table_stats(), _status(m), m.size(), m.num_voxels()) == before
    # a clone of a resident map (device to device)
    c = m.clone()
    assert c.resident()
    _same(c.GetCorrespondences(qt, MD_MIXED, TH, with_index=True), (wsrc, wtgt, widx))
    assert c.resident() and m.resident()
    # after Clear(), and a map that never held a point: 0 pairs
    m.Clear()
    for empty in (m, sage.VoxelHashMap(1.0, 100.0)):
        got = empty.GetCorrespondences(qt, MD_MIXED, TH, with_index=True)
        assert [tuple(x.shape) for x in got] == [(0, 4), (0, 4), (0,)]


# ---- kernel forms ------------------------------------------------------------------------------------------------------
def test_every_lane_width_and_scan_form(scene, scan_form):
    q = scene.queries(700)
    want = scene.reference(q, MD_MIXED, key=(700, MD_MIXED))
    qt = _dev(q)
    old = os.environ.get("SAGEICP_LW")
    try:
        for lw in range(5):
            os.environ["SAGEICP_LW"] = str(lw)
            _same(scene.a.GetCorrespondences(qt, MD_MIXED, TH, with_index=True), want)
    finally:
        if old is None:
            os.environ.pop("SAGEICP_LW", None)
        else:
            os.environ["SAGEICP_LW"] = old


# ---- streams -------------------------------------------------------------------------------------------------------------
def test_a_frame_produced_on_another_stream_is_waited_for(scene):
    q = scene.queries(513)
    want = scene.reference(q, MD_MIXED, key=(513, MD_MIXED))
    half = _dev(q * 0.5)
    busy = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):                          # the stream is busy when the frame's kernel is enqueued
            busy = busy @ busy * 1e-4
        frame = half + half                         # exact: the frame exists once this kernel has run
        got = scene.a.GetCorrespondences(frame, MD_MIXED, TH, with_index=True)      # at once, no synchronisation
        copies = [x.clone() for x in got]           # consumed on that stream
    s.synchronize()
    _same(copies, want)


# ---- alias -----------------------------------------------------------------------------------------------------------------
def test_src_out_may_be_the_frame_itself(scene):
    sage = scene.sage
    q = scene.queries(513)
    want = scene.reference(q, MD_MIXED, key=(513, MD_MIXED))
    k = len(want[2])
    t = _dev(q)
    tgt = torch.full((513, 4), SENTINEL, dtype=torch.float64, device="cuda")
    idx = torch.full((513,), -99, dtype=torch.int64, device="cuda")
    rc, n = _entry(sage, scene.a, _rows_struct(sage, sage.DeviceFrame, t), MD_MIXED,
                   src=_rows_struct(sage, sage.DevicePoints, t), tgt=_rows_struct(sage, sage.DevicePoints, tgt), idx=idx,
                   idx_cap=513)
    assert rc == 0 and n == k
    got = t.cpu().numpy()
    assert np.array_equal(got[:k], want[0]) and np.array_equal(got[k:], q[k:])      # the pairs, then the frame as it was
    assert np.array_equal(tgt.cpu().numpy()[:k], want[1]) and np.array_equal(idx.cpu().numpy()[:k], want[2])


# ---- refusals that need the device ---------------------------------------------------------------------------------------
def test_host_and_pinned_destinations_are_refused(scene):
    sage = scene.sage
    f = _rows_struct(sage, sage.DeviceFrame, _dev(scene.queries(64)))
    for pin in (False, True):
        out = torch.full((64, 4), SENTINEL, dtype=torch.float64, pin_memory=pin)
        ok = torch.full((64, 4), SENTINEL, dtype=torch.float64, device="cuda")
        hidx = torch.full((64,), -99, dtype=torch.int64, pin_memory=pin)
        didx = torch.full((64,), -99, dtype=torch.int64, device="cuda")
        for kw in (dict(src=_rows_struct(sage, sage.DevicePoints, out), tgt=_rows_struct(sage, sage.DevicePoints, ok)),
                   dict(src=_rows_struct(sage, sage.DevicePoints, ok), tgt=_rows_struct(sage, sage.DevicePoints, out)),
                   dict(src=_rows_struct(sage, sage.DevicePoints, ok), idx=hidx, idx_cap=64)):
            rc, n = _entry(sage, scene.a, f, MD_ALL, **kw)
            assert rc == sage.ERR_INVALID and n == 987654321
            assert "device memory" in sage.lib().sageicp_last_error().decode()
            assert (out == SENTINEL).all() and (ok.cpu() == SENTINEL).all()
            assert (hidx == -99).all() and (didx.cpu() == -99).all()


def test_a_tensor_of_another_gpu_index_is_refused(scene):
    sage = scene.sage
    other = sage.VoxelHashMap(1.0, 100.0, device=1)                 # a handle of GPU 1, whether or not there is one
    q = _dev(scene.queries(64))
    with pytest.raises(ValueError, match="the frame is on cuda:0, the pipeline / map on GPU 1"):
        other.GetCorrespondences(q, MD_ALL, TH)
    src = torch.full((64, 4), SENTINEL, dtype=torch.float64, device="cuda")
    rc, n = _entry(sage, other, _rows_struct(sage, sage.DeviceFrame, q), MD_ALL,
                   src=_rows_struct(sage, sage.DevicePoints, src))
    assert rc == sage.ERR_INVALID and n == 987654321
    assert "lives on device 0, the handle on device 1" in sage.lib().sageicp_last_error().decode()
    assert (src.cpu() == SENTINEL).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("col", [0, 2, 3])
def test_a_frame_that_is_not_finite_is_refused(scene, bad, col):
    sage = scene.sage
    q = scene.queries(513).copy()
    q[400, col] = bad
    src = torch.full((513, 4), SENTINEL, dtype=torch.float64, device="cuda")
    tgt = torch.full((513, 4), SENTINEL, dtype=torch.float64, device="cuda")
    idx = torch.full((513,), -99, dtype=torch.int64, device="cuda")
    rc, n = _entry(sage, scene.a, _rows_struct(sage, sage.DeviceFrame, _dev(q)), MD_ALL,
                   src=_rows_struct(sage, sage.DevicePoints, src), tgt=_rows_struct(sage, sage.DevicePoints, tgt), idx=idx,
                   idx_cap=513)
    assert rc == sage.ERR_INVALID and n == 987654321
    assert "not finite" in sage.lib().sageicp_last_error().decode()
    assert (src.cpu() == SENTINEL).all() and (tgt.cpu() == SENTINEL).all() and (idx.cpu() == -99).all()
    with pytest.raises(sage.SageIcpError):
        scene.a.GetCorrespondences(_dev(q), MD_ALL, TH)
