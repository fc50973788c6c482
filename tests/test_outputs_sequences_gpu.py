"""Exports in sequence on one handle (csrc/capi_outputs.hip): rows and records leave through one driver, and every
refusal a kernel raises — a label out of the destination's range, a label out of the record's uint8, a label without a
colour — is a bit in ONE flag word per handle, where the bits of the row and the record kernels overlap in value.  So
after each kind of refusal every sink of the same handle is called: what should succeed does, bit for bit the host rows
(or tests/pc2ref.py's packer of them); what should be refused again is refused with its own text, not the last call's;
a refused call leaves the destination beyond its cap alone.  No fault is constructed: a refusal is a returned code."""
import ctypes

import numpy as np
import pytest
import torch

import pc2ref

DEV = "cuda:0"
ROW_RANGE = "a label does not fit the destination's label type (static_cast<int64_t>(label) out of its range)"
RECORD_RANGE = "a label does not fit the record's uint8 (trunc(label) outside [0, 255])"
NO_COLOUR = "the colour table has no colour for a label"
COLORS = {l: (l * 0x010305 + 7) if l % 3 else -(l * 977 + 1) for l in range(256)}
FILL = 0xEE


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _Source:
    """one exporting handle: the four sinks of its rows, and the host rows once (never written)"""

    def __init__(self, sage, name, rows_call, msg_call, host_cap_call):
        self.sage, self.name, self.rows_call, self.msg_call, self.host_cap_call = sage, name, rows_call, msg_call, host_cap_call
        self.host = rows_call()
        self.host.setflags(write=False)
        self.n = len(self.host)

    # -- the sinks, each to `cap` rows with a guard region behind them -------------------------------------------------------
    def host_rows(self, cap):
        buf = np.full((cap + 2, 4), np.nan)
        n = self.host_cap_call(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if cap else None, cap)
        assert n == self.n, self.name
        k = min(cap, self.n)
        assert np.array_equal(_bits(buf[:k]), _bits(self.host[:k])) and np.isnan(buf[k:]).all(), (self.name, cap)

    def device_rows(self, cap, label_dtype=torch.int32):
        if cap == 0:        # (an empty labels_out has no address to give: the label goes as column 3)
            big = torch.full((2, 4), 7.0, dtype=torch.float64, device=DEV)
            o = self.rows_call(out=big[:0])
            assert o.shape == (0, 4) and (big == 7.0).all(), self.name
            return
        big = torch.full((cap + 2, 3), 7.0, dtype=torch.float32, device=DEV)
        lab = torch.full((cap + 2,), 77, dtype=label_dtype, device=DEV)
        o, l = self.rows_call(out=big[:cap], labels_out=lab[:cap])
        k = min(cap, self.n)
        assert o.shape == (k, 3) and l.shape == (k,), (self.name, cap)
        assert np.array_equal(o.cpu().numpy(), self.host[:k, :3].astype(np.float32)), (self.name, cap)
        assert np.array_equal(l.cpu().numpy(), self.host[:k, 3].astype(np.int64)), (self.name, cap)
        assert (big[k:] == 7.0).all() and (lab[k:] == 77).all(), (self.name, cap)

    def refused_device_rows(self, cap):
        """uint8 labels: refused; nothing at or beyond cap is touched"""
        big = torch.full((cap + 2, 3), 7.0, dtype=torch.float32, device=DEV)
        lab = torch.full((cap + 2,), 77, dtype=torch.uint8, device=DEV)
        with pytest.raises(self.sage.SageIcpError) as e:
            self.rows_call(out=big[:cap], labels_out=lab[:cap])
        assert e.value.code == self.sage.ERR_INVALID and str(e.value).endswith(ROW_RANGE), (self.name, str(e.value))
        assert (big[cap:] == 7.0).all() and (lab[cap:] == 77).all(), self.name

    def records(self, cap, device, colors=COLORS):
        want = pc2ref.pack(self.host[:min(cap, self.n)], colors)
        k = len(want)
        if device:
            big = torch.full((cap * 21 + 32,), FILL, dtype=torch.uint8, device=DEV)
            r = self.msg_call(colors, out=big[1:1 + cap * 21])
            flat = big.cpu().numpy()
            assert r.shape == (k, 21) and np.array_equal(flat[1:1 + k * 21].reshape(k, 21), want), (self.name, cap)
            assert flat[0] == FILL and (flat[1 + k * 21:] == FILL).all(), (self.name, cap)
        else:
            host = np.full(cap * 21 + 32, FILL, dtype=np.uint8)
            r = self.msg_call(colors, out=host[:cap * 21])
            assert r.shape == (k, 21) and np.array_equal(r, want) and (host[k * 21:] == FILL).all(), (self.name, cap)

    def refused_records(self, cap, device, colors, text):
        buf = torch.full((cap * 21 + 32,), FILL, dtype=torch.uint8, device=DEV) if device else \
            np.full(cap * 21 + 32, FILL, dtype=np.uint8)
        with pytest.raises(self.sage.SageIcpError) as e:
            self.msg_call(colors, out=buf[:cap * 21])
        assert e.value.code == self.sage.ERR_INVALID and str(e.value).endswith(text), (self.name, str(e.value))
        tail = buf[cap * 21:]
        assert bool((tail == FILL).all()), self.name


_STATE = {}


def _sources(sage):
    """{name: _Source}: the source cloud, the resident local map and a host map, once with class 40 relabelled 259 (out
    of uint8's and of the record's range) and once as they come (every label has a colour in COLORS)"""
    if _STATE:
        return _STATE
    from sage_icp_amd import synthetic as syn
    frames, _ = syn.make_stream(31, 2, points_per_frame=3000)
    plain = [np.ascontiguousarray(f, dtype=np.float64) for f in frames]
    relabelled = [f.copy() for f in plain]
    for f in relabelled:
        assert (f[:, 3] == 40).any()
        f[f[:, 3] == 40, 3] = 259.0
    L = sage.lib()
    for tag, fs in (("259", relabelled), ("plain", plain)):
        # a label group for 252..259, so that the relabelled points are kept (tests/test_outputs_gpu.py)
        p = sage.SageICP(sage.make_pipeline_config(voxel_labels=sage.KITTI_VOXEL_LABELS + [list(range(252, 260))],
                                                    voxel_size=sage.KITTI_VOXEL_SIZE + [1.0]))
        for f in fs:
            p.RegisterFrame(f)
        h = L.sageicp_pipeline_local_map(p._h)
        assert L.sageicp_map_resident(h)
        m = sage.VoxelHashMap(1.0, 100.0)
        m.AddPoints(fs[0])
        assert not m.resident()

        def source_cap(ptr, cap, p=p):
            k = ctypes.c_uint64(0)
            assert L.sageicp_pipeline_source(p._h, ptr, cap, ctypes.byref(k)) == 0
            return k.value

        def map_cap(handle):
            return lambda ptr, cap: int(L.sageicp_map_pointcloud(handle(), ptr, cap))
        _STATE["source_" + tag] = _Source(sage, "source_" + tag, p.source, p.source_msg, source_cap)
        _STATE["local_map_" + tag] = _Source(sage, "local_map_" + tag, p.LocalMap, p.LocalMapMsg,
                                             map_cap(lambda p=p: L.sageicp_pipeline_local_map(p._h)))
        _STATE["host_map_" + tag] = _Source(sage, "host_map_" + tag, m.Pointcloud, m.PointcloudMsg, map_cap(lambda m=m: m._h))
        _STATE["keep_" + tag] = (p, m)
        assert L.sageicp_map_resident(h) and not m.resident()
    for name, s in _STATE.items():
        if name.startswith("keep_"):
            continue
        # k_egress, k_msg_pack and the gathers run 256 lanes per block: more than one block, and a ragged last one
        assert s.n > 257, (name, s.n)
        has259 = bool((s.host[:s.n - 2, 3] == 259).any())
        assert has259 == name.endswith("259"), name
    return _STATE


WHAT = ["source", "local_map", "host_map"]


def _all_sinks_259(s, cap):
    """what every sink does with rows that hold label 259: rows succeed (int32 labels hold it), records are refused"""
    s.host_rows(cap)
    s.device_rows(cap)
    for device in (False, True):
        s.refused_records(s.n - 2, device, COLORS, RECORD_RANGE)


@pytest.mark.gpu
@pytest.mark.parametrize("what", WHAT)
def test_every_sink_after_a_label_range_refusal_of_device_rows(gpu_sage, what):
    s = _sources(gpu_sage)[what + "_259"]
    for cap in (s.n, 257):
        s.refused_device_rows(s.n - 2)
        _all_sinks_259(s, cap)
    # each sink directly behind the refusal
    for sink in (s.host_rows, s.device_rows):
        s.refused_device_rows(s.n - 2)
        sink(s.n)
    for device in (False, True):
        s.refused_device_rows(s.n - 2)
        s.refused_records(s.n - 2, device, COLORS, RECORD_RANGE)
    assert np.array_equal(_bits(s.rows_call()), _bits(s.host))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["to_host", "to_device"])
@pytest.mark.parametrize("what", WHAT)
def test_every_sink_after_a_label_range_refusal_of_records(gpu_sage, what, device):
    s = _sources(gpu_sage)[what + "_259"]
    for sink in (s.host_rows, s.device_rows):
        s.refused_records(s.n - 2, device, COLORS, RECORD_RANGE)
        sink(s.n)
    s.refused_records(s.n - 2, device, COLORS, RECORD_RANGE)
    s.refused_device_rows(s.n - 2)            # the rows' own refusal, with the rows' text
    s.refused_records(s.n - 2, device, COLORS, RECORD_RANGE)
    _all_sinks_259(s, s.n)
    for cap in (0, 1, 256, 257, s.n):
        s.refused_records(s.n - 2, device, COLORS, RECORD_RANGE)
        s.device_rows(cap)
        s.refused_records(s.n - 2, device, COLORS, RECORD_RANGE)
        s.host_rows(cap)
    assert np.array_equal(_bits(s.rows_call()), _bits(s.host))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["to_host", "to_device"])
@pytest.mark.parametrize("what", WHAT)
def test_every_sink_after_a_missing_colour(gpu_sage, what, device):
    s = _sources(gpu_sage)[what + "_plain"]
    present = sorted({int(l) for l in s.host[:s.n - 2, 3]})
    lacking = {k: v for k, v in COLORS.items() if k != present[len(present) // 2]}
    with pytest.raises(KeyError):
        pc2ref.pack(s.host, lacking)
    for sink in (lambda: s.host_rows(s.n), lambda: s.device_rows(s.n), lambda: s.device_rows(s.n, torch.uint8),
                 lambda: s.records(s.n, False), lambda: s.records(s.n, True)):
        s.refused_records(s.n - 2, device, lacking, NO_COLOUR)
        sink()
    for cap in (0, 1, 256, 257, s.n):
        for sink in (s.host_rows, s.device_rows, lambda c: s.records(c, False), lambda c: s.records(c, True)):
            s.refused_records(s.n - 2, device, lacking, NO_COLOUR)
            sink(cap)
    assert np.array_equal(_bits(s.rows_call()), _bits(s.host))
