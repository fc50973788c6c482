// The archive of a map handle on the host side of libsageicp_hip.so (archive.h): the store (MapArchive), the
// host copy's sweep feeding it, and the C entries — the setting, the info, the records and the three selections of an
// export (the log, its latest generations, the session's map), which leave through export_rows (outputs.h) like every
// other cloud.  The kernels are archive.hip's.  Host code only.
#include "capi_internal.h"

namespace sageicp_impl {

// ---- the store ---------------------------------------------------------------------------------------------------------
void MapArchive::append_host(const int32_t key[3], const Point4 *p, uint32_t count, uint64_t serial) {
    if (full || (max_rows && rows() + count > max_rows)) {      // the first voxel that does not fit: full for good
        full = true;
        dropped_rows += count;
        ++dropped_voxels;
        return;
    }
    h_vox.push_back(ArchiveVoxel{key[0], key[1], key[2], count, rows(), serial});
    h_rows.insert(h_rows.end(), p, p + count);
}

void MapArchive::clear() {
    std::vector<Point4>().swap(h_rows);
    std::vector<ArchiveVoxel>().swap(h_vox);
    d_rows.reset();
    d_vox.reset();
    d_ctr.reset();
    dev_rows = dev_vox = 0;
    full = false;
    dropped_rows = dropped_voxels = 0;
    updates = 0;
}

// the first capacity of the device part (SAGEICP_ARCHIVE_INITIAL_ROWS: a test forces re-allocations with it)
static uint64_t initial_rows() { return static_cast<uint64_t>(knobs().archive_initial_rows.get()); }

static int grow_to(MapArchive &a, uint64_t need_rows, uint64_t need_vox, hipStream_t s) {
    if (need_rows > a.d_rows.capacity()) {
        const uint64_t cap = std::max<uint64_t>(need_rows, std::max<uint64_t>(initial_rows(), 2 * a.d_rows.capacity()));
        HIPCHK(a.d_rows.grow(cap, a.dev_rows, s));
    }
    if (need_vox > a.d_vox.capacity()) {
        const uint64_t cap = std::max<uint64_t>(need_vox, std::max<uint64_t>(initial_rows() / 4 + 1, 2 * a.d_vox.capacity()));
        HIPCHK(a.d_vox.grow(cap, a.dev_vox, s));
    }
    return SAGEICP_OK;
}

int MapArchive::flush_pending(hipStream_t s) {
    if (h_vox.empty()) return SAGEICP_OK;
    if (int rc = grow_to(*this, rows(), voxels(), s)) return rc;
    HIPCHK(hipMemcpyAsync(d_rows.data() + dev_rows, h_rows.data(), h_rows.size() * sizeof(Point4), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_vox.data() + dev_vox, h_vox.data(), h_vox.size() * sizeof(ArchiveVoxel), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    dev_rows += h_rows.size();
    dev_vox += h_vox.size();
    std::vector<Point4>().swap(h_rows);
    std::vector<ArchiveVoxel>().swap(h_vox);
    return SAGEICP_OK;
}

int MapArchive::reserve(uint64_t rows_bound, uint64_t vox_bound, hipStream_t s) {
    if (!d_ctr) HIPCHK(d_ctr.reserve(1));
    if (full) return SAGEICP_OK;                 // evictions are only counted from here on
    uint64_t need_rows = dev_rows + rows_bound, need_vox = dev_vox + vox_bound;
    if (max_rows) {                              // (a voxel holds a row at least)
        need_rows = std::min(need_rows, max_rows);
        need_vox = std::min(need_vox, dev_vox + (max_rows - dev_rows));
    }
    return grow_to(*this, need_rows, need_vox, s);
}

int MapArchive::copy_from(const MapArchive &src, hipStream_t s) {
    enabled = src.enabled;
    full = src.full;
    max_rows = src.max_rows;
    updates = src.updates;
    dropped_rows = src.dropped_rows;
    dropped_voxels = src.dropped_voxels;
    h_rows = src.h_rows;
    h_vox = src.h_vox;
    dev_rows = dev_vox = 0;
    if (src.dev_vox) {
        HIPCHK(d_rows.reserve(src.dev_rows));
        HIPCHK(d_vox.reserve(src.dev_vox));
        HIPCHK(hipMemcpyAsync(d_rows.data(), src.d_rows.data(), src.dev_rows * sizeof(Point4), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(d_vox.data(), src.d_vox.data(), src.dev_vox * sizeof(ArchiveVoxel), hipMemcpyDeviceToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        dev_rows = src.dev_rows;
        dev_vox = src.dev_vox;
    }
    return SAGEICP_OK;
}

void host_remove_far(sageicp_map &m, const double origin[3]) {
    MapArchive &a = m.arc;
    HostMap &h = m.host;
    if (!a.enabled) {
        h.remove_far(origin);
        return;
    }
    const uint64_t serial = a.updates;
    h.remove_far(origin, [&](uint32_t b) { a.append_host(&h.keys[3 * b], &h.pts[h.first_point(b)], h.cnt[b], serial); });
    ++a.updates;             // (a call that evicts nothing takes its serial too)
}

// ---- exports -----------------------------------------------------------------------------------------------------------
namespace {

// ALL into host rows: the device part copied down, the pending tail copied over; no device while no row is in HBM
int all_to_host(sageicp_map &m, uint64_t first, double *out, uint64_t cap, uint64_t *n_out) {
    const MapArchive &a = m.arc;
    const uint64_t total = a.rows();
    *n_out = total;
    if (!out || first >= total) return SAGEICP_OK;
    const uint64_t last = first + std::min(cap, total - first);
    Point4 *dst = reinterpret_cast<Point4 *>(out);
    if (first < a.dev_rows) {
        const uint64_t e = std::min(last, a.dev_rows);
        HIPCHK(hipSetDevice(m.device));
        HIPCHK(hipMemcpy(dst, a.d_rows.data() + first, (e - first) * sizeof(Point4), hipMemcpyDeviceToHost));
    }
    if (last > a.dev_rows) {
        const uint64_t b = std::max(first, a.dev_rows);
        std::memcpy(dst + (b - first), a.h_rows.data() + (b - a.dev_rows), (last - b) * sizeof(Point4));
    }
    return SAGEICP_OK;
}

// Rows [first, first + min(sink.cap, total - first)) of a selection, packed in device memory on the map's stream
// (the whole log on the device first), then out through export_rows as packed rows.
int export_selection(sageicp_map &m, int which, uint64_t first, const RowSink &sink, uint64_t *n_out) {
    MapArchive &a = m.arc;
    *n_out = 0;
    int rc = require_device(m.device);
    if (rc) return rc;
    if ((rc = m.sc.init(m.device))) return rc;
    HIPCHK(hipSetDevice(m.device));
    hipStream_t s = m.sc.stream.get();
    if ((rc = a.flush_pending(s))) return rc;
    const uint64_t map_rows = which == SAGEICP_SESSION ? m.counts().points : 0;
    uint64_t sel_rows = a.dev_rows;
    LatestBuffers lb;
    LatestScratch ls{};
    const bool latest = which != SAGEICP_ARCHIVE_ALL;
    if (latest) {
        sel_rows = 0;
        if (a.dev_vox) {
            if (a.dev_vox >= 0xFFFFFFFFull) return fail(SAGEICP_ERR_CAPACITY, "archive: more than 2^32 - 2 records");
            // the slot table in HBM: the authority's, or the mirror refreshed as before any search (a resident map stays resident)
            if ((rc = refresh_mirror(m))) return rc;
            if ((rc = lb.reserve(a.dev_vox))) return rc;
            ls = lb.view();
            HIPCHK(archive_latest(a.d_vox.data(), static_cast<uint32_t>(a.dev_vox), m.dev.d_table.data(),
                                  static_cast<uint32_t>(m.dev.d_table.capacity() - 1), ls, s));
            // (the counts beyond the selected records are zero: the scan's last entry is the rows of the selection)
            uint32_t rows32 = 0;
            HIPCHK(hipMemcpyAsync(&rows32, ls.offsets + a.dev_vox, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            sel_rows = rows32;
        }
    }
    const uint64_t total = sel_rows + map_rows;
    *n_out = total;
    if (first >= total) return SAGEICP_OK;
    const uint64_t want = std::min(sink.cap, total - first);
    if (!want) return SAGEICP_OK;
    const uint64_t last = first + want;
    const Point4 *rows = nullptr;
    DevBuf<Point4> buf;
    std::vector<double> staged;
    if (!latest && !map_rows) {
        rows = a.d_rows.data() + first;              // the log itself
    } else {
        HIPCHK(buf.reserve(want));
        rows = buf.data();
        if (first < sel_rows) {
            const uint64_t n = std::min(last, sel_rows) - first;
            if (latest) HIPCHK(archive_gather_selected(a.d_rows.data(), a.d_vox.data(), ls, first, n, buf.data(), s));
            else HIPCHK(hipMemcpyAsync(buf.data(), a.d_rows.data() + first, n * sizeof(Point4), hipMemcpyDeviceToDevice, s));
        }
        if (last > sel_rows) {                        // ... then the map, in sageicp_map_pointcloud's order
            const uint64_t b = std::max(first, sel_rows);
            const Point4 *mrows = nullptr;
            if ((rc = map_packed_rows(m, s, staged, &mrows))) {
                (void)hipStreamSynchronize(s);
                return rc;
            }
            HIPCHK(hipMemcpyAsync(buf.data() + (b - first), mrows + (b - sel_rows), (last - b) * sizeof(Point4),
                                  hipMemcpyDeviceToDevice, s));
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    uint64_t n_packed = 0;
    return export_rows(m.out, m.device, RowSource::packed(rows, want, s), sink, &n_packed);
}

int export_archive(const sageicp_map *map, int which, uint64_t first, const RowSink &sink, uint64_t *n_out) {
    if (which != SAGEICP_ARCHIVE_ALL && which != SAGEICP_ARCHIVE_LATEST && which != SAGEICP_SESSION)
        return fail(SAGEICP_ERR_INVALID, "archive export: which is SAGEICP_ARCHIVE_ALL, SAGEICP_ARCHIVE_LATEST or SAGEICP_SESSION");
    sageicp_map &m = internal(map);
    if (which == SAGEICP_ARCHIVE_ALL && sink.kind == RowSink::kHostRows)
        return all_to_host(m, first, static_cast<double *>(sink.out), sink.cap, n_out);
    return export_selection(m, which, first, sink, n_out);
}

}  // namespace
}  // namespace sageicp_impl

extern "C" {

int sageicp_map_set_archive(sageicp_map *m, int enable, uint64_t max_rows) {
    if (!m) return fail(SAGEICP_ERR_INVALID, "null map");
    if (max_rows && max_rows < m->arc.rows())
        return fail(SAGEICP_ERR_INVALID, "sageicp_map_set_archive: max_rows is below the rows the archive holds");
    m->arc.enabled = enable != 0;         // (the first copy of a multi-device map only: the replicas never archive)
    m->arc.max_rows = max_rows;
    return SAGEICP_OK;
}

int sageicp_map_archive_info(const sageicp_map *m, sageicp_archive_info *out) {
    if (!m || !out) return fail(SAGEICP_ERR_INVALID, "null argument");
    const MapArchive &a = m->arc;
    sageicp_archive_info i{};
    i.enabled = a.enabled ? 1 : 0;
    i.full = a.full ? 1 : 0;
    i.rows = a.rows();
    i.voxels = a.voxels();
    i.dropped_rows = a.dropped_rows;
    i.dropped_voxels = a.dropped_voxels;
    i.max_rows = a.max_rows;
    i.updates = a.updates;
    i.device_rows = a.dev_rows;
    i.host_rows = a.h_rows.size();
    i.device_bytes = a.device_bytes();
    *out = i;
    return SAGEICP_OK;
}

int sageicp_map_archive_clear(sageicp_map *m) {
    if (!m) return fail(SAGEICP_ERR_INVALID, "null map");
    if (m->sc.stream) {
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(hipStreamSynchronize(m->sc.stream.get()));
    }
    m->arc.clear();
    return SAGEICP_OK;
}

int sageicp_map_archive_voxels(const sageicp_map *m, uint64_t first, sageicp_archive_voxel *out, uint64_t cap, uint64_t *n_out) {
    if (!m || !n_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    static_assert(sizeof(sageicp_archive_voxel) == sizeof(ArchiveVoxel), "one record");
    const MapArchive &a = m->arc;
    const uint64_t total = a.voxels();
    *n_out = total;
    if (!out || first >= total) return SAGEICP_OK;
    const uint64_t last = first + std::min(cap, total - first);
    if (first < a.dev_vox) {
        const uint64_t e = std::min(last, a.dev_vox);
        HIPCHK(hipSetDevice(m->device));
        HIPCHK(hipMemcpy(out, a.d_vox.data() + first, (e - first) * sizeof(ArchiveVoxel), hipMemcpyDeviceToHost));
    }
    if (last > a.dev_vox) {
        const uint64_t b = std::max(first, a.dev_vox);
        std::memcpy(out + (b - first), a.h_vox.data() + (b - a.dev_vox), (last - b) * sizeof(ArchiveVoxel));
    }
    return SAGEICP_OK;
}

int sageicp_map_archive_rows(const sageicp_map *m, int which, uint64_t first, double *out_xyzl, uint64_t cap, uint64_t *n_out) {
    if (!m || !n_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    return export_archive(m, which, first, RowSink::host_rows(out_xyzl, cap), n_out);
}

int sageicp_map_archive_rows_device(const sageicp_map *m, int which, uint64_t first, const sageicp_device_points *dst, void *stream,
                                    uint64_t *n_out) {
    if (!m || !n_out) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (int rc = check_device_points(dst, stream, m->device)) return rc;
    return export_archive(m, which, first, RowSink::device_rows(dst, stream), n_out);
}

static int archive_msg(const sageicp_map *m, int which, uint64_t first, const sageicp_msg_colors *colors, void *out, uint64_t cap,
                       bool on_device, void *stream, uint64_t *n_out) {
    if (!m || !n_out || (cap && !out)) return fail(SAGEICP_ERR_INVALID, "null argument");
    MsgColorTable t;
    int rc = color_table(colors, t);
    if (rc) return rc;
    if (on_device && (rc = check_records_out(out, cap, stream, m->device))) return rc;
    return export_archive(m, which, first, RowSink::records_out(out, cap, t, on_device, stream), n_out);
}
int sageicp_map_archive_msg(const sageicp_map *m, int which, uint64_t first, const sageicp_msg_colors *colors, void *out,
                            uint64_t cap_points, uint64_t *n_out) {
    return archive_msg(m, which, first, colors, out, cap_points, false, nullptr, n_out);
}
int sageicp_map_archive_msg_device(const sageicp_map *m, int which, uint64_t first, const sageicp_msg_colors *colors, void *out,
                                   uint64_t cap_points, void *stream, uint64_t *n_out) {
    return archive_msg(m, which, first, colors, out, cap_points, true, stream, n_out);
}

int sageicp_pipeline_set_archive(sageicp_pipeline *p, int enable, uint64_t max_rows) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    return sageicp_map_set_archive(&internal(sageicp_pipeline_local_map(p)), enable, max_rows);
}

}  // extern "C"
