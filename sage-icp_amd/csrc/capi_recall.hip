// Recall on the host side of libsageicp_hip.so (recall.h): the checks of the two C entries, the two parts of
// a session's map handed to recall.hip's selection, the one wait for its totals, the destination's capacities, the fill and
// MapDevice's step to "the device is the authority".  Host code only.
#include "capi_internal.h"
#include "recall.h"

namespace sageicp_impl {

// ---- the two parts of a session's map (capi_internal.h: SessionParts) --------------------------------------------------
// the records of src's archive: the whole log on the device, the LATEST verdicts (latest_only == false: every record kept)
int session_archive_part(sageicp_map &src, hipStream_t s, bool latest_only, SessionParts &sp) {
    MapArchive &a = src.arc;
    if (int rc = a.flush_pending(s)) return rc;
    if (a.dev_vox >= 0xFFFFFFFFull) return fail(SAGEICP_ERR_CAPACITY, "recall: more than 2^32 - 2 records");
    // the slot table and the points in HBM: the authority's, or the mirror refreshed as before any search
    if (latest_only)
        if (int rc = refresh_mirror(src)) return rc;
    RecallPart &p = sp.part[0];
    p.n_cand = static_cast<uint32_t>(a.dev_vox);
    if (!p.n_cand) return SAGEICP_OK;
    p.rows = a.d_rows.data();
    p.vox = a.d_vox.data();
    if (!latest_only) {              // (any non-zero word keeps a record)
        HIPCHK(sp.lb.flag.reserve(a.dev_vox));
        HIPCHK(hipMemsetAsync(sp.lb.flag.data(), 0xFF, a.dev_vox * sizeof(uint32_t), s));
        p.latest = sp.lb.flag.data();
        return SAGEICP_OK;
    }
    if (int rc = sp.lb.reserve(a.dev_vox)) return rc;
    const LatestScratch ls = sp.lb.view();
    const MapDevice &d = src.dev;
    HIPCHK(archive_latest(a.d_vox.data(), p.n_cand, d.d_table.data(), static_cast<uint32_t>(d.d_table.capacity() - 1), ls, s));
    p.latest = ls.flag;
    return SAGEICP_OK;
}

// src's live voxels in Pointcloud() order
int session_live_part(sageicp_map &m, hipStream_t s, SessionParts &sp) {
    const HostMap &h = m.host;
    RecallPart &p = sp.part[1];
    p.rows = m.dev.d_pts.data();
    if (m.resident()) {
        p.table = m.dev.d_table.data();
        p.slot_of = m.dev.d_slot_of.data();
        p.n_cand = m.dev.ctr.blocks_hi;
        if (h.track_order) {         // the bucket order of the host's array (VoxelHashMap.cpp:132-142)
            sp.h_list.reserve(h.order.size());
            h.order.for_each([&](uint32_t b) { sp.h_list.push_back(b); });
            p.n_cand = static_cast<uint32_t>(sp.h_list.size());
            if (p.n_cand) {
                HIPCHK(sp.d_list.reserve(p.n_cand));
                HIPCHK(hipMemcpyAsync(sp.d_list.data(), sp.h_list.data(), p.n_cand * sizeof(uint32_t), hipMemcpyHostToDevice, s));
                p.list = sp.d_list.data();
            }
        }
        return SAGEICP_OK;
    }
    // the host copy is the map and HBM mirrors its points: the voxels' slot words as the host lists them
    auto emit = [&](uint32_t b) {
        sp.h_cand.push_back(Slot{h.keys[3 * b], h.keys[3 * b + 1], h.keys[3 * b + 2],
                                 (region_unit(h.regions[b]) << 8) | static_cast<uint32_t>(h.cnt[b])});
    };
    sp.h_cand.reserve(h.num_voxels);
    if (h.track_order) h.order.for_each(emit);
    else
        for (uint32_t b = 0; b < h.blocks_hi; ++b)
            if (h.cnt[b]) emit(b);
    p.n_cand = static_cast<uint32_t>(sp.h_cand.size());
    if (p.n_cand) {
        HIPCHK(sp.d_cand.reserve(p.n_cand));
        HIPCHK(hipMemcpyAsync(sp.d_cand.data(), sp.h_cand.data(), p.n_cand * sizeof(Slot), hipMemcpyHostToDevice, s));
        p.cand = sp.d_cand.data();
    }
    return SAGEICP_OK;
}

namespace {

// the scratch of one part's selection
struct PartBuffers {
    DevBuf<uint32_t> flag, sel, n_sel;
    DevBuf<RecallNeed> need, off;
    int reserve(RecallPart &p) {
        const size_t n = p.n_cand;
        if (!n) return SAGEICP_OK;
        HIPCHK(flag.reserve(n)); HIPCHK(sel.reserve(n)); HIPCHK(n_sel.reserve(1));
        HIPCHK(need.reserve(n + 1)); HIPCHK(off.reserve(n + 1));
        p.flag = flag.data(); p.sel = sel.data(); p.n_sel = n_sel.data();
        p.need = need.data(); p.off = off.data();
        return SAGEICP_OK;
    }
};

// what the one wait of the selection brings back
struct Totals {
    RecallTotals part[2];        // the records, the live voxels
    uint32_t latest_voxels, latest_rows;
};

struct RecallJob {
    sageicp_map &src, &dst;
    const double *center;
    double radius;
    hipStream_t s;               // src's: its archive and its HBM copy are used on it
    SessionParts sp;             // the records and the live voxels of src
    PartBuffers pb[2];
    DevBuf<RecallTotals> d_totals;
    DevBuf<unsigned char> temp;
    Totals t{};
};

// both selections, then the one wait for their totals
int select(RecallJob &j) {
    const double radius2 = j.radius * j.radius;         // formed once, as max_dist2 is
    HIPCHK(j.d_totals.reserve(2));
    HIPCHK(j.temp.reserve(std::max(recall_temp_bytes(j.sp.part[0].n_cand), recall_temp_bytes(j.sp.part[1].n_cand))));
    const DevMap dm = j.dst.dev.view(j.dst.host);       // (the destination's size classes)
    for (int k = 0; k < 2; ++k) {
        if (int rc = j.pb[k].reserve(j.sp.part[k])) return rc;
        HIPCHK(recall_select(j.sp.part[k], dm, j.center, radius2, j.temp.data(), j.temp.capacity(), j.d_totals.data() + k, j.s));
    }
    HIPCHK(hipMemcpyAsync(j.t.part, j.d_totals.data(), 2 * sizeof(RecallTotals), hipMemcpyDeviceToHost, j.s));
    if (const uint32_t nv = j.sp.part[0].n_cand) {         // what LATEST holds: the session's records
        const LatestScratch ls = j.sp.lb.view();
        HIPCHK(hipMemcpyAsync(&j.t.latest_voxels, ls.n_sel, sizeof(uint32_t), hipMemcpyDeviceToHost, j.s));
        HIPCHK(hipMemcpyAsync(&j.t.latest_rows, ls.offsets + nv, sizeof(uint32_t), hipMemcpyDeviceToHost, j.s));
    }
    HIPCHK(hipStreamSynchronize(j.s));
    return SAGEICP_OK;
}

// the destination's arrays for n voxels in `units` units, every one of them as a cleared map's
int reserve_destination(RecallJob &j, uint64_t n, uint64_t units) {
    MapDevice &d = j.dst.dev;
    hipStream_t s = j.s;
    size_t cap = 1024;                                   // HostMap's growth rule: (num_voxels + 1) * 4 <= capacity
    while ((n + 1) * 4 > cap) cap *= 2;
    if (d.d_table.capacity() != cap) HIPCHK(d.d_table.reserve(cap));
    int rc;
    if ((rc = d.grow_blocks(std::max<size_t>(1024, (n + 1023) / 1024 * 1024), 0, s))) return rc;
    if ((rc = d.reserve_points(std::max<size_t>(4096, units), 0, s))) return rc;
    if ((rc = d.reserve_unit_stacks(j.dst.host, 0, /*keep_mine*/ false, s))) return rc;
    HIPCHK(hipMemsetAsync(d.d_table.data(), 0xFF, cap * sizeof(Slot), s));                                  // kEmptySlot
    HIPCHK(hipMemsetAsync(d.d_zeros.data(), 0, d.d_zeros.capacity(), s));
    HIPCHK(hipMemsetAsync(d.d_slot_of.data(), 0xFF, d.d_slot_of.capacity() * sizeof(uint32_t), s));         // kNoSlot
    HIPCHK(hipMemsetAsync(d.d_regions.data(), 0xFF, d.d_regions.capacity() * sizeof(uint32_t), s));         // kNoRegion
    return SAGEICP_OK;
}

int fill(RecallJob &j, sageicp_recall_info *info) {
    const RecallTotals &ta = j.t.part[0], &tm = j.t.part[1];
    const uint64_t n = static_cast<uint64_t>(ta.voxels) + tm.voxels;
    const uint64_t rows = static_cast<uint64_t>(ta.rows) + tm.rows, units = static_cast<uint64_t>(ta.units) + tm.units;
    if (n + 3 >= (1ull << kMaxBlockBits)) return fail(SAGEICP_ERR_CAPACITY, "recall: more than 2^24 voxels");
    if (ta.units == 0xFFFFFFFFu || tm.units == 0xFFFFFFFFu || ta.rows == 0xFFFFFFFFu || tm.rows == 0xFFFFFFFFu || units > kMaxUnits)
        return fail(SAGEICP_ERR_CAPACITY, "recall: voxel storage beyond 2^24 units of 4 points");
    if (int rc = reserve_destination(j, n, units)) return rc;
    MapDevice &d = j.dst.dev;
    const DevMap dm = d.view(j.dst.host);
    const uint32_t n32 = static_cast<uint32_t>(n), u32 = static_cast<uint32_t>(units);
    HIPCHK(recall_fill(j.sp.part[0], dm, 0u, 0u, n32, u32, ta.rows, j.s));
    HIPCHK(recall_fill(j.sp.part[1], dm, ta.voxels, ta.units, n32, u32, tm.rows, j.s));
    HIPCHK(recall_finish(dm, n32, rows, u32, static_cast<uint32_t>(d.units_cap()), j.s));
    HIPCHK(hipMemcpyAsync(d.h_ctr.data(), d.d_ctr.data(), sizeof(MapCounters), hipMemcpyDeviceToHost, j.s));
    HIPCHK(hipStreamSynchronize(j.s));
    j.dst.host.clear_dirty();
    d.became_authority(*d.h_ctr.data());
    if (info) {
        const MapCounts mc = j.src.counts();
        sageicp_recall_info i{};
        i.voxels = n;
        i.rows = rows;
        i.archive_voxels = ta.voxels;
        i.archive_rows = ta.rows;
        i.map_voxels = tm.voxels;
        i.map_rows = tm.rows;
        i.session_voxels = static_cast<uint64_t>(j.t.latest_voxels) + mc.voxels;
        i.session_rows = static_cast<uint64_t>(j.t.latest_rows) + mc.points;
        *info = i;
    }
    return SAGEICP_OK;
}

int recall(sageicp_map &src, const double center[3], double radius, sageicp_map &dst, sageicp_recall_info *info) {
    int rc = require_device(src.device);
    if (rc) return rc;
    if ((rc = src.sc.init(src.device))) return rc;
    if ((rc = dst.sc.init(dst.device))) return rc;
    HIPCHK(hipSetDevice(src.device));
    dst.sc.wait();                       // nothing of the destination's runs any more: its arrays are filled on src's stream
    sageicp_map_clear(&dst);             // (its archive stays as it is)
    RecallJob j{src, dst, center, radius, src.sc.stream.get(), {}, {}, {}, {}, {}};
    if (!(rc = session_archive_part(src, j.s, true, j.sp)) && !(rc = session_live_part(src, j.s, j.sp)) && !(rc = select(j))) rc = fill(j, info);
    if (rc) {                            // the destination stays cleared; nothing is left running on its arrays
        (void)hipStreamSynchronize(j.s);
        dst.dev.invalidate();
    }
    return rc;
}

}  // namespace

bool same_policy(const HostMap &a, const HostMap &b) {
    return a.voxel_size == b.voxel_size && a.basic == b.basic && a.critical == b.critical && a.basic_labels == b.basic_labels;
}

}  // namespace sageicp_impl

extern "C" {

int sageicp_map_recall(const sageicp_map *src, const double center[3], double radius, sageicp_map *dst, sageicp_recall_info *info) {
    if (!src || !dst || !center) return fail(SAGEICP_ERR_INVALID, "null argument");
    if (src == dst) return fail(SAGEICP_ERR_INVALID, "sageicp_map_recall: dst is src");
    if (!finite_n(center, 3)) return fail(SAGEICP_ERR_INVALID, "sageicp_map_recall: the centre is not finite");
    if (!(radius >= 0.0)) return fail(SAGEICP_ERR_INVALID, "sageicp_map_recall: the radius is negative or NaN");
    if (!same_policy(src->host, dst->host))
        return fail(SAGEICP_ERR_INVALID, "sageicp_map_recall: dst's voxel size, points per voxel or basic labels differ from src's");
    if (dst->host.track_order) return fail(SAGEICP_ERR_INVALID, "sageicp_map_recall: dst is in reference-order mode");
    if (!dst->replicas.empty() || dst->device != src->device)
        return fail(SAGEICP_ERR_INVALID, "sageicp_map_recall: dst spans several devices or lives on another device than src's first");
    return recall(internal(src), center, radius, *dst, info);
}

int sageicp_pipeline_recall(const sageicp_pipeline *p, const double center[3], double radius, sageicp_map *dst,
                            sageicp_recall_info *info) {
    if (!p) return fail(SAGEICP_ERR_INVALID, "null pipeline");
    return sageicp_map_recall(sageicp_pipeline_local_map(p), center, radius, dst, info);
}

}  // extern "C"
