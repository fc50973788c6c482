// A session rebuild on the host side of libsageicp_hip.so (rebuild.h): the checks of the two C entries, the
// selection and the stays (closure.h) of the source's session, the scratch of one call, the one wait for the totals, the
// destination's capacities (recall's rules), the fill and MapDevice's step to "the device is the authority".  Host code only.
#include "capi_internal.h"
#include "closure.h"
#include "rebuild.h"

namespace sageicp_impl {
namespace {

// the selection's scratch of one part (closure.h: ClosurePart)
struct PartScratch {
    DevBuf<uint32_t> flag, sel, n_sel, cnt, off, stay;
    int reserve(ClosurePart &c) {
        const size_t n = c.P.n_cand;
        if (!n) return SAGEICP_OK;
        HIPCHK(flag.reserve(n)); HIPCHK(sel.reserve(n)); HIPCHK(n_sel.reserve(1));
        HIPCHK(cnt.reserve(n + 1)); HIPCHK(off.reserve(n + 1)); HIPCHK(stay.reserve(n));
        c.P.flag = flag.data(); c.P.sel = sel.data(); c.P.n_sel = n_sel.data();
        c.cnt = cnt.data(); c.off = off.data(); c.stay = stay.data();
        return SAGEICP_OK;
    }
};

// the scratch of one call, for a bound of n rows (110 n bytes and the primitives' temporaries)
struct RebuildBuffers {
    DevBuf<Point4> moved;
    DevBuf<uint8_t> code, pos_slot;
    DevBuf<unsigned long long> keys, keys_alt;
    DevBuf<uint32_t> idx, idx_alt, head_flag, run_start, pos_run, words;       // words: n_runs, n_rows, flags
    DevBuf<RebuildRun> runs;
    DevBuf<RebuildNeed> need, rank;
    DevBuf<RebuildTotals> totals;
    DevBuf<unsigned char> temp;
    RebuildScratch view;
    int reserve(size_t n) {
        HIPCHK(words.reserve(3)); HIPCHK(totals.reserve(1));
        HIPCHK(need.reserve(n + 1)); HIPCHK(rank.reserve(n + 1));
        if (n) {
            HIPCHK(moved.reserve(n)); HIPCHK(code.reserve(n)); HIPCHK(pos_slot.reserve(n));
            HIPCHK(keys.reserve(n)); HIPCHK(keys_alt.reserve(n));
            HIPCHK(idx.reserve(n)); HIPCHK(idx_alt.reserve(n)); HIPCHK(head_flag.reserve(n)); HIPCHK(run_start.reserve(n));
            HIPCHK(pos_run.reserve(n)); HIPCHK(runs.reserve(n));
            HIPCHK(temp.reserve(rebuild_temp_bytes(n)));
        }
        view = RebuildScratch{moved.data(), code.data(), keys.data(), keys_alt.data(), idx.data(), idx_alt.data(), head_flag.data(),
                              run_start.data(), words.data(), words.data() + 1, words.data() + 2, runs.data(), pos_run.data(),
                              pos_slot.data(), need.data(), rank.data(), totals.data(), temp.data(), temp.capacity()};
        return SAGEICP_OK;
    }
};

struct RebuildJob {
    sageicp_map &src, &dst;
    int which;
    const double *positions, *corrections;
    uint64_t n_poses;
    const double *center;        // nullptr: no crop
    double radius;
    hipStream_t s = nullptr;     // src's: its archive and its HBM copy are used on it
    SessionParts sp;
    PartScratch ps[2];
    ClosurePart part[2]{};
    DevBuf<double> d_pos, d_corr;
    DevBuf<unsigned char> sel_temp;
    RebuildBuffers rb;
    uint32_t bound = 0;          // rows the selection may hold: what the scratch is sized by
    RebuildTotals t{};
    RebuildJob(sageicp_map &a, sageicp_map &b, int w, const double *pos, const double *corr, uint64_t n, const double *c, double r)
        : src(a), dst(b), which(w), positions(pos), corrections(corr), n_poses(n), center(c), radius(r) {}
};

// the selection of `which`, every voxel's stay (as the closure entries take them), the rows moved, keyed, sorted and
// resolved, then the one wait for the totals
int resolve(RebuildJob &j) {
    sageicp_map &m = j.src;
    const bool latest = j.which != SAGEICP_ARCHIVE_ALL;
    int rc;
    if ((rc = session_archive_part(m, j.s, latest, j.sp))) return rc;
    if (j.which == SAGEICP_SESSION && (rc = session_live_part(m, j.s, j.sp))) return rc;
    // (the scans count rows in 32 bits, as LATEST's and recall's do)
    if (m.arc.dev_rows + m.counts().points >= 0xFFFFFFFFull) return fail(SAGEICP_ERR_CAPACITY, "rebuild: more than 2^32 - 2 rows");
    const uint64_t n = j.n_poses;
    HIPCHK(j.d_pos.reserve(3 * n));
    HIPCHK(hipMemcpyAsync(j.d_pos.data(), j.positions, 3 * n * sizeof(double), hipMemcpyHostToDevice, j.s));
    HIPCHK(j.d_corr.reserve(7 * n));
    HIPCHK(hipMemcpyAsync(j.d_corr.data(), j.corrections, 7 * n * sizeof(double), hipMemcpyHostToDevice, j.s));
    HIPCHK(j.sel_temp.reserve(std::max(closure_temp_bytes(j.sp.part[0].n_cand), closure_temp_bytes(j.sp.part[1].n_cand))));
    const double max_dist2 = m.host.max_distance * m.host.max_distance;      // formed once, as the update's is
    for (int k = 0; k < 2; ++k) {
        ClosurePart &c = j.part[k];
        c.P = j.sp.part[k];
        if (!c.P.n_cand) continue;
        if ((rc = j.ps[k].reserve(c))) return rc;
        HIPCHK(closure_select(c, j.sel_temp.data(), j.sel_temp.capacity(), j.s));
        HIPCHK(closure_stays(c, j.d_pos.data(), static_cast<uint32_t>(n), max_dist2, j.s));
    }
    // every record's rows, every live point: no selection holds more, and the host knows both without a wait
    j.bound = static_cast<uint32_t>((j.sp.part[0].n_cand ? m.arc.dev_rows : 0) + (j.sp.part[1].n_cand ? m.counts().points : 0));
    if ((rc = j.rb.reserve(j.bound))) return rc;
    const HostMap &h = j.dst.host;
    RebuildPolicy pol{};
    pol.voxel_size = h.voxel_size;
    pol.basic = h.basic;
    pol.critical = h.critical;
    pol.n_labels = static_cast<int>(h.basic_labels.size());
    for (int i = 0; i < pol.n_labels; ++i) pol.labels[i] = h.basic_labels[i];
    const DevMap dm = j.dst.dev.view(h);                 // (the destination's size classes)
    const double radius2 = j.radius * j.radius;          // formed once, as max_dist2 is
    HIPCHK(rebuild_resolve(j.part, j.d_corr.data(), pol, dm, j.center, radius2, j.rb.view, j.bound, j.s));
    HIPCHK(hipMemcpyAsync(&j.t, j.rb.totals.data(), sizeof(RebuildTotals), hipMemcpyDeviceToHost, j.s));
    HIPCHK(hipStreamSynchronize(j.s));
    if (j.t.flags & 2u) return fail(SAGEICP_ERR_INVALID, "rebuild: a moved coordinate is not finite");
    if (j.t.flags & 1u) return fail(SAGEICP_ERR_CAPACITY, "rebuild: a moved row's voxel index is beyond +-2^20");
    return SAGEICP_OK;
}

// the destination's arrays for n voxels in `units` units, every one of them as a cleared map's (recall's rules)
int reserve_destination(RebuildJob &j, uint64_t n, uint64_t units) {
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

int fill(RebuildJob &j, sageicp_rebuild_info *info) {
    const RebuildTotals &t = j.t;
    const uint64_t n = t.voxels, units = t.units;
    if (n + 3 >= (1ull << kMaxBlockBits)) return fail(SAGEICP_ERR_CAPACITY, "rebuild: more than 2^24 voxels");
    if (t.units == 0xFFFFFFFFu || units > kMaxUnits) return fail(SAGEICP_ERR_CAPACITY, "rebuild: voxel storage beyond 2^24 units of 4 points");
    if (int rc = reserve_destination(j, n, units)) return rc;
    MapDevice &d = j.dst.dev;
    const DevMap dm = d.view(j.dst.host);
    HIPCHK(rebuild_fill(j.rb.view, j.bound, dm, t.voxels, t.units, j.s));
    HIPCHK(recall_finish(dm, t.voxels, t.rows, t.units, static_cast<uint32_t>(d.units_cap()), j.s));
    HIPCHK(hipMemcpyAsync(d.h_ctr.data(), d.d_ctr.data(), sizeof(MapCounters), hipMemcpyDeviceToHost, j.s));
    HIPCHK(hipStreamSynchronize(j.s));
    j.dst.host.clear_dirty();
    d.became_authority(*d.h_ctr.data());
    if (info) {
        sageicp_rebuild_info i{};
        i.voxels = t.voxels;
        i.rows = t.rows;
        i.session_voxels = t.session_voxels;
        i.session_rows = t.session_rows;
        i.built_voxels = t.built_voxels;
        i.built_rows = t.built_rows;
        i.cropped_voxels = static_cast<uint64_t>(t.built_voxels) - t.voxels;
        i.cropped_rows = static_cast<uint64_t>(t.built_rows) - t.rows;
        *info = i;
    }
    return SAGEICP_OK;
}

int rebuild(sageicp_map &src, int which, const double *positions, const double *corrections, uint64_t n, const double *center,
            double radius, sageicp_map &dst, sageicp_rebuild_info *info) {
    int rc = require_device(src.device);
    if (rc) return rc;
    if ((rc = src.sc.init(src.device))) return rc;
    if ((rc = dst.sc.init(dst.device))) return rc;
    HIPCHK(hipSetDevice(src.device));
    dst.sc.wait();                       // nothing of the destination's runs any more: its arrays are filled on src's stream
    sageicp_map_clear(&dst);             // (its archive stays as it is)
    RebuildJob j(src, dst, which, positions, corrections, n, center, radius);
    j.s = src.sc.stream.get();
    if (!(rc = resolve(j))) rc = fill(j, info);
    if (rc) {                            // the destination stays cleared; nothing is left running on its arrays or the scratch
        (void)hipStreamSynchronize(j.s);
        dst.dev.invalidate();
    }
    return rc;
}

}  // namespace
}  // namespace sageicp_impl

extern "C" {

int sageicp_map_session_rebuild(const sageicp_map *src, int which, const double *positions, const double *corrections, uint64_t n,
                                const double center[3], double radius, sageicp_map *dst, sageicp_rebuild_info *info) {
    const char *who = "sageicp_map_session_rebuild";
    if (!dst) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": null argument");
    uint64_t unused = 0;
    if (int rc = check_selection(src, which, positions, n, &unused, who)) return rc;
    if (int rc = check_corrections(corrections, n, who)) return rc;
    if (src == dst) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": dst is src");
    if (center) {
        if (!finite_n(center, 3)) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": the centre is not finite");
        if (!(radius >= 0.0)) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": the radius is negative or NaN");
    }
    if (!same_policy(src->host, dst->host))
        return fail(SAGEICP_ERR_INVALID, std::string(who) + ": dst's voxel size, points per voxel or basic labels differ from src's");
    if (dst->host.basic_labels.size() > static_cast<size_t>(kMaxBasicLabels))
        return fail(SAGEICP_ERR_INVALID, std::string(who) + ": more than 32 basic_parts_labels");
    if (dst->host.track_order) return fail(SAGEICP_ERR_INVALID, std::string(who) + ": dst is in reference-order mode");
    if (!dst->replicas.empty() || dst->device != src->device)
        return fail(SAGEICP_ERR_INVALID, std::string(who) + ": dst spans several devices or lives on another device than src's first");
    return rebuild(internal(src), which, positions, corrections, n, center, center ? radius : 0.0, *dst, info);
}

int sageicp_pipeline_session_rebuild(const sageicp_pipeline *p, int which, const double *corrections, uint64_t n,
                                     const double center[3], double radius, sageicp_map *dst, sageicp_rebuild_info *info) {
    std::vector<double> pos;
    if (int rc = pipeline_positions(p, "sageicp_pipeline_session_rebuild", pos, nullptr)) return rc;
    if (n != pos.size() / 3) return fail(SAGEICP_ERR_INVALID, "sageicp_pipeline_session_rebuild: n is not the pipeline's number of poses");
    return sageicp_map_session_rebuild(sageicp_pipeline_local_map(p), which, pos.data(), corrections, n, center, radius, dst, info);
}

}  // extern "C"
