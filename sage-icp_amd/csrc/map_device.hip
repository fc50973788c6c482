// MapDevice (map_device.h): the HBM copy of a map — its refresh from the host copy (lazily, by the next search), the
// compact copy the scan reads, the download back to the host, the copy of one resident map into another and Update() on
// the device (row f-2: core/VoxelHashMap.cpp:144-184 through map_update.hip) — and the three entries that bring a handle's
// device, stream and host copy to it.  Part of libsageicp_hip.so's host side: capi_internal.h.
#include "capi_internal.h"

namespace sageicp_impl {

// ---- capacities -----------------------------------------------------------------------------
int MapDevice::reserve_stage(size_t bytes) {
    if (bytes <= stage_bytes) return SAGEICP_OK;
    stage_bytes = 0;
    const size_t cap = bytes + bytes / 2 + (1u << 20);
    HIPCHK(h_stage.reserve(cap));
    HIPCHK(d_stage.reserve(cap));
    stage_bytes = cap;
    return SAGEICP_OK;
}

int MapDevice::reserve_lists(size_t n) {
    if (n + 2 > h_lists.capacity()) HIPCHK(h_lists.reserve(n + n / 2 + 4096));
    return SAGEICP_OK;
}

// The point array on the device: at least `units` units (+ one NaN point after them: a harmless
// target for an offset of one past the end), the first `keep` units preserved.
int MapDevice::reserve_points(size_t units, size_t keep, hipStream_t s) {
    if (units <= units_cap()) return SAGEICP_OK;
    HIPCHK(d_pts.grow(units * kUnitPoints + 1, keep * kUnitPoints, s));
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    const Point4 pad{qnan, qnan, qnan, qnan};
    HIPCHK(hipMemcpyAsync(d_pts.data() + units * kUnitPoints, &pad, sizeof(Point4), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    cand_outdated();
    return SAGEICP_OK;
}
// d_regions for at least `blocks` blocks, the first `keep` preserved, the rest marked free
int MapDevice::reserve_regions(size_t blocks, size_t keep, hipStream_t s) {
    if (blocks <= d_regions.capacity()) return SAGEICP_OK;
    keep = std::min(keep, d_regions.capacity());
    HIPCHK(d_regions.grow(blocks, keep, s));
    HIPCHK(hipMemsetAsync(d_regions.data() + keep, 0xFF, (blocks - keep) * sizeof(uint32_t), s));      // kNoRegion
    return SAGEICP_OK;
}

// (re)allocate the per-block device arrays for `blocks` blocks, keeping the first `keep` blocks
int MapDevice::grow_blocks(size_t blocks, size_t keep, hipStream_t s) {
    if (int rc = reserve_regions(blocks, keep, s)) return rc;
    if (blocks > blocks_cap()) {
        keep = std::min(keep, blocks_cap());
        HIPCHK(d_free.grow(blocks, keep, s));
        HIPCHK(d_slot_of.grow(blocks, keep, s));
        HIPCHK(d_zeros.grow(blocks, keep, s));       // (last: its capacity is the arrays')
        HIPCHK(hipMemsetAsync(d_zeros.data() + keep, 0, blocks - keep, s));
        HIPCHK(hipMemsetAsync(d_slot_of.data() + keep, 0xFF, (blocks - keep) * sizeof(uint32_t), s));   // kNoSlot
    }
    if (!h_ctr_aux.data()) {
        HIPCHK(d_ctr.reserve(1));
        HIPCHK(h_ctr.reserve(1));
        HIPCHK(h_ctr_aux.reserve(16));
    }
    return SAGEICP_OK;
}

// the unit allocator's device arrays: per-class stacks able to hold every region the point array
// can be cut into, and the scratch list of one pass's released regions (at most one per point)
int MapDevice::reserve_unit_stacks(const HostMap &h, size_t n, bool keep_mine, hipStream_t s) {
    for (int k = 0; k < h.n_classes; ++k) {
        const size_t need = units_cap() / h.class_units(k) + 1;
        if (need <= d_free_units[k].capacity()) continue;
        const size_t keep = keep_mine ? static_cast<size_t>(std::max(0, ctr.free_units_count[k])) : 0;
        HIPCHK(d_free_units[k].grow(need, keep, s));
    }
    if (units_cap() > d_block_of.capacity()) {
        HIPCHK(d_block_of.grow(units_cap(), keep_mine ? ctr.units_hi : 0, s));
        if (!keep_mine) aux_outdated();        // (derived from the host's view: update(), upload_aux)
    }
    if (n > d_freed.capacity()) HIPCHK(d_freed.reserve(n + n / 2 + 1024));
    return SAGEICP_OK;
}

int MapDevice::reserve_update_scratch(size_t n, size_t nb) {
    UpdateBuffers &u = up;
    if (n > u.n) {
        const size_t c = n + n / 2 + 1024;
        u.n = 0;
        HIPCHK(u.raw.reserve(c));
        HIPCHK(u.w.reserve(c));
        HIPCHK(u.keys.reserve(c));
        HIPCHK(u.keys_alt.reserve(c));
        HIPCHK(u.idx.reserve(c));
        HIPCHK(u.idx_alt.reserve(c));
        HIPCHK(u.head_slot.reserve(c));
        HIPCHK(u.flag.reserve(c + 1));
        HIPCHK(u.rank.reserve(c + 1));
        HIPCHK(u.want.reserve(c));
        HIPCHK(u.new_list.reserve(c));
        u.n = c;
    }
    if (nb > u.nb) {
        const size_t c = nb + nb / 2 + 1024;
        u.nb = 0;
        HIPCHK(u.far_flag.reserve(c));
        HIPCHK(u.far_sel.reserve(c));
        HIPCHK(u.far_list.reserve(c));
        u.nb = c;
    }
    if (!u.n_sel) HIPCHK(u.n_sel.reserve(1));
    // (the archive's scan of nb + 1 counts works in the same storage)
    const size_t tb = std::max(map_update_temp_bytes(static_cast<int>(u.n), static_cast<int>(u.nb)), archive_temp_bytes(u.nb));
    if (tb > u.temp.capacity()) HIPCHK(u.temp.reserve(tb));
    return SAGEICP_OK;
}

int MapDevice::gather_scratch(size_t nb, GatherScratch *out) {
    if (int rc = reserve_update_scratch(0, nb)) return rc;
    *out = GatherScratch{up.far_flag.data(), up.far_sel.data(), reinterpret_cast<uint32_t *>(up.far_list.data()),
                         up.temp.data(), up.temp.capacity()};
    return SAGEICP_OK;
}

// ---- views ----------------------------------------------------------------------------------
DevMap MapDevice::view(const HostMap &h) const {
    DevMap dm{};
    dm.table = d_table.data();
    dm.mask = static_cast<uint32_t>(d_table.capacity() - 1);
    dm.pts = d_pts.data();
    dm.cap = h.cap;
    dm.zeros = d_zeros.data();
    dm.slot_of = d_slot_of.data();
    dm.free_list = d_free.data();
    dm.ctr = d_ctr.data();
    dm.regions = d_regions.data();
    dm.block_of = d_block_of.data();
    for (int k = 0; k < kMaxClasses; ++k) {
        dm.free_units[k] = d_free_units[k].data();
        dm.class_points[k] = k < h.n_classes ? static_cast<uint32_t>(h.class_points[k]) : 0u;
    }
    dm.freed = d_freed.data();
    dm.n_classes = h.n_classes;
    return dm;
}

SearchView MapDevice::search_view() const {
    SearchView v{};
    v.table = d_table.data();
    v.mask = static_cast<uint32_t>(d_table.capacity() - 1);
    v.pts = d_pts.data();
    v.pts_bytes = (static_cast<uint64_t>(units_cap()) * kUnitPoints + 1) * sizeof(Point4);
    v.cand = d_cand.data();
    v.cand_bytes = cand_slots() >= units_cap() * kUnitPoints ? static_cast<uint32_t>(v.pts_bytes / 2) : 0u;
    v.cand_flags = d_cand_flags.data();
    return v;
}

MapDevice::Live MapDevice::live(int part, const MapCounters &c) const {
    switch (part) {
    case kTable: return {d_table.data(), d_table.capacity() * sizeof(Slot)};
    case kPoints: return {d_pts.data(), static_cast<size_t>(c.units_hi) * kUnitPoints * sizeof(Point4)};
    case kRegions: return {d_regions.data(), static_cast<size_t>(c.blocks_hi) * sizeof(uint32_t)};
    case kZeros: return {d_zeros.data(), static_cast<size_t>(c.blocks_hi)};
    case kSlotOf: return {d_slot_of.data(), static_cast<size_t>(c.blocks_hi) * sizeof(uint32_t)};
    case kFreeBlocks: return {d_free.data(), static_cast<size_t>(c.free_count) * sizeof(uint32_t)};
    case kBlockOf: return {d_block_of.data(), static_cast<size_t>(c.units_hi) * sizeof(uint32_t)};
    default: {
        const int k = part - kFreeUnits0;
        return {d_free_units[k].data(), static_cast<size_t>(std::max(0, c.free_units_count[k])) * sizeof(uint32_t)};
    }
    }
}

// ---- device mirror ------------------------------------------------------------------------
// Refresh the HBM mirror from the host-authoritative map.  Everything after a (re)allocation,
// otherwise only the slots and points written since the last sync: they are packed into one
// pinned staging buffer, copied once and scattered by a kernel.
int MapDevice::refresh_from(HostMap &h, hipStream_t s) {
    if (authority()) return SAGEICP_OK;      // the HBM copy is the map
    int rc;
    const bool all = state_ == kNothing;
    bool any = false;
    bool table_full = h.table_all_dirty || all;
    if (h.table.size() != d_table.capacity()) {
        HIPCHK(d_table.reserve(h.table.size()));
        table_full = true;
    }
    // (the host arrays grow by doubling; the map itself never holds more than 2^24 units of 4
    // points — HostMap::add_point refuses the point that would cross the limit)
    // (a small map gets the host vector's doubled capacity — a growing map re-allocates rarely —, a
    // big one what it holds and an eighth)
    bool points_full = h.points_all_dirty || all;
    if (h.units_hi > units_cap()) {
        const size_t want = h.units_hi < (1u << 22)
                                ? std::max<size_t>(h.pts.size() / kUnitPoints, h.units_hi)
                                : std::min<size_t>(kMaxUnits, static_cast<size_t>(h.units_hi) + h.units_hi / 8 + 1024);
        if ((rc = reserve_points(want, 0, s))) return rc;
        points_full = true;
    }
    bool regions_full = h.regions_all_dirty || all;
    if (h.regions.size() > d_regions.capacity()) {
        if ((rc = reserve_regions(h.regions.size(), 0, s))) return rc;
        regions_full = true;
    }
    if (regions_full && h.blocks_hi) {
        HIPCHK(hipMemcpyAsync(d_regions.data(), h.regions.data(), h.blocks_hi * sizeof(uint32_t),
                              hipMemcpyHostToDevice, s));
        any = true;
    }
    if (table_full) {
        HIPCHK(hipMemcpyAsync(d_table.data(), h.table.data(), h.table.size() * sizeof(Slot),
                              hipMemcpyHostToDevice, s));
        any = true;
    }
    if (points_full && h.units_hi) {
        HIPCHK(hipMemcpyAsync(d_pts.data(), h.pts.data(), static_cast<size_t>(h.units_hi) * kUnitPoints * sizeof(Point4),
                              hipMemcpyHostToDevice, s));
        any = true;
    }
    const size_t ns = table_full ? 0 : h.dirty_slots.size();
    const size_t np = points_full ? 0 : h.dirty_pts.size();
    const size_t nr = regions_full ? 0 : h.dirty_regions.size();
    if (ns || np || nr) {
        // staging layout: [slot idx][point idx][region idx][region values][slot values][point values],
        // 32-B aligned parts
        auto up32 = [](size_t x) { return (x + 31) & ~static_cast<size_t>(31); };
        const size_t o_si = 0, o_pi = up32(o_si + ns * 4), o_ri = up32(o_pi + np * 4), o_rv = up32(o_ri + nr * 4),
                     o_sv = up32(o_rv + nr * 4),
                     o_pv = up32(o_sv + ns * sizeof(Slot)), total = o_pv + np * sizeof(Point4);
        if ((rc = reserve_stage(total))) return rc;
        char *hs = h_stage.data();
        uint32_t *si = reinterpret_cast<uint32_t *>(hs + o_si);
        uint32_t *pi = reinterpret_cast<uint32_t *>(hs + o_pi);
        Slot *sv = reinterpret_cast<Slot *>(hs + o_sv);
        Point4 *pv = reinterpret_cast<Point4 *>(hs + o_pv);
        for (size_t i = 0; i < ns; ++i) { si[i] = h.dirty_slots[i]; sv[i] = h.table[h.dirty_slots[i]]; }
        for (size_t i = 0; i < np; ++i) { pi[i] = h.dirty_pts[i]; pv[i] = h.pts[h.dirty_pts[i]]; }
        uint32_t *ri = reinterpret_cast<uint32_t *>(hs + o_ri), *rv = reinterpret_cast<uint32_t *>(hs + o_rv);
        for (size_t i = 0; i < nr; ++i) { ri[i] = h.dirty_regions[i]; rv[i] = h.regions[h.dirty_regions[i]]; }
        HIPCHK(hipMemcpyAsync(d_stage.data(), h_stage.data(), total, hipMemcpyHostToDevice, s));
        char *ds = d_stage.data();
        launch_scatter_u32(reinterpret_cast<uint32_t *>(ds + o_ri), reinterpret_cast<uint32_t *>(ds + o_rv),
                           static_cast<uint32_t>(nr), d_regions.data(), s);
        launch_scatter_slots(reinterpret_cast<uint32_t *>(ds + o_si), reinterpret_cast<Slot *>(ds + o_sv),
                             static_cast<uint32_t>(ns), d_table.data(), s);
        launch_scatter_points(reinterpret_cast<uint32_t *>(ds + o_pi),
                              reinterpret_cast<Point4 *>(ds + o_pv), static_cast<uint32_t>(np),
                              d_pts.data(), s);
        HIPCHK(hipGetLastError());
        any = true;
    }
    if (any) HIPCHK(hipStreamSynchronize(s));
    h.clear_dirty();
    refreshed(any);
    return SAGEICP_OK;
}

// The compact copy the scan reads (kernels.hip, k_derive_cand): rebuilt from the HBM copy of the
// map when that has changed (mirror refresh, device-side update, clone).  One pass over the hash
// table and the live points; the ICP loop that follows reads the map ~150 times.
// (`derive` false: the coming search scans the full records — small frames, sparse voxels — so only
// the allocation is kept in step and the copy stays marked stale for the search that wants it)
int MapDevice::ensure_cand(bool derive, hipStream_t s) {
    const size_t slots = units_cap() * kUnitPoints;
    if (!d_cand_flags.data()) {
        HIPCHK(d_cand_flags.reserve(4));
        HIPCHK(hipMemsetAsync(d_cand_flags.data(), 0, 16, s));
    }
    if (!derive) return SAGEICP_OK;             // (this search reads the full records: no copy is made for it)
    if (slots > cand_slots()) {
        HIPCHK(d_cand.reserve(slots + 1 + kCandSlack));
        cand_outdated();
    }
    if (cand_current()) return SAGEICP_OK;
    HIPCHK(hipMemsetAsync(d_cand_flags.data(), 0, 16, s));
    if (d_table.data() && d_pts.data() && slots)
        launch_derive_cand(d_table.data(), static_cast<uint32_t>(d_table.capacity()), d_pts.data(), d_cand.data(), slots,
                           d_cand_flags.data(), s);
    HIPCHK(hipGetLastError());
    cand_derived();
    return SAGEICP_OK;
}

// Bring `h` up to date after device-side updates: download table, regions, counts and free lists
// and let HostMap rebuild itself from them, then the points.  The host table is rebuilt without tombstones, so the
// device table (and the block -> slot map) is stale afterwards and is re-uploaded on next use.
int MapDevice::download_into(HostMap &h, hipStream_t s) {
    if (!authority()) return SAGEICP_OK;
    const MapCounters c = ctr;
    HostMap::Adopted a;
    a.blocks_cap = std::max<size_t>(blocks_cap(), c.blocks_hi);
    a.blocks_hi = c.blocks_hi;
    a.units_cap = units_cap();
    a.units_hi = c.units_hi;
    a.num_voxels = c.num_voxels;
    a.total_points = c.total_points;
    auto into = [&](int part, size_t bytes) -> void * {      // where the host takes a part (nullptr: it derives it itself)
        switch (part) {
        case kTable: a.table.resize(bytes / sizeof(Slot)); return a.table.data();
        case kRegions: a.regions.resize(bytes / sizeof(uint32_t)); return a.regions.data();
        case kZeros: a.zeros.resize(bytes); return a.zeros.data();
        case kFreeBlocks: a.free_blocks.resize(bytes / sizeof(uint32_t)); return a.free_blocks.data();
        case kPoints: case kSlotOf: case kBlockOf: return nullptr;      // (the points follow adopt(), which sizes their store)
        default: a.free_units[part - kFreeUnits0].resize(bytes / sizeof(uint32_t)); return a.free_units[part - kFreeUnits0].data();
        }
    };
    for (int part = 0; part < kParts; ++part) {
        const Live l = live(part, c);
        void *dst = into(part, l.bytes);
        if (dst && l.bytes) HIPCHK(hipMemcpyAsync(dst, l.p, l.bytes, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    h.adopt(a);
    if (const Live l = live(kPoints, c); l.bytes) {
        HIPCHK(hipMemcpyAsync(h.pts.data(), l.p, l.bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    handed_back();
    return SAGEICP_OK;
}

// This (fresh) copy becomes what `src` is, device to device; the host side is touched on neither.  `h`: this map's
// host copy, configured like the source's.  Nothing runs on src's arrays any more (the caller waited for its stream).
int MapDevice::copy_from(const MapDevice &src, const HostMap &h, hipStream_t s) {
    int rc;
    HIPCHK(d_table.reserve(src.d_table.capacity()));
    if ((rc = grow_blocks(src.blocks_cap(), 0, s))) return rc;
    if ((rc = reserve_points(src.units_cap(), 0, s))) return rc;
    if ((rc = reserve_unit_stacks(h, 0, /*keep_mine*/ false, s))) return rc;
    for (int part = 0; part < kParts; ++part) {
        const Live from = src.live(part, src.ctr);
        if (from.bytes) HIPCHK(hipMemcpyAsync(live(part, src.ctr).p, from.p, from.bytes, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    became_authority(src.ctr);
    return SAGEICP_OK;
}

// ---- device-side Update() (row f-2) -----------------------------------------------------------
// capacity for the worst case (every point opens a voxel); the host rule is load <= 1/4
UpdateNeeds update_needs(const MapCounters &ctr, uint64_t n, const HostMap &h, size_t blocks_cap, size_t units_cap,
                         size_t table_cap) {
    UpdateNeeds u;
    u.need_blocks = static_cast<uint64_t>(ctr.blocks_hi) + n;
    u.too_many_voxels = u.need_blocks + 3 >= (1ull << kMaxBlockBits);
    // (growth: doubling while the arrays are small — a growing map re-allocates rarely —, by a quarter
    // beyond 4 M blocks / units, where a doubled array would be most of the map's footprint)
    auto grown = [](size_t cap) { return cap < (size_t{1} << 22) ? 2 * cap : cap + cap / 4; };
    u.blocks = blocks_cap;
    if (u.need_blocks > blocks_cap) u.blocks = std::max<size_t>(u.need_blocks, std::max<size_t>(1024, grown(blocks_cap)));
    // ... and of units.  One region per voxel run at most: a run into a new voxel takes at most
    // `per_point` units per point of it (one with the reference's capacities: 1 unit for 1-4
    // points, 2 for 5-8, 4 for 9-16, 10 beyond), a run into
    // an existing voxel at worst moves it into a region of the last class — and there are no more
    // such runs than voxels.  What the pass really needs is known on the device only
    // (k_up_heads); should it exceed an array already at its limit of 2^24 units, the pass flags
    // that before anything is written and the call fails (read_back).
    uint64_t per_point = 1;      // (a region of class k is first taken by a run of class_points[k-1] + 1 points)
    for (int k = 0; k < h.n_classes; ++k) {
        const uint64_t least = k ? h.class_points[k - 1] + 1u : 1u;
        per_point = std::max<uint64_t>(per_point, (h.class_units(k) + least - 1) / least);
    }
    const uint64_t moving = std::min<uint64_t>(n, ctr.num_voxels);
    const uint64_t need_units = std::min<uint64_t>(
        kMaxUnits, static_cast<uint64_t>(ctr.units_hi) + n * per_point + moving * h.class_units(h.n_classes - 1));
    if (need_units > units_cap)
        u.units = std::min<size_t>(kMaxUnits, std::max<size_t>(need_units, std::max<size_t>(4096, grown(units_cap))));
    // table: (live + tombstoned + incoming) slots must stay within a quarter of the capacity
    if ((static_cast<uint64_t>(ctr.used_slots) + n) * 4 > table_cap) {
        size_t cap = 1024;
        while ((static_cast<uint64_t>(ctr.num_voxels) + n) * 4 > cap) cap *= 2;
        u.table = std::max(cap, table_cap);
    }
    return u;
}

namespace {
// one Update(points, pose) on the device, as the phases of MapDevice::update() pass it on
struct UpdateJob {
    MapDevice &d;
    HostMap &h;
    const double *xyzl;          // the points on the host, or
    const Point4 *d_points;      // ... already in HBM (the pipeline's down-sampled frame)
    uint64_t n;
    const double *pose;
    hipStream_t s;
    UpdateNeeds needs{};
    DevMap dm{};
    UpdateScratch us{};
    MapArchive *arc = nullptr;   // the handle's archive while it is on
    ArchiveDev ad{};
    ArchiveCtr &arc_back() const { return *reinterpret_cast<ArchiveCtr *>(d.h_ctr_aux.data() + kArchiveAuxWord); }
    MapCounters &back() const { return *d.h_ctr.data(); }      // the counters as the device last handed them back
};

// counters as the host has them (the HBM copy was a mirror until now)
int seed_counters(UpdateJob &j) {
    if (int rc = j.d.refresh_from(j.h, j.s)) return rc;       // table + points as the host has them
    const HostMap &h = j.h;
    MapCounters &c = j.d.ctr;
    c = MapCounters{};
    c.blocks_hi = h.blocks_hi;
    c.free_count = static_cast<uint32_t>(h.free_blocks.size());
    c.num_voxels = h.num_voxels;
    c.used_slots = h.num_voxels;
    c.total_points = h.total_points;
    c.units_hi = h.units_hi;
    for (int k = 0; k < h.n_classes; ++k) c.free_units_count[k] = static_cast<int32_t>(h.free_units[k].size());
    return SAGEICP_OK;
}

// the archive before the pass: its pending tail behind its device part, and room for whatever this update can evict —
// the live points and the frame bound it, numbers the host holds.  (Where the log's rows are kept may change here even
// if the pass then refuses the update — the tail moves to the device, a buffer is re-allocated, the stream waited for —
// what the log holds does not.)
int reserve_archive(UpdateJob &j) {
    MapArchive &a = *j.arc;
    if (int rc = a.flush_pending(j.s)) return rc;
    return a.reserve(j.d.ctr.total_points + j.n, static_cast<uint64_t>(j.d.ctr.num_voxels) + j.n, j.s);
}

int reserve(UpdateJob &j) {
    MapDevice &d = j.d;
    int rc;
    if ((rc = d.grow_blocks(j.needs.blocks, d.ctr.blocks_hi, j.s))) return rc;
    if (j.needs.units && (rc = d.reserve_points(j.needs.units, d.ctr.units_hi, j.s))) return rc;
    if ((rc = d.reserve_unit_stacks(j.h, j.n, d.authority(), j.s))) return rc;
    d.ctr.units_cap = static_cast<uint32_t>(d.units_cap());
    return SAGEICP_OK;
}

// auxiliary arrays from the host's view of the map
int upload_aux(UpdateJob &j) {
    MapDevice &d = j.d;
    const HostMap &h = j.h;
    hipStream_t s = j.s;
    const std::vector<uint32_t> so = h.slot_of_blocks();
    if (h.blocks_hi) {
        HIPCHK(hipMemcpyAsync(d.d_zeros.data(), h.zeros.data(), h.blocks_hi, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d.d_slot_of.data(), so.data(), h.blocks_hi * sizeof(uint32_t),
                              hipMemcpyHostToDevice, s));
    }
    if (!h.free_blocks.empty())
        HIPCHK(hipMemcpyAsync(d.d_free.data(), h.free_blocks.data(), h.free_blocks.size() * sizeof(uint32_t),
                              hipMemcpyHostToDevice, s));
    for (int k = 0; k < h.n_classes; ++k)
        if (!h.free_units[k].empty())
            HIPCHK(hipMemcpyAsync(d.d_free_units[k].data(), h.free_units[k].data(),
                                  h.free_units[k].size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    map_derive_block_of(d.view(h), h.blocks_hi, s);
    HIPCHK(hipStreamSynchronize(s));
    d.aux_uploaded(h.generation);
    return SAGEICP_OK;
}

// the device's counters start from the shadow, the pass's own outputs from zero
int send_counters(UpdateJob &j) {
    MapCounters &c = j.back();
    c = j.d.ctr;
    c.n_new = c.n_far = c.overflow = 0;
    c.unit_overflow = c.n_freed = 0;
    HIPCHK(hipMemcpyAsync(j.d.d_ctr.data(), &c, sizeof(MapCounters), hipMemcpyHostToDevice, j.s));
    return SAGEICP_OK;
}

int rebuild_table(UpdateJob &j) {
    MapDevice &d = j.d;
    const size_t cap = j.needs.table;
    DevBuf<Slot> nt;
    HIPCHK(nt.reserve(cap));
    HIPCHK(map_rebuild_table(j.dm, nt.data(), static_cast<uint32_t>(cap - 1), d.ctr.blocks_hi, j.s));
    HIPCHK(hipStreamSynchronize(j.s));
    d.d_table = std::move(nt);
    d.ctr.used_slots = d.ctr.num_voxels;
    j.dm.table = d.d_table.data();
    j.dm.mask = static_cast<uint32_t>(cap - 1);
    return SAGEICP_OK;
}

// the points into the scratch, the pass over them, the counters back
int run_pass(UpdateJob &j) {
    MapDevice &d = j.d;
    const HostMap &h = j.h;
    hipStream_t s = j.s;
    const uint32_t bound = static_cast<uint32_t>(j.needs.need_blocks);
    // (the archive's append scans bound + 1 counts in far_flag: k_arc_counts writes counts[bound], the scan's total)
    if (int rc = d.reserve_update_scratch(j.n, static_cast<size_t>(bound) + (j.arc ? 1 : 0))) return rc;
    UpdateScratch &us = j.us;
    us = d.up.view();
    if (j.d_points) us.raw = const_cast<Point4 *>(j.d_points);
    else if (j.n) HIPCHK(hipMemcpyAsync(us.raw, j.xyzl, j.n * sizeof(Point4), hipMemcpyHostToDevice, s));
    UpdatePolicy pol{};
    pol.voxel_size = h.voxel_size;
    pol.max_dist2 = h.max_distance * h.max_distance;
    pol.basic = h.basic;
    pol.critical = h.critical;
    pol.n_labels = static_cast<int>(h.basic_labels.size());
    for (int i = 0; i < pol.n_labels; ++i) pol.labels[i] = h.basic_labels[i];
    if (j.arc) {
        // the archive's counters go out as the host has them and come back with the pass's (arc_back: words of h_ctr_aux);
        // its scratch is what the search for far voxels has finished with
        MapArchive &a = *j.arc;
        j.arc_back() = a.counters();
        HIPCHK(hipMemcpyAsync(a.d_ctr.data(), &j.arc_back(), sizeof(ArchiveCtr), hipMemcpyHostToDevice, s));
        ArchiveDev &ad = j.ad;
        ad.rows = a.d_rows.data();
        ad.vox = a.d_vox.data();
        ad.ctr = a.d_ctr.data();
        ad.cap_rows = a.d_rows.capacity();
        ad.cap_vox = a.d_vox.capacity();
        ad.limit_rows = a.max_rows ? a.max_rows : ~0ull;
        ad.serial = a.updates;
        ad.counts = d.up.far_flag.data();
        ad.offsets = reinterpret_cast<uint32_t *>(d.up.far_list.data());
        ad.temp = d.up.temp.data();
        ad.temp_bytes = d.up.temp.capacity();
    }
    if (!h.track_order) {
        us.new_list = nullptr;
        us.far_list = nullptr;
        if (!j.arc) {
            HIPCHK(map_update_device(j.dm, pol, us, static_cast<int>(j.n), j.pose, bound, s));
        } else {
            // map_update_device's launches with the append between the search for the far voxels and their eviction
            HIPCHK(map_update_insert_find_far(j.dm, pol, us, static_cast<int>(j.n), j.pose, bound, s));
            HIPCHK(archive_append(j.dm, j.ad, us.far_sel, us.n_sel, bound, s));
            HIPCHK(map_evict_listed(j.dm, us.far_sel, us.n_sel, bound, s));
        }
    } else {
        // A map in reference-order mode: the bucket array of the reference's robin_map lives on the host (host_map.hpp,
        // RobinTable); the device inserts and FINDS the far voxels, the host replays the new voxels (arrival order) and the
        // erase-while-iterating sweep on that array (VoxelHashMap.cpp:166-172,176-184) — only the voxels concerned, a few
        // thousand words across PCIe — and the device evicts what the sweep reached (replay_reference_order).
        HIPCHK(map_update_insert_find_far(j.dm, pol, us, static_cast<int>(j.n), j.pose, bound, s));
    }
    HIPCHK(hipMemcpyAsync(d.h_ctr.data(), d.d_ctr.data(), sizeof(MapCounters), hipMemcpyDeviceToHost, s));
    if (h.track_order) HIPCHK(hipMemcpyAsync(d.h_ctr_aux.data(), us.n_sel, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    else if (j.arc) HIPCHK(hipMemcpyAsync(&j.arc_back(), j.arc->d_ctr.data(), sizeof(ArchiveCtr), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SAGEICP_OK;
}

// what the pass refused: in each case nothing was inserted or evicted (every kernel checks the flag first)
int refusals(UpdateJob &j) {
    const MapCounters &c = j.back();
    if (c.overflow & 2u)
        return fail(SAGEICP_ERR_INVALID, "Update: a coordinate or label is not finite (NaN / Inf); the map is unchanged");
    if (c.overflow) return fail(SAGEICP_ERR_CAPACITY, "voxel index beyond +-2^20 in the device map update");
    if (c.unit_overflow) return fail(SAGEICP_ERR_CAPACITY, "voxel storage beyond 2^24 units of 4 points");
#ifdef SAGE_UP_TIMING
    {
        const double w = static_cast<double>(c.dbg_sum[7] ? c.dbg_sum[7] : 1);
        std::fprintf(stderr, "k_up_insert phases, us (mean over %llu waves / slowest wave): stage %.2f/%.2f  dry run %.2f/%.2f  "
                             "alloc %.2f/%.2f  claim+move %.2f/%.2f  policy %.2f/%.2f  tail %.2f/%.2f  whole %.2f/%.2f\n",
                     c.dbg_sum[7], c.dbg_sum[0] / w / 100, c.dbg_max[0] / 100.0, c.dbg_sum[1] / w / 100, c.dbg_max[1] / 100.0,
                     c.dbg_sum[2] / w / 100, c.dbg_max[2] / 100.0, c.dbg_sum[3] / w / 100, c.dbg_max[3] / 100.0,
                     c.dbg_sum[4] / w / 100, c.dbg_max[4] / 100.0, c.dbg_sum[5] / w / 100, c.dbg_max[5] / 100.0,
                     c.dbg_sum[6] / w / 100, c.dbg_max[6] / 100.0);
        for (int k = 0; k < 8; ++k) j.back().dbg_sum[k] = j.back().dbg_max[k] = 0;
    }
#endif
    return SAGEICP_OK;
}

// reference-order mode: the host's bucket array takes the new voxels and sweeps the far ones, the device evicts what
// the sweep erased
int replay_reference_order(UpdateJob &j) {
    MapDevice &d = j.d;
    hipStream_t s = j.s;
    const UpdateScratch &us = j.us;
    const uint32_t n_new = j.back().n_new, n_far = d.h_ctr_aux.data()[0];
    if (int rc = d.reserve_lists(static_cast<size_t>(n_new) + n_far)) return rc;
    uint2 *hl = d.h_lists.data();
    if (n_new) HIPCHK(hipMemcpyAsync(hl, us.new_list, n_new * sizeof(uint2), hipMemcpyDeviceToHost, s));
    if (n_far) HIPCHK(hipMemcpyAsync(hl + n_new, us.far_list, n_far * sizeof(uint2), hipMemcpyDeviceToHost, s));
    if (n_new || n_far) HIPCHK(hipStreamSynchronize(s));
    RobinTable &order = j.h.order;
    for (uint32_t k = 0; k < n_new; ++k) order.insert(hl[k].y, hl[k].x);                 // arrival order
    std::vector<std::pair<uint32_t, uint32_t>> far(n_far);
    for (uint32_t k = 0; k < n_far; ++k) far[k] = {hl[n_new + k].y, hl[n_new + k].x};
    uint32_t *erased = reinterpret_cast<uint32_t *>(hl);        // (the lists are consumed: the erased blocks go back in their place)
    uint32_t n_er = 0;
    order.sweep_erase_listed(std::move(far), [&](uint32_t b) { erased[1 + n_er++] = b; });
    erased[0] = n_er;
    if (n_er) {
        // far_sel <- the erased blocks in the order of their erasure (the order they go onto the free list), n_sel <- their number
        HIPCHK(hipMemcpyAsync(us.n_sel, erased, sizeof(uint32_t), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(us.far_sel, erased + 1, n_er * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (j.arc) HIPCHK(archive_append(j.dm, j.ad, us.far_sel, us.n_sel, n_er, s));      // in the order of their erasure
        HIPCHK(map_evict_listed(j.dm, us.far_sel, us.n_sel, n_er, s));
        HIPCHK(hipMemcpyAsync(d.h_ctr.data(), d.d_ctr.data(), sizeof(MapCounters), hipMemcpyDeviceToHost, s));
        if (j.arc) HIPCHK(hipMemcpyAsync(&j.arc_back(), j.arc->d_ctr.data(), sizeof(ArchiveCtr), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } else {
        j.back().n_far = 0;
    }
    return SAGEICP_OK;
}
}  // namespace

// VoxelHashMap::Update(points, pose) on the device.
// `d_points`: the points are already in HBM (the pipeline's down-sampled frame); else `xyzl` (host).
int MapDevice::update(HostMap &h, const double *xyzl, uint64_t n, const double pose[7], const Point4 *d_points,
                      hipStream_t s, MapArchive *arc) {
    UpdateJob j{*this, h, xyzl, d_points, n, pose, s};
    j.arc = arc;
    int rc;
    if (!authority() && (rc = seed_counters(j))) return rc;
    j.needs = update_needs(ctr, n, h, blocks_cap(), units_cap(), d_table.capacity());
    if (j.needs.too_many_voxels) return fail(SAGEICP_ERR_CAPACITY, "more than 2^24 voxels");
    if (arc && (rc = reserve_archive(j))) return rc;       // (refused here, neither the map nor the log has changed)
    if ((rc = reserve(j))) return rc;
    if (!authority() && !aux_current_for(h) && (rc = upload_aux(j))) return rc;
    if ((rc = send_counters(j))) return rc;
    j.dm = view(h);
    if (j.needs.table && (rc = rebuild_table(j))) return rc;
    if ((rc = run_pass(j))) return rc;
    if ((rc = refusals(j))) return rc;
    if (h.track_order && (rc = replay_reference_order(j))) return rc;
    h.clear_dirty();
    became_authority(j.back());
    if (arc) {                  // the call took its serial; the tail is where the device left it
        arc->adopt(j.arc_back());
        ++arc->updates;
    }
    return SAGEICP_OK;
}

// ---- the handle's device, stream and host copy brought to the above ---------------------------------------------
int refresh_mirror(sageicp_map &m) {
    int rc = m.sc.init(m.device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(m.device));
    return m.dev.refresh_from(m.host, m.sc.stream.get());
}

int ensure_host(sageicp_map &m) {
    if (!m.dev.authority()) return SAGEICP_OK;
    HIPCHK(hipSetDevice(m.device));
    return m.dev.download_into(m.host, m.sc.stream.get());
}

int device_update(sageicp_map &m, const double *xyzl, uint64_t n, const double pose[7], const Point4 *d_points) {
    if (m.host.basic_labels.size() > static_cast<size_t>(kMaxBasicLabels))
        return fail(SAGEICP_ERR_INVALID, "device map update supports at most 32 basic_parts_labels");
    if (n > 0x3FFFFFFFull) return fail(SAGEICP_ERR_INVALID, "too many points");
    int rc = m.sc.init(m.device);
    if (rc) return rc;
    HIPCHK(hipSetDevice(m.device));
    return m.dev.update(m.host, xyzl, n, pose, d_points, m.sc.stream.get(), m.arc.enabled ? &m.arc : nullptr);
}

// Non-finite input (NaN / Inf coordinates or labels).  The reference turns such values into voxel
// indices and label classes with static_cast<int> — undefined behaviour (INT_MIN on x86, 0 or a
// saturated value on gfx950) — so there is nothing to be faithful to: every entry that would cast one
// refuses the whole call with SAGEICP_ERR_INVALID before anything is changed (host buffers are checked
// here, device-resident frames by the first kernel that reads them: sort.hip, map_update.hip,
// preprocess.hip).  Where the reference's behaviour IS defined it is kept: Preprocess() drops a point
// whose norm is not finite (both range comparisons fail, Preprocessing.cpp:176-177), TransformPoints
// and AlignClouds propagate.
bool all_finite(const double *xyzl, uint64_t n) {
    // (x - x is 0 for every finite x and NaN otherwise: four of them summed stay 0 exactly)
    double acc = 0.0;
    for (uint64_t i = 0; i < 4 * n; ++i) acc += xyzl[i] - xyzl[i];
    return acc == 0.0;
}

}  // namespace sageicp_impl
