// MapDevice: the copy of a map in HBM and everything that belongs to it (map_device.hip) — the slot table, the point
// array and its region words, the unit allocator's stacks, the compact copy the scan reads, the staging pair of the
// scattered refresh, the per-block arrays and counters of the device-side Update() and its scratch.  The handle
// (sageicp_map, capi_internal.h) holds one beside its HostMap; the operations take the stream they work on.
//
// Which copy counts is `state`, and it changes in the four transition functions below and nowhere else:
//   kNothing    nothing in HBM is valid: the next refresh uploads the host copy as a whole
//   kMirror     HBM mirrors the host copy up to the host's dirty lists; the host copy is the authority
//   kAuthority  a device-side update left the HBM copy as the map; the host copy is stale until download_into()
// Beside it, two derived things are current or not: the compact copy (`cand_current`: derived from table and points as
// they are now) and the auxiliary arrays of the update (`aux_current` for host generation `aux_generation`: d_zeros,
// d_slot_of, d_free, the free-unit stacks and d_block_of as uploaded from the host's view).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "dev_buffer.h"
#include "host_map.hpp"
#include "kernels.h"
#include "map_update.h"
#include "sageicp_types.h"

namespace sageicp_impl {
using namespace sageicp;

struct MapArchive;      // archive.h: the log of evicted voxels a handle may keep

// what the authoritative copy holds (sageicp_map::counts())
struct MapCounts {
    uint64_t points = 0;
    uint32_t voxels = 0, units_hi = 0;
    uint64_t table_capacity = 0, used_slots = 0;      // (the host table deletes by backward shift: used == voxels there)
};

// what a search reads of the HBM copy (icp_params)
struct SearchView {
    const Slot *table;
    uint32_t mask;
    const Point4 *pts;
    uint64_t pts_bytes;
    const uint4 *cand;
    uint32_t cand_bytes;          // 0: the compact copy does not cover the point array (this search reads the full records)
    const uint32_t *cand_flags;
};

// Capacities one device-side update of n points needs, from the counters before it: pure arithmetic, no HIP call.
struct UpdateNeeds {
    bool too_many_voxels = false; // "more than 2^24 voxels": refuse
    uint64_t need_blocks = 0;     // blocks_hi + n: the worst case, every point opens a voxel (also the pass's bound)
    size_t blocks = 0;            // ... and what the per-block arrays are grown to (>= their capacity now)
    size_t units = 0;             // what the point array is grown to; 0: it is large enough
    size_t table = 0;             // capacity of the rebuilt slot table; 0: the table is large enough
};
UpdateNeeds update_needs(const MapCounters &ctr, uint64_t n, const HostMap &h, size_t blocks_cap, size_t units_cap,
                         size_t table_cap);

struct MapDevice {
    enum State { kNothing, kMirror, kAuthority };

    DevBuf<Slot> d_table;
    DevBuf<Point4> d_pts;                // units of 4 points, + one NaN point after them (reserve_points)
    DevBuf<uint32_t> d_regions;          // per block: (class << 28) | first unit of its region
    DevBuf<uint32_t> d_free_units[kMaxClasses];   // device-side update: per-class stacks of free regions
    DevBuf<uint32_t> d_freed;            // regions released by one insertion pass
    DevBuf<uint32_t> d_block_of;         // device-side update: unit -> block (slot words carry units)
    // compact copy of d_pts for k_icp's scan (fp32 x, y, z, label), derived on the device whenever
    // the HBM copy of the map has changed since the last search: a record per point slot, one more, and
    // kCandSlack records nothing reads (k_icp loads a record's neighbour at a constant offset that the
    // buffer load's range check does not cover)
    static constexpr size_t kCandSlack = 64;
    DevBuf<uint4> d_cand;
    DevBuf<uint32_t> d_cand_flags;
    // pinned staging + device landing buffers for the scattered refresh of changed records
    PinnedBuf<char> h_stage;
    DevBuf<char> d_stage;
    size_t stage_bytes = 0;              // what both hold (0 after a failed reserve)
    // the update's per-block arrays: as many blocks as d_zeros holds (d_regions holds at least as many)
    DevBuf<uint8_t> d_zeros;
    DevBuf<uint32_t> d_slot_of;
    DevBuf<uint32_t> d_free;
    DevBuf<MapCounters> d_ctr;
    PinnedBuf<MapCounters> h_ctr;
    PinnedBuf<uint32_t> h_ctr_aux;       // 16 words: what else a device update hands back (far voxels found)
    // reference-order maps: the lists a device update exchanges with the host's bucket array (pinned)
    PinnedBuf<uint2> h_lists;
    MapCounters ctr{};                   // the host's shadow of the device counters (kAuthority; seeded by update())
    // the update's scratch (reserve_update_scratch); map_update.hip gets the view
    struct UpdateBuffers {
        DevBuf<Point4> raw, w;
        DevBuf<unsigned long long> keys, keys_alt;
        DevBuf<uint32_t> idx, idx_alt, head_slot;
        DevBuf<UpdateEvents> flag, rank;
        DevBuf<int8_t> want;
        DevBuf<uint2> new_list;
        size_t n = 0;                            // points the buffers above hold (0 after a failed reserve)
        DevBuf<uint32_t> far_flag, far_sel;
        DevBuf<uint2> far_list;
        size_t nb = 0;                           // blocks the three above hold (0 after a failed reserve)
        DevBuf<uint32_t> n_sel;
        DevBuf<unsigned char> temp;
        UpdateScratch view() const {
            UpdateScratch v{};
            v.raw = raw.data(); v.w = w.data();
            v.keys = keys.data(); v.keys_alt = keys_alt.data();
            v.idx = idx.data(); v.idx_alt = idx_alt.data(); v.head_slot = head_slot.data();
            v.flag = flag.data(); v.rank = rank.data(); v.want = want.data();
            v.far_flag = far_flag.data(); v.far_sel = far_sel.data(); v.n_sel = n_sel.data();
            v.new_list = new_list.data(); v.far_list = far_list.data();
            v.temp = temp.data(); v.temp_bytes = temp.capacity();
            return v;
        }
    };
    UpdateBuffers up;

    // ---- which copy counts ----
    State state() const { return state_; }
    bool authority() const { return state_ == kAuthority; }
    bool cand_current() const { return cand_current_; }
    bool aux_current_for(const HostMap &h) const { return aux_current_ && aux_generation_ == h.generation; }
    // Clear(), a fresh copy of a host map, a new replica: whatever HBM holds is dropped
    void invalidate() { state_ = kNothing; cand_current_ = aux_current_ = false; }
    // the end of refresh_from(): HBM mirrors the host copy; `changed`: something was uploaded
    void refreshed(bool changed) {
        state_ = kMirror;
        if (changed) cand_current_ = false;
    }
    // the end of update() and of copy_from(): the HBM copy, which holds what `c` counts, is the map
    void became_authority(const MapCounters &c) {
        ctr = c;
        state_ = kAuthority;
        cand_current_ = false;
    }
    // the end of download_into(): the host copy is the map again (its table rebuilt without tombstones: marked dirty as a
    // whole there), and what the device holds beside table, points and regions is not what the host would upload
    void handed_back() { state_ = kMirror; aux_current_ = false; }
    // the derived things: the compact copy after a re-allocation of it or of the points / after k_derive_cand, the
    // auxiliary arrays after their upload from host generation `g` / when one of them was re-allocated under a mirror
    void cand_outdated() { cand_current_ = false; }
    void cand_derived() { cand_current_ = true; }
    void aux_uploaded(uint64_t g) { aux_current_ = true; aux_generation_ = g; }
    void aux_outdated() { aux_current_ = false; }

    // ---- capacities ----
    size_t units_cap() const { return d_pts.capacity() / kUnitPoints; }       // units the point array holds
    size_t blocks_cap() const { return d_zeros.capacity(); }
    size_t cand_slots() const { return d_cand.capacity() ? d_cand.capacity() - 1 - kCandSlack : 0; }
    int reserve_points(size_t units, size_t keep, hipStream_t s);
    int reserve_regions(size_t blocks, size_t keep, hipStream_t s);
    int grow_blocks(size_t blocks, size_t keep, hipStream_t s);
    // `keep_mine`: the stacks and d_block_of hold this map's entries (`ctr` counts them) and a re-allocation keeps them
    int reserve_unit_stacks(const HostMap &h, size_t n, bool keep_mine, hipStream_t s);
    int reserve_update_scratch(size_t n, size_t nb);
    int reserve_stage(size_t bytes);
    int reserve_lists(size_t n);

    // ---- operations (the device current, `s` a stream of it) ----
    int refresh_from(HostMap &h, hipStream_t s);             // no-op while the HBM copy is the authority
    int ensure_cand(bool derive, hipStream_t s);
    int download_into(HostMap &h, hipStream_t s);            // no-op unless the HBM copy is the authority
    // `arc`: the handle's archive while it is on (the evicted voxels are appended to it before their blocks are freed), else nullptr
    int update(HostMap &h, const double *xyzl, uint64_t n, const double pose[7], const Point4 *d_points, hipStream_t s,
               MapArchive *arc = nullptr);
    int copy_from(const MapDevice &src, const HostMap &h, hipStream_t s);   // src: an authority; `h`: this map's configuration
    DevMap view(const HostMap &h) const;                     // map_update.hip's view of the arrays
    SearchView search_view() const;
    // Pointcloud() of the authority (capi_outputs.hip): the scratch of its gather, for `nb` blocks or listed voxels
    struct GatherScratch {
        uint32_t *flag, *sel, *list;             // [nb] each (list: room for nb block indices)
        unsigned char *temp;
        size_t temp_bytes;
    };
    int gather_scratch(size_t nb, GatherScratch *out);

private:
    State state_ = kNothing;
    bool cand_current_ = false, aux_current_ = false;
    uint64_t aux_generation_ = 0;

    // The arrays that make up the map in HBM, and how much of each is live under counters `c`: download_into() and
    // copy_from() walk this one table.
    enum Part { kTable, kPoints, kRegions, kZeros, kSlotOf, kFreeBlocks, kBlockOf, kFreeUnits0, kParts = kFreeUnits0 + kMaxClasses };
    struct Live {
        void *p;
        size_t bytes;
    };
    Live live(int part, const MapCounters &c) const;
};

}  // namespace sageicp_impl
