// Recall: the voxels of a session's map — the LATEST records of a handle's archive in log order, then its
// live voxels in Pointcloud() order — whose FIRST row is not far from a centre, laid straight into a cleared second map.
//
//   selection  per part (the records, the live voxels) one verdict per candidate: k_rc_flags reads the candidate's first
//              row and evaluates the eviction test of k_far_flags / HostMap::remove_far the other way round (kept iff NOT
//              SAGE_SQNORM3_FAR(..) > radius^2; a record also needs archive_latest's verdict) -> rocprim::select in
//              candidate order -> k_rc_needs (rows and units of each selected voxel) -> one exclusive scan of the pairs.
//              The host waits once for the six totals (voxels, rows, units of each part): they size the destination.
//   fill       k_rc_fill, lane per row as k_arc_gather: voxel j of a part becomes block base + j, its region the smallest
//              class that holds its count, first unit = unit base + scan; the lane of a voxel's first row writes regions,
//              block_of, slot_of and claims the slot (one compare-and-swap down the probe chain: keys are unique, so it
//              decides only where in the table the key sits); zeros[b] is counted from the rows' labels.  k_rc_after sets
//              the counters.
// No atomic decides a block, a unit or a row: the same bytes come out on every run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "archive.h"
#include "map_update.h"
#include "sageicp_types.h"

namespace sageicp {

// rows and storage units of a voxel; the scan's element
struct RecallNeed {
    uint32_t rows, units;
};

// One part of a session's map as the kernels see it.  Exactly one of `vox` (the archive's records: candidate i is record
// i, kept only if latest[i]) and the live forms is set: `cand` (the live voxels' slots as the host lists them, in
// Pointcloud() order), or the resident map's own arrays — candidate i is block list[i] (reference-order mode: the bucket
// order) or block i, live iff slot_of says so.
struct RecallPart {
    const Point4 *rows;          // the log's rows / the source's point array
    uint32_t n_cand;
    const ArchiveVoxel *vox;
    const uint32_t *latest;
    const Slot *cand;
    const Slot *table;
    const uint32_t *slot_of;
    const uint32_t *list;
    // scratch
    uint32_t *flag, *sel;        // [n_cand]
    uint32_t *n_sel;             // [1]
    RecallNeed *need, *off;      // [n_cand + 1]; off[n_cand]: the totals
};

// a candidate as the kernels read it (recall.hip; closure.hip enumerates the session through the same function)
struct Cand {
    int32_t x, y, z;
    uint32_t count;
    uint64_t first;              // its first row in P.rows
};

// candidate i of a part; false: not a voxel of the session (an older generation of its key, a free block)
__device__ __forceinline__ bool cand_of(const RecallPart &P, uint32_t i, Cand &c) {
    if (P.vox) {
        if (!P.latest[i]) return false;
        const ArchiveVoxel v = P.vox[i];
        c.x = v.x; c.y = v.y; c.z = v.z;
        c.count = v.count;
        c.first = v.first_row;
        return true;
    }
    Slot e;
    if (P.cand) {
        e = P.cand[i];
    } else {
        const uint32_t s = P.slot_of[P.list ? P.list[i] : i];
        if (s == kNoSlot) return false;
        e = P.table[s];
    }
    c.x = e.x; c.y = e.y; c.z = e.z;
    c.count = e.blk & 255u;
    c.first = static_cast<uint64_t>(e.blk >> 8) * kDevUnitPoints;
    return true;
}

struct RecallTotals {            // what the host waits for, per part
    uint32_t voxels, rows, units;
};

size_t recall_temp_bytes(size_t n_cand);

// the verdicts, the selection and its scanned needs of one part (M: the destination's classes); *totals (device memory)
// written last.  On s; nothing waits.
hipError_t recall_select(const RecallPart &P, const DevMap &M, const double center[3], double radius2, void *temp,
                         size_t temp_bytes, RecallTotals *totals, hipStream_t s);

// the selected voxels of P (n_rows rows: the grid) into blocks [block0, ..), units [unit0, ..) of M (cleared, its table
// empty, zeros[] zero); nothing is written at or beyond block_end / unit_end
hipError_t recall_fill(const RecallPart &P, const DevMap &M, uint32_t block0, uint32_t unit0, uint32_t block_end, uint32_t unit_end,
                       uint32_t n_rows, hipStream_t s);

// the counters of a map that holds exactly `voxels` voxels in blocks [0, voxels), `rows` rows and `units` units
hipError_t recall_finish(const DevMap &M, uint32_t voxels, uint64_t rows, uint32_t units, uint32_t units_cap, hipStream_t s);

}  // namespace sageicp
