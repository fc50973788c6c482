// The device side of a session rebuild: the rows of a session's map, moved by the corrections of their
// voxels' stays (closure.h), voxelised again under the destination's retention policy and laid straight into a cleared map.
//
//   move, key  k_rb_move, a lane per row of the selection (both parts in one launch): k_cl_move's arithmetic, then the
//              voxel index of the MOVED row, packed as k_up_keys packs it; the moved row, its label class (a byte) and
//              the flag word (bit 0: an index beyond +-2^20, bit 1: a coordinate that is not finite).  Positions from the
//              selection's rows up to the host's bound carry a key above every real one: the host never waits for the count.
//   sort       rocprim::radix_sort_pairs of (key, arrival index): stable, so a run is in arrival order
//   runs       k_rb_heads -> rocprim::select: the first position of every run
//   resolve    k_rb_resolve, a group of 16 lanes per run, steps of 16 arrivals with carried counts (rebuild_rule.h): the
//              slot every arrival ends in (or none), the run's final count, unlabelled count and slot-0 row; that row
//              decides the crop.  The run's needs (a voxel, its units, its rows) are laid at the ARRIVAL index of its first
//              row and one exclusive scan over arrival positions ranks the kept runs in order of first arrival, as
//              k_up_heads' events are ranked.
//   fill       k_rb_fill, a lane per sorted position: block = rank, region = first unit of the rank, row into its slot;
//              the lane of a run's first position writes regions, block_of, zeros, slot_of and claims the table slot (a
//              compare-and-swap down the probe chain: keys are unique, so it decides only where in the table the key sits).
// No atomic decides a block, a unit or a row's place: the same bytes come out on every run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "closure.h"
#include "map_update.h"
#include "rebuild_rule.h"
#include "sageicp_types.h"

namespace sageicp {

// what a run asks for, laid at the arrival index of its first row; its exclusive scan ranks the kept runs
struct RebuildNeed {
    uint32_t voxels, units, rows;    // of kept runs (units saturating)
    uint32_t built_rows;             // of every run: before the crop
};

struct RebuildRun {
    uint32_t head;                   // arrival index of the run's first row: where its rank is
    uint32_t word;                   // count | unlabelled << 8 | kept << 31
};

struct RebuildTotals {               // what the host waits for
    uint32_t flags;                  // bit 0: a voxel index out of range, bit 1: a coordinate that is not finite
    uint32_t session_voxels, session_rows;
    uint32_t built_voxels, built_rows;
    uint32_t voxels, units, rows;    // after the crop (units: 0xFFFFFFFF = too many)
};

struct RebuildPolicy {
    double voxel_size;
    int basic, critical;
    int n_labels;
    int labels[kMaxBasicLabels];
};

struct RebuildScratch {              // n: the host's bound on the rows of the selection
    Point4 *moved;                   // [n] by arrival index
    uint8_t *code;                   // [n] label class, by arrival index
    unsigned long long *keys, *keys_alt;   // [n]
    uint32_t *idx, *idx_alt;         // [n]
    uint32_t *head_flag;             // [n]
    uint32_t *run_start;             // [n]
    uint32_t *n_runs;                // [1]
    uint32_t *n_rows;                // [1] the rows of the selection
    uint32_t *flags;                 // [1]
    RebuildRun *runs;                // [n]
    uint32_t *pos_run;               // [n] by sorted position
    uint8_t *pos_slot;               // [n] by sorted position
    RebuildNeed *need, *rank;        // [n + 1]; rank[n]: the totals
    RebuildTotals *totals;           // [1]
    void *temp;
    size_t temp_bytes;
};

size_t rebuild_temp_bytes(size_t n);

// Everything up to the totals.  part[0 .. 2): as closure_select / closure_stays left them (a part with n_cand == 0 is
// skipped); corrections: device memory; center == nullptr: no crop; M: the destination's size classes.  On s; nothing waits.
hipError_t rebuild_resolve(const ClosurePart part[2], const double *corrections, const RebuildPolicy &pol, const DevMap &M,
                           const double *center, double radius2, const RebuildScratch &S, uint32_t n, hipStream_t s);

// the kept runs into blocks [0, block_end), units [0, unit_end) of M (cleared, its table empty); nothing is written at or
// beyond either
hipError_t rebuild_fill(const RebuildScratch &S, uint32_t n, const DevMap &M, uint32_t block_end, uint32_t unit_end, hipStream_t s);

}  // namespace sageicp
