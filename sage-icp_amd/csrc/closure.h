// The device side of a loop closure: which pose every voxel of a session's map belongs to, and the
// session's map re-posed by the corrections of those poses.
//
// A voxel is evicted by its FIRST row alone (k_far_flags, HostMap::remove_far), so from its insertion to its eviction no
// sensor position was far from that row.  Its stay is the maximal run of consecutive positions, ending just before its
// eviction (an archive record: serial `update`; a live voxel: now), that are all not far from its first row; the pose it
// is tied to is the one of that run nearest to the row, the later one on a tie.
//
//   selection  per part (the records, the live voxels — RecallPart, enumerated by recall.h's cand_of) k_cl_flags ->
//              rocprim::select in candidate order -> k_cl_counts -> one exclusive scan: voxel j of the part, its rows at
//              off[j] of the part's rows
//   stays      k_cl_stays, a lane per voxel.  The 64 voxels of a wave carry nearly equal serials, so the wave walks ONE k
//              down from the largest `hi` among them: positions[k] is one scalar load per step, and a lane takes part
//              from its own hi down to its first far position.  The walk ends when every lane has met one (or k = 0):
//              its length is the stay's, not n.
//   move       k_cl_move, a lane per row: the row's voxel by bisection of off[], the row from where the part keeps it,
//              moved by corrections[stay] with quat_to_mat / mat_apply (sageicp_transform_points' point action, bit for
//              bit; the label untouched), packed into the export's buffer.
// No atomic anywhere: the same bytes come out on every run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "recall.h"
#include "sageicp_types.h"

namespace sageicp {

struct ClosurePart {
    RecallPart P;                // the candidates; flag, sel [n_cand] and n_sel [1] are this selection's (need, off unused)
    uint32_t *cnt, *off;         // [n_cand + 1]: rows of selected voxel j, scanned; off[n_cand]: the rows of the part
    uint32_t *stay;              // [n_cand]: of selected voxel j
};

size_t closure_temp_bytes(size_t n_cand);

// sel, n_sel, off of one part.  On s; nothing waits.
hipError_t closure_select(const ClosurePart &C, void *temp, size_t temp_bytes, hipStream_t s);

// stay[j] of every selected voxel against positions[0 .. n) (device memory, n >= 1, 3 doubles each)
hipError_t closure_stays(const ClosurePart &C, const double *positions, uint32_t n, double max_dist2, hipStream_t s);

// rows [row_a, row_b) of the part (row_b <= off[n_cand], as the host read it), moved, into out[0 .. row_b - row_a);
// corrections: device memory, 7 doubles for each of the n poses the stays were taken against
hipError_t closure_move(const ClosurePart &C, const double *corrections, uint32_t row_a, uint32_t row_b, Point4 *out,
                        hipStream_t s);

}  // namespace sageicp
