// What follows the search of GetCorrespondences on the device (correspond.hip): the acceptance test, the ordered
// compaction of the accepted pairs into the reference's order (VoxelHashMap.cpp:119-127: query order), the gather of the
// target rows from the HBM copy of the map and the write into a caller's layouts (egress.h).  Launch interface between
// capi_query.hip (host side) and correspond.hip; the search itself is kernels.hip's, unchanged.
//
// Positions come from a scan and from nothing else: a workgroup of kCorrBlock consecutive queries counts its accepted
// ones (wave ballot + popcount), ONE workgroup scans the counts in tiles of kCorrScanTile with a running carry, and a
// lane's position is its workgroup's offset + its wave's offset + the accepted lanes below it.  No atomic hands out a
// position and no workgroup waits for another, so the order is the host entry's and the result is the same every run.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "egress.h"
#include "sageicp_types.h"

namespace sageicp {

constexpr int kCorrBlock = 256;            // queries per workgroup of the count and write kernels: one count each
constexpr int kCorrScanTile = 256;         // counts the scanning workgroup takes per step

struct CorrespondArgs {
    int n;
    const Point4 *frame;                // [n] the queries in the caller's order (already moved by the pose)
    const Point4 *sorted;               // [n] the same rows in the order they were searched in (sort.hip)
    const uint32_t *perm;               // [n] sorted position j holds query perm[j]
    const int32_t *nn;                  // [n] by sorted position: index into `pts` of the semantic nearest neighbour, or -1
    const Point4 *pts;                  // the map's point array (MapDevice::d_pts)
    double accept_r2;                   // accept_threshold(max_correspondence_distance): as the fused loop's test
    int32_t *by_query;                  // scratch [n]: by query, nn if the pair is accepted, else -1
    uint32_t *counts;                   // scratch [2 * blocks]: the workgroups' counts, then their exclusive scan
    unsigned long long *total;          // device word: the number of pairs
    // the destinations (any may be absent); `src` / `tgt`.flags: the word egress.h's label refusal is raised in
    bool has_src, has_tgt;
    EgressArgs src, tgt;
    long long *idx;                     // nullptr: none; else pair k's query index at idx[k] for k < idx_cap
    unsigned long long idx_cap;
};
inline uint32_t correspond_blocks(int n) { return static_cast<uint32_t>((n + kCorrBlock - 1) / kCorrBlock); }
// flag, count, scan, write: enqueued on s (n > 0)
void launch_correspond(const CorrespondArgs &a, hipStream_t s);
// the flag alone: by_query for a pass that needs no compaction (quality.h); reads n, sorted, perm, nn, pts, accept_r2
void launch_corr_flag(const CorrespondArgs &a, hipStream_t s);

}  // namespace sageicp
