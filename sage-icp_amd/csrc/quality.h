// Registration quality on the device (quality.hip): one pass over the queries, behind the search and k_corr_flag
// (correspond.hip), that forms every sum of sageicp_quality (include/sageicp.h) over the accepted pairs — the
// Gauss-Newton sums of AlignClouds (Registration.cpp:59-94), the squared residuals, the unweighted moments of the moved
// queries, the counts, the split of the pairs by the label rule of VoxelHashMap.cpp:88 and the per-class tables.  Launch
// interface between capi.hip (host side: quality_finish turns the sums into fitness, rmse, step and covariances) and
// quality.hip; the search itself is kernels.hip's, unchanged.
//
// Reduction.  No floating-point atomic anywhere.  At most kQualGroups workgroups take the tiles of
// kQualTile consecutive queries in a fixed deal (tile = group + k * groups); a thread adds its own queries' terms in
// that order, the workgroup adds its threads' sums in a fixed tree (wave butterfly, then the four waves) and stores one
// slab of kQualReals + kQualBins fp64 numbers; one reducer workgroup per number adds the slabs in a fixed tree.  A
// class's sum of squared residuals is added by ONE thread per class and workgroup, over the tile's pairs in query order
// (staged in LDS).  Counts are integers: LDS atomics, one global flush per workgroup and non-empty bin.  The bits of
// every result depend on the rows, their order and n, and on nothing else — not on arrival order, not on the entry.
// fp64 throughout, nothing is scaled into a fixed-point range: coordinates of any finite size keep their relative error.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sageicp_types.h"

namespace sageicp {

constexpr int kQualTile = 256;             // queries per tile: one per thread of a workgroup
constexpr int kQualGroups = 256;           // workgroups at most == slabs the reducer adds in one step
constexpr int kQualClasses = 256;          // classes counted on their own; bin kQualClasses: everything else
constexpr int kQualBins = kQualClasses + 1;

// the real sums: the 16 of sageicp_types.h's Sum first, in its order
enum QualSum : int {
    kQR2 = kCount,                         // sum |r|^2
    kQWR2,                                 // sum w |r|^2
    kQSx, kQSy, kQSz,                      // sum s
    kQSxx, kQSxy, kQSxz, kQSyy, kQSyz, kQSzz,      // sum s s^T
    kQualReals,
};
static_assert(kQualReals == 27, "16 weighted sums, the two residual sums, 3 + 6 unweighted moments");

enum QualCount : int { kQPairs = 0, kQSame, kQUnlabelled, kQCross, kQOtherQueries, kQOtherPairs, kQualCounts };

// what the two kernels leave (device memory, zeroed before the launch; copied to the host whole)
struct QualityRaw {
    unsigned long long counts[kQualCounts];
    unsigned long long class_queries[kQualClasses];
    unsigned long long class_pairs[kQualClasses];
    double real[kQualReals];
    double class_r2[kQualBins];            // [kQualClasses]: the pairs of every other class
};

struct QualityArgs {
    int n;
    const Point4 *frame;                // [n] the queries in the caller's order, already moved by the pose
    const int32_t *by_query;            // [n] k_corr_flag's answer: index into `pts` of the accepted neighbour, or -1
    const Point4 *pts;                  // the map's point array
    double kernel;                      // k of w = k^2 / (k + |r|^2)^2
    double *slabs;                      // scratch [(kQualReals + kQualBins) * kQualGroups], number-major
    QualityRaw *out;
};
inline uint32_t quality_tiles(int n) { return static_cast<uint32_t>((n + kQualTile - 1) / kQualTile); }
inline uint32_t quality_groups(int n) { return quality_tiles(n) < kQualGroups ? quality_tiles(n) : kQualGroups; }
constexpr size_t kQualSlabDoubles = static_cast<size_t>(kQualReals + kQualBins) * kQualGroups;
// the pass and the reducer, enqueued on s (n > 0; *a.out zeroed on s before)
void launch_quality(const QualityArgs &a, hipStream_t s);

}  // namespace sageicp
