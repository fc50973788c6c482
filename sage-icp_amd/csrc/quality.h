// Registration quality on the device (quality.hip): one pass over the queries, behind the search and k_corr_flag
// (correspond.hip), that forms every sum of sageicp_quality (include/sageicp.h) over the accepted pairs — the
// Gauss-Newton sums of AlignClouds (Registration.cpp:59-94), the squared residuals, the unweighted moments of the moved
// queries, the counts, the split of the pairs by the label rule of VoxelHashMap.cpp:88 and the per-class tables.  Launch
// interface between capi_query.hip (host side: quality_finish turns the sums into fitness, rmse, step and covariances) and
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
// ---- what k_quality and the batch's k_score (score.hip) share: one pair's terms, the lanes' tree ----------------------
// v of every lane of the wave, added in a fixed tree; every lane gets the same bits (a + b == b + a)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the split of the pairs a lane has seen, by the label rule of VoxelHashMap.cpp:88
struct QualPairCounts {
    uint32_t pairs = 0, same = 0, unlabelled = 0, cross = 0;
};

// One accepted pair — moved query s, map point g — added to a lane's running sums: acc[0 .. kQWR2] always, the nine
// unweighted moments acc[kQSx .. kQSzz] with kMoments (acc then holds kQualReals numbers, else kQWR2 + 1).  Returns
// e = |r|^2.  The plain IEEE sequence of k_gn (kernels.hip); k2 = k * k.
template <bool kMoments>
__device__ __forceinline__ double quality_pair_term(const Point4 &s, const Point4 &g, double k, double k2, double *acc,
                                                    QualPairCounts &n) {
    const double sx = s.x, sy = s.y, sz = s.z;
    const double rx = sx - g.x, ry = sy - g.y, rz = sz - g.z;
    const double e = SAGE_SQNORM3_RESID(rx * rx, ry * ry, rz * rz);
    const double den = k + e;
    const double w = k2 / (den * den);   // square(th) / square(th + residual2), Registration.cpp:79-81
    const double wsx = w * sx, wsy = w * sy, wsz = w * sz;
    acc[kW] += w;
    acc[kWsx] += wsx; acc[kWsy] += wsy; acc[kWsz] += wsz;
    acc[kWxx] += wsx * sx; acc[kWxy] += wsx * sy; acc[kWxz] += wsx * sz;
    acc[kWyy] += wsy * sy; acc[kWyz] += wsy * sz; acc[kWzz] += wsz * sz;
    acc[kWrx] += w * rx; acc[kWry] += w * ry; acc[kWrz] += w * rz;
    acc[kWcx] += w * (sy * rz - sz * ry);
    acc[kWcy] += w * (sz * rx - sx * rz);
    acc[kWcz] += w * (sx * ry - sy * rx);
    acc[kQR2] += e;
    acc[kQWR2] += w * e;
    if constexpr (kMoments) {
        acc[kQSx] += sx; acc[kQSy] += sy; acc[kQSz] += sz;
        acc[kQSxx] += sx * sx; acc[kQSxy] += sx * sy; acc[kQSxz] += sx * sz;
        acc[kQSyy] += sy * sy; acc[kQSyz] += sy * sz; acc[kQSzz] += sz * sz;
    }
    // the label rule of VoxelHashMap.cpp:88, on the truncated labels
    const double lq = trunc(g.l), ls = trunc(s.l);
    const bool eq = lq == ls;
    const bool un = !eq && trunc(g.l * s.l) == 0.0;
    ++n.pairs;
    n.same += eq ? 1u : 0u;
    n.unlabelled += un ? 1u : 0u;
    n.cross += (!eq && !un) ? 1u : 0u;
    return e;
}

inline uint32_t quality_tiles(int n) { return static_cast<uint32_t>((n + kQualTile - 1) / kQualTile); }
inline uint32_t quality_groups(int n) { return quality_tiles(n) < kQualGroups ? quality_tiles(n) : kQualGroups; }
constexpr size_t kQualSlabDoubles = static_cast<size_t>(kQualReals + kQualBins) * kQualGroups;
// the pass and the reducer, enqueued on s (n > 0; *a.out zeroed on s before)
void launch_quality(const QualityArgs &a, hipStream_t s);

}  // namespace sageicp
