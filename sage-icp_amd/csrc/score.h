// A batch of candidate poses scored in one pass (score.hip): moved by K poses, a frame of n rows is
// K * n independent queries against the same map.  Launch interface between capi_relocalize.hip (host side: chunking,
// the search, score_finish) and score.hip; the search between the two kernels is kernels.hip's, unchanged.
//
//   k_score_move    row c * n + i of the chunk = R_c p_i + t_c, label kept: k_tf's operand order, so row for row the
//                   bits of sageicp_transform_points(poses[c])
//   (the search)    sort_frame, launch_rows, launch_icp search-only, launch_corr_flag over the kc * n rows: by_query
//   k_score         candidate c owns quality_groups(n) workgroups and is dealt exactly as k_quality deals a single frame
//                   of n rows: workgroup g of it takes the tiles g, g + groups, ... of kQualTile consecutive queries of
//                   THAT candidate, a thread adds its own queries' terms (quality_pair_term, quality.h: the same code)
//                   in that order, the lanes meet in k_quality's tree; slabs go to [candidate][number][group]
//   k_score_reduce  one workgroup per (candidate, number): thread t holds slab t, k_quality_reduce's tree, one store
// So every real sum of candidate c has the bits k_quality gives the frame moved by poses[c] alone, whatever the other
// candidates are and however the host cut the batch into chunks.  No floating-point atomic; the four pair counts are
// integers (one 64-bit atomic per workgroup and non-empty word).  The class tables and the unweighted moments of
// sageicp_quality are not formed here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "quality.h"
#include "sageicp_types.h"

namespace sageicp {

constexpr int kScoreReals = kQWR2 + 1;      // the 16 Gauss-Newton sums, sum e, sum w e
static_assert(kScoreReals == 18 && static_cast<int>(kQR2) == static_cast<int>(kCount), "quality.h's real sums begin with sageicp_types.h's Sum");

// a candidate as the device applies it: quat_to_mat of the pose on the host, as fill_state does
struct ScorePose {
    double R[9];
    double t[3];
};

// what the two kernels leave per candidate (device memory, zeroed before the launch; copied to the host whole)
struct ScoreRaw {
    double real[kScoreReals];
    unsigned long long counts[4];           // kQPairs, kQSame, kQUnlabelled, kQCross
};

struct ScoreArgs {
    int n;                                  // rows of the frame
    uint32_t kc;                            // candidates of this chunk; kc * n <= kMaxQueries
    const Point4 *frame;                    // [n] the pristine rows
    const ScorePose *poses;                 // [kc]
    Point4 *rows;                           // [kc * n] the moved rows, candidate-major
    const int32_t *by_query;                // [kc * n] k_corr_flag's answer for `rows`
    const Point4 *pts;                      // the map's point array
    double kernel;
    double *slabs;                          // scratch [kc][kScoreReals][quality_groups(n)]
    ScoreRaw *out;                          // [kc]
};
inline size_t score_slab_doubles(int n, uint32_t kc) {
    return static_cast<size_t>(kc) * kScoreReals * quality_groups(n);
}
// the moved rows of the chunk, enqueued on s (n > 0, kc > 0)
void launch_score_move(const ScoreArgs &a, hipStream_t s);
// the pass and the reducer, enqueued on s (n > 0, kc > 0; a.out[0 .. kc) zeroed on s before)
void launch_score(const ScoreArgs &a, hipStream_t s);

}  // namespace sageicp
