// A batch of candidate poses scored in one pass (score.h), gfx950.
//
//   k_score_move    one thread per row of the chunk, the grid linear over the kc * n rows (a candidate is not a grid
//                   dimension: n = 1 with 2^20 candidates is 4096 workgroups).  A row is 32 B: read and written as two
//                   16-B pieces.  x' = R[0] x + R[1] y + R[2] z + t: k_tf's operand order (kernels.hip), no contraction.
//   k_score         grid linear over (candidate, group): workgroup b is group b % groups of candidate b / groups and
//                   walks that candidate's tiles g, g + groups, ... as k_quality walks a frame's.  18 running sums per
//                   lane, k_quality's tree at the end, the slab entry [candidate][number][group].
//   k_score_reduce  grid linear over (candidate, number): k_quality_reduce's tree over the candidate's `groups` slabs.
// No workgroup reads what another wrote inside a kernel; the kernel boundary orders the two.  No floating-point atomic.
//
// Built with -ffp-contract=off like the rest: a term is the plain IEEE sequence of quality_pair_term (quality.h).
#include <hip/hip_runtime.h>

#include "score.h"

namespace sageicp {

static_assert(kQualTile == 256 && kQualGroups == 256, "four waves of 64; one thread per slab in the reducer");
static_assert(sizeof(Point4) == 32 && sizeof(double2) == 16, "a row is two 16-byte pieces");

__global__ __launch_bounds__(256) void k_score_move(ScoreArgs a) {
    const uint32_t rows = a.kc * static_cast<uint32_t>(a.n);          // <= kMaxQueries < 2^26
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= rows) return;
    const uint32_t c = row / static_cast<uint32_t>(a.n), i = row - c * static_cast<uint32_t>(a.n);
    const double2 *in = reinterpret_cast<const double2 *>(a.frame + i);
    const double2 xy = in[0], zl = in[1];
    const ScorePose &P = a.poses[c];
    const double *R = P.R;
    const double x = R[0] * xy.x + R[1] * xy.y + R[2] * zl.x + P.t[0];
    const double y = R[3] * xy.x + R[4] * xy.y + R[5] * zl.x + P.t[1];
    const double z = R[6] * xy.x + R[7] * xy.y + R[8] * zl.x + P.t[2];
    double2 *out = reinterpret_cast<double2 *>(a.rows + row);
    out[0] = make_double2(x, y);
    out[1] = make_double2(z, zl.y);
}

__global__ __launch_bounds__(256) void k_score(ScoreArgs a, uint32_t groups) {
    __shared__ double wave_real[4][kScoreReals];
    __shared__ uint32_t wave_cnt[4][4];
    const int t = static_cast<int>(threadIdx.x);
    const uint32_t c = blockIdx.x / groups, g = blockIdx.x - c * groups;
    const size_t base = static_cast<size_t>(c) * static_cast<size_t>(a.n);
    const Point4 *frame = a.rows + base;
    const int32_t *by_query = a.by_query + base;

    double acc[kScoreReals];
#pragma unroll
    for (int r = 0; r < kScoreReals; ++r) acc[r] = 0.0;
    QualPairCounts cnt;
    const double k = a.kernel, k2 = k * k;
    const uint32_t tiles = (static_cast<uint32_t>(a.n) + 255u) / 256u;
    for (uint32_t tile = g; tile < tiles; tile += groups) {
        const uint32_t i = tile * 256u + static_cast<uint32_t>(t);
        if (i >= static_cast<uint32_t>(a.n)) continue;
        const int32_t nn = by_query[i];
        if (nn < 0) continue;
        (void)quality_pair_term<false>(frame[i], a.pts[nn], k, k2, acc, cnt);
    }

    // the lanes' sums: wave, then the four waves (k_quality's tree)
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int r = 0; r < kScoreReals; ++r) {
        const double v = wave_sum_f64(acc[r]);
        if (lane == 0) wave_real[wv][r] = v;
    }
    {
        const uint32_t p = wave_sum_u32(cnt.pairs), q = wave_sum_u32(cnt.same), u = wave_sum_u32(cnt.unlabelled), x = wave_sum_u32(cnt.cross);
        if (lane == 0) {
            wave_cnt[wv][0] = p; wave_cnt[wv][1] = q; wave_cnt[wv][2] = u; wave_cnt[wv][3] = x;
        }
    }
    __syncthreads();
    if (t < kScoreReals)
        a.slabs[(static_cast<size_t>(c) * kScoreReals + static_cast<size_t>(t)) * groups + g] =
            (wave_real[0][t] + wave_real[1][t]) + (wave_real[2][t] + wave_real[3][t]);
    // the counts: one integer atomic per workgroup and non-empty word
    if (t < 4) {
        const unsigned long long v = static_cast<unsigned long long>(wave_cnt[0][t]) + wave_cnt[1][t] + wave_cnt[2][t] + wave_cnt[3][t];
        if (v) atomicAdd(&a.out[c].counts[t], v);
    }
}
static_assert(kQPairs == 0 && kQSame == 1 && kQUnlabelled == 2 && kQCross == 3, "the order the four counters leave in");

__global__ __launch_bounds__(256) void k_score_reduce(const double *slabs, uint32_t groups, ScoreRaw *out) {
    __shared__ double wave_v[4];
    const uint32_t t = threadIdx.x;
    const uint32_t c = blockIdx.x / static_cast<uint32_t>(kScoreReals), num = blockIdx.x - c * static_cast<uint32_t>(kScoreReals);
    const double v = wave_sum_f64(t < groups ? slabs[(static_cast<size_t>(c) * kScoreReals + num) * groups + t] : 0.0);
    if ((t & 63u) == 0u) wave_v[t >> 6] = v;
    __syncthreads();
    if (t != 0u) return;
    out[c].real[num] = (wave_v[0] + wave_v[1]) + (wave_v[2] + wave_v[3]);
}

void launch_score_move(const ScoreArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.kc == 0) return;
    const uint64_t rows = static_cast<uint64_t>(a.kc) * static_cast<uint64_t>(a.n);
    hipLaunchKernelGGL(k_score_move, dim3(static_cast<uint32_t>((rows + 255u) / 256u)), dim3(256), 0, s, a);
}

void launch_score(const ScoreArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.kc == 0) return;
    const uint32_t groups = quality_groups(a.n);
    hipLaunchKernelGGL(k_score, dim3(a.kc * groups), dim3(256), 0, s, a, groups);
    hipLaunchKernelGGL(k_score_reduce, dim3(a.kc * static_cast<uint32_t>(kScoreReals)), dim3(256), 0, s, a.slabs, groups, a.out);
}

}  // namespace sageicp
