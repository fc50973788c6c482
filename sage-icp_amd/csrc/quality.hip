// Registration quality on the device, behind the search and k_corr_flag (quality.h): every sum of sageicp_quality
// over the accepted pairs in one pass over the queries (gfx950).
//
//   k_quality         at most kQualGroups workgroups; workgroup g takes the tiles g, g + groups, ... of kQualTile
//                     consecutive queries.  A lane reads by_query[i], its moved row frame[i] and, accepted, pts[nn]; it
//                     adds the pair's kQualReals terms to its own running sums and counts the query and the pair in the
//                     workgroup's class tables (LDS integer atomics).  Per tile the pairs' (class, |r|^2) are staged in
//                     LDS and thread c adds those of class c in query order.  At the end the lanes' sums meet in a fixed
//                     tree — xor butterfly over the wave, then (w0 + w1) + (w2 + w3) — and the workgroup stores its slab;
//                     the counts leave through one 64-bit integer atomic per workgroup and non-empty word.
//   k_quality_reduce  one workgroup per real number: thread t holds slab t, the same fixed tree, one store.
// No workgroup reads what another wrote inside a kernel; the kernel boundary orders the two.  No floating-point atomic.
//
// Built with -ffp-contract=off like the rest: a term is the plain IEEE sequence written below (k_gn's, kernels.hip).
#include <hip/hip_runtime.h>

#include "quality.h"

namespace sageicp {

static_assert(kQualTile == 256 && kQualGroups == 256 && kQualClasses == 256, "four waves of 64; one thread per class and slab");

// the class a label is counted in: static_cast<int>(l) where that lies in 0 .. 255, else the bin of the others
__device__ __forceinline__ int quality_class(double l) { return (l > -1.0 && l < 256.0) ? static_cast<int>(l) : kQualClasses; }

__global__ __launch_bounds__(256) void k_quality(QualityArgs a) {
    __shared__ uint32_t cls_queries[kQualBins], cls_pairs[kQualBins];
    __shared__ int stage_c[kQualTile];
    __shared__ double stage_e[kQualTile];
    __shared__ double wave_real[4][kQualReals];
    __shared__ uint32_t wave_cnt[4][4];
    const int t = static_cast<int>(threadIdx.x);
    for (int b = t; b < kQualBins; b += 256) cls_queries[b] = cls_pairs[b] = 0u;
    __syncthreads();

    double acc[kQualReals];
#pragma unroll
    for (int c = 0; c < kQualReals; ++c) acc[c] = 0.0;
    QualPairCounts cnt;
    double cls_r2 = 0.0, other_r2 = 0.0;         // class t's; thread 0: also the other classes'
    const double k = a.kernel, k2 = k * k;
    const uint32_t tiles = (static_cast<uint32_t>(a.n) + 255u) / 256u;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t i = tile * 256u + static_cast<uint32_t>(t);
        const bool valid = i < static_cast<uint32_t>(a.n);
        const int32_t nn = valid ? a.by_query[i] : -1;
        int pair_class = -1;
        double e = 0.0;
        if (valid) {
            const Point4 s = a.frame[i];
            const int c = quality_class(s.l);
            atomicAdd(&cls_queries[c], 1u);
            if (nn >= 0) {
                e = quality_pair_term<true>(s, a.pts[nn], k, k2, acc, cnt);
                atomicAdd(&cls_pairs[c], 1u);
                pair_class = c;
            }
        }
        // a class's squared residuals: its thread adds them in query order
        stage_c[t] = pair_class;
        stage_e[t] = e;
        if (__syncthreads_or(pair_class >= 0)) {
            for (int j = 0; j < kQualTile; ++j) {
                const int c = stage_c[j];
                if (c == t) cls_r2 += stage_e[j];
                if (t == 0 && c == kQualClasses) other_r2 += stage_e[j];
            }
        }
        __syncthreads();
    }

    // the lanes' sums: wave, then the four waves
    const int lane = t & 63, wv = t >> 6;
#pragma unroll
    for (int c = 0; c < kQualReals; ++c) {
        const double v = wave_sum_f64(acc[c]);
        if (lane == 0) wave_real[wv][c] = v;
    }
    {
        const uint32_t p = wave_sum_u32(cnt.pairs), q = wave_sum_u32(cnt.same), u = wave_sum_u32(cnt.unlabelled), x = wave_sum_u32(cnt.cross);
        if (lane == 0) {
            wave_cnt[wv][0] = p; wave_cnt[wv][1] = q; wave_cnt[wv][2] = u; wave_cnt[wv][3] = x;
        }
    }
    __syncthreads();
    const size_t g = blockIdx.x;
    if (t < kQualReals)
        a.slabs[static_cast<size_t>(t) * kQualGroups + g] = (wave_real[0][t] + wave_real[1][t]) + (wave_real[2][t] + wave_real[3][t]);
    a.slabs[static_cast<size_t>(kQualReals + t) * kQualGroups + g] = cls_r2;
    if (t == 0) a.slabs[static_cast<size_t>(kQualReals + kQualClasses) * kQualGroups + g] = other_r2;
    // the counts: one integer atomic per workgroup and non-empty word
    if (t < 4) {
        const unsigned long long v = static_cast<unsigned long long>(wave_cnt[0][t]) + wave_cnt[1][t] + wave_cnt[2][t] + wave_cnt[3][t];
        if (v) atomicAdd(&a.out->counts[kQPairs + t], v);
    }
    if (cls_queries[t]) atomicAdd(&a.out->class_queries[t], static_cast<unsigned long long>(cls_queries[t]));
    if (cls_pairs[t]) atomicAdd(&a.out->class_pairs[t], static_cast<unsigned long long>(cls_pairs[t]));
    if (t == 0) {
        if (cls_queries[kQualClasses]) atomicAdd(&a.out->counts[kQOtherQueries], static_cast<unsigned long long>(cls_queries[kQualClasses]));
        if (cls_pairs[kQualClasses]) atomicAdd(&a.out->counts[kQOtherPairs], static_cast<unsigned long long>(cls_pairs[kQualClasses]));
    }
}
static_assert(kQPairs == 0 && kQSame == 1 && kQUnlabelled == 2 && kQCross == 3, "the order the four counters leave in");

__global__ __launch_bounds__(256) void k_quality_reduce(const double *slabs, uint32_t groups, QualityRaw *out) {
    __shared__ double wave_v[4];
    const uint32_t t = threadIdx.x, num = blockIdx.x;
    const double v = wave_sum_f64(t < groups ? slabs[static_cast<size_t>(num) * kQualGroups + t] : 0.0);
    if ((t & 63u) == 0u) wave_v[t >> 6] = v;
    __syncthreads();
    if (t != 0u) return;
    const double total = (wave_v[0] + wave_v[1]) + (wave_v[2] + wave_v[3]);
    if (num < static_cast<uint32_t>(kQualReals)) out->real[num] = total;
    else out->class_r2[num - kQualReals] = total;
}

void launch_quality(const QualityArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    const uint32_t groups = quality_groups(a.n);
    hipLaunchKernelGGL(k_quality, dim3(groups), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_quality_reduce, dim3(kQualReals + kQualBins), dim3(256), 0, s, a.slabs, groups, a.out);
}

}  // namespace sageicp
