// GetCorrespondences on the device, behind the search (correspond.h): accept, compact in query order, gather the target
// rows from the HBM copy of the map, write both sides and the query indices into the caller's memory (gfx950).
//
//   k_corr_flag   one lane per SORTED position j (the order the search answered in): the acceptance test on the
//                 unscaled distance, scattered to the query's own place: by_query[perm[j]] = accepted ? nn : -1
//   k_corr_count  one workgroup per kCorrBlock consecutive QUERIES: wave ballot + popcount -> counts[b]
//   k_corr_scan   one workgroup: the exclusive scan of the counts, kCorrScanTile at a time with a carry; the total
//   k_corr_write  the same workgroups as the count: rank = offsets[b] + the waves below + mbcnt of the ballot; the
//                 accepted lanes write their row through an EgressWriter (egress.h) and their index as one 8-B store
// Kernel boundaries order the four; inside a kernel no workgroup reads what another wrote.  The write kernel is
// launched once per side (the queries' rows with the indices, the map's rows), each launch an instance for ONE writer:
// the 24 layouts of a destination stay 24 instances, not 24 x 24.
//
// Built with -ffp-contract=off like the rest: the acceptance is the plain IEEE sequence the host entry evaluates.
#include <hip/hip_runtime.h>

#include "correspond.h"

namespace sageicp {

static_assert(kCorrBlock == 256 && kCorrScanTile == 256, "four waves of 64 per workgroup");

__global__ __launch_bounds__(256) void k_corr_flag(CorrespondArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const int32_t nn = a.nn[j];
    bool ok = false;
    if (nn >= 0) {
        // (closest_neighboor - point).head<3>().norm() < max_correspondance_distance (VoxelHashMap.cpp:111), in the
        // exact form of the fused loop (icp_body.h): accept_r2 is the largest r2 with sqrt(r2) < max
        const Point4 q = a.sorted[j], t = a.pts[nn];
        const double dx = t.x - q.x, dy = t.y - q.y, dz = t.z - q.z;
        ok = SAGE_SQNORM3_ACCEPT(dx * dx, dy * dy, dz * dz) <= a.accept_r2;
    }
    a.by_query[a.perm[j]] = ok ? nn : -1;
}

// accepted lanes of this workgroup's waves -> wave_count[4]; returns the ballot of the caller's wave
__device__ __forceinline__ unsigned long long corr_ballot(bool ok, uint32_t *wave_count) {
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63u) == 0u) wave_count[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(b));
    __syncthreads();
    return b;
}

__global__ __launch_bounds__(256) void k_corr_count(CorrespondArgs a) {
    __shared__ uint32_t wave_count[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool ok = i < a.n && a.by_query[i] >= 0;
    (void)corr_ballot(ok, wave_count);
    if (threadIdx.x == 0) a.counts[blockIdx.x] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

__global__ __launch_bounds__(256) void k_corr_scan(const uint32_t *counts, uint32_t *offsets, uint32_t blocks,
                                                   unsigned long long *total) {
    __shared__ uint32_t wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long carry = 0;           // (the same in every lane)
    for (uint32_t base = 0; base < blocks; base += kCorrScanTile) {
        const uint32_t at = base + threadIdx.x;
        const uint32_t v = at < blocks ? counts[at] : 0u;
        uint32_t x = v;                     // inclusive scan over the wave
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wave_sum[w] = x;
        __syncthreads();
        uint32_t below = 0, tile = 0;
        for (uint32_t k = 0; k < 4u; ++k) {
            if (k < w) below += wave_sum[k];
            tile += wave_sum[k];
        }
        if (at < blocks) offsets[at] = static_cast<uint32_t>(carry) + below + (x - v);
        carry += tile;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// a side that is not asked for (the indices alone)
struct NoWriter {
    __device__ __forceinline__ void operator()(size_t, const Point4 &) const {}
};

// kTarget: the map's rows; else the queries' rows and the indices
template <typename W, bool kTarget>
__global__ __launch_bounds__(256) void k_corr_write(CorrespondArgs a, W w) {
    __shared__ uint32_t wave_count[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int32_t nn = i < a.n ? a.by_query[i] : -1;
    const bool ok = nn >= 0;
    const unsigned long long b = corr_ballot(ok, wave_count);
    if (!ok) return;
    uint32_t rank = a.counts[gridDim.x + blockIdx.x];
    for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) rank += wave_count[k];
    rank += __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(b), 0u));
    if constexpr (kTarget) {
        w(rank, a.pts[nn]);
    } else {
        w(rank, a.frame[i]);
        if (a.idx && rank < a.idx_cap) a.idx[rank] = i;
    }
}

void launch_corr_flag(const CorrespondArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_corr_flag, dim3(correspond_blocks(a.n)), dim3(256), 0, s, a);
}

void launch_correspond(const CorrespondArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    const uint32_t blocks = correspond_blocks(a.n);
    const dim3 grid(blocks), block(256);
    hipLaunchKernelGGL(k_corr_flag, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_corr_count, grid, block, 0, s, a);
    hipLaunchKernelGGL(k_corr_scan, dim3(1), block, 0, s, a.counts, a.counts + blocks, blocks, a.total);
    if (a.has_src)
        with_egress_writer(a.src, [&](auto w) { hipLaunchKernelGGL((k_corr_write<decltype(w), false>), grid, block, 0, s, a, w); });
    else if (a.idx)
        hipLaunchKernelGGL((k_corr_write<NoWriter, false>), grid, block, 0, s, a, NoWriter{});
    if (a.has_tgt)
        with_egress_writer(a.tgt, [&](auto w) { hipLaunchKernelGGL((k_corr_write<decltype(w), true>), grid, block, 0, s, a, w); });
}

}  // namespace sageicp
