// The device side of a loop closure (gfx950) — see closure.h and DESIGN.md D18.
//
//   selection  k_cl_flags -> rocprim::select -> k_cl_counts -> rocprim::exclusive_scan, per part
//   stays      k_cl_stays per part (lane per voxel, a wave walks one k)
//   move       k_cl_move per part (lane per row)
//
// The far test is the eviction test of map_update.hip's k_far_flags and HostMap::remove_far, same expression and
// association, on the voxel's first stored row; max_distance^2 is formed once on the host, as max_dist2 is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>

#include <rocprim/rocprim.hpp>

#include "closure.h"
#include "se3_math.h"

namespace sageicp {

namespace {

constexpr unsigned kStayBlocks = 512;        // the walk's launch: voxels beyond 512 x 256 are reached by striding
constexpr unsigned kMoveBlocks = 1024;       // the move's launch: rows beyond 1024 x 256 likewise

__global__ __launch_bounds__(256) void k_cl_flags(RecallPart P) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n_cand) return;
    Cand c;
    P.flag[i] = cand_of(P, i, c) ? 1u : 0u;
}

// rows of the selected voxels; zero from *n_sel on (cnt[n_cand]: the scan's total)
__global__ __launch_bounds__(256) void k_cl_counts(ClosurePart C) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > C.P.n_cand) return;
    uint32_t n = 0;
    Cand c;
    if (j < C.P.n_cand && j < *C.P.n_sel && cand_of(C.P, C.P.sel[j], c)) n = c.count;
    C.cnt[j] = n;
}

// A lane per selected voxel; the lanes of a wave walk the positions together.  top = hi + 1: the number of positions
// the voxel's walk may look at, min(update, n) for a record, n for a live voxel.
__global__ __launch_bounds__(256) void k_cl_stays(ClosurePart C, const double *__restrict__ positions, uint32_t n,
                                                  double max_dist2) {
    const RecallPart &P = C.P;
    const uint32_t nv = min(*P.n_sel, P.n_cand);
    const uint32_t lane = threadIdx.x & 63u;
    // (whole waves go round: the bound is the same for the 64 lanes)
    for (uint64_t base = static_cast<uint64_t>(blockIdx.x) * 256 + (threadIdx.x - lane); base < nv;
         base += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t j = base + lane;
        double px = 0.0, py = 0.0, pz = 0.0;
        uint32_t top = 0;
        bool valid = false;
        if (j < nv) {
            const uint32_t i = P.sel[j];
            Cand c;
            if (cand_of(P, i, c)) {
                valid = true;
                const Point4 p = P.rows[c.first];
                px = p.x; py = p.y; pz = p.z;
                top = n;
                if (P.vox) {
                    const uint64_t u = P.vox[i].update;
                    if (u < n) top = static_cast<uint32_t>(u);
                }
            }
        }
        uint32_t best = top ? top - 1u : 0u;         // nothing walked: max(hi, 0)
        double best_d = std::numeric_limits<double>::infinity();
        bool walking = valid && top > 0u;
        uint32_t wave_top = top;
        for (int o = 32; o; o >>= 1) wave_top = max(wave_top, static_cast<uint32_t>(__shfl_xor(static_cast<int>(wave_top), o)));
        uint32_t k = __builtin_amdgcn_readfirstlane(wave_top);
        while (k > 0u && __ballot(walking) != 0ull) {
            --k;                                     // (k < wave_top <= n: inside the table)
            const double cx = positions[3 * static_cast<size_t>(k)];
            const double cy = positions[3 * static_cast<size_t>(k) + 1];
            const double cz = positions[3 * static_cast<size_t>(k) + 2];
            if (walking && k < top) {
                const double dx = px - cx, dy = py - cy, dz = pz - cz;
                const double d = SAGE_SQNORM3_FAR(dx * dx, dy * dy, dz * dz);
                if (d > max_dist2) {
                    walking = false;                 // the stay began after position k
                } else if (d < best_d) {             // strictly: a tie stays with the later pose
                    best_d = d;
                    best = k;
                }
            }
        }
        if (valid) C.stay[j] = best;
    }
}

// the last j in [0, nv) with off[j] <= r (off[0] == 0 <= r < off[nv])
__device__ __forceinline__ uint32_t voxel_of_row(const uint32_t *off, uint32_t nv, uint32_t r) {
    uint32_t lo = 0, hi = nv;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_cl_move(ClosurePart C, const double *__restrict__ corrections, uint32_t row_a,
                                                 uint32_t row_b, Point4 *__restrict__ out) {
    const RecallPart &P = C.P;
    const uint32_t nv = min(*P.n_sel, P.n_cand);
    if (nv == 0) return;
    const uint32_t total = min(row_b, C.off[nv]);
    for (uint64_t r64 = static_cast<uint64_t>(row_a) + blockIdx.x * 256 + threadIdx.x; r64 < total;
         r64 += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint32_t r = static_cast<uint32_t>(r64);
        const uint32_t j = voxel_of_row(C.off, nv, r);
        Cand c;
        if (!cand_of(P, P.sel[j], c)) continue;
        const uint32_t k = r - C.off[j];
        if (k >= c.count) continue;
        const double *T = corrections + 7 * static_cast<size_t>(C.stay[j]);
        const double q[4] = {T[0], T[1], T[2], T[3]}, t[3] = {T[4], T[5], T[6]};
        double R[9], o[3];
        quat_to_mat(q, R);
        Point4 p = P.rows[c.first + k];
        const double v[3] = {p.x, p.y, p.z};
        mat_apply(R, t, v, o);
        p.x = o[0]; p.y = o[1]; p.z = o[2];
        out[r - row_a] = p;
    }
}

}  // namespace

size_t closure_temp_bytes(size_t n_cand) {
    size_t a = 0, b = 0;
    uint32_t *v = nullptr;
    (void)rocprim::select(nullptr, a, rocprim::counting_iterator<uint32_t>(0), v, v, v, n_cand);
    (void)rocprim::exclusive_scan(nullptr, b, v, v, 0u, n_cand + 1, rocprim::plus<uint32_t>());
    return std::max(a, b) + 256;
}

hipError_t closure_select(const ClosurePart &C, void *temp, size_t temp_bytes, hipStream_t s) {
    const RecallPart &P = C.P;
    if (P.n_cand == 0) return hipSuccess;
    const int gb = static_cast<int>((P.n_cand + 255u) / 256u);
    hipLaunchKernelGGL(k_cl_flags, dim3(gb), dim3(256), 0, s, P);
    size_t tb = temp_bytes;
    hipError_t e = rocprim::select(temp, tb, rocprim::counting_iterator<uint32_t>(0), P.flag, P.sel, P.n_sel,
                                   static_cast<size_t>(P.n_cand), s);
    if (e != hipSuccess) return e;
    const int gc = static_cast<int>((static_cast<uint64_t>(P.n_cand) + 1u + 255u) / 256u);
    hipLaunchKernelGGL(k_cl_counts, dim3(gc), dim3(256), 0, s, C);
    tb = temp_bytes;
    e = rocprim::exclusive_scan(temp, tb, C.cnt, C.off, 0u, static_cast<size_t>(P.n_cand) + 1, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t closure_stays(const ClosurePart &C, const double *positions, uint32_t n, double max_dist2, hipStream_t s) {
    if (C.P.n_cand == 0 || n == 0) return hipSuccess;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(kStayBlocks, (static_cast<uint64_t>(C.P.n_cand) + 255) / 256));
    hipLaunchKernelGGL(k_cl_stays, dim3(grid), dim3(256), 0, s, C, positions, n, max_dist2);
    return hipGetLastError();
}

hipError_t closure_move(const ClosurePart &C, const double *corrections, uint32_t row_a, uint32_t row_b, Point4 *out,
                        hipStream_t s) {
    if (C.P.n_cand == 0 || row_b <= row_a) return hipSuccess;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(kMoveBlocks, (static_cast<uint64_t>(row_b - row_a) + 255) / 256));
    hipLaunchKernelGGL(k_cl_move, dim3(grid), dim3(256), 0, s, C, corrections, row_a, row_b, out);
    return hipGetLastError();
}

}  // namespace sageicp
