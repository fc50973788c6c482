// The device side of recall (gfx950) — see recall.h and DESIGN.md D17.
//
//   selection  k_rc_flags -> rocprim::select -> k_rc_needs -> rocprim::exclusive_scan (pairs) -> k_rc_totals, per part
//   fill       k_rc_fill per part (lane per row, as archive.hip's gathers), k_rc_after
//
// The near test is the eviction test of map_update.hip's k_far_flags and HostMap::remove_far, same expression and
// association, on the candidate's first stored row; radius^2 is formed once on the host, as max_dist2 is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "recall.h"

namespace sageicp {

namespace {

constexpr unsigned kFillBlocks = 2048;       // the fill's launch: rows beyond 2048 x 256 are reached by striding

// saturating: a session whose kept rows or units do not fit 32 bits reads as "too many" on the host, never as a small number
struct NeedPlus {
    __host__ __device__ RecallNeed operator()(const RecallNeed &a, const RecallNeed &b) const {
        RecallNeed r;
        r.rows = a.rows + b.rows;
        if (r.rows < a.rows) r.rows = 0xFFFFFFFFu;
        r.units = a.units + b.units;
        if (r.units < a.units) r.units = 0xFFFFFFFFu;
        return r;
    }
};

// the smallest size class that holds `count` points (the last one holds a full voxel)
__device__ __forceinline__ uint32_t class_of(const DevMap &M, uint32_t count) {
    uint32_t k = 0;
    while (k + 1 < static_cast<uint32_t>(M.n_classes) && count > M.class_points[k]) ++k;
    return k;
}

// one lane per candidate: kept iff its first row is not far from the centre
__global__ __launch_bounds__(256) void k_rc_flags(RecallPart P, double cx, double cy, double cz, double radius2) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n_cand) return;
    uint32_t keep = 0;
    Cand c;
    if (cand_of(P, i, c)) {
        const Point4 p = P.rows[c.first];
        const double dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
        keep = (SAGE_SQNORM3_FAR(dx * dx, dy * dy, dz * dz) > radius2) ? 0u : 1u;
    }
    P.flag[i] = keep;
}

// rows and units of the selected voxels; zero from *n_sel on (need[n_cand]: the scan's totals)
__global__ __launch_bounds__(256) void k_rc_needs(RecallPart P, DevMap M) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > P.n_cand) return;
    RecallNeed n{0u, 0u};
    Cand c;
    if (j < P.n_cand && j < *P.n_sel && cand_of(P, P.sel[j], c)) {
        n.rows = c.count;
        n.units = M.class_points[class_of(M, c.count)] / kDevUnitPoints;
    }
    P.need[j] = n;
}

__global__ void k_rc_totals(RecallPart P, RecallTotals *out) {
    if (threadIdx.x || blockIdx.x) return;
    out->voxels = *P.n_sel;
    out->rows = P.off[P.n_cand].rows;
    out->units = P.off[P.n_cand].units;
}

// one 32-byte row as two 16-byte accesses; returns the label
__device__ __forceinline__ double copy_row(Point4 *dst, const Point4 *src) {
    const double2 a = reinterpret_cast<const double2 *>(src)[0];
    const double2 b = reinterpret_cast<const double2 *>(src)[1];
    reinterpret_cast<double2 *>(dst)[0] = a;
    reinterpret_cast<double2 *>(dst)[1] = b;
    return b.y;
}

// the last j in [0, nv) with off[j].rows <= r (off[0].rows == 0 <= r < off[nv].rows)
__device__ __forceinline__ uint32_t voxel_of_row(const RecallNeed *off, uint32_t nv, uint32_t r) {
    uint32_t lo = 0, hi = nv;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid].rows <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// lane per row: row r of the part belongs to its voxel j = voxel_of_row(r), block block0 + j, and goes to its place in
// the region that starts at unit0 + off[j].units; the lane of a voxel's first row also writes what the update pass
// writes for a new voxel.  Nothing is written at or beyond block_end / unit_end (what the host reserved).
__global__ __launch_bounds__(256) void k_rc_fill(RecallPart P, DevMap M, uint32_t block0, uint32_t unit0, uint32_t block_end,
                                                 uint32_t unit_end) {
    const uint32_t nv = min(*P.n_sel, P.n_cand);
    if (nv == 0) return;
    const uint32_t total = P.off[nv].rows;
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < total; r += gridDim.x * 256) {
        const uint32_t j = voxel_of_row(P.off, nv, r);
        const RecallNeed o = P.off[j];
        Cand c;
        if (!cand_of(P, P.sel[j], c)) continue;
        const uint32_t k = r - o.rows, b = block0 + j, unit = unit0 + o.units;
        const uint32_t cls = class_of(M, c.count);
        if (b >= block_end || unit + M.class_points[cls] / kDevUnitPoints > unit_end || k >= M.class_points[cls]) continue;
        const double label = copy_row(M.pts + static_cast<size_t>(unit) * kDevUnitPoints + k, P.rows + c.first + k);
        // zeros[b]: an integer add into its byte of the word that holds it (a voxel has at most 255 rows: no carry)
        if (static_cast<int>(label) == 0) atomicAdd(reinterpret_cast<uint32_t *>(M.zeros) + (b >> 2), 1u << (8u * (b & 3u)));
        if (k == 0) {
            M.regions[b] = (cls << 28) | unit;
            M.block_of[unit] = b;
            const uint32_t word = (unit << 8) | c.count;
            uint32_t s = voxel_hash(c.x, c.y, c.z) & M.mask;
            for (;;) {           // (the table is at most a quarter full: the chain ends)
                if (atomicCAS(&M.table[s].blk, kEmptySlot, word) == kEmptySlot) break;
                s = (s + 1) & M.mask;
            }
            M.table[s].x = c.x;
            M.table[s].y = c.y;
            M.table[s].z = c.z;
            M.slot_of[b] = s;
        }
    }
}

__global__ void k_rc_after(MapCounters *ctr, uint32_t voxels, uint64_t rows, uint32_t units, uint32_t units_cap) {
    if (threadIdx.x || blockIdx.x) return;
    MapCounters c{};
    c.blocks_hi = c.num_voxels = c.used_slots = voxels;
    c.total_points = rows;
    c.units_hi = units;
    c.units_cap = units_cap;
    *ctr = c;                    // (free_count, the free stacks' counts and the last pass's outputs: zero)
}

}  // namespace

size_t recall_temp_bytes(size_t n_cand) {
    size_t a = 0, b = 0;
    uint32_t *v = nullptr;
    RecallNeed *n = nullptr;
    (void)rocprim::select(nullptr, a, rocprim::counting_iterator<uint32_t>(0), v, v, v, n_cand);
    (void)rocprim::exclusive_scan(nullptr, b, n, n, RecallNeed{0u, 0u}, n_cand + 1, NeedPlus());
    return std::max(a, b) + 256;
}

hipError_t recall_select(const RecallPart &P, const DevMap &M, const double center[3], double radius2, void *temp,
                         size_t temp_bytes, RecallTotals *totals, hipStream_t s) {
    if (P.n_cand == 0) return hipMemsetAsync(totals, 0, sizeof(RecallTotals), s);
    const int gb = static_cast<int>((P.n_cand + 255u) / 256u);
    hipLaunchKernelGGL(k_rc_flags, dim3(gb), dim3(256), 0, s, P, center[0], center[1], center[2], radius2);
    size_t tb = temp_bytes;
    hipError_t e = rocprim::select(temp, tb, rocprim::counting_iterator<uint32_t>(0), P.flag, P.sel, P.n_sel,
                                   static_cast<size_t>(P.n_cand), s);
    if (e != hipSuccess) return e;
    const int gc = static_cast<int>((P.n_cand + 1u + 255u) / 256u);
    hipLaunchKernelGGL(k_rc_needs, dim3(gc), dim3(256), 0, s, P, M);
    tb = temp_bytes;
    e = rocprim::exclusive_scan(temp, tb, P.need, P.off, RecallNeed{0u, 0u}, static_cast<size_t>(P.n_cand) + 1, NeedPlus(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rc_totals, dim3(1), dim3(64), 0, s, P, totals);
    return hipGetLastError();
}

hipError_t recall_fill(const RecallPart &P, const DevMap &M, uint32_t block0, uint32_t unit0, uint32_t block_end, uint32_t unit_end,
                       uint32_t n_rows, hipStream_t s) {
    if (n_rows == 0) return hipSuccess;
    const unsigned grid = static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>(kFillBlocks, (static_cast<uint64_t>(n_rows) + 255) / 256)));
    hipLaunchKernelGGL(k_rc_fill, dim3(grid), dim3(256), 0, s, P, M, block0, unit0, block_end, unit_end);
    return hipGetLastError();
}

hipError_t recall_finish(const DevMap &M, uint32_t voxels, uint64_t rows, uint32_t units, uint32_t units_cap, hipStream_t s) {
    hipLaunchKernelGGL(k_rc_after, dim3(1), dim3(64), 0, s, M.ctr, voxels, rows, units, units_cap);
    return hipGetLastError();
}

}  // namespace sageicp
