// The device side of a map's archive (gfx950) — see archive.h and DESIGN.md D15.
//
//   append    k_arc_counts -> rocprim::exclusive_scan -> k_arc_gather -> k_arc_after, between the search for the far
//             voxels (map_update.hip: k_far_flags + select, or the list the host's sweep hands over in reference-order
//             mode) and their eviction (k_far_apply), which frees the regions the rows are read from
//   LATEST    k_lat_keys -> stable radix sort of (key, record) -> k_lat_flags (the last record of each run, unless the
//             map's slot table holds the key) -> rocprim::select in log order -> k_lat_counts -> scan; the rows follow
//             through k_lat_gather
//
// No atomic decides a position: a voxel's rows land at tail + (exclusive scan of the counts), the records at
// voxels + j, so the same bytes come out on every run.  The gathers are fixed, grid-strided launches that read their
// totals from device memory: one 32-byte row per lane, consecutive lanes write consecutive rows, the lane finds its voxel
// by bisection of the scanned offsets (a dozen cached loads for a few thousand voxels).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "archive.h"

namespace sageicp {

namespace {

constexpr int kKeyBias = 1 << 20;
constexpr unsigned kGatherBlocks = 2048;     // the gathers' launch: rows beyond 2048 x 256 are reached by striding

// one 32-byte row as two 16-byte accesses
__device__ __forceinline__ void copy_row(Point4 *dst, const Point4 *src) {
    const double2 a = reinterpret_cast<const double2 *>(src)[0];
    const double2 b = reinterpret_cast<const double2 *>(src)[1];
    reinterpret_cast<double2 *>(dst)[0] = a;
    reinterpret_cast<double2 *>(dst)[1] = b;
}

// the last j in [0, nv) with offsets[j] <= r (offsets[0] == 0 <= r < offsets[nv])
__device__ __forceinline__ uint32_t voxel_of_row(const uint32_t *offsets, uint32_t nv, uint32_t r) {
    uint32_t lo = 0, hi = nv;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- append ----------------------------------------------------------------------------------------------------------
// counts of the selected voxels from their slot words; counts[j] = 0 from *n_sel on (counts[bound]: the scan's total)
__global__ __launch_bounds__(256) void k_arc_counts(DevMap M, const uint32_t *sel, const uint32_t *n_sel, uint32_t bound,
                                                    uint32_t *counts) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > bound) return;
    uint32_t c = 0;
    if (j < bound && j < *n_sel) c = M.table[M.slot_of[sel[j]]].blk & 255u;
    counts[j] = c;
}

// does voxel j (rows [o, o + cnt) of this call) still fit?  Monotone in j: what is kept is a prefix.
__device__ __forceinline__ bool arc_fits(const ArchiveDev &A, const ArchiveCtr &c, uint32_t j, uint32_t end) {
    return c.rows + end <= A.limit_rows && c.rows + end <= A.cap_rows && c.voxels + j < A.cap_vox;
}

// lane per row: row r of this call belongs to voxel j = voxel_of_row(r) and goes to rows[tail + r]; the lane of a voxel's
// first row also writes its record
__global__ __launch_bounds__(256) void k_arc_gather(DevMap M, ArchiveDev A, const uint32_t *sel, const uint32_t *n_sel,
                                                    uint32_t bound) {
    const uint32_t nv = min(*n_sel, bound);
    if (nv == 0) return;
    const ArchiveCtr c = *A.ctr;
    if (c.full) return;
    const uint32_t total = A.offsets[nv];
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < total; r += gridDim.x * 256) {
        const uint32_t j = voxel_of_row(A.offsets, nv, r);
        const uint32_t o = A.offsets[j], end = A.offsets[j + 1];
        if (!arc_fits(A, c, j, end)) break;        // (so does no later row of this lane)
        const uint32_t b = sel[j];
        const Point4 *src = M.pts + static_cast<size_t>(M.regions[b] & 0x0FFFFFFFu) * kDevUnitPoints + (r - o);
        copy_row(A.rows + c.rows + r, src);
        if (r == o) {
            const Slot e = M.table[M.slot_of[b]];
            ArchiveVoxel v;
            v.x = e.x; v.y = e.y; v.z = e.z;
            v.count = end - o;
            v.first_row = c.rows + o;
            v.update = A.serial;
            A.vox[c.voxels + j] = v;
        }
    }
}

// the tail advanced by the voxels that fitted (a prefix: bisection of the monotone end offsets), the rest counted
__global__ void k_arc_after(ArchiveDev A, const uint32_t *n_sel, uint32_t bound) {
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t nv = min(*n_sel, bound);
    if (nv == 0) return;
    ArchiveCtr c = *A.ctr;
    const uint32_t total = A.offsets[nv];
    uint32_t k = 0;                                // voxels kept
    if (!c.full) {
        if (arc_fits(A, c, nv - 1, total)) k = nv;
        else {
            uint32_t lo = 0, hi = nv;              // lo voxels fit, hi do not
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (arc_fits(A, c, mid - 1, A.offsets[mid])) lo = mid; else hi = mid;
            }
            k = lo;
        }
    }
    const uint32_t kept_rows = A.offsets[k];
    c.rows += kept_rows;
    c.voxels += k;
    if (k < nv) {
        c.full = 1u;
        c.dropped_rows += total - kept_rows;
        c.dropped_voxels += nv - k;
    }
    *A.ctr = c;
}

// ---- LATEST ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long pack_key(int x, int y, int z) {      // as the update packs it (map_update.hip)
    return (static_cast<unsigned long long>(static_cast<uint32_t>(x + kKeyBias)) << 42) |
           (static_cast<unsigned long long>(static_cast<uint32_t>(y + kKeyBias)) << 21) |
           static_cast<unsigned long long>(static_cast<uint32_t>(z + kKeyBias));
}

__global__ __launch_bounds__(256) void k_lat_keys(const ArchiveVoxel *vox, uint32_t nv, unsigned long long *keys, uint32_t *idx) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const ArchiveVoxel v = vox[i];
    keys[i] = pack_key(v.x, v.y, v.z);
    idx[i] = i;
}

// sorted position p: the last of its run (the sort is stable: the latest record of the key) survives unless the map
// holds the key; the verdict goes to the record's own place, so the selection that follows is in log order
__global__ __launch_bounds__(256) void k_lat_flags(const unsigned long long *keys, const uint32_t *idx, uint32_t nv,
                                                   const ArchiveVoxel *vox, const Slot *table, uint32_t mask, uint32_t *flag) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nv) return;
    const uint32_t i = idx[p];
    uint32_t keep = (p + 1 == nv || keys[p + 1] != keys[p]) ? 1u : 0u;
    if (keep && table) {
        const ArchiveVoxel v = vox[i];
        uint32_t s = voxel_hash(v.x, v.y, v.z) & mask;
        for (uint32_t step = 0; step <= mask; ++step) {       // (the table is never full: the probe ends at an empty slot)
            const Slot e = table[s];
            if (e.blk == kEmptySlot) break;
            if (e.x == v.x && e.y == v.y && e.z == v.z) {     // tombstones never match
                keep = 0u;
                break;
            }
            s = (s + 1) & mask;
        }
    }
    flag[i] = keep;
}

__global__ __launch_bounds__(256) void k_lat_counts(const ArchiveVoxel *vox, const uint32_t *sel, const uint32_t *n_sel, uint32_t nv,
                                                    uint32_t *counts) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j > nv) return;
    counts[j] = (j < nv && j < *n_sel) ? vox[sel[j]].count : 0u;
}

// rows [first, first + n) of the selection into out[0 .. n)
__global__ __launch_bounds__(256) void k_lat_gather(const Point4 *rows, const ArchiveVoxel *vox, const uint32_t *sel,
                                                    const uint32_t *n_sel, const uint32_t *offsets, uint64_t first, uint64_t n,
                                                    Point4 *out) {
    const uint32_t nv = *n_sel;
    if (nv == 0) return;
    const uint32_t total = offsets[nv];
    for (uint64_t q = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; q < n; q += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint64_t r64 = first + q;
        if (r64 >= total) break;
        const uint32_t r = static_cast<uint32_t>(r64);
        const uint32_t j = voxel_of_row(offsets, nv, r);
        copy_row(out + q, rows + vox[sel[j]].first_row + (r - offsets[j]));
    }
}

unsigned gather_grid(uint64_t rows) {
    return static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>(kGatherBlocks, (rows + 255) / 256)));
}

}  // namespace

size_t archive_temp_bytes(size_t nb) {
    size_t a = 0;
    uint32_t *v = nullptr;
    (void)rocprim::exclusive_scan(nullptr, a, v, v, 0u, nb + 1, rocprim::plus<uint32_t>());
    return a + 256;
}

hipError_t archive_append(const DevMap &M, const ArchiveDev &A, const uint32_t *sel, const uint32_t *n_sel, uint32_t bound,
                          hipStream_t s) {
    if (bound == 0) return hipSuccess;
    const int gb = static_cast<int>((bound + 1u + 255u) / 256u);
    hipLaunchKernelGGL(k_arc_counts, dim3(gb), dim3(256), 0, s, M, sel, n_sel, bound, A.counts);
    size_t tb = A.temp_bytes;
    hipError_t e = rocprim::exclusive_scan(A.temp, tb, A.counts, A.offsets, 0u, static_cast<size_t>(bound) + 1,
                                           rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    // the rows one update can evict are not known here: the grid is fixed, sized for the blocks it may select (a voxel
    // holds a handful of rows), and strides over whatever the scan found
    hipLaunchKernelGGL(k_arc_gather, dim3(gather_grid(static_cast<uint64_t>(bound) * 4)), dim3(256), 0, s, M, A, sel, n_sel, bound);
    hipLaunchKernelGGL(k_arc_after, dim3(1), dim3(64), 0, s, A, n_sel, bound);
    return hipGetLastError();
}

size_t archive_latest_temp_bytes(size_t nv) {
    size_t a = 0, b = 0, c = 0;
    unsigned long long *k = nullptr;
    uint32_t *v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, k, k, v, v, nv, 0, 63);
    (void)rocprim::select(nullptr, b, rocprim::counting_iterator<uint32_t>(0), v, v, v, nv);
    (void)rocprim::exclusive_scan(nullptr, c, v, v, 0u, nv + 1, rocprim::plus<uint32_t>());
    return std::max(a, std::max(b, c)) + 256;
}

hipError_t archive_latest(const ArchiveVoxel *vox, uint32_t nv, const Slot *table, uint32_t mask, const LatestScratch &S,
                          hipStream_t s) {
    if (nv == 0) return hipMemsetAsync(S.n_sel, 0, sizeof(uint32_t), s);
    const int gb = static_cast<int>((nv + 255u) / 256u);
    hipLaunchKernelGGL(k_lat_keys, dim3(gb), dim3(256), 0, s, vox, nv, S.keys, S.idx);
    size_t tb = S.temp_bytes;
    hipError_t e = rocprim::radix_sort_pairs(S.temp, tb, S.keys, S.keys_alt, S.idx, S.idx_alt, static_cast<size_t>(nv), 0, 63, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lat_flags, dim3(gb), dim3(256), 0, s, S.keys_alt, S.idx_alt, nv, vox, table, mask, S.flag);
    tb = S.temp_bytes;
    e = rocprim::select(S.temp, tb, rocprim::counting_iterator<uint32_t>(0), S.flag, S.sel, S.n_sel, static_cast<size_t>(nv), s);
    if (e != hipSuccess) return e;
    const int gc = static_cast<int>((nv + 1u + 255u) / 256u);
    hipLaunchKernelGGL(k_lat_counts, dim3(gc), dim3(256), 0, s, vox, S.sel, S.n_sel, nv, S.counts);
    tb = S.temp_bytes;
    e = rocprim::exclusive_scan(S.temp, tb, S.counts, S.offsets, 0u, static_cast<size_t>(nv) + 1, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t archive_gather_selected(const Point4 *rows, const ArchiveVoxel *vox, const LatestScratch &S, uint64_t first, uint64_t n,
                                   Point4 *out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lat_gather, dim3(gather_grid(n)), dim3(256), 0, s, rows, vox, S.sel, S.n_sel, S.offsets, first, n, out);
    return hipGetLastError();
}

}  // namespace sageicp
