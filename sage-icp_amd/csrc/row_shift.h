// Index arithmetic of a neighbourhood row that follows its query into a NEIGHBOURING voxel (icp_body.h, the stale-row
// section): which of the 27 voxels of the new 3 x 3 x 3 block are new, which are kept and where those stood in the old
// row, and what becomes of the occupancy mask.  Plain integer code, __host__ __device__: tests/row_shift_check.cpp
// checks it exhaustively on the CPU.
//
// A voxel of a block is v = 9 x + 3 y + z, x, y, z in 0..2 (the enumeration order of the row).  The home voxel moved
// by d = (dx, dy, dz), every component -1, 0 or +1, not all zero.  Voxel v' = (x', y', z') of the NEW block is the
// voxel (x' + dx, y' + dy, z' + dz) of the old one: kept if that lies in [0, 2]^3 — its row word moves from
// v' + 9 dx + 3 dy + dz to v' — and new otherwise: 9 new voxels through a face, 15 through an edge, 19 through a corner.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAGE_RS_HD __host__ __device__ __forceinline__
#define SAGE_RS_UNROLL _Pragma("unroll")
#else
#define SAGE_RS_HD inline
#define SAGE_RS_UNROLL
#endif

namespace sageicp {
namespace rowshift {

constexpr uint32_t kAll = 0x7FFFFFFu;                       // the 27 voxels
constexpr uint32_t kX0 = 0x00001FFu, kX2 = kX0 << 18;       // the layers x == 0 / x == 2 ...
constexpr uint32_t kY0 = 0x01C0E07u, kY2 = kY0 << 6;
constexpr uint32_t kZ0 = 0x1249249u, kZ2 = kZ0 << 2;

SAGE_RS_HD uint32_t popcount(uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__popc(m));
#else
    return static_cast<uint32_t>(__builtin_popcount(m));
#endif
}
SAGE_RS_HD uint32_t lowest(uint32_t m) {                    // index of the lowest set bit (m != 0)
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__ffs(static_cast<int>(m)) - 1);
#else
    return static_cast<uint32_t>(__builtin_ctz(m));
#endif
}

// where a kept voxel's word stood in the old row, relative to its place in the new one
SAGE_RS_HD int delta(int dx, int dy, int dz) { return 9 * dx + 3 * dy + dz; }

// the voxels of the new block that the old block had as well
SAGE_RS_HD uint32_t kept_mask(int dx, int dy, int dz) {
    const uint32_t gx = dx > 0 ? kX2 : (dx < 0 ? kX0 : 0u);   // the layer that entered on each axis
    const uint32_t gy = dy > 0 ? kY2 : (dy < 0 ? kY0 : 0u);
    const uint32_t gz = dz > 0 ? kZ2 : (dz < 0 ? kZ0 : 0u);
    return kAll & ~(gx | gy | gz);
}
SAGE_RS_HD uint32_t new_mask(int dx, int dy, int dz) { return kAll & ~kept_mask(dx, dy, dz); }
SAGE_RS_HD uint32_t new_count(int dx, int dy, int dz) { return popcount(new_mask(dx, dy, dz)); }

// old position of the kept voxel v of the new block
SAGE_RS_HD uint32_t old_position(uint32_t v, int dx, int dy, int dz) {
    return static_cast<uint32_t>(static_cast<int>(v) + delta(dx, dy, dz));
}

// the occupancy mask of the kept voxels under the new enumeration: bit v' takes bit v' + delta of the old mask
// (one shift by 9 dx + 3 dy + dz; what a shift by 9, by 3 and by 1 would carry across a layer lies outside `kept`)
SAGE_RS_HD uint32_t shifted_mask(uint32_t occ, int dx, int dy, int dz) {
    const int d = delta(dx, dy, dz);
    const uint32_t m = d >= 0 ? occ >> d : occ << -d;
    return m & kept_mask(dx, dy, dz);
}

// ---- dealing the new voxels over the W lanes of a query, by rank in enumeration order ---------------------------
// m with its lowest set bit cleared if `on` (m == 0 stays 0)
SAGE_RS_HD uint32_t drop_lowest_if(uint32_t m, bool on) {
    const uint32_t c = on ? 1u : 0u;
    return m & ((m - c) | (c - 1u));
}
// rank -> voxel: the r-th (from 0) voxel of `m` in enumeration order; r < popcount(m)
SAGE_RS_HD uint32_t nth_voxel(uint32_t m, uint32_t r) {
    for (uint32_t i = 0; i < r; ++i) m &= m - 1u;
    return lowest(m);
}
// Lane ci of W takes the ranks ci, ci + W, ...: `lane_first` leaves the voxels of rank >= ci, the lane's next voxel is
// then lowest(m) while m != 0, and `lane_next` steps over the W - 1 voxels of the query's other lanes.
template <int W>
SAGE_RS_HD uint32_t lane_first(uint32_t m, uint32_t ci) {
    SAGE_RS_UNROLL
    for (uint32_t t = 0; t + 1 < static_cast<uint32_t>(W); ++t) m = drop_lowest_if(m, t < ci);
    return m;
}
template <int W>
SAGE_RS_HD uint32_t lane_next(uint32_t m) {
    SAGE_RS_UNROLL
    for (int t = 0; t < W; ++t) m &= m - 1u;
    return m;
}

}  // namespace rowshift
}  // namespace sageicp
