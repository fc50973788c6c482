// Exhaustive CPU check of csrc/row_shift.h, the index arithmetic of a neighbourhood row that follows its query into a
// neighbouring voxel.  Stand-alone: g++ -O2 -I sage-icp_amd/csrc tests/row_shift_check.cpp && ./a.out [all]
// For all 26 shifts: the new voxels number 9 (face), 15 (edge) or 19 (corner); every rank maps to a distinct new voxel,
// in enumeration order; kept and new voxels together are the 27; the old position of every kept voxel lies in the block
// and is the voxel the geometry says; the lanes' dealing (4, 8 and 16 lanes) visits rank ci, ci + W, ...; the shifted
// occupancy mask equals the mask built voxel by voxel — for a seeded million masks, or with `all` for all 2^27.
// Prints one line per failure and "row_shift_check: OK <checks>" at the end; exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "row_shift.h"

using namespace sageicp::rowshift;

static long checks = 0, failures = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        ++checks;                             \
        if (!(c)) {                           \
            ++failures;                       \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");                \
        }                                     \
    } while (0)

template <int W>
static void check_dealing(uint32_t nm, int dx, int dy, int dz) {
    const uint32_t n = popcount(nm);
    uint32_t seen = 0u;
    for (uint32_t ci = 0; ci < static_cast<uint32_t>(W); ++ci) {
        uint32_t m = lane_first<W>(nm, ci);
        for (uint32_t r = ci;; r += W) {
            if (r >= n) {
                CHECK(m == 0u, "W=%d shift %d %d %d lane %u: voxels left after rank %u", W, dx, dy, dz, ci, r);
                break;
            }
            CHECK(m != 0u, "W=%d shift %d %d %d lane %u: no voxel at rank %u", W, dx, dy, dz, ci, r);
            if (m == 0u) break;
            const uint32_t v = lowest(m);
            CHECK(v == nth_voxel(nm, r), "W=%d shift %d %d %d lane %u rank %u: voxel %u", W, dx, dy, dz, ci, r, v);
            CHECK(!((seen >> v) & 1u), "W=%d shift %d %d %d: voxel %u dealt twice", W, dx, dy, dz, v);
            seen |= 1u << v;
            m = lane_next<W>(m);
        }
    }
    CHECK(seen == nm, "W=%d shift %d %d %d: dealt %07x of %07x", W, dx, dy, dz, seen, nm);
}

static uint32_t mask_by_voxel(uint32_t occ, int dx, int dy, int dz) {
    uint32_t m = 0u;
    for (int v = 0; v < 27; ++v) {
        const int a = v / 9 + dx, b = (v / 3) % 3 + dy, c = v % 3 + dz;
        if (a < 0 || a > 2 || b < 0 || b > 2 || c < 0 || c > 2) continue;
        m |= ((occ >> (a * 9 + b * 3 + c)) & 1u) << v;
    }
    return m;
}

int main(int argc, char **argv) {
    const bool all = argc > 1 && !std::strcmp(argv[1], "all");
    int shifts = 0;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                if (!dx && !dy && !dz) continue;
                ++shifts;
                const int axes = (dx != 0) + (dy != 0) + (dz != 0);
                const uint32_t want = axes == 1 ? 9u : axes == 2 ? 15u : 19u;
                const uint32_t kept = kept_mask(dx, dy, dz), nm = new_mask(dx, dy, dz);
                CHECK(new_count(dx, dy, dz) == want, "shift %d %d %d: %u new voxels", dx, dy, dz, new_count(dx, dy, dz));
                CHECK((kept | nm) == kAll && (kept & nm) == 0u, "shift %d %d %d: kept %07x new %07x", dx, dy, dz, kept, nm);
                // voxel by voxel: new exactly where the old position leaves the block; kept ones come from inside it
                for (int v = 0; v < 27; ++v) {
                    const int a = v / 9 + dx, b = (v / 3) % 3 + dy, c = v % 3 + dz;
                    const bool in = a >= 0 && a <= 2 && b >= 0 && b <= 2 && c >= 0 && c <= 2;
                    CHECK((((kept >> v) & 1u) != 0u) == in, "shift %d %d %d voxel %d: kept bit", dx, dy, dz, v);
                    if (in) {
                        const uint32_t o = old_position(static_cast<uint32_t>(v), dx, dy, dz);
                        CHECK(o <= 26u && o == static_cast<uint32_t>(a * 9 + b * 3 + c), "shift %d %d %d voxel %d: old position %u",
                              dx, dy, dz, v, o);
                    }
                }
                // rank -> voxel: distinct, ascending, all new
                uint32_t seen = 0u, last = 0u;
                for (uint32_t r = 0; r < want; ++r) {
                    const uint32_t v = nth_voxel(nm, r);
                    CHECK(v <= 26u && ((nm >> v) & 1u) && !((seen >> v) & 1u) && (r == 0u || v > last),
                          "shift %d %d %d rank %u: voxel %u", dx, dy, dz, r, v);
                    seen |= 1u << (v & 31u);
                    last = v;
                }
                CHECK(seen == nm, "shift %d %d %d: ranks cover %07x of %07x", dx, dy, dz, seen, nm);
                check_dealing<4>(nm, dx, dy, dz);
                check_dealing<8>(nm, dx, dy, dz);
                check_dealing<16>(nm, dx, dy, dz);
                // the shifted occupancy mask
                if (all) {
                    for (uint32_t occ = 0u; occ <= kAll; ++occ) {
                        ++checks;
                        if (shifted_mask(occ, dx, dy, dz) != mask_by_voxel(occ, dx, dy, dz)) {
                            ++failures;
                            std::printf("FAIL shift %d %d %d mask %07x\n", dx, dy, dz, occ);
                            break;
                        }
                    }
                } else {
                    uint64_t s = 0x9E3779B97F4A7C15ull + static_cast<uint64_t>(shifts);     // splitmix64, seeded per shift
                    for (int i = 0; i < 1000000; ++i) {
                        s += 0x9E3779B97F4A7C15ull;
                        uint64_t z = s;
                        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                        z ^= z >> 31;
                        // (sparse, dense and uniform masks; the first few are the corner cases)
                        uint32_t occ = static_cast<uint32_t>(z) & kAll;
                        if (i % 3 == 1) occ &= static_cast<uint32_t>(z >> 32);
                        if (i % 3 == 2) occ |= static_cast<uint32_t>(z >> 32) & kAll;
                        if (i == 0) occ = 0u;
                        if (i == 1) occ = kAll;
                        if (i >= 2 && i < 29) occ = 1u << (i - 2);
                        ++checks;
                        if (shifted_mask(occ, dx, dy, dz) != mask_by_voxel(occ, dx, dy, dz)) {
                            ++failures;
                            std::printf("FAIL shift %d %d %d mask %07x\n", dx, dy, dz, occ);
                            break;
                        }
                    }
                }
            }
    CHECK(shifts == 26, "%d shifts", shifts);
    if (failures) {
        std::printf("row_shift_check: %ld of %ld checks FAILED\n", failures, checks);
        return 1;
    }
    std::printf("row_shift_check: OK %ld\n", checks);
    return 0;
}
