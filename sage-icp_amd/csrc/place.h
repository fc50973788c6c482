// Place recognition (include/sageicp.h, sageicp_place_*): the semantic scan context of a frame and the brute-force
// matcher of a database of them (place.hip).  A descriptor is 2 * R * S bytes — the height plane [R][S], then the class
// plane [R][S] — and everything that decides a byte or a rank is an integer or a plain fp64 comparison against the two
// host-made tables (ring edges squared, sector directions), so the bytes are the same on every run and for every split
// of the rows over workgroups.  The host side is capi_place.hip.  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "sageicp_types.h"

namespace sageicp {

// two u32 planes of R * S cells are drawn in one workgroup's LDS (128 KiB of a CU's 160 KiB)
constexpr uint32_t kPlaceMaxCells = 16384;
constexpr int kPlaceMaxRings = 64, kPlaceMinSectors = 3, kPlaceMaxSectors = 360;
constexpr uint32_t kPlaceMaxTop = 16;
constexpr uint64_t kPlaceMaxEntries = 1ull << 20;

// what the kernels read of a parameter set: the tables live in device memory
struct PlaceGrid {
    double z_lo, z_hi;
    int rings, sectors;
    const double *edge2;        // [R + 1]
    const double *dir;          // [S][2]: cos, sin
    const uint8_t *rank;        // [256]
};

// an occupied cell of the query as the matcher reads it: where it is, and the window of entry cells that agree with it
//   at = r << 16 | s;  base = class << 8 | max(1, h - h_tol);  span = min(255, h + h_tol) - max(1, h - h_tol)
// an entry cell v = class << 8 | h agrees exactly when (uint32_t)(v - base) <= span
struct PlaceQueryCell {
    uint32_t at;
    uint32_t base_span;         // base | span << 16
};

// per considered entry, what the scoring pass leaves
struct PlaceScore {
    uint32_t agree, shift, n_entry, reserved;
};

// the records of a match as they are downloaded, once
struct PlaceTop {
    uint32_t n_query, count, reserved[2];
    struct Rec {
        uint32_t index, agree, shift, n_entry;
    } rec[kPlaceMaxTop];
};

// Two zeroed u32 planes [2][R * S] (heights, then semantic keys rank << 8 | class) take the integer maxima of n rows; a
// coordinate that is not finite raises kOccNonFinite (kernels.h) in *flags (if not null) and draws nothing.
void launch_place_draw(const Point4 *in, int n, const PlaceGrid &g, uint32_t *planes, int *flags, hipStream_t s);
// the planes' low bytes: 2 * R * S bytes
void launch_place_pack(const uint32_t *planes, uint32_t cells, uint8_t *desc, hipStream_t s);
// The query's occupied cells (at most R * S of them, in no particular order: only sums are formed over them) and their
// count into *n_query, which must be zeroed first.
void launch_place_compile(const uint8_t *desc, int rings, int sectors, uint32_t h_tol, PlaceQueryCell *cells,
                          uint32_t *n_query, hipStream_t s);
// entries [0, n) of `db` ([n][2][R][S] bytes) scored under all S shifts against the compiled query.  wrap (the default,
// the faster of the two on MI355X: profiles/r34): the entry is held once in LDS and the sector index wrapped; otherwise
// it is held twice along S where that fits (SAGEICP_PLACE_DOUBLED=1, for experiments).
void launch_place_score(const uint8_t *db, uint32_t n, int rings, int sectors, const PlaceQueryCell *cells,
                        const uint32_t *n_query, PlaceScore *scores, bool wrap, hipStream_t s);
// whether the doubled layout fits a workgroup's LDS for this shape
bool place_score_doubled_fits(int rings, int sectors);
// one workgroup: the first top_k of n scores under the exact ranking, into *top
void launch_place_select(const PlaceScore *scores, uint32_t n, const uint32_t *n_query, uint32_t top_k, PlaceTop *top,
                         hipStream_t s);

}  // namespace sageicp
