// Place recognition on the device (place.h; the rules are stated at sageicp_place_* in include/sageicp.h).
//
// The descriptor of a frame is a polar grid of R rings by S sectors around the sensor: per cell the highest return as a
// byte and the class of highest rank.  Nothing on the way to a byte is rounded differently from the host's restatement:
//   ring     r2 = x * x + y * y against the table of squared edges (no square root): the number of inner edges not above r2
//   sector   the s with f(s) and not f(s + 1), f(s) = (dir[s].x * y - dir[s].y * x >= 0), dir the host's table of cos and
//            sin: an fp32 atan2 only guesses where to start, the exact predicate steps from there and decides
//   height   1 + (int)floor(clamp((z - z_lo) / (z_hi - z_lo), 0, 1) * 254), fp64 with a true division
//   class    the label truncated toward zero; key = rank[class] << 8 | class
// and both planes are integer maxima, so any order of rows and any split over workgroups gives the same bytes.
//
//   k_place_draw     one pass over the rows: both u32 planes in LDS with integer atomicMax, the non-empty cells merged
//                    into memory with integer atomicMax (as k_occ_draw merges its bitmaps)
//   k_place_pack     the planes' low bytes: the descriptor
//   k_place_compile  the query's occupied cells as the windows the scoring pass tests (place.h, PlaceQueryCell)
//   k_place_score    one workgroup per entry at a time, a lane per shift: the entry's cells as class << 8 | height in
//                    LDS (u16: a wave's 64 shifts read 64 consecutive halfwords, 32 banks, no conflict), every occupied
//                    query cell read once per wave through the scalar cache and tested against the 64 shifted entry
//                    cells with one subtraction and one unsigned comparison.  The four waves take the query cells in
//                    turn and add their counts per shift in LDS (integer sums: any order).  Then the smallest shift of
//                    maximal agreement as the maximum of agree << 9 | (511 - shift).  The entry is held once and the
//                    sector index wrapped with one subtraction and one unsigned minimum; held twice along S the
//                    wrap goes, but a workgroup takes twice the LDS and the pass was 2 - 7 % slower at 20 x 60
//                    (profiles/r34/): that layout stays behind SAGEICP_PLACE_DOUBLED=1 for experiments.
//   k_place_select   one workgroup: top_k rounds of "the first candidate after the last one taken" under the exact
//                    ranking (cross products in u64, ties to the lower index), each round a tree of comparisons — no
//                    atomic decides an order
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "place.h"

namespace sageicp {

namespace {
constexpr int kThreads = 256;
constexpr int kSelectThreads = 1024;
constexpr uint32_t kScoreHeadWords = kPlaceMaxSectors + 2;      // per-shift sums, the entry's count, the best key
constexpr uint32_t kScoreDoubledLds = 32768;

__device__ __forceinline__ bool finite3(const Point4 &p) {
    return fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308 &&
           fabs(p.z) <= 1.7976931348623157e308;
}

__device__ __forceinline__ bool left_of(const double *dir, int s, double x, double y) {
    return dir[2 * s] * y - dir[2 * s + 1] * x >= 0.0;
}

// the sector of (x, y), or -1 when no s has f(s) and not f(s + 1) (x = y = 0 under an edge table that admits it)
__device__ __forceinline__ int place_sector(double x, double y, const double *dir, int S) {
    float a = atan2f(static_cast<float>(y), static_cast<float>(x));
    if (a < 0.0f) a += 6.2831855f;
    int s = static_cast<int>(a * (static_cast<float>(S) * 0.15915494f));
    if (!(s >= 0 && s < S)) s = 0;
    for (int it = 0; it <= S + 1; ++it) {
        if (!left_of(dir, s, x, y)) {
            s = s ? s - 1 : S - 1;
            continue;
        }
        const int s1 = s + 1 == S ? 0 : s + 1;
        if (!left_of(dir, s1, x, y)) return s;
        s = s1;
    }
    return -1;
}
}  // namespace

__global__ __launch_bounds__(kThreads) void k_place_draw(const Point4 *__restrict__ in, int n, PlaceGrid g,
                                                         uint32_t *planes, int *flags, uint32_t cells) {
    extern __shared__ uint32_t s_planes[];      // [2 * cells]: heights, then keys
    for (uint32_t w = threadIdx.x; w < 2 * cells; w += kThreads) s_planes[w] = 0;
    __syncthreads();
    const int R = g.rings, S = g.sectors;
    const double lo2 = g.edge2[0], hi2 = g.edge2[R];
    const double z_span = g.z_hi - g.z_lo;
    bool bad = false;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const Point4 p = in[i];
        if (!finite3(p)) {
            bad = true;
            continue;
        }
        if (!(p.l > -1.0 && p.l < 256.0)) continue;         // the class after truncation lies outside 0 .. 255 (or NaN)
        const int c = static_cast<int>(p.l);
        const uint32_t rk = g.rank[c];
        if (!rk) continue;
        const double r2 = p.x * p.x + p.y * p.y;
        if (r2 < lo2 || !(r2 < hi2)) continue;
        int ring = 0;
        for (int k = 1; k < R; ++k) ring += r2 >= g.edge2[k] ? 1 : 0;
        const int sec = place_sector(p.x, p.y, g.dir, S);
        if (sec < 0) continue;
        const double t = (p.z - g.z_lo) / z_span;
        const double v = t > 0.0 ? (t < 1.0 ? t : 1.0) : 0.0;
        const uint32_t h = 1u + static_cast<uint32_t>(static_cast<int>(floor(v * 254.0)));
        const uint32_t cell = static_cast<uint32_t>(ring * S + sec);
        atomicMax(&s_planes[cell], h);
        atomicMax(&s_planes[cells + cell], rk << 8 | static_cast<uint32_t>(c));
    }
    if (bad && flags) atomicOr(flags, kOccNonFinite);
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < 2 * cells; w += kThreads) {
        const uint32_t v = s_planes[w];
        if (v) atomicMax(planes + w, v);
    }
}

__global__ __launch_bounds__(kThreads) void k_place_pack(const uint32_t *planes, uint32_t bytes, uint8_t *desc) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < bytes) desc[i] = static_cast<uint8_t>(planes[i] & 0xffu);
}

__global__ __launch_bounds__(kThreads) void k_place_compile(const uint8_t *__restrict__ desc, int R, int S, uint32_t h_tol,
                                                            PlaceQueryCell *cells, uint32_t *n_query) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint32_t RS = static_cast<uint32_t>(R) * static_cast<uint32_t>(S);
    for (uint32_t i = threadIdx.x; i < RS; i += kThreads) {
        const uint32_t h = desc[i];
        if (!h) continue;
        const uint32_t c = desc[RS + i];
        const uint32_t lo = h > h_tol + 1 ? h - h_tol : 1u, hi = h + h_tol < 255u ? h + h_tol : 255u;
        const uint32_t r = i / static_cast<uint32_t>(S), s = i - r * static_cast<uint32_t>(S);
        // (the slot is whichever comes: the scoring pass only sums over the list)
        const uint32_t slot = atomicAdd(&s_n, 1u);
        cells[slot] = PlaceQueryCell{r << 16 | s, (c << 8 | lo) | (hi - lo) << 16};
    }
    __syncthreads();
    if (threadIdx.x == 0) *n_query = s_n;
}

template <bool Wrap>
__global__ __launch_bounds__(kThreads) void k_place_score(const uint8_t *__restrict__ db, uint32_t n, int R, int S,
                                                          const PlaceQueryCell *__restrict__ cells,
                                                          const uint32_t *__restrict__ n_query,
                                                          PlaceScore *__restrict__ scores) {
    extern __shared__ uint32_t s_mem[];
    uint32_t *s_agree = s_mem;                          // [S]
    uint32_t *s_word = s_mem + kPlaceMaxSectors;        // [0] the entry's occupied cells, [1] the best key
    uint16_t *s_e = reinterpret_cast<uint16_t *>(s_mem + kScoreHeadWords);      // [R][stride]
    const uint32_t uS = static_cast<uint32_t>(S), RS = static_cast<uint32_t>(R) * uS;
    const uint32_t stride = Wrap ? uS : 2 * uS;
    const uint32_t nq = *n_query;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
        const uint8_t *d = db + static_cast<size_t>(e) * 2 * RS;
        for (uint32_t k = threadIdx.x; k < uS; k += kThreads) s_agree[k] = 0;
        if (threadIdx.x == 0) s_word[0] = s_word[1] = 0;
        __syncthreads();                                // (the last entry's reads of s_e and s_word are done)
        uint32_t occupied = 0;
        for (uint32_t i = threadIdx.x; i < RS; i += kThreads) {
            const uint32_t h = d[i], c = d[RS + i];
            const uint16_t v = static_cast<uint16_t>(c << 8 | h);
            const uint32_t r = i / uS, s = i - r * uS;
            s_e[r * stride + s] = v;
            if (!Wrap) s_e[r * stride + uS + s] = v;
            occupied += h ? 1u : 0u;
        }
        if (occupied) atomicAdd(&s_word[0], occupied);
        __syncthreads();
        for (uint32_t k0 = 0; k0 < uS; k0 += 64) {
            const uint32_t k = k0 + lane;
            const uint32_t kk = k < uS ? k : 0u;
            uint32_t acc = 0;
#pragma unroll 4
            for (uint32_t i = wave; i < nq; i += kThreads / 64) {
                const PlaceQueryCell q = cells[i];      // the same for the whole wave
                const uint32_t r = q.at >> 16, s = q.at & 0xffffu;
                uint32_t j = s + kk;
                if (Wrap) j = min(j, j - uS);
                const uint32_t v = s_e[r * stride + j];
                acc += (v - (q.base_span & 0xffffu)) <= (q.base_span >> 16) ? 1u : 0u;
            }
            if (k < uS && acc) atomicAdd(&s_agree[k], acc);
        }
        __syncthreads();
        // agree <= R * S < 2^15 and shift < 2^9: the largest key is the largest agreement at its smallest shift
        for (uint32_t k = threadIdx.x; k < uS; k += kThreads) atomicMax(&s_word[1], s_agree[k] << 9 | (511u - k));
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t key = s_word[1];
            scores[e] = PlaceScore{key >> 9, 511u - (key & 511u), s_word[0], 0u};
        }
    }
}

namespace {
struct Cand {
    unsigned long long a, m;
    uint32_t idx;               // 0xFFFFFFFF: none
};
__device__ __forceinline__ Cand cand_of(const PlaceScore &sc, uint32_t nq, uint32_t idx) {
    const uint32_t m = nq > sc.n_entry ? nq : sc.n_entry;
    return Cand{m ? sc.agree : 0u, m ? m : 1u, idx};
}
// x comes before y in the ranking
__device__ __forceinline__ bool before(const Cand &x, const Cand &y) {
    const unsigned long long l = x.a * y.m, r = y.a * x.m;
    return l > r || (l == r && x.idx < y.idx);
}
__device__ __forceinline__ Cand better(const Cand &x, const Cand &y) {
    const bool take_x = y.idx == 0xFFFFFFFFu || (x.idx != 0xFFFFFFFFu && before(x, y));
    return Cand{take_x ? x.a : y.a, take_x ? x.m : y.m, take_x ? x.idx : y.idx};      // (field by field: registers)
}
}  // namespace

__global__ __launch_bounds__(kSelectThreads) void k_place_select(const PlaceScore *__restrict__ scores, uint32_t n,
                                                                 const uint32_t *__restrict__ n_query, uint32_t top_k,
                                                                 PlaceTop *top) {
    __shared__ unsigned long long s_a[kSelectThreads], s_m[kSelectThreads];
    __shared__ uint32_t s_i[kSelectThreads];
    const uint32_t nq = *n_query;
    const uint32_t rounds = top_k < n ? top_k : n;
    Cand last{0, 1, 0xFFFFFFFFu};
    for (uint32_t t = 0; t < rounds; ++t) {
        Cand best{0, 1, 0xFFFFFFFFu};
        for (uint32_t i = threadIdx.x; i < n; i += kSelectThreads) {
            const Cand c = cand_of(scores[i], nq, i);
            if (t && !before(last, c)) continue;        // taken in an earlier round
            best = better(best, c);
        }
        s_a[threadIdx.x] = best.a;
        s_m[threadIdx.x] = best.m;
        s_i[threadIdx.x] = best.idx;
        __syncthreads();
        for (uint32_t off = kSelectThreads / 2; off; off >>= 1) {
            if (threadIdx.x < off) {
                const Cand x{s_a[threadIdx.x], s_m[threadIdx.x], s_i[threadIdx.x]};
                const Cand y{s_a[threadIdx.x + off], s_m[threadIdx.x + off], s_i[threadIdx.x + off]};
                const Cand b = better(x, y);
                s_a[threadIdx.x] = b.a;
                s_m[threadIdx.x] = b.m;
                s_i[threadIdx.x] = b.idx;
            }
            __syncthreads();
        }
        last = Cand{s_a[0], s_m[0], s_i[0]};
        __syncthreads();                                // (everyone has read the winner before the next round writes)
        if (threadIdx.x == 0) {
            const PlaceScore sc = scores[last.idx];
            top->rec[t] = PlaceTop::Rec{last.idx, sc.agree, sc.shift, sc.n_entry};
        }
    }
    if (threadIdx.x == 0) {
        top->n_query = nq;
        top->count = rounds;
    }
}

void launch_place_draw(const Point4 *in, int n, const PlaceGrid &g, uint32_t *planes, int *flags, hipStream_t s) {
    if (n <= 0) return;
    const uint32_t cells = static_cast<uint32_t>(g.rings) * static_cast<uint32_t>(g.sectors);
    // a workgroup zeroes and merges its private planes once: it takes at least as many rows as it has cells
    const unsigned per = std::max<unsigned>(4 * kThreads, cells);
    const unsigned blocks = std::min<unsigned>((static_cast<unsigned>(n) + per - 1) / per, 512u);
    const size_t lds = 2ull * cells * sizeof(uint32_t);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(k_place_draw), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(2ull * kPlaceMaxCells * sizeof(uint32_t))) != hipSuccess)
        return;                                         // (the caller reads hipGetLastError)
    hipLaunchKernelGGL(k_place_draw, dim3(blocks), dim3(kThreads), lds, s, in, n, g, planes, flags, cells);
}

void launch_place_pack(const uint32_t *planes, uint32_t cells, uint8_t *desc, hipStream_t s) {
    const uint32_t bytes = 2 * cells;
    hipLaunchKernelGGL(k_place_pack, dim3((bytes + kThreads - 1) / kThreads), dim3(kThreads), 0, s, planes, bytes, desc);
}

void launch_place_compile(const uint8_t *desc, int rings, int sectors, uint32_t h_tol, PlaceQueryCell *cells,
                          uint32_t *n_query, hipStream_t s) {
    hipLaunchKernelGGL(k_place_compile, dim3(1), dim3(kThreads), 0, s, desc, rings, sectors, h_tol, cells, n_query);
}

bool place_score_doubled_fits(int rings, int sectors) {
    return kScoreHeadWords * 4 + 4ull * static_cast<uint32_t>(rings) * static_cast<uint32_t>(sectors) <= kScoreDoubledLds;
}

void launch_place_score(const uint8_t *db, uint32_t n, int rings, int sectors, const PlaceQueryCell *cells,
                        const uint32_t *n_query, PlaceScore *scores, bool wrap, hipStream_t s) {
    if (!n) return;
    const uint32_t cells_n = static_cast<uint32_t>(rings) * static_cast<uint32_t>(sectors);
    const unsigned blocks = std::min<uint32_t>(n, 2048u);
    if (wrap || !place_score_doubled_fits(rings, sectors))
        hipLaunchKernelGGL(k_place_score<true>, dim3(blocks), dim3(kThreads), kScoreHeadWords * 4 + 2ull * cells_n, s, db, n,
                           rings, sectors, cells, n_query, scores);
    else
        hipLaunchKernelGGL(k_place_score<false>, dim3(blocks), dim3(kThreads), kScoreHeadWords * 4 + 4ull * cells_n, s, db, n,
                           rings, sectors, cells, n_query, scores);
}

void launch_place_select(const PlaceScore *scores, uint32_t n, const uint32_t *n_query, uint32_t top_k, PlaceTop *top,
                         hipStream_t s) {
    hipLaunchKernelGGL(k_place_select, dim3(1), dim3(kSelectThreads), 0, s, scores, n, n_query, top_k, top);
}

}  // namespace sageicp
