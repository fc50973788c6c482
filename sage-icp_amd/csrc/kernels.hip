// Hand-written HIP kernels for gfx950 (CDNA4, wave64) — SAGE-ICP registration hot path.
// One ICP iteration = k_icp -> k_fin, both on one stream, no host round trip.
//
// One translation unit in five files.  This one holds the lane helpers, the small kernels (k_derive_cand, k_rows, k_gn,
// k_tf, the scatter kernels), the fixed-point sums, what the search body and the one-launch loop share (LoopGroup, the
// LDS header words, LoopLds — the one description of a k_loop workgroup's LDS —, chain_wait_pose), k_icp and every
// launcher.  Included below, by this file only:
//   icp_body.h     the search body k_icp and k_loop share (icp_body: everything between a wave's queries and their sums)
//   fin_kernel.h   the launch-per-iteration finish: WaveLanes, the reductions, solve_and_publish, exchange_sums, k_fin
//   loop_kernel.h  the one-launch loop: the solving wave (loop_finish_iteration, k_loop_solve) and k_loop with its phases
//   probes.h       the instrumentation of the probe builds (included first; empty in the product)
//
//   k_icp    VoxelHashMap::GetCorrespondences (core/VoxelHashMap.cpp:48-130) and the accumulation
//            of AlignClouds (core/Registration.cpp:59-90) in ONE launch.  W = 1..16 lanes own a
//            query (few lanes for frames that fill the chip: fewest instructions per query; many
//            for small frames / shards: shortest dependent chain).  Per query: apply the
//            cumulative pose to the pristine frame point (TransformPoints, Registration.cpp:
//            103-111,133 — `source` is never rewritten in place); home voxel by the reference's
//            exact fp64 divide + truncation (VoxelHashMap.cpp:52-54); the query's cached
//            neighbourhood row (27 x map_.find, VoxelHashMap.cpp:66-78, redone only when the home
//            voxel changed) staged in LDS; scan of the home voxel, then ONLY of the neighbour
//            voxels whose cell can still hold a better point (exact lower bound, see below);
//            lexicographic (distance, enumeration order) argmin = the reference's sequential
//            strict-< scan, index for index.  Fused epilogue: acceptance test on the unscaled
//            distance (VoxelHashMap.cpp:111), robust weight and the 16 closed-form fp64 sums of
//            JtJ / Jtr per accepted pair, added as exact fixed-point digits into shared accumulators (below).
//   k_rows   builds every query's neighbourhood row after a (re-)sort of the frame (27 lanes probe
//            the GPU-resident open-addressed hash per query).
//   k_fin    one workgroup: exact sum of the accumulators' copies (integers: bit-reproducible; the
//            fixed-order reduction of fp64 partials remains for k_gn's), [exchange of the sums
//            with the peer GPUs,] 6x6 LDL^T solve and SE3 exp with their divisions /
//            sincos spread over lanes, pose composition and the convergence test
//            (Registration.cpp:92-93,135-137).
//   k_gn     the accumulation alone on explicit pairs (the stand-alone AlignClouds entry).
//   k_tf     TransformPoints for the stand-alone API entry (Registration.cpp:103-111).
//   k_scatter_points / k_scatter_slots   refresh of the HBM mirror of the host map.
//
// Pruning (exact).  A point stored in voxel v lies in v's cell — it was inserted by the same fp64
// divide + truncation (VoxelHashMap.cpp:165) — so its squared distance to the query is at least
// the squared distance from the query to the cell, and its semantically scaled distance
// (VoxelHashMap.cpp:87-88: d2 * th for matching labels, d2 otherwise) at least min(th, 1) times
// that.  If this lower bound — taken with a relative slack of 1e-9 and an absolute slack on
// every face, both far above fp64 rounding — is strictly above the scaled distance the query
// already holds after its home voxel, no point of v can win or tie, and v is skipped.  On the
// synthetic street scenes 75-85 % of the (query, map point) pairs the reference evaluates are
// never loaded.
//
// Compact candidates (exact).  What the kernel is made of is bytes through the eight L2s, so the
// scan does not read the 32-B fp64 records: k_derive_cand keeps a 16-B copy of every map point
// (fp32 x, y, z, label) and the scan evaluates THAT — fp32 distance, label class — against a
// threshold that no point able to win or tie can exceed (the fp32 error is bounded per query; see
// `set_thresholds`, icp_body.h).  Only a candidate under the threshold is fetched as fp64 and goes through
// the reference's comparison.  With the previous answer as seed almost nothing passes, so a
// scanned point costs 16 bytes and ~11 fp32 instructions instead of 32 bytes and 22 fp64 ones,
// and the decision — every comparison that can change the result is the fp64 one — is the
// sequential scan's, index for index.
//
// Roofline: cache-gather bound integer/byte + fp64 compare work (~0.1 flop/B) — no MFMA (a 6x6
// outer product sum is not a dense contraction).  What matters here: one 32-B record per lane
// and step through a raw buffer resource (no address arithmetic), rows staged once in LDS with a
// conflict-free stride, a branch-light per-lane state machine with the next point's load in
// flight while the current one is evaluated, no device-scope atomics, and load balance by
// hardware dispatch of many small workgroups in XCD-aware stripes of the spatially sorted frame.
//
// Built with -ffp-contract=off: distances are the plain IEEE sequence
// SAGE_SQNORM3_*(dx*dx, dy*dy, dz*dz) (sageicp_types.h) the CPU evaluates, so the argmin is
// index-exact against the oracle.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <type_traits>
#include <vector>

#ifndef SAGE_ICP_STRIPE
#define SAGE_ICP_STRIPE 8      // workgroups of the sorted frame per XCD stripe
#endif
#ifndef SAGE_ICP_OCC
#define SAGE_ICP_OCC 6         // waves per SIMD k_icp's register allocation must allow at least (<= 80 registers); the
                               // variants that matter sit at 72 and run 7 (tools/resource_usage.sh)
#endif

#include "kernels.h"
#include "se3_math.h"
#include "sageicp_types.h"
#include "probes.h"

namespace sageicp {


// ---------------------------------------------------------------------------- cross-lane helpers
// DPP moves run on the VALU (no LDS traffic, no scalar instructions); the patterns used are
// involutions (quad swaps, half-row and row mirrors), so each step is an exchange and every lane
// of a segment ends with the segment's result.  (bound_ctrl with no `old` operand: a lane without a
// source — only the row shifts of the block sums have such lanes, and nobody reads them — gets zero, and
// the move is ONE instruction per dword; with old = the value itself the compiler first copied the value
// into the destination: 4 instructions per fp64 exchange instead of 2, 64 of them in every pass's sums.)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
constexpr int kDppXor1 = 0xB1;          // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;          // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;   // lane i <-> 7 - i   within each 8
constexpr int kDppMirror = 0x140;       // lane i <-> 15 - i  within each 16

// v_min_f64 without the quieting v_max_f64 x, x pairs the compiler puts around fmin(): one
// operand (the running best) is never NaN, and a NaN candidate leaves it unchanged.
__device__ __forceinline__ double min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// min(v, v of the partner lane) in one VOP2-DPP instruction.  The s_nop covers the two wait
// states a DPP read needs after a VALU write of the same register (the compiler's hazard
// recogniser does not look into inline assembly).
#define SAGE_MIN_U32_DPP(name, ctrl)                                                          \
    __device__ __forceinline__ unsigned name(unsigned v) {                                    \
        unsigned r;                                                                           \
        asm("s_nop 1\n\tv_min_u32_dpp %0, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf"         \
            : "=v"(r)                                                                         \
            : "v"(v));                                                                        \
        return r;                                                                             \
    }
SAGE_MIN_U32_DPP(min_u32_xor1, "quad_perm:[1,0,3,2]")
SAGE_MIN_U32_DPP(min_u32_xor2, "quad_perm:[2,3,0,1]")
SAGE_MIN_U32_DPP(min_u32_half_mirror, "row_half_mirror")
SAGE_MIN_U32_DPP(min_u32_mirror, "row_mirror")
#undef SAGE_MIN_U32_DPP

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v) {
    return static_cast<unsigned>(
        __builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xF, 0xF, true));
}
template <int W>
__device__ __forceinline__ unsigned seg_or_u32(unsigned m) {   // over segments of W <= 16 lanes
    if (W >= 2) m |= dpp_u32<kDppXor1>(m);
    if (W >= 4) m |= dpp_u32<kDppXor2>(m);
    if (W >= 8) m |= dpp_u32<kDppHalfMirror>(m);
    if (W >= 16) m |= dpp_u32<kDppMirror>(m);
    return m;
}
template <int W>
__device__ __forceinline__ unsigned seg_add_u32(unsigned m) {
    if (W >= 2) m += dpp_u32<kDppXor1>(m);
    if (W >= 4) m += dpp_u32<kDppXor2>(m);
    if (W >= 8) m += dpp_u32<kDppHalfMirror>(m);
    if (W >= 16) m += dpp_u32<kDppMirror>(m);
    return m;
}
template <int W>
__device__ __forceinline__ double seg_min_f64(double m) {      // over segments of W <= 16 lanes
    if (W >= 2) m = min_f64(m, dpp_f64<kDppXor1>(m));
    if (W >= 4) m = min_f64(m, dpp_f64<kDppXor2>(m));
    if (W >= 8) m = min_f64(m, dpp_f64<kDppHalfMirror>(m));
    if (W >= 16) m = min_f64(m, dpp_f64<kDppMirror>(m));
    return m;
}
template <int W>
__device__ __forceinline__ unsigned seg_min_u32(unsigned m) {
    if (W >= 2) m = min_u32_xor1(m);
    if (W >= 4) m = min_u32_xor2(m);
    if (W >= 8) m = min_u32_half_mirror(m);
    if (W >= 16) m = min_u32_mirror(m);
    return m;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// (what the workgroups of a launch share with each other and with the solving wave: agent-scope atomics only —
// the eight L2s are not coherent with each other)
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


// One map point through the buffer path: `off` is the point's byte offset, the resource carries the
// 64-bit base, so a load costs no 64-bit address arithmetic.  (The point array stays under 4 GiB:
// 2^24 storage units of 128 B, capi.hip.)
__device__ __forceinline__ Point4 load_point(__amdgpu_buffer_rsrc_t pts, uint32_t off) {
    const v4u a = __builtin_amdgcn_raw_buffer_load_b128(pts, off, 0, 0);
    const v4u b = __builtin_amdgcn_raw_buffer_load_b128(pts, off + 16u, 0, 0);
    Point4 q;
    q.x = __hiloint2double(static_cast<int>(a.y), static_cast<int>(a.x));
    q.y = __hiloint2double(static_cast<int>(a.w), static_cast<int>(a.z));
    q.z = __hiloint2double(static_cast<int>(b.y), static_cast<int>(b.x));
    q.l = __hiloint2double(static_cast<int>(b.w), static_cast<int>(b.z));
    return q;
}

// One compact candidate record (16 B): fp32 x, y, z, label.  `off` is its byte offset; `imm` (a constant) travels in the
// instruction's scalar offset: a second record at a fixed distance from the first costs no address arithmetic.
__device__ __forceinline__ uint4 load_cand(__amdgpu_buffer_rsrc_t cands, uint32_t off, int imm = 0) {
    const v4u a = __builtin_amdgcn_raw_buffer_load_b128(cands, off, imm, 0);
    return make_uint4(a.x, a.y, a.z, a.w);
}

// ------------------------------------------------------------------------------- k_derive_cand
// The compact copy of the map: one thread per hash slot converts the points of its voxel.  A label
// that is not an integer of magnitude < 2^24 cannot be classified in fp32: it is stored as a NaN
// and raises bit 0 of *flags, which makes k_icp use the looser of its two thresholds everywhere.
__global__ __launch_bounds__(256) void k_derive_cand(const Slot *table, uint32_t nslots, const Point4 *pts,
                                                     uint4 *cand, uint64_t nslots_pts, uint32_t *flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nslots) return;
    const uint32_t w = table[i].blk;
    if (w == kEmptySlot || w == kTombstone) return;
    const uint32_t cnt = w & 255u;
    const uint64_t first = static_cast<uint64_t>(w >> 8) * kUnitPoints;      // the voxel's region
    bool inexact = false;
    for (uint32_t j = 0; j < cnt && first + j < nslots_pts; ++j) {
        const Point4 q = pts[first + j];
        float lf = static_cast<float>(q.l);
        if (!(static_cast<double>(lf) == q.l && q.l == trunc(q.l) && fabs(q.l) < 16777216.0)) {
            lf = __uint_as_float(0x7FC00000u);
            inexact = true;
        }
        cand[first + j] = make_uint4(__float_as_uint(static_cast<float>(q.x)), __float_as_uint(static_cast<float>(q.y)),
                                     __float_as_uint(static_cast<float>(q.z)), __float_as_uint(lf));
    }
    if (inexact) atomicOr(flags, 1u);
}
void launch_derive_cand(const Slot *table, uint32_t nslots, const Point4 *pts, uint4 *cand, uint64_t nslots_pts,
                        uint32_t *flags, hipStream_t s) {
    if (nslots) hipLaunchKernelGGL(k_derive_cand, dim3((nslots + 255u) / 256u), dim3(256), 0, s, table, nslots,
                                   pts, cand, nslots_pts, flags);
}

// --------------------------------------------------------------------------------- hash probing
// The GPU-resident open-addressed hash: linear probing, 16-B slots, load factor <= 0.25, one 16-B
// load per step.  Returns the slot's packed word (first unit of the voxel's points << 8) | count —
// what a neighbourhood row keeps of a found voxel — or kEmptySlot.
__device__ __forceinline__ uint32_t probe_resolve(const Slot *table, uint32_t mask, uint32_t sl,
                                                  int4 e, int vx, int vy, int vz) {
    for (;;) {
        if (static_cast<uint32_t>(e.w) == kEmptySlot) return kEmptySlot;
        if (e.x == vx && e.y == vy && e.z == vz) return static_cast<uint32_t>(e.w);
        sl = (sl + 1u) & mask;                    // tombstones (map_update.hip) never match
        e = reinterpret_cast<const int4 *>(table)[sl];
    }
}
__device__ __forceinline__ uint32_t probe_voxel(const Slot *table, uint32_t mask, int vx, int vy,
                                                int vz) {
    const uint32_t sl = voxel_hash(vx, vy, vz) & mask;
    const int4 e = reinterpret_cast<const int4 *>(table)[sl];
    return probe_resolve(table, mask, sl, e, vx, vy, vz);
}

// The query as searched: cumulative pose applied to the pristine frame point
// (Registration.cpp:103-111), home voxel by exact fp64 divide + truncation toward zero
// (VoxelHashMap.cpp:52-54).
struct Query {
    double x, y, z, l;
    int kx, ky, kz;
};
// QUAD: the lanes of a query come in aligned groups of four (k_icp with 4+ lanes per query) that
// all hold the same point: lane a < 3 of a quad then divides axis a only (an fp64 divide is ~15
// instructions) and the three voxel indices are handed round by quad broadcasts — the same
// divisions, a third of them per lane.
// The voxel index is trunc(fl(x / voxel_size)) — the reference's fp64 divide, to the bit.  An fp64 division is ~35
// instructions; x * fl(1 / voxel_size) is one, and differs from the quotient by a few ulps at most: wherever it lies
// farther than 1e-9 (1 + |q|) from an integer its truncation IS the quotient's, and only a wave that holds a lane
// closer than that to a cell face (one pass in thousands) pays for the division (`inv_vs` = 0: always divide).
__device__ __forceinline__ int voxel_index(double x, double voxel_size, double inv_vs) {
    const double q = x * inv_vs;
    const bool unsure = !(fabs(q - __builtin_rint(q)) > 1e-9 * (1.0 + fabs(q))) || inv_vs == 0.0;
    int k = static_cast<int>(q);
    if (__ballot(unsure)) {
        asm volatile("" ::: "memory");         // (keeps this a branch: if-converted, the division ran in every pass)
        k = static_cast<int>(x / voxel_size);
    }
    return k;
}
// (`quad_lane`, QUAD only: the caller's lane index — k_loop derives it anew in every pass, icp_body)
template <bool QUAD = false>
__device__ __forceinline__ Query make_query(const Point4 &f, const double *R, const double *t, int apply_pose,
                                            double voxel_size, double inv_vs = 0.0, unsigned quad_lane = 0u) {
    Query q;
    q.x = f.x; q.y = f.y; q.z = f.z; q.l = f.l;
    if (apply_pose) {
        q.x = R[0] * f.x + R[1] * f.y + R[2] * f.z + t[0];
        q.y = R[3] * f.x + R[4] * f.y + R[5] * f.z + t[1];
        q.z = R[6] * f.x + R[7] * f.y + R[8] * f.z + t[2];
    }
    if constexpr (QUAD) {
        const unsigned a = quad_lane & 3u;
        const double num = a == 0u ? q.x : (a == 1u ? q.y : q.z);
        const unsigned k = static_cast<unsigned>(voxel_index(num, voxel_size, inv_vs));
        q.kx = static_cast<int>(dpp_u32<0x00>(k));       // quad_perm [0,0,0,0]
        q.ky = static_cast<int>(dpp_u32<0x55>(k));       // quad_perm [1,1,1,1]
        q.kz = static_cast<int>(dpp_u32<0xAA>(k));       // quad_perm [2,2,2,2]
    } else {
        q.kx = voxel_index(q.x, voxel_size, inv_vs);
        q.ky = voxel_index(q.y, voxel_size, inv_vs);
        q.kz = voxel_index(q.z, voxel_size, inv_vs);
    }
    return q;
}

// ------------------------------------------------------------------------------------ k_rows
// Builds the neighbourhood row of every query: 32 lanes per query, lane v < 27 probes voxel v.
__global__ __launch_bounds__(256) void k_rows(IcpParams P) {
    const int lane = static_cast<int>(threadIdx.x & 63u);
    const unsigned v = threadIdx.x & 31u;
    const unsigned q = blockIdx.x * 8u + (threadIdx.x >> 5);
    const bool valid = q < static_cast<unsigned>(P.n);
    const Point4 f = P.frame[valid ? q : 0u];
    const Query s = make_query(f, P.st->R, P.st->T + 4, P.apply_pose, P.voxel_size);
    uint32_t w = kEmptySlot;
    if (valid && v < 27u)
        w = probe_voxel(P.table, P.mask, s.kx + static_cast<int>(v / 9u) - 1,
                        s.ky + static_cast<int>((v / 3u) % 3u) - 1, s.kz + static_cast<int>(v % 3u) - 1);
    const unsigned c = (w == kEmptySlot) ? 0u : (w & 255u);
    const unsigned long long b = __ballot(c != 0u);
    const unsigned occ = static_cast<unsigned>(b >> (lane & 32));
    unsigned cq = c;                          // sum over the 32 lanes of the query
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) cq += __shfl_xor(cq, d, 32);
    if (!valid) return;
    uint32_t out = w;
    if (v == kRowCq) out = cq;
    if (v == kRowKey) out = static_cast<uint32_t>(s.kx);
    if (v == kRowKey + 1) out = static_cast<uint32_t>(s.ky);
    if (v == kRowKey + 2) out = static_cast<uint32_t>(s.kz);
    if (v == kRowOcc) out = occ;
    P.rows[static_cast<size_t>(q) * kRowWords + v] = out;
}

// ------------------------------------------------------------------------------------- k_icp

// per-workgroup LDS header of k_icp (words): arrival counter | the workgroup's fixed-point accumulators
// (kWgAccWords 64-bit words)
constexpr unsigned kWgAccWords = 52;         // (16 sums + pair count) x 3 digits = 51 | [51] overflow flag
constexpr unsigned kWgArrive = 0, kWgGo = 1, kWgAcc = 2;      // kWgGo: chained launches: 0 go on, else leave
constexpr unsigned kWgPose = kWgAcc + 2u * kWgAccWords;       // chained launches: R[9], t[3] of this iteration (16-B aligned)
constexpr unsigned kWgHeaderWords = (kWgPose + 24u + 15u) & ~15u;
__host__ __device__ constexpr unsigned icp_wave_words(int lw) {
    // the rows of the wave's queries (kRowLdsStride words each); reused by the epilogue's
    // transposed reduction, 16 components x (queries + 2) fp64
    return static_cast<unsigned>(kRowLdsStride * (64 >> lw) + 64);
}

// ---- the Gauss-Newton sums as exact fixed-point numbers ---------------------------------------------
// The unit that is rounded is a BLOCK of four consecutive queries of the (sorted) frame: the 16 pair terms
// of its queries are added as (t0 + t1) + (t2 + t3) in fp64, and that block sum is split exactly into three
// signed digits of 40 bits (weights 2^0, 2^-40, 2^-80; what lies below 2^-80 is dropped).  From there on
// everything is integer addition — over the blocks of a wave (DPP), the waves and groups of a workgroup
// (LDS atomics), the workgroups (global atomics into the shared accumulators, kernels.h) — which is
// associative: the accumulated bits depend on the order of the frame and on NOTHING else.  Not on the lanes
// per query (round 4 rounded once per wave: a frame registered with 4 and with 8 lanes per query differed
// in the last bits), not on how queries are cut into waves, groups and workgroups, not on which loop ran,
// not on the order of arrival.  (Blocks never straddle waves: a wave holds 4, 8, 16, 32 or 64 queries.)
//
// to_digits: v = a + b 2^-40 + c 2^-80 exactly (three integers of at most 40 bits and a sign, each exactly
// representable), each as int64 through the 2^52 + 2^51 trick (both numbers lie in [2^52, 2^53): their
// bit patterns differ by exactly the integer).  `ok` is cleared when |a| leaves the range the accumulators
// have room for: the overflow flag (IcpState::acc_overflow) makes the host register the frame again with the sums scaled
// down (capi_run.hip, acc_shift), and report it when that is not enough.
__device__ __forceinline__ void to_digits(double v, double limit, long long &d0, long long &d1, long long &d2, bool &ok) {
    const double a = __builtin_rint(v);
    const double r1 = (v - a) * 1099511627776.0;             // 2^40, exact
    const double b = __builtin_rint(r1);
    const double c2 = __builtin_rint((r1 - b) * 1099511627776.0);
    ok &= fabs(a) < limit;
    d0 = __double_as_longlong(a + 6755399441055744.0) - 0x4338000000000000ll;
    d1 = __double_as_longlong(b + 6755399441055744.0) - 0x4338000000000000ll;
    d2 = __double_as_longlong(c2 + 6755399441055744.0) - 0x4338000000000000ll;
}
// |a| of one block stays below a limit.  k_icp + k_fin: IcpParams::digit_limit — k_fin adds the 32 copies of the
// accumulators in plain 64-bit integers, so what has to stay inside 63 bits is the sum over ALL the blocks of the
// frame: the host passes 2^62 / blocks rounded down to a power of two, at most 2^46 (capi_run.hip, icp_params; a
// frame of 500k points: 2^45 — coordinates of 3 10^6 m; ADVICE r05: a fixed 2^46 let a frame of 1M+ points at UTM
// coordinates wrap silently).  k_loop: 2^40, its words also carry a count in their low byte (coordinates of 10^5 m:
// 4 x (10^5)^2 = 4 10^10 < 2^40 = 1.1 10^12; plan_loop checks the number of blocks per copy).  The lower digits
// are below 2^39 in magnitude: 2^24 - 1 blocks at most (kMaxQueries).
constexpr double kDigitLimitCounted = 1099511627776.0;

template <int CTRL>
__device__ __forceinline__ long long dpp_i64(long long v) {
    int lo = static_cast<int>(v), hi = static_cast<int>(v >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return (static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo);
}
// lane i <- lane i + N (the lanes whose results are used — those of the first query of a block — always have
// their partner inside the wave; shifts below 16 stay inside a row of 16 lanes: DPP row_shl, no LDS traffic)
template <int N>
__device__ __forceinline__ double lane_shl_f64(double v) {
    if constexpr (N < 16) return dpp_f64<0x100 + N>(v);
    else return __shfl_down(v, N, 64);
}
// ... for k_loop: `lane` is the caller's lane index, derived inside the iteration loop — __shfl_down takes its own from a
// builtin the compiler hoists out of that loop and keeps.  (Lanes whose partner would lie beyond the wave get another
// lane's value instead of their own: their results are not used.)
template <int N>
__device__ __forceinline__ double lane_shl_f64_at(double v, int lane) {
    if constexpr (N < 16) {
        return dpp_f64<0x100 + N>(v);
    } else {
        const int a = ((lane + N) & 63) << 2;
        const int lo = __builtin_amdgcn_ds_bpermute(a, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(a, __double2hiint(v));
        return __hiloint2double(hi, lo);
    }
}

// A wave's 16 pair terms per query -> block sums -> digits -> added into the workgroup's accumulators `wgacc`
// (LDS, kWgAccWords 64-bit words).  The terms are spread over the W lanes of a query: lane ci holds components
// ci K .. ci K + K - 1 (K = 16 / W; zeros for a query without a pair).  `red` = LDS scratch of this wave, 16 fp64
// per block.
template <int LW, bool FRESH = false>
__device__ __forceinline__ void wave_terms_to_wgacc(const double (&t)[kCount >> LW], unsigned pairs, int lane, double *red,
                                                    unsigned long long *wgacc, double limit, double scale) {
    constexpr int W = 1 << LW, QW = 64 >> LW, NBLK = QW / 4, K = kCount >> LW;
    // A. block sums, (t0 + t1) + (t2 + t3), on the lanes of the first query of every block
    double y[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if constexpr (FRESH) {
            const double x = t[k] + lane_shl_f64_at<W>(t[k], lane);
            y[k] = x + lane_shl_f64_at<2 * W>(x, lane);
        } else {
            const double x = t[k] + lane_shl_f64<W>(t[k]);
            y[k] = x + lane_shl_f64<2 * W>(x);
        }
    }
    // B. four blocks at a time (512 B of scratch whatever the lanes per query): the lanes of the blocks' first
    // queries park their K sums each (component-major: the block's 16 in order), C. lane (c, j) = (lane >> 2,
    // lane & 3) converts component c of block j
    const int c = lane >> 2, j = lane & 3;
    long long d0 = 0, d1 = 0, d2 = 0;
    bool ok = true;
    const int blk = lane / (4 * W);
    const bool first = (lane & (4 * W - 1)) < W;
#pragma unroll
    for (int r = 0; r < NBLK; r += 4) {
        if (first && blk >= r && blk < r + 4) {
            double *dst = red + (blk - r) * kCount + (lane & (W - 1)) * K;
#pragma unroll
            for (int k = 0; k < K; ++k) dst[k] = y[k];
        }
        // (values pass from lane to lane through LDS here: the hardware serves a wave's LDS instructions in
        // order, but the COMPILER has to be told that the loads below see other lanes' stores)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const double v = r + j < NBLK ? red[j * kCount + c] : 0.0;
        long long e0, e1, e2;
        to_digits(v * scale, limit, e0, e1, e2, ok);       // (scale: a power of two, 1 normally)
        d0 += e0; d1 += e1; d2 += e2;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    // D. every lane adds its digits into the workgroup's accumulators (integers: any order; three
    // fire-and-forget LDS atomics — reducing the four lanes of a component first costs 24 more instructions)
    (void)__hip_atomic_fetch_add(wgacc + 3 * c, static_cast<unsigned long long>(d0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(wgacc + 3 * c + 1, static_cast<unsigned long long>(d1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(wgacc + 3 * c + 2, static_cast<unsigned long long>(d2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (!ok) (void)__hip_atomic_fetch_or(wgacc + kWgAccWords - 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (lane == 0)
        (void)__hip_atomic_fetch_add(wgacc + 3 * kCount, static_cast<unsigned long long>(pairs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The lane index, derived anew: what the compiler can trace to threadIdx it knows to be the same in every iteration
// of a loop inside the kernel (k_loop's, the solving wave's), and it would keep every select mask and address made
// from it alive across that loop — in registers the pass needs, or in scratch.
__device__ __forceinline__ int lane_now() {
    unsigned l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return static_cast<int>(l);
}
// A wave-uniform value of the set-up (k_loop: its wave, its units, its workgroup's index) as the iteration loop uses
// it: the value stays in its scalar register, what is derived from it is derived where it is used — behind this the
// compiler cannot see that it is the same in every iteration.
__device__ __forceinline__ unsigned opaque_s(unsigned x) {
    asm volatile("" : "+s"(x));
    return x;
}

// ... and an LDS index behind which a word is read AGAIN instead of being carried in a register from its first read
// (an index, not a pointer or a volatile access: either would lose the LDS address space and read through flat memory)
__device__ __forceinline__ unsigned opaque_v(unsigned x) {
    asm volatile("" : "+v"(x));
    return x;
}

// The workgroup's accumulators (LDS) -> the shared ones: lane l sends word l (digit l % 3 of value l / 3) as ONE
// fire-and-forget 64-bit integer atomic into the copy `dst`, and clears the word for the next iteration.
// COUNTED (k_loop): every word also counts its contributions — a workgroup adds (digit << 8) + 1, the low
// byte of a word says how many workgroups are in it — so that whoever reads the accumulators inside the
// launch knows, word by word, when they are complete, and the workgroup neither waits for its atomics to
// be acknowledged nor keeps a separate arrival counter.  (The form that did both — s_waitcnt vmcnt(0), then
// one of eight counters — ran an iteration in the same time, profiles/r04/loop_times_counted_words.txt against
// loop_times_xcd_stripes_rowshift.txt: this one is kept for having one protocol less and no ordering
// assumption at all.)
// FRESH (k_loop, inside its iteration loop): the lane index is derived here (lane_now) and the zero that clears the
// words is made here — neither lives across the loop.
template <bool COUNTED = false, bool FRESH = false>
__device__ __forceinline__ void wgacc_flush(unsigned long long *wgacc, long long *dst, long long *overflow) {
    const int lane = FRESH ? lane_now() : static_cast<int>(threadIdx.x & 63u);
    const int l = min(lane, static_cast<int>(kWgAccWords) - 1);
    const long long x = static_cast<long long>(wgacc[l]);
    const bool ok = wgacc[kWgAccWords - 1] == 0ull;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    unsigned long long zero = 0ull;
    if constexpr (FRESH) {
        unsigned zl, zh;
        asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0" : "=v"(zl), "=v"(zh));
        zero = (static_cast<unsigned long long>(zh) << 32) | zl;
    }
    if (lane < static_cast<int>(kWgAccWords)) wgacc[lane] = zero;
    if constexpr (COUNTED) {
        // (the overflow travels IN the counted words: word 3 kAccValues of the copy counts its workgroups like the
        // others and carries, as its "digit", how many of them overflowed — whoever finds the counts complete has
        // the flags of exactly those workgroups; a flag at another address could land after the counts)
        (void)overflow;
        if (lane <= 3 * kAccValues)
            (void)__hip_atomic_fetch_add(dst + lane, lane == 3 * kAccValues ? (ok ? 1ll : 257ll) : (ok ? x * 256 + 1 : 1ll),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (lane < 3 * kAccValues) {
        {
            if (ok) (void)__hip_atomic_fetch_add(dst + lane, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else (void)__hip_atomic_fetch_or(overflow, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- k_loop (the whole ICP loop in one launch, below) shares the body --------------------------
// A GROUP = the 64 >> LW consecutive queries one wave of k_icp would hold.  A workgroup of k_loop owns
// a few groups for the whole call and keeps per query, in LDS: the neighbourhood row (kRowLdsStride
// words) and a state record of kLoopStateWords words —
//   [0..7]   f   the pristine frame point (fp64 x, y, z, label)
//   [8..15]  pp  the previous answer's fp64 record (the seed of the next search and, while the
//                answer stays, the target of the pair: no load)
//   [16,17]  the previous answer {key = (voxel << 8) | slot, byte offset of its record}
//   [18..21] the home voxel the row was built for | the row's occupancy mask
// One copy per QUERY (its lanes read the same address: a broadcast), where the first k_loop kept a
// copy per LANE in 22 registers: the search now compiles at k_icp's budget (7 waves per SIMD) and a
// wave is no longer tied to one group — the waves of a workgroup take its groups from an LDS counter.
struct LoopGroup {
    uint32_t *rows;            // LDS: the rows of ALL the workgroup's queries, [slot][kRowLdsStride]
    uint32_t *state;           // LDS: ... and their state records, [slot][kLoopStateWords]
    const uint32_t *perm;      // LDS: the workgroup's blocks of four queries in the order of this iteration (heaviest first)
    uint32_t *work;            // LDS: per block, the most points one of its queries was handed this iteration
    unsigned unit;             // which (64 >> LW) / 4 blocks of `perm` this pass takes
    double *red;               // LDS: the running wave's scratch for the epilogue's transposed block sums
    unsigned long long *wgacc; // LDS: the workgroup's fixed-point accumulators (wave_terms_to_wgacc)
    unsigned q_first;          // the workgroup's first query (slot 0; a multiple of four)
    unsigned slot;             // this pass's slot in the per-wave counters (IcpParams::counters)
    PROBE_LOOP_GROUP_FIELDS    // probe builds: cycles per phase of the body in this pass (probes.h); nothing in the product
};
constexpr int kLoopMaxWaves = kLoopMaxWavesHost;   // waves per workgroup of k_loop (<= 512 threads)
constexpr unsigned kLoopStripe = kLoopStripeHost;  // workgroups of k_loop per XCD stripe (its grid: a multiple of 32)
constexpr int kNoVoxel = 0x7FFFFFFF;        // a home voxel no point has (|index| < 2^20): row not built yet
constexpr unsigned kStPrev = 16, kStKey = 18;
// LDS of a k_loop workgroup (words).  Its header: arrival counter | next unit | done | the iteration the workgroup is in
// (counted by the wave that closes one; nobody holds the number in a register through a pass) | the pose of this iteration
// (R[9], t[3]) | the probe builds' counts | the waves' first units | the workgroup's fixed-point accumulators; what
// follows the header is laid out by LoopLds below.
constexpr unsigned kLpArrive = 0, kLpNext = 1, kLpDone = 2, kLpIter = 3;
constexpr unsigned kLpPose = 4;                                    // 12 doubles, 16-B aligned
constexpr unsigned kLpDbg = kLpPose + 24u;                         // probe builds: max points of a query | stale queries | points
constexpr unsigned kLpFirst = kLpDbg + 4u;                         // per wave: the unit it takes first in every iteration (LoopParams::deal)
constexpr unsigned kLpAcc = kLpFirst + 8u;                         // kWgAccWords 64-bit words
constexpr unsigned kLpHeaderWords = (kLpAcc + 2u * kWgAccWords + 15u) & ~15u;
__host__ __device__ constexpr unsigned loop_red_words() { return 2u * kCount * 4u; }    // 16 fp64 for each of four blocks of queries
__host__ __device__ constexpr unsigned loop_perm_words(unsigned nblk) { return 2u * ((nblk + 7u) & ~7u); }   // perm | work, 32-B aligned
// THE layout of that LDS, as word offsets from its start, for 2^lw lanes per query, nw waves and gpw units of
// 64 >> lw queries per workgroup:
//   header | perm[blocks] | work[blocks] | rows of the workgroup's queries | their state records | nw x scratch
// (blocks = gpw x (64 >> lw) / 4, rounded up to eight).  k_loop takes its pointers from it and the host the size it asks
// for (`end`): there is no second spelling.  (W: unsigned in the kernel; size_t on the host, where a gpw from the
// environment must not wrap.)
template <typename W>
struct LoopLds {
    W perm, work, rows, state, red, end;       // red: wave 0's scratch, wave w's at red + w loop_red_words()
    __host__ __device__ constexpr LoopLds(int lw, W nw, W gpw)
        : perm(kLpHeaderWords),
          work(perm + loop_perm_words(static_cast<unsigned>(gpw) * ((64u >> lw) / 4u)) / 2u),
          rows(perm + loop_perm_words(static_cast<unsigned>(gpw) * ((64u >> lw) / 4u))),
          state(rows + gpw * static_cast<W>(64 >> lw) * static_cast<W>(kRowLdsStride)),
          red(state + gpw * static_cast<W>(64 >> lw) * static_cast<W>(kLoopStateWords)),
          end(red + nw * loop_red_words()) {}
};

// Chained launches (IcpParams::chain): wave 0 of a workgroup of the launch of iteration `it` waits for the pose the solving
// wave publishes after iteration it - 1 (25 self-tagged granules, tag = it; kernels.h, LoopShared) and hands it to the
// workgroup through LDS.  smem[kWgGo] != 0: the workgroup leaves — the loop ended before this iteration (the done granule
// carries an older tag, or this tag with its done word set), or a wait timed out somewhere.
// Which of the kLoopPoseCopies copies of the pose workgroup b looks at (kernels.h): its XCD's by default.
__device__ __forceinline__ unsigned loop_pose_copy(int pose_map, unsigned b = blockIdx.x) {
    return pose_map == 1 ? 0u : ((pose_map == 2 ? b + 3u : b) & static_cast<unsigned>(kLoopPoseCopies - 1));
}
__device__ __forceinline__ void chain_wait_pose(const IcpParams &P, uint32_t *smem, int lane) {
    LoopShared *sh = P.chain;
    const unsigned long long tag = static_cast<unsigned long long>(P.chain_iter);
    const unsigned long long *src = lane < kLoopPoseGranules ? &sh->pose[loop_pose_copy(P.chain_pose_map)][lane] : &sh->abort_word[0];
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    unsigned go = 0u;
    unsigned long long g;
    for (;;) {
        g = ld_agent(src);
        const unsigned long long g24 = static_cast<unsigned long long>(static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(g), 24))) |
                                       (static_cast<unsigned long long>(static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(g >> 32), 24))) << 32);
        const bool ok = lane >= kLoopPoseGranules || (g >> 32) == tag;
        if (__all(ok)) {
            if (static_cast<uint32_t>(g24) != 0u) go = 1u;             // the pose after the LAST iteration: nothing left to do
            break;
        }
        if ((g24 >> 32) < tag && static_cast<uint32_t>(g24) != 0u) {   // the loop ended before this iteration
            go = 1u;
            break;
        }
        const bool late = __builtin_amdgcn_s_memrealtime() - t0 > P.chain_timeout;
        if (__any(lane == kLoopPoseGranules && g != 0ull) || late) {
            if (lane == 0 && late) {
                st_agent(&sh->abort_word[0], 1ull);
                const_cast<IcpState *>(P.st)->loop_aborted = 1;
            }
            go = 2u;
            break;
        }
        __builtin_amdgcn_s_sleep(8);
    }
    if (!go && lane < 24) smem[kWgPose + static_cast<unsigned>(lane)] = static_cast<uint32_t>(g);
    if (lane == 0) smem[kWgGo] = go;
}

}  // namespace sageicp

// icp_body, the search both k_icp and k_loop run on the queries of a wave; it calls the helpers above
#include "row_shift.h"
#include "icp_body.h"

namespace sageicp {

template <int LW, bool FUSED, bool FILT, bool FLATQ>
__global__ __launch_bounds__(64 * kIcpWavesPerBlock) __attribute__((amdgpu_waves_per_eu(SAGE_ICP_OCC, 8)))
void k_icp(IcpParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    if (P.chain) {
        // chained launches: whether the loop has ended travels with the pose (chain_wait_pose); launch 0 tells the solving
        // wave that the shared block has been zeroed and the loop starts — or that it never will (a non-finite frame point)
        if (P.chain_iter == 0) {
            const bool bad = P.st->done != 0;
            if (blockIdx.x == 0 && threadIdx.x == 0) st_agent(&P.chain->go[0], P.chain_epoch | (bad ? 0x8000000000000000ull : 0ull));
            if (bad) return;
        }
    } else if (P.check_done && P.st->done) {
        return;
    }
    icp_body<LW, FUSED, FILT, false, FLATQ>(P, smem);
    PROBE_DELAY_REPEAT(P, (icp_body<LW, FUSED, FILT, false, FLATQ>(P, smem)));
}

}  // namespace sageicp

// the launch-per-iteration finish (k_fin) and the one-launch loop (k_loop, k_loop_solve)
#include "fin_kernel.h"
#include "loop_kernel.h"

namespace sageicp {

// ------------------------------------------------------------------------------------ k_gn
// AlignClouds' accumulation (Registration.cpp:62-90) on explicit pairs: every pair is taken.
__global__ __launch_bounds__(256) void k_gn(GnParams P) {
    // block reduction scratch: component c of thread t at red[c][(t >> 4) * 17 + (t & 15)]
    // (rows of 16 values padded to 17 doubles: conflict-free for both the write and the read)
    __shared__ double red[kCount][16 * 17];
    double acc[kCount];
#pragma unroll
    for (int i = 0; i < kCount; ++i) acc[i] = 0.0;
    const double k = P.kernel;
    const double k2 = k * k;
    const int stride = gridDim.x * 256;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < P.n; q += stride) {
        const Point4 s = P.src[q], g = P.tgt[q];
        const double sx = s.x, sy = s.y, sz = s.z;
        const double rx = sx - g.x, ry = sy - g.y, rz = sz - g.z;
        const double r2 = SAGE_SQNORM3_RESID(rx * rx, ry * ry, rz * rz);
        const double den = k + r2;
        const double w = k2 / (den * den);   // square(th) / square(th + residual2)
        const double wsx = w * sx, wsy = w * sy, wsz = w * sz;
        acc[kW] += w;
        acc[kWsx] += wsx; acc[kWsy] += wsy; acc[kWsz] += wsz;
        acc[kWxx] += wsx * sx; acc[kWxy] += wsx * sy; acc[kWxz] += wsx * sz;
        acc[kWyy] += wsy * sy; acc[kWyz] += wsy * sz; acc[kWzz] += wsz * sz;
        acc[kWrx] += w * rx; acc[kWry] += w * ry; acc[kWrz] += w * rz;
        acc[kWcx] += w * (sy * rz - sz * ry);
        acc[kWcy] += w * (sz * rx - sx * rz);
        acc[kWcz] += w * (sx * ry - sy * rx);
    }
    // fixed-order block reduction: every thread parks its 16 sums in LDS, then 16 threads per
    // component each add 16 parked values and finish with four DPP exchange steps
    const int t = static_cast<int>(threadIdx.x);
    const int slot = (t >> 4) * 17 + (t & 15);
#pragma unroll
    for (int c = 0; c < kCount; ++c) red[c][slot] = acc[c];
    __syncthreads();
    const double *row = &red[t >> 4][(t & 15) * 17];
    double v = row[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) v += row[i];
    v += dpp_f64<kDppXor1>(v);
    v += dpp_f64<kDppXor2>(v);
    v += dpp_f64<kDppHalfMirror>(v);
    v += dpp_f64<kDppMirror>(v);
    double *out = P.partials + static_cast<size_t>(blockIdx.x) * kNumSums;
    if ((t & 15) == 0) out[t >> 4] = v;
    if (t == 0) {
        const int lo = blockIdx.x * 256;
        int cnt = 0;                         // pairs this block owns (grid-stride)
        for (int q = lo; q < P.n; q += stride) cnt += min(256, P.n - q);
        out[kCount] = static_cast<double>(cnt);
    }
    if (t > kCount && t < kNumSums) out[t] = 0.0;
}

// ------------------------------------------------------------------------------------ k_tf
__global__ __launch_bounds__(256) void k_tf(Point4 *pts, int n, const IcpState *st) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Point4 p = pts[i];
    const double *R = st->R;
    const double x = R[0] * p.x + R[1] * p.y + R[2] * p.z + st->T[4];
    const double y = R[3] * p.x + R[4] * p.y + R[5] * p.z + st->T[5];
    const double z = R[6] * p.x + R[7] * p.y + R[8] * p.z + st->T[6];
    p.x = x; p.y = y; p.z = z;
    pts[i] = p;
}

// ------------------------------------------------------------------------------- mirror refresh
// Scatter the records the host changed since the last sync into the HBM mirror: one staged copy
// + one kernel per array instead of thousands of small hipMemcpy calls.
__global__ __launch_bounds__(256) void k_scatter_points(const uint32_t *idx, const Point4 *vals,
                                                        uint32_t n, Point4 *pts) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) pts[idx[i]] = vals[i];
}
__global__ __launch_bounds__(256) void k_scatter_slots(const uint32_t *idx, const Slot *vals,
                                                       uint32_t n, Slot *table) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) table[idx[i]] = vals[i];
}

// sums of k_icp's per-wave counters {candidates in the neighbourhood, pairs handed out} into the
// loop state (one workgroup; it rides on the state copy the host makes anyway)
__global__ __launch_bounds__(1024) void k_sum_counters(const unsigned long long *c, int n,
                                                       IcpState *st) {
    __shared__ unsigned long long part[2][16];
    unsigned long long v = 0, w = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        v += c[2 * i];
        w += c[2 * i + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v += __shfl_down(v, off, 64);
        w += __shfl_down(w, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = v;
        part[1][threadIdx.x >> 6] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0, u = 0;
        for (int i = 0; i < 16; ++i) {
            t += part[0][i];
            u += part[1][i];
        }
        st->sum_candidates = t;
        st->sum_pairs = u;
    }
}

// ------------------------------------------------------------------------------------ launchers
void launch_sum_counters(const unsigned long long *c, int n, IcpState *st, hipStream_t s) {
    hipLaunchKernelGGL(k_sum_counters, dim3(1), dim3(1024), 0, s, c, n, st);
}
void launch_scatter_points(const uint32_t *idx, const Point4 *vals, uint32_t n, Point4 *pts,
                           hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_scatter_points, dim3((n + 255) / 256), dim3(256), 0, s, idx, vals, n, pts);
}
__global__ __launch_bounds__(256) void k_scatter_u32(const uint32_t *idx, const uint32_t *vals, uint32_t n,
                                                     uint32_t *dst) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[idx[i]] = vals[i];
}
void launch_scatter_u32(const uint32_t *idx, const uint32_t *vals, uint32_t n, uint32_t *dst, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_scatter_u32, dim3((n + 255) / 256), dim3(256), 0, s, idx, vals, n, dst);
}
void launch_scatter_slots(const uint32_t *idx, const Slot *vals, uint32_t n, Slot *table,
                          hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_scatter_slots, dim3((n + 255) / 256), dim3(256), 0, s, idx, vals, n, table);
}

int icp_stripes_for(int n, int lw) { return icp_blocks_for(n, lw) / SAGE_ICP_STRIPE; }
int icp_blocks_for(int n, int lw) {
    // one wave per 64 >> lw queries, kIcpWavesPerBlock waves per workgroup, rounded up to whole
    // stripes on all 8 XCDs
    const long qw = 64 >> lw;
    const long waves = (static_cast<long>(n) + qw - 1) / qw;
    const long blocks = (waves + kIcpWavesPerBlock - 1) / kIcpWavesPerBlock;
    const long per_round = 8L * SAGE_ICP_STRIPE;
    const long r = ((blocks + per_round - 1) / per_round) * per_round;
    return static_cast<int>(r < per_round ? per_round : r);
}
size_t icp_lds_bytes(int lw) {
    return sizeof(uint32_t) * (kWgHeaderWords + kIcpWavesPerBlock * icp_wave_words(lw));
}

void launch_rows(const IcpParams &p, hipStream_t s) {
    if (p.n <= 0) return;
    hipLaunchKernelGGL(k_rows, dim3((p.n + 7) / 8), dim3(256), 0, s, p);
}

template <int LW>
static void launch_icp_lw(const IcpParams &p, bool fused, hipStream_t s) {
    const int grid = icp_blocks_for(p.n, LW);
    const size_t lds = icp_lds_bytes(LW);
    const dim3 g(grid), b(64 * kIcpWavesPerBlock);
    // flat order: always with 8 and 16 lanes per query, never with one (it is the same thing), on request between
    constexpr bool kBoth = LW == 1 || LW == 2;
    const bool flat = LW >= 3 || (kBoth && p.flat);
    auto go = [&](auto flat_c) {
        constexpr bool F = decltype(flat_c)::value;
        if (p.filter) {
            if (fused) hipLaunchKernelGGL((k_icp<LW, true, true, F>), g, b, lds, s, p);
            else hipLaunchKernelGGL((k_icp<LW, false, true, F>), g, b, lds, s, p);
        } else {
            if (fused) hipLaunchKernelGGL((k_icp<LW, true, false, F>), g, b, lds, s, p);
            else hipLaunchKernelGGL((k_icp<LW, false, false, F>), g, b, lds, s, p);
        }
    };
    if constexpr (kBoth) {
        if (flat) go(std::true_type{});
        else go(std::false_type{});
    } else if constexpr (LW >= 3) {
        go(std::true_type{});
    } else {
        go(std::false_type{});
    }
}
void launch_icp(const IcpParams &p, int lw, bool fused, hipStream_t s) {
    if (p.n <= 0) return;
    switch (lw) {
        case 0: launch_icp_lw<0>(p, fused, s); break;
        case 1: launch_icp_lw<1>(p, fused, s); break;
        case 2: launch_icp_lw<2>(p, fused, s); break;
        case 3: launch_icp_lw<3>(p, fused, s); break;
        default: launch_icp_lw<4>(p, fused, s); break;
    }
}

size_t loop_lds_bytes(int lw, int nw, int gpw) {
    return sizeof(uint32_t) * LoopLds<size_t>(lw, static_cast<size_t>(nw), static_cast<size_t>(gpw)).end;
}
// the kernel of a shape, as an untyped pointer (what the occupancy query and the launch take)
static const void *loop_kernel(int lw, bool filter) {
#define SAGE_LOOP_K(LW_, F_) reinterpret_cast<const void *>(&k_loop<LW_, F_>)
    switch (lw) {
        case 1: return filter ? SAGE_LOOP_K(1, true) : SAGE_LOOP_K(1, false);
        case 2: return filter ? SAGE_LOOP_K(2, true) : SAGE_LOOP_K(2, false);
        case 3: return filter ? SAGE_LOOP_K(3, true) : SAGE_LOOP_K(3, false);
        case 4: return filter ? SAGE_LOOP_K(4, true) : SAGE_LOOP_K(4, false);
        default: return nullptr;
    }
#undef SAGE_LOOP_K
}
int loop_blocks_per_cu(int lw, bool filter, int nw, size_t lds) {
    if (nw < 1 || nw > kLoopMaxWaves || lds > 160 * 1024) return 0;
    const void *k = loop_kernel(lw, filter);
    if (!k) return 0;
    // (a workgroup that owns many units can ask for more than the 64 KB a kernel gets by default)
    if (lds > 64 * 1024 && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return 0;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, 64 * nw, lds) != hipSuccess) return 0;
    return nb;
}
void launch_loop(const IcpParams &p, const LoopParams &l, int lw, hipStream_t s) {
    const size_t lds = loop_lds_bytes(lw, l.nw, l.gpw);
    LoopArgs a;
    a.P = p;
    a.L = l;
    a.face_slack = 1e-9 * p.voxel_size;        // (one IEEE product of the same two numbers, here as in k_icp's passes)
    void *args[] = {&a};
#ifdef SAGE_LOOP_INGRID
    (void)hipLaunchKernel(loop_kernel(lw, p.filter != 0), dim3(l.wgs + 1), dim3(64 * l.nw), args, lds, s);
#else
    (void)hipLaunchKernel(loop_kernel(lw, p.filter != 0), dim3(l.wgs), dim3(64 * l.nw), args, lds, s);
#endif
}
void launch_loop_solve(const LoopParams &l, const P2pParams &x, hipStream_t s) {
    SolveArgs a;
    a.L = l;
    a.X = x;
    if (l.copies == kChainReplicas) hipLaunchKernelGGL(k_loop_solve<kChainReplicas>, dim3(1), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_loop_solve<kLoopReplicas>, dim3(1), dim3(64), 0, s, a);
}

int launch_gn(const GnParams &p, hipStream_t s) {
    long blocks = (static_cast<long>(p.n) + 255) / 256;
    if (blocks > 128) blocks = 128;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_gn, dim3(static_cast<int>(blocks)), dim3(256), 0, s, p);
    return static_cast<int>(blocks);
}

void launch_fin(const FinParams &p, hipStream_t s) {
    hipLaunchKernelGGL(k_fin, dim3(1), dim3(kFinThreads), 0, s, p);
}

void launch_tf(Point4 *pts, int n, const IcpState *st, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_tf, dim3((n + 255) / 256), dim3(256), 0, s, pts, n, st);
}

}  // namespace sageicp
