// Hand-written HIP kernels for gfx950 (CDNA4, wave64) — SAGE-ICP registration hot path.
// One ICP iteration = k_icp -> k_fin, both on one stream, no host round trip.
//
// This file holds the kernels, their helpers and the launchers; the search body that k_icp and k_loop share
// (icp_body: everything between a wave's queries and their sums) lives in icp_body.h, included below.
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
//            JtJ / Jtr per accepted pair, reduced in a fixed order to one partial per workgroup.
//   k_rows   builds every query's neighbourhood row after a (re-)sort of the frame (27 lanes probe
//            the GPU-resident open-addressed hash per query).
//   k_fin    one workgroup: fixed-order reduction of the partials (bit-reproducible), [exchange of
//            the sums with the peer GPUs,] 6x6 LDL^T solve and SE3 exp with their divisions /
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
template <bool QUAD = false>
__device__ __forceinline__ Query make_query(const Point4 &f, const double *R, const double *t, int apply_pose,
                                            double voxel_size, double inv_vs = 0.0) {
    Query q;
    q.x = f.x; q.y = f.y; q.z = f.z; q.l = f.l;
    if (apply_pose) {
        q.x = R[0] * f.x + R[1] * f.y + R[2] * f.z + t[0];
        q.y = R[3] * f.x + R[4] * f.y + R[5] * f.z + t[1];
        q.z = R[6] * f.x + R[7] * f.y + R[8] * f.z + t[2];
    }
    if constexpr (QUAD) {
        const unsigned a = threadIdx.x & 3u;
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
// have room for: the overflow flag then sends the frame through the fp64 partials (capi.hip).
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

// A wave's 16 pair terms per query -> block sums -> digits -> added into the workgroup's accumulators `wgacc`
// (LDS, kWgAccWords 64-bit words).  The terms are spread over the W lanes of a query: lane ci holds components
// ci K .. ci K + K - 1 (K = 16 / W; zeros for a query without a pair).  `red` = LDS scratch of this wave, 16 fp64
// per block.
template <int LW>
__device__ __forceinline__ void wave_terms_to_wgacc(const double (&t)[kCount >> LW], unsigned pairs, int lane, double *red,
                                                    unsigned long long *wgacc, double limit, double scale) {
    constexpr int W = 1 << LW, QW = 64 >> LW, NBLK = QW / 4, K = kCount >> LW;
    // A. block sums, (t0 + t1) + (t2 + t3), on the lanes of the first query of every block
    double y[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double x = t[k] + lane_shl_f64<W>(t[k]);
        y[k] = x + lane_shl_f64<2 * W>(x);
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

// The workgroup's accumulators (LDS) -> the shared ones: lane l sends word l (digit l % 3 of value l / 3) as ONE
// fire-and-forget 64-bit integer atomic into the copy `dst`, and clears the word for the next iteration.
// COUNTED (k_loop): every word also counts its contributions — a workgroup adds (digit << 8) + 1, the low
// byte of a word says how many workgroups are in it — so that whoever reads the accumulators inside the
// launch knows, word by word, when they are complete, and the workgroup neither waits for its atomics to
// be acknowledged nor keeps a separate arrival counter.  (The form that did both — s_waitcnt vmcnt(0), then
// one of eight counters — ran an iteration in the same time, profiles/r04/loop_times_counted_words.txt against
// loop_times_xcd_stripes_rowshift.txt: this one is kept for having one protocol less and no ordering
// assumption at all.)
template <bool COUNTED = false>
__device__ __forceinline__ void wgacc_flush(unsigned long long *wgacc, long long *dst, long long *overflow) {
    const int lane = static_cast<int>(threadIdx.x & 63u);
    const int l = min(lane, static_cast<int>(kWgAccWords) - 1);
    const long long x = static_cast<long long>(wgacc[l]);
    const bool ok = wgacc[kWgAccWords - 1] == 0ull;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (lane < static_cast<int>(kWgAccWords)) wgacc[lane] = 0ull;
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
#ifdef SAGE_LOOP_TIMING
    unsigned long long ph[8], tprev;           // probe builds: cycles per phase of the body, summed over the iterations
#endif
};
constexpr int kLoopMaxWaves = kLoopMaxWavesHost;   // waves per workgroup of k_loop (<= 512 threads)
constexpr unsigned kLoopStripe = kLoopStripeHost;  // workgroups of k_loop per XCD stripe (its grid: a multiple of 32)
constexpr int kNoVoxel = 0x7FFFFFFF;        // a home voxel no point has (|index| < 2^20): row not built yet
constexpr unsigned kStPrev = 16, kStKey = 18;
// LDS of a k_loop workgroup (words): header { arrival counter | next group | the pose of this iteration
// (R[9], t[3]) | done | the workgroup's fixed-point accumulators } | the groups { rows, state } |
// one scratch for the transposed block sums per wave
constexpr unsigned kLpArrive = 0, kLpNext = 1, kLpDone = 2;
constexpr unsigned kLpPose = 4;                                    // 12 doubles, 16-B aligned
constexpr unsigned kLpDbg = kLpPose + 24u;                         // probe builds: max points of a query | stale queries | points
constexpr unsigned kLpFirst = kLpDbg + 4u;                         // per wave: the unit it takes first in every iteration (LoopParams::deal)
constexpr unsigned kLpAcc = kLpFirst + 8u;                         // kWgAccWords 64-bit words
constexpr unsigned kLpHeaderWords = (kLpAcc + 2u * kWgAccWords + 15u) & ~15u;
__host__ __device__ constexpr unsigned loop_group_words(int lw) {
    return static_cast<unsigned>((kRowLdsStride + kLoopStateWords) * (64 >> lw));
}
__host__ __device__ constexpr unsigned loop_red_words() { return 2u * kCount * 4u; }    // 16 fp64 for each of four blocks of queries
__host__ __device__ constexpr unsigned loop_perm_words(unsigned nblk) { return 2u * ((nblk + 7u) & ~7u); }   // perm | work, 32-B aligned

// Chained launches (IcpParams::chain): wave 0 of a workgroup of the launch of iteration `it` waits for the pose the solving
// wave publishes after iteration it - 1 (25 self-tagged granules, tag = it; kernels.h, LoopShared) and hands it to the
// workgroup through LDS.  smem[kWgGo] != 0: the workgroup leaves — the loop ended before this iteration (the done granule
// carries an older tag, or this tag with its done word set), or a wait timed out somewhere.
// Which of the kLoopPoseCopies copies of the pose workgroup b looks at (kernels.h): its XCD's by default.
__device__ __forceinline__ unsigned loop_pose_copy(int pose_map) {
    const unsigned b = blockIdx.x;
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

// ------------------------------------------------------------------------------------ WaveLanes
// Lane policy (se3_math.h) for the wave that finishes an iteration: its 64 lanes all hold the
// same (uniform) values, so independent fp64 divisions / sincos arguments are moved to separate
// lanes, evaluated by ONE vector instruction sequence, and read back with v_readlane.  A serial
// lane spent ~2 us of every iteration in the 21 divisions of the 6x6 LDL^T alone.
// Must be called with lanes 0..5 active and uniform operands.
struct WaveLanes {
    static __device__ __forceinline__ void divide6(const double (&n)[6], const double (&d)[6],
                                                   double (&q)[6]) {
        const int lane = static_cast<int>(threadIdx.x & 63u);
        double nn = n[0], dd = d[0];
#pragma unroll
        for (int i = 1; i < 6; ++i) {
            nn = (lane == i) ? n[i] : nn;
            dd = (lane == i) ? d[i] : dd;
        }
        const double qq = nn / dd;
#pragma unroll
        for (int i = 0; i < 6; ++i) q[i] = readlane_f64(qq, i);
    }
    static __device__ __forceinline__ void sincos2(double a0, double a1, double &s0, double &c0,
                                                   double &s1, double &c1) {
        const int lane = static_cast<int>(threadIdx.x & 63u);
        double sv, cv;
        sincos(lane == 1 ? a1 : a0, &sv, &cv);
        s0 = readlane_f64(sv, 0); c0 = readlane_f64(cv, 0);
        s1 = readlane_f64(sv, 1); c1 = readlane_f64(cv, 1);
    }
    static __device__ __forceinline__ void sqrt2(double a0, double a1, double &r0, double &r1) {
        const int lane = static_cast<int>(threadIdx.x & 63u);
        const double v = sqrt(lane == 1 ? a1 : a0);
        r0 = readlane_f64(v, 0);
        r1 = readlane_f64(v, 1);
    }
    // (the operands are uniform, so is b: taken as the wave's, a scalar branch)
    static __device__ __forceinline__ bool uniform(bool b) { return __all(b); }
};

// ------------------------------------------------------------------------------ finish_iteration
// Executed by ONE workgroup of 1024 threads once per ICP iteration (k_fin): fixed-order reduction
// of the workgroup partials of k_icp (bit-reproducible), then the first wave solves the normal
// equations from the 16 closed-form sums (se3_math.h solve_normal_equations_t: the block-structured
// solve, the register-resident pivoted 6x6 LDL^T where its guard refuses), applies SE3 exp, composes
// the pose and tests convergence (Registration.cpp:92-93,135-137).
#ifdef SAGE_GN_TIMING
__device__ unsigned long long g_gn_phase[16];
#define FIN_STAMP(i) do { if (threadIdx.x == 0) fin_t[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define FIN_STAMP(i) do { } while (0)
#endif

constexpr int kFinThreads = 1024;
constexpr int kFinSlices = 102;             // 10 fp64 pairs per partial x 102 slices = 1020 threads

// Returns false (on every thread) when *done is set: the loop has finished and this launch is a
// no-op.  The flag is fetched together with the partials — one memory round trip, not two.
__device__ __forceinline__ bool reduce_partials(const double *partials, int nparts, double *S /* LDS [kNumSums] */,
                                                const int32_t *done) {
    __shared__ double part[kFinSlices][kNumSums];
    __shared__ double part2[6][kNumSums];
    const int t = static_cast<int>(threadIdx.x);
    const int pr = t % 10, sl = t / 10;
    if (sl < kFinSlices) {
        // fixed summation order; the loads are independent: up to 24 in flight per thread (one
        // memory round trip for up to 2,448 partials, the cold-L2 latency is what this kernel costs)
        double2 v = make_double2(0.0, 0.0);
        const double2 *src = reinterpret_cast<const double2 *>(partials) + pr;
        bool first = true;
        for (int b = sl; b < nparts; b += 24 * kFinSlices) {
            double2 u[24];
#pragma unroll
            for (int k = 0; k < 24; ++k) {
                const int bb = b + k * kFinSlices;
                u[k] = bb < nparts ? src[static_cast<size_t>(bb) * 10] : make_double2(0.0, 0.0);
            }
            if (first && done) {
                // a vector load like the ones above (the index is zero, but formally per lane), so
                // that it travels with them: a scalar load would be waited for before the partials
                // are even requested
                const int32_t d = done[__builtin_amdgcn_mbcnt_lo(0u, 0u)];
                if (__builtin_amdgcn_readfirstlane(d)) return false;
                first = false;
            }
#pragma unroll
            for (int k = 0; k < 24; ++k) { v.x += u[k].x; v.y += u[k].y; }
        }
        if (first && done) {                   // no partials at all (an empty frame)
            const int32_t d = done[__builtin_amdgcn_mbcnt_lo(0u, 0u)];
            if (__builtin_amdgcn_readfirstlane(d)) return false;
        }
        part[sl][2 * pr] = v.x;
        part[sl][2 * pr + 1] = v.y;
    } else if (done) {
        const int32_t d = done[__builtin_amdgcn_mbcnt_lo(0u, 0u)];
        if (__builtin_amdgcn_readfirstlane(d)) return false;
    }
    __syncthreads();
    if (t < 6 * kNumSums) {
        const int c = t % kNumSums, g = t / kNumSums;
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < kFinSlices / 6; ++k) v += part[g * (kFinSlices / 6) + k][c];
        part2[g][c] = v;
    }
    __syncthreads();
    if (t < kNumSums) {
        double v = part2[0][t];
#pragma unroll
        for (int g = 1; g < 6; ++g) v += part2[g][t];
        S[t] = v;
    }
    __syncthreads();
    return true;
}

// The sums from the fixed-point accumulators k_icp's workgroups added into (kernels.h): one round
// trip for 16 KB, the replicas added exactly (integers), three digits -> one fp64 per sum, and the
// accumulators cleared for the next iteration.  Returns false when *done is set (see above).
__device__ __forceinline__ bool reduce_accumulators(long long *acc, double *S /* LDS [kNumSums] */,
                                                    const int32_t *done, int32_t *overflow, double unscale) {
    __shared__ long long part[kAccReplicas][kAccWords];
    __shared__ long long part2[8][kAccWords];
    const int t = static_cast<int>(threadIdx.x);
    // 2,048 words over 1,024 threads: 16 B each, one coalesced round trip
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    ll2 *src = reinterpret_cast<ll2 *>(acc);
    const ll2 v = src[t];
    if (done) {
        const int32_t d = done[__builtin_amdgcn_mbcnt_lo(0u, 0u)];      // travels with the load above
        if (__builtin_amdgcn_readfirstlane(d)) return false;
    }
    ll2 z;
    z.x = 0; z.y = 0;
    src[t] = z;                                                          // cleared for the next launch of k_icp
    reinterpret_cast<ll2 *>(&part[0][0])[t] = v;
    __syncthreads();
    if (t < 8 * kAccWords) {
        const int w = t % kAccWords, g = t / kAccWords;
        long long s = 0;
#pragma unroll
        for (int k = 0; k < kAccReplicas / 8; ++k) s += part[g * (kAccReplicas / 8) + k][w];
        part2[g][w] = s;
    }
    __syncthreads();
    if (t < kAccWords) {
        long long s = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) s += part2[g][t];
        part[0][t] = s;
    }
    __syncthreads();
    if (t < kNumSums) {
        double r = 0.0;
        if (t < kAccValues) {
            const double a = static_cast<double>(part[0][3 * t]);
            const double b = static_cast<double>(part[0][3 * t + 1]);
            const double c = static_cast<double>(part[0][3 * t + 2]);
            r = a + (b * 9.094947017729282e-13 + c * 8.271806125530277e-25);      // 2^-40, 2^-80
            if (t < kCount) r *= unscale;      // (a power of two; the pair count is not scaled)
        }
        S[t] = r;
        if (t == 0 && part[0][kAccWords - 1] != 0) *overflow = 1;
    }
    __syncthreads();
    return true;
}

// the solve: wave 0, all 64 lanes, uniform data (see WaveLanes); lane 0 / lane 1 publish the state
// The loop state the finish needs (the two poses the estimate is composed with, the iteration
// count), requested by the first wave BEFORE the reduction so that its cold round trip (~0.7 us)
// runs under it instead of after the solve.
struct FinState {
    double rhs[7];            // lane 1: T_icp, the other lanes: T
    int iter;
};
__device__ __forceinline__ FinState prefetch_state(const IcpState *st) {
    FinState f;
    const int lane = static_cast<int>(threadIdx.x);
    const double *src = (lane == 1) ? st->T_icp : st->T;
#pragma unroll
    for (int i = 0; i < 7; ++i) f.rhs[i] = src[i];
    f.iter = st->iter;
    return f;
}

__device__ __forceinline__ void solve_and_publish(IcpState *st, const double *S, const FinState &pre) {
#ifdef SAGE_GN_TIMING
    unsigned long long fin_t[8];
#endif
    FIN_STAMP(1);
    const int lane = static_cast<int>(threadIdx.x);
    double x[6], est[7], nrm;
    solve_normal_equations_t<WaveLanes>(S, x);
    FIN_STAMP(2);
    se3_exp_sqrt_t<WaveLanes>(x, est, SAGE_SQNORM6(x), nrm);        // nrm = |x|, beside the exponential's sqrt
    FIN_STAMP(3);

    // the two compositions (Registration.cpp:135 and the cumulative pose) on lanes 0 and 1
    double Tn[7];
    se3_mul(est, pre.rhs, Tn);
    if (lane < 2) {
        double *dst = (lane == 1) ? st->T_icp : st->T;
#pragma unroll
        for (int i = 0; i < 7; ++i) dst[i] = Tn[i];
    }
    if (lane != 0) return;
    quat_to_mat(Tn, st->R);

    // ||log(exp(x))|| == ||x|| on the principal branch up to a few ulps, so the reference's
    // estimation.log().norm() (Registration.cpp:137) is taken from x without the atan2 / sincos
    // round trip on one serial lane — except where those ulps could matter: a step within 1e-12
    // (relative 1e-8; the two differ by ~1e-19 there) of the stop threshold, or |omega| >= 3,
    // goes through the exact log so that the stop iteration is the reference's in every case.
    if (!(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] < 9.0) ||
        fabs(nrm - kEstimationThreshold) < 1e-12) {
        double lg[6];
        se3_log(est, lg);
        nrm = sqrt(SAGE_SQNORM6(lg));          // the reduction order of a 6-vector's norm(): sageicp_types.h
    }
    st->last_step_norm = nrm;
    const int it = pre.iter;
    if (it < kHistory) st->n_corr[it] = static_cast<uint32_t>(S[kCount]);
    st->iter = it + 1;
    unsigned long long done = 0;
    if (nrm < kEstimationThreshold) {
        st->converged = 1;
        st->done = 1;
        done = 1;
    } else if (it + 1 >= kMaxIterations) {
        st->done = 1;
        done = 1;
    }
    if (st->done) done = 1;                    // e.g. stopped by a failed multi-GPU exchange
    if (IcpProgress *pg = st->progress) {
        // host-mapped, a relaxed system-scope (write-through) store: the host only steers its
        // look-ahead by this word and reads the final state through an ordinary copy after the loop
        const unsigned long long seq = static_cast<unsigned long long>(it + 1);
        __hip_atomic_store(&pg->word, (done << 32) | seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#ifdef SAGE_GN_TIMING
    fin_t[4] = __builtin_amdgcn_s_memrealtime();
    for (int i = 1; i < 4; ++i) atomicAdd(&g_gn_phase[8 + i], fin_t[i + 1] - fin_t[i]);
    atomicAdd(&g_gn_phase[4], 1ull);
#endif
}

// --------------------------------------------------------------------------------- exchange_sums
// One workgroup per rank (the last arriver of k_gn), see P2pBlock.  st->sums holds this rank's
// sums on entry and the sums over all ranks on exit.  Stores to the peers are system-scope
// write-through atomics, completed (s_waitcnt) and fenced before the tag goes out; the tags are
// polled with system-scope loads and an acquire fence precedes the reads of the rows.
__device__ __forceinline__ void exchange_sums(IcpState *st, const P2pParams &X) {
    const int t = static_cast<int>(threadIdx.x);
    const unsigned long long g = *X.exchanges;
    const int slot = static_cast<int>(g & 1ull);
    const unsigned long long tag = g + 1ull;
    if (t < kNumSums) {
        const double v = st->sums[t];
        for (int r = 0; r < X.nranks; ++r)
            __hip_atomic_store(&X.block[r]->sums[slot][X.rank][t], v, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        for (int r = 0; r < X.nranks; ++r)
            __hip_atomic_store(&X.block[r]->flag[X.rank], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    P2pBlock *mine = X.block[X.rank];
    __shared__ int s_late;
    if (t == 0) s_late = 0;
    __syncthreads();
    if (t < X.nranks) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(&mine->flag[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < tag) {
            __builtin_amdgcn_s_sleep(4);
            if (__builtin_amdgcn_s_memrealtime() - t0 > X.timeout_ticks) {
                s_late = 1;
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        // a peer gave up its one-launch loop at this exchange (P2pBlock::abort_tag)
        if (__hip_atomic_load(&mine->abort_tag[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == tag) s_late = 2;
    }
    __syncthreads();
    if (t == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    __syncthreads();
    if (t < kNumSums) {
        double s = 0.0;
        for (int r = 0; r < X.nranks; ++r)       // rank order: the same sum on every rank
            s += __hip_atomic_load(&mine->sums[slot][r][t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        st->sums[t] = s;
    }
    if (t == 0) {
        *X.exchanges = tag;
        if (s_late == 2) {                     // every rank leaves this exchange and starts the frame again (run_icp)
            st->peer_aborted = 1;
            st->done = 1;
        } else if (s_late) {                   // stop the loop; the host reports the failure
            st->exchange_failed = 1;
            st->done = 1;
        }
    }
}

// ------------------------------------------------------------------------------------ k_fin
__global__ __launch_bounds__(kFinThreads) void k_fin(FinParams P) {
    __shared__ double S[kNumSums];
    IcpState *st = P.st;
    if (P.mode == 2 && !P.standalone && st->done) return;
#ifdef SAGE_GN_TIMING
    const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
#endif
    FinState pre{};
    if (threadIdx.x < 64) pre = prefetch_state(st);
    if (P.mode != 2) {
        if (P.acc) {
            if (!reduce_accumulators(P.acc, S, P.standalone ? nullptr : &st->done, &st->acc_overflow, P.acc_unscale)) return;
        } else if (!reduce_partials(P.partials, P.nparts, S, P.standalone ? nullptr : &st->done)) return;
#ifdef SAGE_GN_TIMING
        if (threadIdx.x == 0) atomicAdd(&g_gn_phase[8], __builtin_amdgcn_s_memrealtime() - t_start);
#endif
        if (threadIdx.x < kNumSums) st->sums[threadIdx.x] = S[threadIdx.x];
        if (P.mode == 1) return;
        if (P.mode == 3) {
            __syncthreads();
            exchange_sums(st, P.p2p);
            __syncthreads();
            if (threadIdx.x < kNumSums) S[threadIdx.x] = st->sums[threadIdx.x];
            __syncthreads();
        }
    } else {
        if (threadIdx.x < kNumSums) S[threadIdx.x] = st->sums[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x >= 64) return;
    solve_and_publish(st, S, pre);
}

// ------------------------------------------------------------------------------------ k_loop
// The whole loop of Registration.cpp:127-138 in one launch of the query workgroups (k_loop) beside a
// one-wave solving kernel (k_loop_solve) on a second stream (kernels.h, LoopShared).  Per iteration:
//   every wave        takes the workgroup's groups one after another from an LDS counter and runs
//                     icp_body<PERSIST> on each — pose from LDS, per-query state and rows in LDS —,
//                     which parks the group's sums in the workgroup's LDS;
//   last wave of a    adds the workgroup's sums into the fixed-point accumulators: (digit << 8) + 1 per
//   workgroup         word, fire and forget — the low byte of every word counts who is in it;
//   the solving       reads this iteration's set of accumulators until every word counts all its
//   wave              workgroups (two sets alternate; the one just read is cleared for the iteration
//                     after the next), [exchanges the sums with the peer GPUs,] solves, composes, tests,
//                     and publishes the next pose as 25 self-tagged 8-byte granules (tag = iteration
//                     + 1: the data is the flag, no fence on either side), one copy per XCD;
//   wave 0 of every   polls its XCD's granules (one relaxed agent-scope load per lane and pass), hands the
//   workgroup         pose to its workgroup through LDS;  __syncthreads();  next iteration.
// Every word the workgroups share is accessed with agent-scope atomics only.  Every wait is bounded:
// a timeout raises LoopShared::abort_word and IcpState::loop_aborted, everybody leaves, and the host
// registers the frame through the launch-per-iteration loop instead (a grid that is not fully
// resident — another process or stream holding CUs — ends this way, not in a hang).
#ifdef SAGE_LOOP_TIMING
// probe builds: 100-MHz stamps of the first kLoopTimedIters iterations — per workgroup when it counted
// itself in and when it had the next pose; for the solving wave when all counts were in, the sums
// read, the step solved, the pose published
constexpr int kLoopTimedIters = 32, kLoopTimedWgs = 2048;
__device__ unsigned long long g_loop_wg[kLoopTimedIters][kLoopTimedWgs][4];     // counted in | pose held | a wave took a unit beyond one per wave | ... finished it
__device__ unsigned g_loop_wginfo[kLoopTimedIters][kLoopTimedWgs][4];     // HW_ID | max points of a query | stale queries | points
__device__ unsigned long long g_loop_solver[kLoopTimedIters][4];
__device__ unsigned long long g_loop_solver2[kLoopTimedIters][4];      // inside the solve: after the solve | the exponential (and the sqrt of the step norm) | the composition | the norm test
__device__ unsigned long long g_loop_wave[kLoopTimedIters][kLoopTimedWgs][8][2];      // per wave: its FIRST unit of the iteration: end stamp | start stamp (low 32) << 32 ... see LOOP_STAMP_WAVE
__device__ unsigned long long g_loop_phase[16];     // [0..7] cycles per body phase, [8] wait for the pose, [9] closing a workgroup, [10] group passes
#define LOOP_STAMP_SOLVER(it, k) do { if ((it) < kLoopTimedIters && (threadIdx.x & 63u) == 0u) g_loop_solver[it][k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define LOOP_STAMP_SOLVER2(it, k) do { if ((it) < kLoopTimedIters && (threadIdx.x & 63u) == 0u) g_loop_solver2[it][k] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" void sageicp_debug_loop_solver2(unsigned long long *out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_solver2), sizeof(unsigned long long) * kLoopTimedIters * 4);
}
#define LOOP_STAMP_WG(it, k) do { if ((it) < kLoopTimedIters && blockIdx.x < kLoopTimedWgs && (threadIdx.x & 63u) == 0u) g_loop_wg[it][blockIdx.x][k] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" void sageicp_debug_loop_phases(unsigned long long *out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_phase), sizeof(unsigned long long) * 16);
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_loop_phase), z, sizeof(z));
    }
}
extern "C" void sageicp_debug_loop_waves(unsigned long long *out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_wave), sizeof(unsigned long long) * kLoopTimedIters * kLoopTimedWgs * 8 * 2);
}
extern "C" void sageicp_debug_loop_info(unsigned *info) {
    (void)hipMemcpyFromSymbol(info, HIP_SYMBOL(g_loop_wginfo), sizeof(unsigned) * kLoopTimedIters * kLoopTimedWgs * 4);
}
extern "C" void sageicp_debug_loop_times(unsigned long long *wg, unsigned long long *solver) {
    (void)hipMemcpyFromSymbol(wg, HIP_SYMBOL(g_loop_wg), sizeof(unsigned long long) * kLoopTimedIters * kLoopTimedWgs * 4);
    (void)hipMemcpyFromSymbol(solver, HIP_SYMBOL(g_loop_solver), sizeof(unsigned long long) * kLoopTimedIters * 4);
}
#else
#define LOOP_STAMP_SOLVER(it, k) do { } while (0)
#define LOOP_STAMP_SOLVER2(it, k) do { } while (0)
#define LOOP_STAMP_WG(it, k) do { } while (0)
#endif


// exchange_sums for ONE wave (the solving wave of k_loop_solve): S (LDS) holds this rank's sums on entry
// and the sums over all ranks, added in rank order, on exit; `g` is the exchange counter (the same on
// every rank).  Returns 0, 1 when a peer's sums did not arrive in time, 2 when a peer gave up its one-launch loop at
// this exchange (P2pBlock::abort_tag).
__device__ __forceinline__ int exchange_sums_wave(double *S, const P2pParams &X, unsigned long long g) {
    const int lane = static_cast<int>(threadIdx.x & 63u);
    const int slot = static_cast<int>(g & 1ull);
    const unsigned long long tag = g + 1ull;
    if (lane < kNumSums) {
        const double v = S[lane];
        for (int r = 0; r < X.nranks; ++r)
            __hip_atomic_store(&X.block[r]->sums[slot][X.rank][lane], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0)
        for (int r = 0; r < X.nranks; ++r)
            __hip_atomic_store(&X.block[r]->flag[X.rank], tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    P2pBlock *mine = X.block[X.rank];
    bool late = false, gone = false;
    if (lane < X.nranks) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(&mine->flag[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < tag) {
            __builtin_amdgcn_s_sleep(2);
            if (__builtin_amdgcn_s_memrealtime() - t0 > X.timeout_ticks) {
                late = true;
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        gone = __hip_atomic_load(&mine->abort_tag[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == tag;
    }
    late = __any(late);
    gone = __any(gone);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    if (lane < kNumSums) {
        double s = 0.0;
        for (int r = 0; r < X.nranks; ++r)       // rank order: the same sum on every rank
            s += __hip_atomic_load(&mine->sums[slot][r][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        S[lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    return gone ? 2 : (late ? 1 : 0);
}
// This rank leaves its one-launch loop at exchange `g` (a wait inside the launch timed out): the peers are told through
// the flag of that exchange, so that everybody leaves it together.
__device__ __forceinline__ void exchange_abort_wave(const P2pParams &X, unsigned long long g) {
    const int lane = static_cast<int>(threadIdx.x & 63u);
    if (lane == 0)
        for (int r = 0; r < X.nranks; ++r)
            __hip_atomic_store(&X.block[r]->abort_tag[X.rank], g + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0)          // ... and the flag of the exchange, so that nobody waits for this rank's sums
        for (int r = 0; r < X.nranks; ++r)
            __hip_atomic_store(&X.block[r]->flag[X.rank], g + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One iteration's finish by the solving wave (all 64 lanes, uniform data).  Returns the value of the
// done granule it published: 0 go on, 1 finished, 2 aborted.
struct SolveLds {
    double T[14];              // T[7] | T_icp[7]
    double S[kNumSums];
};
// 64 bits of lane `src` (wave-uniform), on every lane
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int src) {
    const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<unsigned>(v)), src));
    const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<unsigned>(v >> 32)), src));
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}
// The lane index, derived anew: what the compiler can trace to threadIdx it knows to be the same in every iteration
// of the solving wave's loop, and it would keep every select mask and address made from it alive across the solve.
__device__ __forceinline__ int lane_now() {
    unsigned l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return static_cast<int>(l);
}
template <int COPIES>
__device__ __forceinline__ unsigned loop_finish_iteration(const LoopParams &L, const P2pParams &X, SolveLds &m, int it,
                                                          unsigned long long &xg) {
    LoopShared *sh = L.sh;
    IcpState *st = L.st;
    const int lane = static_cast<int>(threadIdx.x & 63u);          // (one wave)
    double *sT = m.T, *S = m.S;
    const unsigned long long tag = static_cast<unsigned long long>(it) + 1ull;

    double sum = 0.0;          // lane l < kAccValues: value l of this iteration's sums
    bool overflow;
    // 1. the sums of this iteration's set of accumulators: read (one round trip per pass) until every word
    // says that all the workgroups adding into it are in (its low byte counts them, wgacc_flush) —
    // the read that finds them complete IS the read of the sums.  The set is then cleared for the
    // iteration after the next (the clears are complete long before that pose is published: the waits
    // of the next iteration's passes cover them).
    {
        const long long per = static_cast<long long>(L.wgs / COPIES);      // workgroups adding into each copy
        long long (*acc)[kAccWords] = COPIES == kLoopReplicas ? sh->acc[it & 1] : sh->acc32[it & 1];
        long long v[COPIES];
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
#pragma unroll
            for (int r = 0; r < COPIES; ++r)
                v[r] = __hip_atomic_load(&acc[r][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bool ok = true;
            if (lane <= 3 * kAccValues) {          // (word 3 kAccValues: the overflow count, counted like the sums)
#pragma unroll
                for (int r = 0; r < COPIES; ++r) ok &= (v[r] & 255ll) == per;
            }
            if (__all(ok)) break;
            unsigned long long ab = 0ull;
            if (lane == 0) ab = ld_agent(&sh->abort_word[0]);
            // (its own workgroups' counts are a local matter: the short wait also under a communicator, where the
            // workgroups' patience — timeout_ticks — has to outlast the exchange with the peers)
            const bool late = __builtin_amdgcn_s_memrealtime() - t0 > L.count_timeout_ticks;
            if (__any(ab != 0ull) || late) {
                if (lane == 0) {
                    st_agent(&sh->abort_word[0], 1ull);
                    st->loop_aborted = 1;
                    if (L.progress)        // (chained launches: the host stops enqueuing)
                        __hip_atomic_store(&L.progress->word, (1ull << 32) | static_cast<unsigned long long>(it), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                }
                if (const int al = lane_now(); al < kLoopPoseCopies) st_agent(&sh->pose[al][24], (tag << 32) | 2ull);      // (every copy's done word)
                if (X.nranks > 1) {
                    // the peers are inside (or on their way to) this very exchange: they leave it with us, and every
                    // rank registers the frame again through the launch-per-iteration form, in step (run_icp)
                    exchange_abort_wave(X, xg);
                    xg += 1ull;
                    if (lane == 0) *X.exchanges = xg;
                }
                return 2u;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        LOOP_STAMP_SOLVER(it, 0);
        long long d = 0;
        if (lane <= 3 * kAccValues) {
#pragma unroll
            for (int r = 0; r < COPIES; ++r) d += (v[r] - per) >> 8;       // (exact: the low byte is the count)
        }
#pragma unroll
        for (int r = 0; r < COPIES; ++r)
            __hip_atomic_store(&acc[r][lane], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the three digits of value l, held by the lanes 3 l .. 3 l + 2, come to lane l across the lanes (no trip
        // through LDS and no barrier in the chain the grid waits for)
        const int sl = lane_now();
        const int s3 = 3 * (sl < kAccValues ? sl : 0);
        const double a = static_cast<double>(__shfl(d, s3));
        const double b = static_cast<double>(__shfl(d, s3 + 1));
        const double c = static_cast<double>(__shfl(d, s3 + 2));
        if (lane < kAccValues) {
            sum = a + (b * 9.094947017729282e-13 + c * 8.271806125530277e-25);      // 2^-40, 2^-80
            if (lane < kCount) sum *= L.acc_unscale;     // (a power of two; the pair count is not scaled)
        }
        if (lane < kNumSums) S[lane] = sum;
        overflow = readlane_u64(static_cast<unsigned long long>(d), 3 * kAccValues) != 0ull;      // workgroups whose sums left the range (wgacc_flush)
        __builtin_amdgcn_wave_barrier();
    }
    LOOP_STAMP_SOLVER(it, 1);

    // 2. multi-GPU: this rank's sums -> the sums over all ranks (direct exchange over xGMI, P2pBlock)
    bool exchange_failed = false;
    if (X.nranks > 1) {
        const int ex = exchange_sums_wave(S, X, xg);
        xg += 1ull;
        if (lane == 0) *X.exchanges = xg;
        exchange_failed = ex == 1;
        if (ex == 2) {
            // a peer gave up its one-launch loop at this exchange: so does this rank (its workgroups see the abort word)
            if (lane == 0) {
                st_agent(&sh->abort_word[0], 1ull);
                st->loop_aborted = 1;
                st->peer_aborted = 1;
                if (L.progress)        // (chained launches: the host stops enqueuing)
                    __hip_atomic_store(&L.progress->word, (1ull << 32) | static_cast<unsigned long long>(it), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
            }
            if (const int al = lane_now(); al < kLoopPoseCopies) st_agent(&sh->pose[al][24], (tag << 32) | 2ull);      // (every copy's done word)
            return 2u;
        }
    }

    // 3. solve, compose, test (Registration.cpp:92-93,135-137) — as k_fin's solve_and_publish
    double x[6], est[7], nrm;
    solve_normal_equations_t<WaveLanes>(S, x);
    LOOP_STAMP_SOLVER2(it, 0);
    se3_exp_sqrt_t<WaveLanes>(x, est, SAGE_SQNORM6(x), nrm);        // nrm = |x|, beside the exponential's sqrt
    LOOP_STAMP_SOLVER2(it, 1);
    double rhs[7], Tn[7];
    {
        const double *src = sT + (lane == 1 ? 7 : 0);      // lane 1: T_icp, the other lanes: T
#pragma unroll
        for (int i = 0; i < 7; ++i) rhs[i] = src[i];
    }
    se3_mul(est, rhs, Tn);
    __builtin_amdgcn_wave_barrier();
    if (lane < 2) {
        double *dst = sT + (lane == 1 ? 7 : 0);
#pragma unroll
        for (int i = 0; i < 7; ++i) dst[i] = Tn[i];
    }
    double Rn[9];
    quat_to_mat(Tn, Rn);
    LOOP_STAMP_SOLVER2(it, 2);
    if (!(x[3] * x[3] + x[4] * x[4] + x[5] * x[5] < 9.0) || fabs(nrm - kEstimationThreshold) < 1e-12) {
        double lg[6];                                      // see solve_and_publish
        se3_log(est, lg);
        nrm = sqrt(SAGE_SQNORM6(lg));
    }
    LOOP_STAMP_SOLVER2(it, 3);
    const bool converged = nrm < kEstimationThreshold;
    unsigned done = (converged || it + 1 >= L.max_iterations) ? 1u : 0u;
    // (under a communicator an overflow on this rank alone must not end its loop: the peers would wait
    // for its sums; the flag is raised and the host reports it when the loop has ended everywhere)
    if (overflow && !L.shared_loop) done = 1u;
    if (exchange_failed) done = 1u;
    // 4. publish: 24 halves of R, t and the done word, each with its tag, once per copy of the pose — before the
    // bookkeeping below: the grid waits for these words, nobody for the history (and the wait that follows would
    // otherwise sit out those stores' round trip).  Every lane but lane 1 (which composed T_icp) holds the same R and t:
    // the lanes 2 + l and 34 + l select granule l from their own registers — no trip through LDS —, one store
    // instruction writes two copies, four write them all, fire and forget.
    const int pl = lane_now();
    const int gl = (pl & 31) - 2;
    uint32_t word = done;                  // granule 24
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const unsigned long long v = static_cast<unsigned long long>(__double_as_longlong(i < 9 ? Rn[i] : Tn[i - 5]));
        if ((gl >> 1) == i) word = static_cast<uint32_t>((gl & 1) ? v >> 32 : v);
    }
    LOOP_STAMP_SOLVER(it, 2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the clears of step 1, issued microseconds ago)
    if (gl >= 0 && gl < kLoopPoseGranules) {
#pragma unroll
        for (int c = 0; c < kLoopPoseCopies; c += 2)
            st_agent(&sh->pose[c + (pl >> 5)][gl], (tag << 32) | word);
    }
    if (lane == 0) {
        if (it < kHistory) st->n_corr[it] = static_cast<uint32_t>(S[kCount]);
        if (overflow) st->acc_overflow = 1;
        if (exchange_failed) st->exchange_failed = 1;
        if (done) {
            // the final loop state, for the host (ordinary stores: the end of the kernel publishes them)
#pragma unroll
            for (int i = 0; i < 7; ++i) st->T[i] = Tn[i];
#pragma unroll
            for (int i = 0; i < 9; ++i) st->R[i] = Rn[i];
            st->last_step_norm = nrm;
            st->iter = it + 1;
            st->done = 1;
            st->converged = (converged && !exchange_failed) ? 1 : 0;
        }
    }
    if (done && lane == 1) {
#pragma unroll
        for (int i = 0; i < 7; ++i) st->T_icp[i] = Tn[i];
    }
    if (L.progress && lane == 0)       // (chained launches: the host keeps a few launches enqueued ahead and stops at `done`)
        __hip_atomic_store(&L.progress->word, (static_cast<unsigned long long>(done ? 1u : 0u) << 32) | static_cast<unsigned long long>(it + 1),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (done && lane < kNumSums) st->sums[lane] = S[lane];
    LOOP_STAMP_SOLVER(it, 3);
    return done;
}

// The solving wave: one workgroup of one wave, launched on its own stream beside k_loop's grid (the
// solve needs ~120 registers, the search 72: in one kernel every wave would pay for the solver).
struct SolveArgs {
    LoopParams L;
    P2pParams X;
};
template <int COPIES>      // (two kernels: the one beside k_loop keeps its registers — 157, the grid's residency margin was measured with it)
__global__ __launch_bounds__(64) void k_loop_solve(SolveArgs A) {
    __shared__ SolveLds m;
    __builtin_amdgcn_s_setprio(3);             // (the grid waits for this wave: its SIMD's other waves can)
    {
        // Launched before the frame is even sorted, so that this wave holds its registers when the grid
        // of k_loop fills the machine; it waits here until the grid's first workgroup says that the
        // shared block has been zeroed and the loop has started (LoopShared::go == this call's epoch).
        const int lane = static_cast<int>(threadIdx.x & 63u);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            const unsigned long long g = ld_agent(&A.L.sh->go[0]);
            if ((g & 0x7FFFFFFFFFFFFFFFull) == A.L.epoch) {
                if (g >> 63) return;                        // (sort.hip found a non-finite point: the host reports it)
                break;
            }
            // (the sort, the upload of a frame and a mirror refresh precede the grid: seconds, not the
            // microseconds of the waits inside the loop)
            if (__builtin_amdgcn_s_memrealtime() - t0 > 1000ull * A.L.timeout_ticks + 1000000000ull) {
                if (lane == 0) A.L.st->loop_aborted = 1;
                return;
            }
            __builtin_amdgcn_s_sleep(32);
        }
        if (lane < 14) m.T[lane] = lane < 7 ? A.L.T0[lane] : (lane == 10 ? 1.0 : 0.0);     // T | T_icp = identity (x, y, z, w | t)
    }
    unsigned long long xg = A.X.nranks > 1 ? *A.X.exchanges : 0ull;
    __builtin_amdgcn_wave_barrier();
    for (int it = 0;; ++it) {
        // (the arguments are re-read from the kernel-argument segment every iteration: see k_loop)
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const SolveArgs &K = *(const SolveArgs *)(ka);
        if (loop_finish_iteration<COPIES>(K.L, K.X, m, it, xg)) return;
    }
}

#ifndef SAGE_LOOP_POLL_SLEEP
#define SAGE_LOOP_POLL_SLEEP 8     // x 64 clocks between two looks of a workgroup at the pose granules
#endif
// (Tried and dropped, profiles/r05/mix_ab_*.txt: a workgroup with more units of queries than waves registering
// PAIRS of units at half the lanes per query, one wave per pair, so that every wave makes one pass — bit-identical,
// the sums being exact from the blocks of four queries on, and slower: 37.5 against 34.6 us per iteration on c2.  A
// wave's pass lasts as long as its lanes have points to look at: two units at half the lanes are two passes' worth.)
template <int LW, bool FILT>
__global__ __launch_bounds__(64 * kLoopMaxWaves) __attribute__((amdgpu_waves_per_eu(SAGE_LOOP_OCC, 8)))
void k_loop(LoopArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    constexpr int QW = 64 >> LW;
    const IcpParams &P = A.P;
    const LoopParams &L = A.L;
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int nw = L.nw;
    const unsigned gpw = static_cast<unsigned>(L.gpw);
    double *s_pose = reinterpret_cast<double *>(smem + kLpPose);

    {
        // (sort.hip found a non-finite point: nobody starts, the host reports it — except under a communicator,
        // where the ranks must keep exchanging in step)
        const bool bad = !L.shared_loop && P.st->bad_input;
        if (blockIdx.x == 0 && threadIdx.x == 0)
            st_agent(&L.sh->go[0], L.epoch | (bad ? 0x8000000000000000ull : 0ull));      // the solving wave may start
        if (bad) return;
    }

#ifdef SAGE_LOOP_INGRID
    // Counter-collection twin (profiles/run_profiles.sh builds it as a variant library): rocprofv3 --pmc runs one
    // kernel at a time, which the grid and its solving wave — two kernels that talk to each other — do not survive.
    // Here the solving wave is one more workgroup of THIS grid (its path spills under the search's register budget:
    // the twin is for bytes and instruction counts, not for time).
    if (blockIdx.x == gridDim.x - 1u) {
        if (threadIdx.x >= 64u) return;
        SolveLds &m = *reinterpret_cast<SolveLds *>(smem);
        const int lane = static_cast<int>(threadIdx.x & 63u);
        if (lane < 14) m.T[lane] = lane < 7 ? L.T0[lane] : (lane == 10 ? 1.0 : 0.0);
        __builtin_amdgcn_wave_barrier();
        P2pParams X{};
        X.nranks = 1;
        unsigned long long xg = 0ull;
        for (int it = 0;; ++it)
            if (loop_finish_iteration<kLoopReplicas>(L, X, m, it, xg)) return;
    }
#endif

    // ---- the units (of QW queries) this workgroup owns for the whole call ----------------------------
    // Workgroup b is dispatched to XCD b % 8 (observed; speed only).  Striped: XCD x serves the stripes
    // x, x + 8, ... of kLoopStripe workgroups' worth of the spatially sorted frame (every XCD gets the
    // same mix of dense and sparse regions, every L2 sees the whole map).  Contiguous: XCD x serves the
    // units [xcd_first[x], xcd_first[x + 1]) — one compact region of the map per L2, the boundaries
    // chosen by the host so that the XCDs hold equal work.
    // Either way the units are dealt out EVENLY over the workgroups that serve them — floor or ceil of
    // units / workgroups each, never more than gpw: a frame of 7,500 units on 1,664 resident workgroups
    // of four waves gives 844 of them a fifth unit instead of leaving 200 with none.
    unsigned g0, gcnt;
    {
        const unsigned xcd = blockIdx.x & 7u, jb = blockIdx.x >> 3;
        const unsigned ngroups = (static_cast<unsigned>(P.n) + QW - 1u) / QW;
        unsigned lo = 0u, cnt = ngroups, idx, nwg;
        if (L.contiguous == 1) {
            lo = L.xcd_first[xcd];
            cnt = L.xcd_first[xcd + 1u] - lo;
            idx = jb;
            nwg = static_cast<unsigned>(L.wgs) >> 3;
        } else {
            idx = ((jb / kLoopStripe) * 8u + xcd) * kLoopStripe + (jb % kLoopStripe);
            nwg = static_cast<unsigned>(L.wgs);
        }
        const unsigned base = cnt / nwg, extra = cnt - base * nwg;      // `extra` workgroups serve base + 1 groups
        g0 = lo + idx * base + min(idx, extra);
        gcnt = min(gpw, base + (idx < extra ? 1u : 0u));
    }
    unsigned long long *wgacc = reinterpret_cast<unsigned long long *>(smem + kLpAcc);
    // LDS after the header: perm[gpw * QW / 4] | work[gpw * QW / 4] | rows of the workgroup's queries | their state
    // records | one scratch for the transposed block sums per wave
    constexpr unsigned BPW = QW / 4;                                  // blocks of four queries per pass
    const unsigned nblk_max = gpw * BPW, nblk = gcnt * BPW;
    uint32_t *perm = smem + kLpHeaderWords;
    uint32_t *work = perm + loop_perm_words(nblk_max) / 2u;
    uint32_t *rows = perm + loop_perm_words(nblk_max);
    uint32_t *state = rows + gpw * QW * kRowLdsStride;
    double *red = reinterpret_cast<double *>(state + gpw * QW * kLoopStateWords + static_cast<unsigned>(wv) * loop_red_words());

    // ---- set-up: the initial pose, the state records of the groups' queries --------------------------
    if (threadIdx.x < 9) s_pose[threadIdx.x] = P.st->R[threadIdx.x];
    else if (threadIdx.x < 12) s_pose[threadIdx.x] = P.st->T[4 + threadIdx.x - 9];
    if (threadIdx.x == 0) {
        smem[kLpArrive] = 0u;
        smem[kLpNext] = 0u;
        smem[kLpDone] = 0u;
#ifdef SAGE_LOOP_TIMING
        smem[kLpDbg] = 0u; smem[kLpDbg + 1] = 0u; smem[kLpDbg + 2] = 0u;
#endif
    }
    if (L.deal && (threadIdx.x & 63u) == 0u) {
        // The heaviest unit of a workgroup (its blocks are ordered by work) should not meet the heaviest units of the
        // other workgroups of its CU on one SIMD: a workgroup's four waves sit on the four SIMDs, one wave of every
        // workgroup of the CU per SIMD, and a SIMD's issue slots are what its waves share.  Workgroup r of the CU
        // (its waves' slot number) hands unit (s + r) mod waves to its wave on SIMD s: every SIMD gets the same mix.
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        smem[kLpFirst + static_cast<unsigned>(wv)] = (((hw >> 4) & 3u) + (hw & 15u)) % static_cast<unsigned>(nw);
    }
    for (unsigned i = threadIdx.x; i < 2u * kWgAccWords; i += blockDim.x) smem[kLpAcc + i] = 0u;
    for (unsigned i = threadIdx.x; i < nblk_max; i += blockDim.x) {
        perm[i] = i;                           // the order of the frame, until the blocks' work is known
        work[i] = 0u;
    }
    for (unsigned sl = threadIdx.x; sl < gcnt * QW; sl += blockDim.x) {
        const unsigned q = g0 * QW + sl;       // slot sl of this workgroup
        const Point4 f = P.frame[q < static_cast<unsigned>(P.n) ? q : 0u];
        {
            uint32_t *lst = state + sl * kLoopStateWords;
            *reinterpret_cast<Point4 *>(lst) = f;
            Point4 z;
            z.x = z.y = z.z = z.l = 0.0;
            *reinterpret_cast<Point4 *>(lst + 8) = z;
            *reinterpret_cast<uint4 *>(lst + kStPrev) = make_uint4(0xFFFFFFFFu, 0u, static_cast<uint32_t>(kNoVoxel),
                                                                   static_cast<uint32_t>(kNoVoxel));   // no answer, no row yet:
            *reinterpret_cast<uint4 *>(lst + kStPrev + 4) = make_uint4(static_cast<uint32_t>(kNoVoxel), 0u, 0u, 0u);   // the first pass builds it
        }
    }
    __syncthreads();
    if (L.deal) {
        // (two waves of a workgroup on one SIMD would ask for the same unit: the first keeps it, the others take what is
        // left — every wave derives the same table, wave 0 stores it)
        unsigned claimed = 0u, kept = 0u, table[kLoopMaxWaves];
        for (int w2 = 0; w2 < nw; ++w2) {
            const unsigned pr = smem[kLpFirst + static_cast<unsigned>(w2)];
            table[w2] = pr;
            if (!((claimed >> pr) & 1u)) { claimed |= 1u << pr; kept |= 1u << w2; }
        }
        for (int w2 = 0; w2 < nw; ++w2)
            if (!((kept >> w2) & 1u)) {
                const unsigned pr = static_cast<unsigned>(__builtin_ctz(~claimed));
                table[w2] = pr;
                claimed |= 1u << pr;
            }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w2 = 0; w2 < nw; ++w2) smem[kLpFirst + static_cast<unsigned>(w2)] = table[w2];
            smem[kLpNext] = static_cast<unsigned>(nw);
        }
        __syncthreads();
    }
#ifdef SAGE_LOOP_TIMING
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long t_wait = 0, t_close = 0, n_pass = 0;
#endif

    for (int it = 0;; ++it) {
        // Every iteration (and every pass of the body) re-reads its arguments from the kernel-argument
        // segment — scalar loads from the constant cache, as a wave of k_icp does at its start — and
        // re-derives its lane index: values the compiler knows to be invariant across this loop it would
        // hoist out of it and keep alive, ~50 scalars and a dozen vector registers the scan needs.
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const LoopArgs &K = *(const LoopArgs *)(ka);
        const LoopParams &L = K.L;
        LoopShared *sh = L.sh;
        unsigned lane_u;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_u));
        const int lane = static_cast<int>(lane_u);
        // the workgroup's groups, first come first served: a wave held up by a heavy query takes fewer
        bool dealt = L.deal != 0;
        for (;;) {
            unsigned gi = 0u;
            if (dealt) {
                // (this wave's first unit is fixed by where it sits; the units beyond one per wave go first come first served)
                dealt = false;
                gi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(smem[kLpFirst + static_cast<unsigned>(wv)])));
                if (gi >= gcnt) continue;
            } else {
                if (lane == 0)
                    gi = __hip_atomic_fetch_add(&smem[kLpNext], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                gi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(gi)));
                if (gi >= gcnt) break;
            }
            if (L.prio) {
                // A SIMD's issue slots go to its waves by priority: the wave with the heaviest unit of its workgroup (the
                // units are ordered by last iteration's work) runs at the highest, the lightest at the lowest, a unit beyond
                // one per wave — it starts late — at `prio` (3 by default).  The work of a SIMD does not change with the order, but
                // its END does: the long chains run while there is other work to fill their stalls with, and what
                // is left to run alone at the end of an iteration are the short ones (c2: 31.2 -> 28.2 us per iteration,
                // profiles/r06/deal_ab.txt).
                const unsigned rk = gi >= static_cast<unsigned>(nw) ? static_cast<unsigned>(L.prio) : 3u - min(gi, 3u);
                switch (rk) {
                    case 0: __builtin_amdgcn_s_setprio(0); break;
                    case 1: __builtin_amdgcn_s_setprio(1); break;
                    case 2: __builtin_amdgcn_s_setprio(2); break;
                    default: __builtin_amdgcn_s_setprio(3); break;
                }
            }
#ifdef SAGE_LOOP_TIMING
            if (gi >= static_cast<unsigned>(nw)) LOOP_STAMP_WG(it, 2);
            const unsigned long long t_unit = __builtin_amdgcn_s_memrealtime();
#endif
            LoopGroup G;
            G.rows = rows;
            G.state = state;
            G.perm = perm;
            G.work = work;
            G.unit = gi;
            G.red = red;
            G.wgacc = wgacc;
            G.q_first = g0 * QW;
            G.slot = g0 + gi;
#ifdef SAGE_LOOP_TIMING
            for (int i = 0; i < 8; ++i) G.ph[i] = 0;
            G.tprev = __builtin_amdgcn_s_memtime();
            ++n_pass;
#endif
            {
                auto kb = __builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(kb));
                icp_body<LW, true, FILT, true>(((const LoopArgs *)(kb))->P, smem, &G, s_pose);
            }
#ifdef SAGE_LOOP_TIMING
            if (gi >= static_cast<unsigned>(nw)) LOOP_STAMP_WG(it, 3);
            if (it < kLoopTimedIters && blockIdx.x < kLoopTimedWgs && lane == 0 && wv < 8 && gi < static_cast<unsigned>(nw)) {
                unsigned hw;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                g_loop_wave[it][blockIdx.x][wv][0] = __builtin_amdgcn_s_memrealtime();
                g_loop_wave[it][blockIdx.x][wv][1] = (t_unit << 24) | (static_cast<unsigned long long>(gi & 0xFFu) << 16) | (hw & 0xFFFFu);
            }
#endif
#ifdef SAGE_LOOP_TIMING
            for (int i = 0; i < 8; ++i) ph[i] += G.ph[i];
#endif
        }
#ifdef SAGE_LOOP_TIMING
        const unsigned long long t_a = __builtin_amdgcn_s_memtime();
#endif
        // (what the ticket orders — the groups' sums — lives in LDS, which serves a CU's waves in order)
        unsigned prior = 0u;
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if (lane == 0)
            prior = __hip_atomic_fetch_add(&smem[kLpArrive], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        prior = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(prior)));
        const bool last = prior == static_cast<unsigned>(nw) - 1u;
        if (last) {
            // this wave closes the workgroup's iteration
            wgacc_flush<true>(wgacc, &sh->acc[it & 1][blockIdx.x & (kLoopReplicas - 1)][0], &sh->acc[it & 1][0][kAccWords - 1]);
            if (lane == 0) {                   // everybody is in: ready for the next iteration
                smem[kLpArrive] = 0u;
                smem[kLpNext] = L.deal ? static_cast<unsigned>(nw) : 0u;
            }
            // The next iteration's order of the workgroup's blocks: heaviest first, by what they cost in this one (a
            // rank sort on one wave: lane i counts the blocks that go before block i).  Blocks of like work then
            // share a wave — whose pass lasts as long as its heaviest query — and the heaviest waves start first.
            // (Which blocks share a wave does not reach the sums: they are exact from the block on.)
            if (nblk <= 64u && nblk > BPW) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                const unsigned i = static_cast<unsigned>(lane);
                const unsigned wi = i < nblk ? work[i] : 0u;
                unsigned rank = 0u;
                for (unsigned j = 0; j < nblk; ++j) {
                    const unsigned wj = work[j];
                    rank += (wj > wi || (wj == wi && j < i)) ? 1u : 0u;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (i < nblk) {
                    perm[rank] = i;
                    work[i] = 0u;
                }
            }
#ifdef SAGE_LOOP_TIMING
            if (lane == 0 && it < kLoopTimedIters && blockIdx.x < kLoopTimedWgs) {
                unsigned hw;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                unsigned xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                unsigned *o = g_loop_wginfo[it][blockIdx.x];
                o[0] = (xcc << 28) | (hw & 0x0FFFFFFFu);
                o[1] = smem[kLpDbg]; o[2] = smem[kLpDbg + 1]; o[3] = smem[kLpDbg + 2];
                smem[kLpDbg] = 0u; smem[kLpDbg + 1] = 0u; smem[kLpDbg + 2] = 0u;
            }
#endif
            LOOP_STAMP_WG(it, 0);
        }
        if (wv == 0) {
            // the next pose, for this workgroup
            const unsigned long long tag = static_cast<unsigned long long>(it) + 1ull;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
            unsigned long long g = tag << 32;
            bool aborted = false;
            for (;;) {
                if (lane < kLoopPoseGranules) g = ld_agent(&sh->pose[loop_pose_copy(L.pose_map)][lane]);
                const bool ok = (g >> 32) == tag;
                if (__all(ok)) break;
                unsigned long long ab = 0ull;
                if (lane == 0) ab = ld_agent(&sh->abort_word[0]);
                const bool late = __builtin_amdgcn_s_memrealtime() - t0 > L.timeout_ticks;
                if (__any(ab != 0ull) || late) {
                    if (lane == 0 && late) {
                        st_agent(&sh->abort_word[0], 1ull);
                        L.st->loop_aborted = 1;
                    }
                    aborted = true;
                    break;
                }
                // (more than a thousand workgroups wait here for most of an iteration — since the pose has a copy per
                // XCD, some two hundred per copy, on four cache lines of their own: a pass every ~0.3 us each keeps
                // the L2 that serves them, and the accumulators the solving wave is reading, quiet)
                __builtin_amdgcn_s_sleep(SAGE_LOOP_POLL_SLEEP);
                // (a big grid backs off twice as long: c2's 1,664 workgroups 30.7 -> 30.3 us per iteration, flat from there
                // to six times as long; c1's 640 prefer the short one — same-box A/B, profiles/r05/poll_sleep.txt, taken
                // when all of them polled ONE block; with a copy per XCD: profiles/r15/README.md)
                if (L.wgs > 1024) __builtin_amdgcn_s_sleep(SAGE_LOOP_POLL_SLEEP);
            }
            if (aborted) {
                if (lane == 0) smem[kLpDone] = 2u;
            } else {
                if (lane < 24) reinterpret_cast<uint32_t *>(s_pose)[lane] = static_cast<uint32_t>(g);
                if (lane == 24) smem[kLpDone] = static_cast<uint32_t>(g);
            }
            LOOP_STAMP_WG(it, 1);
        }
#ifdef SAGE_LOOP_TIMING
        const unsigned long long t_b = __builtin_amdgcn_s_memtime();
        if (last) t_close += t_b - t_a;
#endif
        __syncthreads();
#ifdef SAGE_LOOP_TIMING
        t_wait += __builtin_amdgcn_s_memtime() - t_b;
#endif
        if (smem[kLpDone]) break;
    }
#ifdef SAGE_LOOP_TIMING
    if ((threadIdx.x & 63u) == 0u) {
        for (int i = 0; i < 8; ++i) atomicAdd(&g_loop_phase[i], ph[i]);
        atomicAdd(&g_loop_phase[8], t_wait);
        atomicAdd(&g_loop_phase[9], t_close);
        atomicAdd(&g_loop_phase[10], n_pass);
    }
#endif
}

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

#ifdef SAGE_GN_TIMING
extern "C" void sageicp_debug_gn_phases(unsigned long long out[16], int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gn_phase), sizeof(unsigned long long) * 16);
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_gn_phase), z, sizeof(z));
    }
}
#endif
#ifdef SAGE_NN_TIMING
extern "C" void sageicp_debug_nn_spans(unsigned long long *out, unsigned nwaves, int next_iter) {
    // raw {start, end, HW_ID, pairs of lane 0} of the first `nwaves` waves of the k_icp launch of
    // the iteration chosen by the previous call; `next_iter` chooses the one the next loop records
    if (nwaves > kNnTimingSlots) nwaves = kNnTimingSlots;
    if (out) (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_span), 4ull * nwaves * sizeof(unsigned long long));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_nn_span_iter), &next_iter, sizeof(int));
}
extern "C" void sageicp_debug_nn_raw(unsigned long long *out, unsigned nwaves) {
    // per wave slot, summed over the launches since the last reset: 5 phases and the lifetime
    // (shader cycles), the lifetime in 100-MHz ticks, launches
    if (nwaves > kNnTimingSlots) nwaves = kNnTimingSlots;
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_phase), 8ull * nwaves * sizeof(unsigned long long));
}
extern "C" void sageicp_debug_nn_phases(unsigned long long out[16], int reset) {
    // out: [0..4] summed cycles of the five phases (loads, row, home scan, rest of the search,
    // epilogue), [5] summed wave lifetime (shader cycles), [6] the same in 100-MHz ticks, [7] waves,
    // [8] the slowest wave slot's mean lifetime (cycles), [9] slots used
    std::vector<unsigned long long> h(8ull * kNnTimingSlots);
    (void)hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_nn_phase), h.size() * sizeof(unsigned long long));
    for (int i = 0; i < 16; ++i) out[i] = 0;
    for (unsigned s = 0; s < kNnTimingSlots; ++s) {
        const unsigned long long *t = &h[8ull * s];
        if (!t[7]) continue;
        for (int k = 0; k < 8; ++k) out[k] += t[k];
        if (t[5] / t[7] > out[8]) out[8] = t[5] / t[7];
        ++out[9];
    }
    if (reset) {
        std::fill(h.begin(), h.end(), 0ull);
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_nn_phase), h.data(), h.size() * sizeof(unsigned long long));
    }
}
#endif

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
    return sizeof(uint32_t) * (kLpHeaderWords + loop_perm_words(static_cast<unsigned>(gpw) * ((64u >> lw) / 4u)) +
                               static_cast<size_t>(gpw) * loop_group_words(lw) + static_cast<size_t>(nw) * loop_red_words());
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
