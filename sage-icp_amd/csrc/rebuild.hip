// The device side of a session rebuild (gfx950) — see rebuild.h, rebuild_rule.h and DESIGN.md D21.
//
//   k_rb_move -> radix_sort_pairs -> k_rb_heads -> select -> k_rb_resolve -> exclusive_scan -> k_rb_totals | k_rb_fill
//
// The far test is the eviction test of map_update.hip's k_far_flags and HostMap::remove_far, same expression and
// association, on the run's final first stored row; radius^2 is formed once on the host, as max_dist2 is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "rebuild.h"
#include "se3_math.h"

namespace sageicp {

namespace {

constexpr unsigned kMoveBlocks = 1024;       // the move's launch: rows beyond 1024 x 256 are reached by striding
constexpr unsigned kResolveBlocks = 2048;    // the resolve's: runs beyond 2048 x (256 / kGroup) likewise
constexpr unsigned kFillBlocks = 2048;       // the fill's: positions beyond 2048 x 256 likewise
constexpr int kGroup = 16;                   // lanes that resolve one run together (divides 64)
constexpr int kKeyBias = 1 << 20;
constexpr unsigned long long kPadKey = ~0ull;         // (no packed voxel key has bit 63 set)

// (k_up_keys' packing: runs come out in the order the update's would)
__device__ __forceinline__ unsigned long long pack_key(int x, int y, int z) {
    return (static_cast<unsigned long long>(static_cast<uint32_t>(x + kKeyBias)) << 42) |
           (static_cast<unsigned long long>(static_cast<uint32_t>(y + kKeyBias)) << 21) |
           static_cast<unsigned long long>(static_cast<uint32_t>(z + kKeyBias));
}
__device__ __forceinline__ void unpack_key(unsigned long long k, int &x, int &y, int &z) {
    x = static_cast<int>((k >> 42) & 0x1FFFFFull) - kKeyBias;
    y = static_cast<int>((k >> 21) & 0x1FFFFFull) - kKeyBias;
    z = static_cast<int>(k & 0x1FFFFFull) - kKeyBias;
}

struct NeedPlus {
    __host__ __device__ RebuildNeed operator()(const RebuildNeed &a, const RebuildNeed &b) const {
        RebuildNeed r;
        r.voxels = a.voxels + b.voxels;
        r.rows = a.rows + b.rows;
        r.built_rows = a.built_rows + b.built_rows;
        r.units = a.units + b.units;
        if (r.units < a.units || a.units == 0xFFFFFFFFu || b.units == 0xFFFFFFFFu) r.units = 0xFFFFFFFFu;
        return r;
    }
};

// the smallest size class that holds `count` points (the last one holds a full voxel)
__device__ __forceinline__ uint32_t class_of(const DevMap &M, uint32_t count) {
    uint32_t k = 0;
    while (k + 1 < static_cast<uint32_t>(M.n_classes) && count > M.class_points[k]) ++k;
    return k;
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

// the selected voxels and the rows of a part (0 for one without candidates)
__device__ __forceinline__ uint32_t part_voxels(const ClosurePart &C) { return C.P.n_cand ? min(*C.P.n_sel, C.P.n_cand) : 0u; }
__device__ __forceinline__ uint32_t part_rows(const ClosurePart &C) { return C.P.n_cand ? C.off[C.P.n_cand] : 0u; }

// Lane per position r < n of the export's order: row r of the selection moved as k_cl_move moves it (the same
// expressions, so the same bytes), keyed by the voxel of the moved row (k_up_keys: fp64 divide, truncation).  Positions
// from the selection's rows on are padding.
__global__ __launch_bounds__(256) void k_rb_move(ClosurePart A, ClosurePart B, const double *__restrict__ corrections,
                                                 RebuildPolicy pol, RebuildScratch S, uint32_t n) {
    const uint32_t ra = part_rows(A), rb = part_rows(B);
    const uint32_t total = min(n, ra + rb);
    if (blockIdx.x == 0 && threadIdx.x == 0) *S.n_rows = total;
    for (uint64_t r64 = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; r64 < n; r64 += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint32_t r = static_cast<uint32_t>(r64);
        S.idx[r] = r;
        unsigned long long key = kPadKey;
        if (r < total) {
            const bool first = r < ra;
            const ClosurePart &C = first ? A : B;
            const RecallPart &P = C.P;
            const uint32_t lr = first ? r : r - ra;
            const uint32_t nv = part_voxels(C);
            Cand c;
            uint32_t j = 0, k = 0;
            bool ok = nv > 0;
            if (ok) {
                j = voxel_of_row(C.off, nv, lr);
                ok = cand_of(P, P.sel[j], c);
                k = lr - C.off[j];
                ok = ok && k < c.count;
            }
            Point4 p{0.0, 0.0, 0.0, 0.0};
            if (ok) {
                const double *T = corrections + 7 * static_cast<size_t>(C.stay[j]);
                const double q[4] = {T[0], T[1], T[2], T[3]}, t[3] = {T[4], T[5], T[6]};
                double R[9], o[3];
                quat_to_mat(q, R);
                p = P.rows[c.first + k];
                const double v[3] = {p.x, p.y, p.z};
                mat_apply(R, t, v, o);
                p.x = o[0]; p.y = o[1]; p.z = o[2];
            }
            S.moved[r] = p;
            S.code[r] = static_cast<uint8_t>(rule_code(static_cast<int>(p.l), pol.labels, pol.n_labels));
            const int vx = static_cast<int>(p.x / pol.voxel_size);
            const int vy = static_cast<int>(p.y / pol.voxel_size);
            const int vz = static_cast<int>(p.z / pol.voxel_size);
            const int lim = kKeyBias - 1;
            if (!(fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308 && fabs(p.z) <= 1.7976931348623157e308))
                atomicOr(S.flags, 2u);
            else if (vx < -lim || vx > lim || vy < -lim || vy > lim || vz < -lim || vz > lim) atomicOr(S.flags, 1u);
            key = pack_key(vx, vy, vz) & 0x7FFFFFFFFFFFFFFFull;      // (a refused call's key may be anything below the padding)
        }
        S.keys[r] = key;
    }
}

__global__ __launch_bounds__(256) void k_rb_heads(RebuildScratch S, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    S.head_flag[i] = (i < *S.n_rows && (i == 0 || S.keys_alt[i] != S.keys_alt[i - 1])) ? 1u : 0u;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int o = 32; o; o >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o)));
    return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

// A group of G lanes per run; the 64 / G groups of a wave step together (every loop bound is the wave's, every lane
// takes part in every ballot and shuffle, and a group reads only its own G bits).  Step: G arrivals; carried: K (critical
// later arrivals), R (replacers), Z (rebuild_rule.h) and the arrival index of the first replacer.
template <int G>
__global__ __launch_bounds__(256) void k_rb_resolve(RebuildScratch S, RebuildPolicy pol, DevMap M, bool crop, double cx, double cy,
                                                    double cz, double radius2) {
    static_assert(64 % G == 0, "a group is a part of one wave");
    constexpr uint32_t kPerBlock = 256 / G;
    constexpr unsigned long long kMask = G == 64 ? ~0ull : (1ull << (G % 64)) - 1ull;
    const RulePolicy rp = rule_policy(pol.basic, pol.critical);
    const uint32_t n_runs = *S.n_runs, n_rows = *S.n_rows;
    const uint32_t lane = threadIdx.x & 63u, gl = lane % G, gbase = lane - gl;
    const uint32_t wave_group0 = (threadIdx.x - lane) / G;         // the wave's first group within the block
    const unsigned long long below = (1ull << gl) - 1ull;
    for (uint64_t w0 = static_cast<uint64_t>(blockIdx.x) * kPerBlock + wave_group0; w0 < n_runs;
         w0 += static_cast<uint64_t>(gridDim.x) * kPerBlock) {
        const uint64_t r64 = w0 + gbase / G;
        const bool valid = r64 < n_runs;
        const uint32_t r = static_cast<uint32_t>(r64);
        uint32_t start = 0, L = 0;
        if (valid) {
            start = S.run_start[r];
            const uint32_t end = r + 1 < n_runs ? S.run_start[r + 1] : n_rows;
            L = end > start ? end - start : 0u;
        }
        const uint32_t maxL = wave_max(L);
        uint32_t K = 0, R = 0, first_repl = 0;
        RuleZ z;
        rule_z_clear(z);
        for (uint32_t at = 0; at < maxL; at += G) {
            const uint32_t p = at + gl;
            const bool act = valid && p < L;
            uint32_t a = 0;
            int code = kRuleUnlabelled;
            if (act) {
                a = S.idx_alt[start + p];
                code = S.code[a];
            }
            const unsigned long long bz = (__ballot(act && p < rp.P1 && code == kRuleUnlabelled) >> gbase) & kMask;
            if (at < 256) rule_z_or(z, at >> 6, at & 63u, bz);
            const unsigned long long bc = (__ballot(act && p >= rp.P1 && code == kRuleCritical) >> gbase) & kMask;
            const uint32_t k = K + static_cast<uint32_t>(__popcll(bc & below));
            const int kind = act ? rule_kind(rp, p, code, k) : kRuleDrop;
            const unsigned long long br = (__ballot(kind == kRuleReplace) >> gbase) & kMask;
            const uint32_t m = R + static_cast<uint32_t>(__popcll(br & below));
            // the first replacer's arrival index, to every lane of its group
            const int src = br ? __ffsll(static_cast<long long>(br)) - 1 : 0;
            const uint32_t a_first = static_cast<uint32_t>(__shfl(static_cast<int>(a), static_cast<int>(gbase) + src, 64));
            if (R == 0 && br) first_repl = a_first;
            if (act) {
                S.pos_run[start + p] = r;
                if (kind != kRuleFirst) S.pos_slot[start + p] = static_cast<uint8_t>(rule_later_slot(rp, kind, k, m, z));
            }
            K += static_cast<uint32_t>(__popcll(bc));
            R += static_cast<uint32_t>(__popcll(br));
        }
        // the arrivals below P1, now that the replacers are counted
        const uint32_t maxF = min(maxL, rp.P1);
        for (uint32_t at = 0; at < maxF; at += G) {
            const uint32_t p = at + gl;
            if (valid && p < L && p < rp.P1) {
                const int code = S.code[S.idx_alt[start + p]];
                S.pos_slot[start + p] = static_cast<uint8_t>(rule_first_slot(p, code, R, z));
            }
        }
        if (valid && gl == 0 && L > 0) {
            const uint32_t head = S.idx_alt[start];
            const uint32_t count = rule_final_count(rp, L, K), zeros = rule_final_zeros(R, z);
            uint32_t keep = 1;
            if (crop) {
                const Point4 q = S.moved[rule_slot0_replaced(R, z) ? first_repl : head];
                const double dx = q.x - cx, dy = q.y - cy, dz = q.z - cz;
                keep = (SAGE_SQNORM3_FAR(dx * dx, dy * dy, dz * dz) > radius2) ? 0u : 1u;
            }
            S.runs[r] = RebuildRun{head, count | (zeros << 8) | (keep << 31)};
            RebuildNeed nd{0u, 0u, 0u, count};
            if (keep) {
                nd.voxels = 1u;
                nd.rows = count;
                nd.units = M.class_points[class_of(M, count)] / kDevUnitPoints;
            }
            S.need[head] = nd;
        }
    }
}

__global__ void k_rb_totals(ClosurePart A, ClosurePart B, RebuildScratch S, uint32_t n) {
    if (threadIdx.x || blockIdx.x) return;
    RebuildTotals t{};
    t.flags = *S.flags;
    t.session_voxels = part_voxels(A) + part_voxels(B);
    t.session_rows = *S.n_rows;
    t.built_voxels = *S.n_runs;
    const RebuildNeed total = S.rank[n];
    t.built_rows = total.built_rows;
    t.voxels = total.voxels;
    t.units = total.units;
    t.rows = total.rows;
    *S.totals = t;
}

// one 32-byte row as two 16-byte accesses
__device__ __forceinline__ void copy_row(Point4 *dst, const Point4 *src) {
    const double2 a = reinterpret_cast<const double2 *>(src)[0];
    const double2 b = reinterpret_cast<const double2 *>(src)[1];
    reinterpret_cast<double2 *>(dst)[0] = a;
    reinterpret_cast<double2 *>(dst)[1] = b;
}

// Lane per sorted position: the row into its slot of its run's region; the lane of a run's first position also writes
// what the update pass writes for a new voxel.  Nothing is written at or beyond block_end / unit_end (what the host reserved).
__global__ __launch_bounds__(256) void k_rb_fill(RebuildScratch S, DevMap M, uint32_t n, uint32_t block_end, uint32_t unit_end) {
    const uint32_t n_rows = min(*S.n_rows, n), n_runs = *S.n_runs;
    for (uint64_t i64 = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; i64 < n_rows; i64 += static_cast<uint64_t>(gridDim.x) * 256) {
        const uint32_t i = static_cast<uint32_t>(i64);
        const uint32_t r = S.pos_run[i];
        if (r >= n_runs) continue;
        const RebuildRun run = S.runs[r];
        if (!(run.word >> 31) || run.head >= n) continue;
        const RebuildNeed at = S.rank[run.head];
        const uint32_t count = run.word & 255u, cls = class_of(M, count);
        const uint32_t b = at.voxels, unit = at.units;
        if (b >= block_end || unit >= unit_end || M.class_points[cls] / kDevUnitPoints > unit_end - unit) continue;
        const uint32_t slot = S.pos_slot[i];
        if (slot < count && slot < M.class_points[cls])
            copy_row(M.pts + static_cast<size_t>(unit) * kDevUnitPoints + slot, S.moved + S.idx_alt[i]);
        if (i == S.run_start[r]) {
            int vx, vy, vz;
            unpack_key(S.keys_alt[i], vx, vy, vz);
            M.regions[b] = (cls << 28) | unit;
            M.block_of[unit] = b;
            M.zeros[b] = static_cast<uint8_t>((run.word >> 8) & 255u);
            const uint32_t word = (unit << 8) | count;
            uint32_t s = voxel_hash(vx, vy, vz) & M.mask;
            for (;;) {           // (the table is at most a quarter full: the chain ends)
                if (atomicCAS(&M.table[s].blk, kEmptySlot, word) == kEmptySlot) break;
                s = (s + 1) & M.mask;
            }
            M.table[s].x = vx;
            M.table[s].y = vy;
            M.table[s].z = vz;
            M.slot_of[b] = s;
        }
    }
}

}  // namespace

size_t rebuild_temp_bytes(size_t n) {
    size_t a = 0, b = 0, c = 0;
    unsigned long long *k = nullptr;
    uint32_t *v = nullptr;
    RebuildNeed *nd = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, k, k, v, v, n, 0, 64);
    (void)rocprim::select(nullptr, b, rocprim::counting_iterator<uint32_t>(0), v, v, v, n);
    (void)rocprim::exclusive_scan(nullptr, c, nd, nd, RebuildNeed{0u, 0u, 0u, 0u}, n + 1, NeedPlus());
    return std::max(a, std::max(b, c)) + 256;
}

hipError_t rebuild_resolve(const ClosurePart part[2], const double *corrections, const RebuildPolicy &pol, const DevMap &M,
                           const double *center, double radius2, const RebuildScratch &S, uint32_t n, hipStream_t s) {
    hipError_t e;
    if ((e = hipMemsetAsync(S.flags, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(S.n_runs, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(S.n_rows, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(S.rank, 0, sizeof(RebuildNeed), s)) != hipSuccess) return e;     // (n == 0: rank[0] is the totals)
    if (n) {
        if ((e = hipMemsetAsync(S.need, 0, (static_cast<size_t>(n) + 1) * sizeof(RebuildNeed), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(S.pos_run, 0xFF, static_cast<size_t>(n) * sizeof(uint32_t), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(S.pos_slot, 0xFF, static_cast<size_t>(n), s)) != hipSuccess) return e;
        const uint64_t blocks = (static_cast<uint64_t>(n) + 255) / 256;
        hipLaunchKernelGGL(k_rb_move, dim3(static_cast<unsigned>(std::min<uint64_t>(kMoveBlocks, blocks))), dim3(256), 0, s, part[0],
                           part[1], corrections, pol, S, n);
        size_t tb = S.temp_bytes;
        e = rocprim::radix_sort_pairs(S.temp, tb, S.keys, S.keys_alt, S.idx, S.idx_alt, static_cast<size_t>(n), 0, 64, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rb_heads, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, S, n);
        tb = S.temp_bytes;
        e = rocprim::select(S.temp, tb, rocprim::counting_iterator<uint32_t>(0), S.head_flag, S.run_start, S.n_runs,
                            static_cast<size_t>(n), s);
        if (e != hipSuccess) return e;
        const uint64_t gblocks = (static_cast<uint64_t>(n) + (256 / kGroup) - 1) / (256 / kGroup);       // (at most n runs)
        hipLaunchKernelGGL(k_rb_resolve<kGroup>, dim3(static_cast<unsigned>(std::min<uint64_t>(kResolveBlocks, gblocks))), dim3(256), 0,
                           s, S, pol, M, center != nullptr, center ? center[0] : 0.0, center ? center[1] : 0.0,
                           center ? center[2] : 0.0, radius2);
        tb = S.temp_bytes;
        e = rocprim::exclusive_scan(S.temp, tb, S.need, S.rank, RebuildNeed{0u, 0u, 0u, 0u}, static_cast<size_t>(n) + 1, NeedPlus(), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_rb_totals, dim3(1), dim3(64), 0, s, part[0], part[1], S, n);
    return hipGetLastError();
}

hipError_t rebuild_fill(const RebuildScratch &S, uint32_t n, const DevMap &M, uint32_t block_end, uint32_t unit_end, hipStream_t s) {
    if (n == 0 || block_end == 0) return hipSuccess;
    const uint64_t blocks = (static_cast<uint64_t>(n) + 255) / 256;
    hipLaunchKernelGGL(k_rb_fill, dim3(static_cast<unsigned>(std::min<uint64_t>(kFillBlocks, blocks))), dim3(256), 0, s, S, M, n,
                       block_end, unit_end);
    return hipGetLastError();
}

}  // namespace sageicp
