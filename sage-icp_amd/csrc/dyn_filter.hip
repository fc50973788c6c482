// The dynamic vehicle filter of Preprocess() on the device: core/Preprocessing.cpp:95-172.
// The reference crops the frame, clusters the vehicle-labelled points (PCL EuclideanClusterExtraction, tolerance
// 0.5 m, at least 5 points) and keeps a cluster only if its points see more than dy_th * size landmark points
// (parking / sidewalk) within 0.5 m — a parked car; every other cluster (a moving car) and every vehicle point of a
// component smaller than 5 is dropped.  Output: the other kept points in frame order, then the kept clusters in PCL's
// cluster order, each in ascending frame order.
//
// Device form (all on the Prep's stream; DynFilter, the buffers, is declared with Prep in prep.h):
//   k_dyn_classify   crop + label zeroing as in the filter-off branch; a flag per point (dropped / inlier / vehicle)
//                    and the landmark points L appended by wave-aggregated atomics (their order does not matter)
//   exclusive scan   inlier and vehicle positions in one 64-bit scan (inliers low 32 bits, vehicles high)
//   k_dyn_compact    inliers straight into the output; vehicle points V (fp32 xyz, frame index, 0.5 m cell key)
//   -- round trip 1: |V| and |L| (the sorts need their sizes) --
//   radix sorts      V and L by packed cell: a neighbour within 0.5 m lies in one of the 27 surrounding cells
//   k_dyn_link       union-find over V: every pair (i < j) with d2 < 0.25f hooks the larger root under the smaller
//                    (atomicCAS), so each root ends as its component's smallest vehicle index — the labelling does
//                    not depend on the schedule, and the walks have bounds that hold under any schedule (find_root)
//   k_dyn_count      compress; per point the L neighbours within radius; size and count per root (integer atomics)
//   k_dyn_records    the components of >= 5 points, in ascending root order = the order PCL finds them
//   -- round trip 2: the per-component table (root, size, count); the host replays PCL's std::sort of the clusters
//      (cluster_emission_order, dyn_rules.h), applies the static test and uploads each kept cluster's offset --
//   k_dyn_scatter    the kept clusters' points behind the inliers (points grouped by root with a stable sort)
//
// Distances follow FLANN's L2_Simple in fp32 on the float copies PCL makes: d2 = (dx*dx + dy*dy) + dz*dz with
// dx = fl(a - b), no FMA (-ffp-contract=off), neighbour iff d2 < 0.25f.
#include <hip/hip_runtime.h>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "capi_internal.h"

namespace sageicp {

namespace {

constexpr int kCellBits = 21;
constexpr long long kCellHalf = 1ll << (kCellBits - 1);   // cells -2^20 .. 2^20 - 1 per axis (|x| < 524288 m)
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct DynParams {
    const Point4 *in;
    int n;
    double max_range, min_range, label_max_range;
    const uint32_t *labels;            // [n_dyn] dynamic labels, then [n_lm] landmark labels
    int n_dyn, n_lm;
    Point4 *tmp;                       // [n] the cropped points, labels zeroed
    unsigned long long *cnt;           // [n] 1: inlier, 1 << 32: vehicle
    const unsigned long long *pos;     // [n] exclusive scan of cnt
    Point4 *out;                       // the filtered cloud
    float4 *vp;                        // [|V|] vehicle points, frame order
    uint32_t *vframe;                  // [|V|] their frame index
    unsigned long long *vkey;          // [|V|] cell key
    uint32_t *vval;                    // [|V|] 0, 1, 2, ...
    float4 *lp;                        // [|L|] landmark points (append order)
    unsigned long long *lkey;
    uint32_t *lval;
    uint32_t *ctr;                     // [0] inliers [1] |V| [2] |L| [3] components of >= 5
    int *ovf;                          // 1: cell index out of range, 2: non-finite label, 4: union-find invariant broken
};

__device__ __forceinline__ bool cell_of(float x, float y, float z, long long c[3]) {
    c[0] = static_cast<long long>(floorf(2.0f * x));
    c[1] = static_cast<long long>(floorf(2.0f * y));
    c[2] = static_cast<long long>(floorf(2.0f * z));
    for (int k = 0; k < 3; ++k)
        if (c[k] < -kCellHalf || c[k] >= kCellHalf) return false;
    return true;
}
__device__ __forceinline__ unsigned long long pack_cell(long long x, long long y, long long z) {
    return (static_cast<unsigned long long>(x + kCellHalf) << (2 * kCellBits)) |
           (static_cast<unsigned long long>(y + kCellHalf) << kCellBits) | static_cast<unsigned long long>(z + kCellHalf);
}

// FLANN L2_Simple on the fp32 copies: ((0 + dx*dx) + dy*dy) + dz*dz (the leading 0 + is exact)
__device__ __forceinline__ float dist2(const float4 &a, const float4 &b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ bool has_label(const uint32_t *l, int cnt, uint32_t v) {
    for (int k = 0; k < cnt; ++k)
        if (l[k] == v) return true;
    return false;
}

__global__ __launch_bounds__(256) void k_dyn_classify(DynParams P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool lm = false;
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned long long key = 0;
    if (i < P.n) {
        Point4 p = P.in[i];
        // Preprocessing.cpp:103-106: the crop of the filter-off branch
        const double norm = sqrt(SAGE_SQNORM3_CROP(p.x * p.x, p.y * p.y, p.z * p.z));
        bool kept = norm < P.max_range && norm > P.min_range;
        if (kept && norm > P.label_max_range) p.l = 0.0;
        if (kept && !(fabs(p.l) <= 1.7976931348623157e308)) {   // a label the reference would cast: undefined
            atomicOr(P.ovf, 2);
            kept = false;
        }
        unsigned long long c = 0;
        if (kept) {
            // :107-111 — static_cast<uint32_t> of the zeroed label as x86 converts it (dyn_rules.h); the int lists
            // compare as unsigned
            const uint32_t lab = label_code(p.l);
            c = has_label(P.labels, P.n_dyn, lab) ? (1ull << 32) : 1ull;
            lm = has_label(P.labels + P.n_dyn, P.n_lm, lab);
            P.tmp[i] = p;
            if (lm) {
                f = make_float4(static_cast<float>(p.x), static_cast<float>(p.y), static_cast<float>(p.z), 0.f);
                long long cc[3];
                if (cell_of(f.x, f.y, f.z, cc)) {
                    key = pack_cell(cc[0], cc[1], cc[2]);
                } else {
                    atomicOr(P.ovf, 1);
                    lm = false;
                }
            }
        }
        P.cnt[i] = c;
    }
    // landmark points: one atomic per wave
    const unsigned long long m = __ballot(lm);
    if (m) {
        const int lane = __lane_id();
        const int leader = __ffsll(static_cast<long long>(m)) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(P.ctr + 2, static_cast<uint32_t>(__popcll(m)));
        base = __shfl(base, leader);
        if (lm) {
            const uint32_t k = base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                                __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
            P.lp[k] = f;
            P.lkey[k] = key;
            P.lval[k] = k;
        }
    }
}

__global__ __launch_bounds__(256) void k_dyn_compact(DynParams P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    const unsigned long long c = P.cnt[i], q = P.pos[i];
    if (c == 1ull) {
        P.out[static_cast<uint32_t>(q)] = P.tmp[i];
    } else if (c) {
        const uint32_t v = static_cast<uint32_t>(q >> 32);
        const Point4 p = P.tmp[i];
        const float4 f = make_float4(static_cast<float>(p.x), static_cast<float>(p.y), static_cast<float>(p.z), 0.f);
        long long cc[3];
        unsigned long long key = 0;
        if (cell_of(f.x, f.y, f.z, cc)) key = pack_cell(cc[0], cc[1], cc[2]);
        else atomicOr(P.ovf, 1);
        P.vp[v] = f;
        P.vframe[v] = static_cast<uint32_t>(i);
        P.vkey[v] = key;
        P.vval[v] = v;
    }
    if (i == P.n - 1) {
        const unsigned long long t = q + c;
        P.ctr[0] = static_cast<uint32_t>(t);
        P.ctr[1] = static_cast<uint32_t>(t >> 32);
    }
}

// sorted copies (coalesced neighbour scans) + union-find state
__global__ __launch_bounds__(256) void k_dyn_gather(const float4 *vp, const uint32_t *vidx, uint32_t nv, float4 *vs,
                                                    const float4 *lp, const uint32_t *lidx, uint32_t nl, float4 *ls,
                                                    uint32_t *parent, uint32_t *size, unsigned long long *count,
                                                    uint32_t *rec_of_root) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p < nv) {
        vs[p] = vp[vidx[p]];
        parent[p] = p;
        size[p] = 0;
        count[p] = 0;
        rec_of_root[p] = kNone;
    }
    if (p < nl) ls[p] = lp[lidx[p]];
}

__device__ __forceinline__ uint32_t ld(const uint32_t *a) {
    return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving (a parent only ever moves to an ancestor, so the plain halving stores are safe next to
// the CAS on roots).  Every parent is smaller than its child: a root is hooked only under a smaller root, and a halving
// store writes an ancestor.  So each step lowers x, and a walk from x < nv ends within nv - 1 steps whatever the other
// threads do; more steps mean the invariant is broken, and the walk stops with `broken` set.
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t x, uint32_t nv, bool &broken) {
    for (uint32_t steps = 0;; ++steps) {
        const uint32_t p = ld(parent + x);
        if (p == x) return p;
        if (steps >= nv) { broken = true; return p; }
        const uint32_t g = ld(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
}

// first index in sorted keys[0, m) whose key is >= k
__device__ __forceinline__ uint32_t lower_bound_key(const unsigned long long *keys, uint32_t m, unsigned long long k) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// calls f(q) for every sorted position q of the 27 cells around cell c (three runs of three consecutive z cells)
template <typename F>
__device__ __forceinline__ void for_neighbour_cells(const unsigned long long *keys, uint32_t m, const long long c[3], F &&f) {
    for (long long dx = -1; dx <= 1; ++dx) {
        const long long x = c[0] + dx;
        if (x < -kCellHalf || x >= kCellHalf) continue;
        for (long long dy = -1; dy <= 1; ++dy) {
            const long long y = c[1] + dy;
            if (y < -kCellHalf || y >= kCellHalf) continue;
            const long long z0 = c[2] > -kCellHalf ? c[2] - 1 : c[2];
            const long long z1 = c[2] + 1 < kCellHalf ? c[2] + 1 : c[2];
            const unsigned long long lo = pack_cell(x, y, z0), hi = pack_cell(x, y, z1);
            for (uint32_t q = lower_bound_key(keys, m, lo); q < m && keys[q] <= hi; ++q) f(q);
        }
    }
}

__global__ __launch_bounds__(256) void k_dyn_link(const float4 *vs, const unsigned long long *vkey_s, const uint32_t *vidx,
                                                  uint32_t nv, uint32_t *parent, int *ovf) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nv) return;
    const float4 a = vs[p];
    const uint32_t i = vidx[p];
    long long c[3];
    cell_of(a.x, a.y, a.z, c);
    bool broken = false;
    for_neighbour_cells(vkey_s, nv, c, [&](uint32_t q) {
        const uint32_t j = vidx[q];
        if (j <= i || broken || !(dist2(a, vs[q]) < 0.25f)) return;
        // unite(i, j): hook the larger root under the smaller.  A failed CAS means that root was just hooked elsewhere
        // and is never a root again, so the retries of one unite fail on distinct roots: fewer than nv of them, as a
        // frame has at most nv - 1 hooks.  Neither bound depends on the schedule; they only catch a broken invariant.
        uint32_t ra = find_root(parent, i, nv, broken), rb = find_root(parent, j, nv, broken);
        for (uint32_t failed = 0; !broken; ++failed) {
            if (ra == rb) return;
            if (ra > rb) { const uint32_t t = ra; ra = rb; rb = t; }
            const uint32_t old = atomicCAS(parent + rb, rb, ra);
            if (old == rb) return;
            if (failed + 1 >= nv) { broken = true; return; }
            rb = find_root(parent, old, nv, broken);
            ra = find_root(parent, ra, nv, broken);
        }
    });
    if (broken) atomicOr(ovf, 4);
}

__global__ __launch_bounds__(256) void k_dyn_count(const float4 *vs, const uint32_t *vidx, uint32_t nv,
                                                   const float4 *ls, const unsigned long long *lkey_s, uint32_t nl,
                                                   uint32_t *parent, uint32_t *root, uint32_t *size,
                                                   unsigned long long *count, int *ovf) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nv) return;
    const uint32_t i = vidx[p];
    bool broken = false;
    const uint32_t r = find_root(parent, i, nv, broken);
    if (broken) atomicOr(ovf, 4);
    root[i] = r;
    // Preprocessing.cpp:139-158: the landmark points of map_all within radius of this vehicle point
    const float4 a = vs[p];
    long long c[3];
    cell_of(a.x, a.y, a.z, c);
    uint32_t k = 0;
    if (nl) for_neighbour_cells(lkey_s, nl, c, [&](uint32_t q) { k += dist2(a, ls[q]) < 0.25f ? 1u : 0u; });
    atomicAdd(size + r, 1u);
    if (k) atomicAdd(count + r, static_cast<unsigned long long>(k));
}

__global__ __launch_bounds__(256) void k_dyn_root_flags(const uint32_t *root, const uint32_t *size, uint32_t nv,
                                                        unsigned long long *flag) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < nv) flag[i] = (root[i] == i && size[i] >= 5u) ? 1ull : 0ull;
}

__global__ __launch_bounds__(256) void k_dyn_records(const unsigned long long *flag, const unsigned long long *pos,
                                                     uint32_t nv, const uint32_t *size, const unsigned long long *count,
                                                     uint4 *rec, uint32_t *rec_of_root, uint32_t *ctr) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const uint32_t k = static_cast<uint32_t>(pos[i]);
    if (flag[i]) {
        const unsigned long long c = count[i];
        rec[k] = make_uint4(i, size[i], static_cast<uint32_t>(c), static_cast<uint32_t>(c >> 32));
        rec_of_root[i] = k;
    }
    if (i == nv - 1) ctr[3] = k + static_cast<uint32_t>(flag[i]);
}

// rkey: the vehicle points' roots after a stable sort, rval their V index: a root's points are one run, in frame order
__global__ __launch_bounds__(256) void k_dyn_starts(const uint32_t *rkey, uint32_t nv, uint32_t *start_of) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p < nv && (p == 0 || rkey[p - 1] != rkey[p])) start_of[rkey[p]] = p;
}

__global__ __launch_bounds__(256) void k_dyn_scatter(const uint32_t *rkey, const uint32_t *rval, uint32_t nv,
                                                     const uint32_t *start_of, const uint32_t *rec_of_root,
                                                     const uint32_t *offset, const uint32_t *vframe, const Point4 *tmp,
                                                     Point4 *out) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nv) return;
    const uint32_t r = rkey[p];
    const uint32_t k = rec_of_root[r];
    if (k == kNone) return;                    // a component of fewer than 5 points
    const uint32_t o = offset[k];
    if (o == kNone) return;                    // a moving vehicle
    out[o + (p - start_of[r])] = tmp[vframe[rval[p]]];
}

inline unsigned grid_of(uint64_t n) { return static_cast<unsigned>((n + 255) / 256); }

}  // namespace

int DynFilter::reserve(size_t n, size_t nlabels) {
    if (nlabels > d_labels.capacity()) HIPCHK(d_labels.reserve(nlabels + 16));
    if (!h_ctr) {
        HIPCHK(d_ctr.reserve(4));
        HIPCHK(h_ctr.reserve(8));
    }
    if (n <= cap) return SAGEICP_OK;
    cap = 0;
    const size_t c = n + n / 4 + 1024;
    const size_t nrec = c / 5 + 2;
    HIPCHK(d_cnt.reserve(c));
    HIPCHK(d_pos.reserve(c));
    HIPCHK(d_vp.reserve(c));
    HIPCHK(d_vs.reserve(c));
    HIPCHK(d_lp.reserve(c));
    HIPCHK(d_ls.reserve(c));
    HIPCHK(d_vkey.reserve(2 * c));
    HIPCHK(d_lkey.reserve(2 * c));
    HIPCHK(d_vval.reserve(2 * c));
    HIPCHK(d_lval.reserve(2 * c));
    HIPCHK(d_vframe.reserve(c));
    HIPCHK(d_parent.reserve(c));
    HIPCHK(d_root.reserve(c));
    HIPCHK(d_size.reserve(c));
    HIPCHK(d_count.reserve(c));
    HIPCHK(d_rec_of_root.reserve(c));
    HIPCHK(d_start.reserve(c));
    HIPCHK(d_rkv.reserve(2 * c));
    HIPCHK(d_rec.reserve(nrec));
    HIPCHK(d_off.reserve(nrec));
    HIPCHK(h_rec.reserve(nrec));
    HIPCHK(h_off.reserve(nrec));
    size_t b = 0, t = 0;
    unsigned long long *k64 = nullptr;
    uint32_t *k32 = nullptr;
    HIPCHK(rocprim::exclusive_scan(nullptr, t, k64, k64, 0ull, c, rocprim::plus<unsigned long long>()));
    b = std::max(b, t);
    HIPCHK(rocprim::radix_sort_pairs(nullptr, t, k64, k64, k32, k32, c, 0, 3 * kCellBits));
    b = std::max(b, t);
    HIPCHK(rocprim::radix_sort_pairs(nullptr, t, k32, k32, k32, k32, c, 0, 32));
    b = std::max(b, t);
    HIPCHK(d_temp.reserve(b));
    cap = c;
    return SAGEICP_OK;
}

int DynFilter::run(const Point4 *in, uint64_t n, double max_range, double min_range, double label_max_range,
                   const DynFilterConfig &cfg, Point4 *tmp, Point4 *out, int *d_ovf, uint64_t &n_out, hipStream_t s) {
    const double t0 = now_us();
    info = sageicp_dynfilter_info{};
    n_out = 0;
    const size_t nlab = cfg.dynamic_labels.size() + cfg.landmark_labels.size();
    int rc = reserve(n, nlab);
    if (rc) return rc;
    if (n == 0) return SAGEICP_OK;
    size_t temp_bytes = d_temp.capacity();     // (rocprim takes the size by reference)
    const bool prof = g_profiling != 0;
    if (prof && !ev[0])
        for (auto &e : ev) HIPCHK(e.create(hipEventDefault));
    std::vector<uint32_t> lab(cfg.dynamic_labels.begin(), cfg.dynamic_labels.end());
    lab.insert(lab.end(), cfg.landmark_labels.begin(), cfg.landmark_labels.end());

    DynParams P{};
    P.in = in; P.n = static_cast<int>(n);
    P.max_range = max_range; P.min_range = min_range; P.label_max_range = label_max_range;
    P.labels = d_labels.data(); P.n_dyn = static_cast<int>(cfg.dynamic_labels.size()); P.n_lm = static_cast<int>(cfg.landmark_labels.size());
    P.tmp = tmp; P.cnt = d_cnt.data(); P.pos = d_pos.data(); P.out = out;
    P.vp = d_vp.data(); P.vframe = d_vframe.data(); P.vkey = d_vkey.data(); P.vval = d_vval.data();
    P.lp = d_lp.data(); P.lkey = d_lkey.data(); P.lval = d_lval.data();
    P.ctr = d_ctr.data(); P.ovf = d_ovf;

    // ---- classify, compact -------------------------------------------------------------------------------------
    if (prof) HIPCHK(hipEventRecord(ev[0].get(), s));
    if (!lab.empty()) HIPCHK(hipMemcpyAsync(d_labels.data(), lab.data(), lab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_ctr.data(), 0, 4 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_dyn_classify, dim3(grid_of(n)), dim3(256), 0, s, P);
    HIPCHK(rocprim::exclusive_scan(d_temp.data(), temp_bytes, d_cnt.data(), d_pos.data(), 0ull, static_cast<size_t>(n),
                                   rocprim::plus<unsigned long long>(), s));
    hipLaunchKernelGGL(k_dyn_compact, dim3(grid_of(n)), dim3(256), 0, s, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_ctr.data(), d_ctr.data(), 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_ctr.data() + 4, d_ovf, sizeof(int), hipMemcpyDeviceToHost, s));
    if (prof) HIPCHK(hipEventRecord(ev[1].get(), s));
    HIPCHK(hipStreamSynchronize(s));
    const int ovf1 = static_cast<int>(h_ctr.data()[4]);
    if (ovf1 & 2) return fail(SAGEICP_ERR_INVALID, "a label is not finite (NaN / Inf)");
    if (ovf1 & 1) return fail(SAGEICP_ERR_CAPACITY, "dynamic vehicle filter: a point lies beyond +-2^19 m");
    const uint32_t n_in = h_ctr.data()[0], nv = h_ctr.data()[1], nl = h_ctr.data()[2];
    info.vehicle_points = nv;
    info.landmark_points = nl;
    n_out = n_in;
    if (nv == 0) {
        info.us_wall = now_us() - t0;
        if (prof) {
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, ev[0].get(), ev[1].get()));
            info.us_device = 1e3 * ms;
        }
        return SAGEICP_OK;
    }

    // ---- grids, components, counts, the component table ------------------------------------------------------------
    if (prof) HIPCHK(hipEventRecord(ev[2].get(), s));
    unsigned long long *vkey_s = d_vkey.data() + cap, *lkey_s = d_lkey.data() + cap;
    uint32_t *vidx = d_vval.data() + cap, *lidx = d_lval.data() + cap;
    HIPCHK(rocprim::radix_sort_pairs(d_temp.data(), temp_bytes, d_vkey.data(), vkey_s, d_vval.data(), vidx, nv, 0, 3 * kCellBits, s));
    if (nl) HIPCHK(rocprim::radix_sort_pairs(d_temp.data(), temp_bytes, d_lkey.data(), lkey_s, d_lval.data(), lidx, nl, 0, 3 * kCellBits, s));
    hipLaunchKernelGGL(k_dyn_gather, dim3(grid_of(std::max(nv, nl))), dim3(256), 0, s, d_vp.data(), vidx, nv, d_vs.data(), d_lp.data(), lidx,
                       nl, d_ls.data(), d_parent.data(), d_size.data(), d_count.data(), d_rec_of_root.data());
    hipLaunchKernelGGL(k_dyn_link, dim3(grid_of(nv)), dim3(256), 0, s, d_vs.data(), vkey_s, vidx, nv, d_parent.data(), d_ovf);
    hipLaunchKernelGGL(k_dyn_count, dim3(grid_of(nv)), dim3(256), 0, s, d_vs.data(), vidx, nv, d_ls.data(), lkey_s, nl, d_parent.data(),
                       d_root.data(), d_size.data(), d_count.data(), d_ovf);
    hipLaunchKernelGGL(k_dyn_root_flags, dim3(grid_of(nv)), dim3(256), 0, s, d_root.data(), d_size.data(), nv, d_cnt.data());
    HIPCHK(rocprim::exclusive_scan(d_temp.data(), temp_bytes, d_cnt.data(), d_pos.data(), 0ull, static_cast<size_t>(nv),
                                   rocprim::plus<unsigned long long>(), s));
    hipLaunchKernelGGL(k_dyn_records, dim3(grid_of(nv)), dim3(256), 0, s, d_cnt.data(), d_pos.data(), nv, d_size.data(), d_count.data(), d_rec.data(),
                       d_rec_of_root.data(), d_ctr.data());
    HIPCHK(hipGetLastError());
    const size_t max_rec = nv / 5;             // components of >= 5 points
    HIPCHK(hipMemcpyAsync(h_ctr.data(), d_ctr.data(), 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_ctr.data() + 4, d_ovf, sizeof(int), hipMemcpyDeviceToHost, s));
    if (max_rec) HIPCHK(hipMemcpyAsync(h_rec.data(), d_rec.data(), max_rec * sizeof(uint4), hipMemcpyDeviceToHost, s));
    if (!ev_table) HIPCHK(ev_table.create(hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev_table.get(), s));
    // grouping of the points by component runs while the host works on the table
    uint32_t *rkey = d_rkv.data(), *rval = d_rkv.data() + cap;
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) < nv) ++bits;
    HIPCHK(rocprim::radix_sort_pairs(d_temp.data(), temp_bytes, d_root.data(), rkey, d_vval.data(), rval, nv, 0, bits, s));
    hipLaunchKernelGGL(k_dyn_starts, dim3(grid_of(nv)), dim3(256), 0, s, rkey, nv, d_start.data());
    HIPCHK(hipGetLastError());
    if (prof) HIPCHK(hipEventRecord(ev[3].get(), s));
    const double th0 = now_us();
    HIPCHK(hipEventSynchronize(ev_table.get()));
    if (h_ctr.data()[4] & 4) return fail(SAGEICP_ERR_HIP, "dynamic vehicle filter: union-find invariant broken");
    const uint32_t ncl = h_ctr.data()[3];
    if (ncl > max_rec) return fail(SAGEICP_ERR_HIP, "dynamic vehicle filter: inconsistent component table");

    // ---- host: PCL's cluster order and the static test (Preprocessing.cpp:130-170) --------------------------------
    const uint4 *rec = h_rec.data();
    order_scratch.resize(ncl);
    size_scratch.resize(ncl);
    for (uint32_t k = 0; k < ncl; ++k) size_scratch[k] = rec[k].y;
    cluster_emission_order(size_scratch.data(), ncl, order_scratch.data());
    uint64_t at = n_in, kept = 0, kept_pts = 0;
    for (uint32_t k = 0; k < ncl; ++k) h_off.data()[k] = kNone;
    for (uint32_t e = 0; e < ncl; ++e) {
        const uint32_t k = order_scratch[e];
        const uint32_t sz = rec[k].y;
        const uint64_t count = static_cast<uint64_t>(rec[k].z) | (static_cast<uint64_t>(rec[k].w) << 32);
        if (cluster_is_static(count, sz, cfg.dy_th)) {
            h_off.data()[k] = static_cast<uint32_t>(at);
            at += sz;
            ++kept;
            kept_pts += sz;
        }
    }
    info.clusters = ncl;
    info.clusters_kept = kept;
    info.points_removed = nv - kept_pts;
    n_out = at;
    info.us_host = now_us() - th0;

    // ---- scatter ---------------------------------------------------------------------------------------------------
    if (kept) {
        if (prof) HIPCHK(hipEventRecord(ev[4].get(), s));
        HIPCHK(hipMemcpyAsync(d_off.data(), h_off.data(), ncl * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_dyn_scatter, dim3(grid_of(nv)), dim3(256), 0, s, rkey, rval, nv, d_start.data(), d_rec_of_root.data(),
                           d_off.data(), d_vframe.data(), tmp, out);
        HIPCHK(hipGetLastError());
        if (prof) HIPCHK(hipEventRecord(ev[5].get(), s));
    }
    // h_off is read by the copy above: it must not be rewritten by the next frame before the copy ran.  The caller
    // synchronises the stream before its next use of this filter (the down-sampling levels wait for their counts).
    info.us_wall = now_us() - t0;
    if (prof) {
        HIPCHK(hipStreamSynchronize(s));
        float a = 0, b = 0, c = 0;
        HIPCHK(hipEventElapsedTime(&a, ev[0].get(), ev[1].get()));
        HIPCHK(hipEventElapsedTime(&b, ev[2].get(), ev[3].get()));
        if (kept) HIPCHK(hipEventElapsedTime(&c, ev[4].get(), ev[5].get()));
        info.us_device = 1e3 * (static_cast<double>(a) + b + c);
    }
    return SAGEICP_OK;
}

}  // namespace sageicp
