// The search body of k_icp and k_loop: VoxelHashMap::GetCorrespondences (core/VoxelHashMap.cpp:48-130) plus the fused
// terms of AlignClouds (core/Registration.cpp:59-90) for the 64 >> LW queries of one wave.
//
// Part of kernels.hip's translation unit: included there, once, after the helpers it calls (the cross-lane moves,
// load_point / load_cand, make_query, probe_resolve, wave_terms_to_wgacc, wgacc_flush, LoopGroup, chain_wait_pose),
// and inlined into every instantiation of k_icp and k_loop.
//
// icp_body at the end of the file is the pass.  In front of it stand the pieces of it that are functions, each with what
// it reads and writes: icp_wave_of_stripe (which queries a wave of k_icp takes), axis_gaps (the face gaps of one axis),
// round_up_f32 (the fp32 filter's thresholds), reduce_argmin (the query's answer from its lanes').  The rest of the
// body — prologue, stale-row rebuild, `evaluate` and the fp32 filter, `scan` with its `next` / `issue` / `consume` steps,
// the seed, the 26 bound tests, the counters, the fused Gauss-Newton epilogue — follows its section comments inside
// icp_body and shares that function's locals.
#pragma once

namespace sageicp {

#ifndef SAGE_LOOP_FLAT_MINW
#define SAGE_LOOP_FLAT_MINW 8      // k_loop: flat-order scan from this many lanes per query (icp_body)
#endif
#ifndef SAGE_SCAN_AHEAD
#define SAGE_SCAN_AHEAD 1          // per-voxel restart scan: open a lane's next voxel one step ahead (icp_body)
#endif
#ifndef SAGE_ROW_SHIFT_LAYER
#define SAGE_ROW_SHIFT_LAYER 1     // stale row after a step into a neighbouring voxel: probe only the new layer (icp_body, row_shift.h)
#endif                             // (2, measurements only: the path compiled in but never taken, results as with 0)
#ifndef SAGE_ROW_SHIFT_MAXW
#define SAGE_ROW_SHIFT_MAXW 4      // ... in k_loop up to this many lanes per query (8, 16: trial builds, profiles/r20)
#endif

// a pair of scanned points in flight: compact records (FILT) or full ones
struct PairCompact {
    uint4 a, b;
    unsigned ka, oa;                // key / compact offset of a; b: key + W, offset + W records
    bool ha, hb;
};
struct PairFull {
    Point4 a, b;
    unsigned ka;
    bool ha, hb;
};
// ... of a scan in flat order (below): b may lie in another voxel than a
struct PairCompactFlat {
    uint4 a, b;
    unsigned ka, oa, kb, ob;
    bool ha, hb;
};
struct PairFullFlat {
    Point4 a, b;
    unsigned ka, kb;
    bool ha, hb;
};

// Which queries this wave of k_icp takes: returns the wave's index in the frame, `stripe_id`: the stripe it serves.
// Workgroup b is dispatched to XCD b % 8 (observed; speed only): XCD x serves the stripes
// x, x+8, x+16, ... of kStripe consecutive workgroups' worth of the spatially sorted frame,
// so each private L2 sees a few compact regions of the map and every XCD gets the same mix
// of dense and sparse regions.  (k_loop: stripes of kLoopStripe workgroups; one contiguous eighth
// of the frame per XCD left the XCDs with 57k to 97k points to look at per iteration on a c2 shard,
// and the iteration ends with the slowest, profiles/r04/loop_times.txt.)
__device__ __forceinline__ unsigned icp_wave_of_stripe(const IcpParams &P, int wv, unsigned &stripe_id) {
    constexpr unsigned kStripe = SAGE_ICP_STRIPE;
    const unsigned xcd = blockIdx.x & 7u, jb = blockIdx.x >> 3;
    unsigned stripe = (jb / kStripe) * 8u + xcd;            // the stripe dispatched at this position ...
    if (P.stripe_order) {
        // ... in the order of the work an earlier iteration measured, heaviest first (kernels.h): what runs last is
        // light.  Within a SIMD the waves of the heavier stripes go first as well (s_setprio by the quarter of the
        // order this stripe lies in: the long chains run while there is other work to cover their stalls).
        const unsigned nstripes = gridDim.x / kStripe;
        switch (stripe * 4u / nstripes) {
            case 0: __builtin_amdgcn_s_setprio(3); break;
            case 1: __builtin_amdgcn_s_setprio(2); break;
            case 2: __builtin_amdgcn_s_setprio(1); break;
            default: break;
        }
        stripe = P.stripe_order[stripe];
    }
    stripe_id = stripe;
    const unsigned wg = stripe * kStripe + (jb % kStripe);
    return wg * static_cast<unsigned>(kIcpWavesPerBlock) + static_cast<unsigned>(wv);
}

// one axis of the face gaps (icp_body): g[0] / g[2] the pre-scaled squared gap to the layer below / above, g[1] = 0
// (GIVEN, k_loop: `fs` = fl(1e-9 vs) comes from LoopArgs::face_slack — an fp64 literal has to sit in a register pair, and
// k_loop kept this one in scratch memory across its iteration loop; k_icp forms the product here, as it always did)
template <bool GIVEN>
__device__ __forceinline__ void axis_gaps(double v, int k, double vs, double sc, double fs, double (&g)[3]) {
    const double below_hi = static_cast<double>(k <= 0 ? k - 1 : k) * vs;
    const double above_lo = static_cast<double>(k >= 0 ? k + 1 : k) * vs;
    const double slack = (GIVEN ? fs : 1e-9 * vs) + 1e-13 * fabs(v);
    const double lo = fmax((v - below_hi) - slack, 0.0);
    const double hi = fmax((above_lo - v) - slack, 0.0);
    g[0] = (lo * lo) * sc;
    g[1] = 0.0;
    g[2] = (hi * hi) * sc;
}

__device__ __forceinline__ float round_up_f32(double x) {      // the next fp32 above x (an infinity becomes a NaN:
    return __uint_as_float(__float_as_uint(static_cast<float>(x)) + 1u);   // `D32 > NaN` is false, nothing is dropped)
}

// argmin over the W lanes of the query: first the minimum distance (never NaN: a NaN distance
// fails every comparison), then the smallest key among the lanes that hold it; the winner's
// offset follows from its key and the row.
// Reads the lanes' best / bkey and the row; returns whether the query has an answer (else: empty neighbourhood, hazard
// H1), its key `mkey` and the byte offset `woff` of its full record.
template <int LW>
__device__ __forceinline__ bool reduce_argmin(double best, unsigned bkey, bool valid, const uint32_t *lrow, unsigned &mkey, unsigned &woff) {
    constexpr int W = 1 << LW, SH = 5;
    const double m = seg_min_f64<W>(best);
    const unsigned mine = (best == m) ? bkey : 0xFFFFFFFFu;
    mkey = seg_min_u32<W>(mine);
    const bool found = valid && mkey != 0xFFFFFFFFu;
    woff = (lrow[found ? mkey >> 8 : 0u] >> 8) * (kUnitPoints * 32u) + ((mkey & 255u) << SH);
    return found;
}

// k_loop: what a pass holds when it reaches its first use of the pose — the front of the body, which k_loop runs in
// front of its wait for that pose (HALF below).  One member per value, no vectors: what is read from LDS as four words and
// carried as four words stays a register quadruple to the allocator, alive as long as its longest-lived word — the label
// lives through the scans, and its quadruple went to scratch memory.
struct LoopStaged {
    unsigned qslot;            // the query's slot in the workgroup (its row and its state record)
    double fx, fy, fz, fl;     // the frame point
    unsigned prev_key, prev_off;               // the previous answer
    unsigned kx, ky, kz, occ;  // the home voxel the row was built for | the row's occupancy
    int pli;                   // the query's label class
};

// PERSIST (k_loop): the body runs on group `G` — rows and per-query state in LDS — with the pose from
// `pose` (LDS: R[9], t[3]); nothing is read from or written to the global rows / nn_prev arrays;
// the body ends with the group's sums added to the workgroup's accumulators G->wgacc.
// HALF (k_loop): the pass is cut at the line where the pose is first used.  1, the stage half: everything in front of
// that line — the lane, the block's slot from `perm`, the query's state record, the buffer resources, the label class —
// into `S`, and nothing else: no store, no use of `pose`.  2, the run half: from make_query on, out of `S`.  0: both,
// back to back (k_icp).
template <int LW, bool FUSED, bool FILT, bool PERSIST = false, bool FLATQ = false, int HALF = 0>
__device__ __forceinline__ void icp_body(const IcpParams &P, uint32_t *smem, LoopGroup *G = nullptr, const double *pose = nullptr,
                                         LoopStaged *S = nullptr) {
    static_assert(!PERSIST || FUSED, "the persistent loop always accumulates");
    static_assert(PERSIST ? (HALF == 1 || HALF == 2) : HALF == 0, "k_loop runs the pass in two halves, k_icp in one");
    constexpr int W = 1 << LW;                 // lanes per query
    constexpr int QW = 64 >> LW;               // queries per wave
    constexpr int SH = 5;                      // points are addressed by byte offset
    PROBE_NN_BEGIN(np);
    PROBE_DELAY_BEGIN(t0);
    int lane;
    if constexpr (PERSIST) {
        // (k_loop: re-derived in every pass — what the compiler knows to be invariant across the iteration
        // loop it hoists out of it and keeps, with everything computed from it, in registers the scan needs)
        unsigned l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        lane = static_cast<int>(l);
    } else {
        lane = static_cast<int>(threadIdx.x & 63u);
    }
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    if (FUSED && !PERSIST) {
        if (threadIdx.x == 0) {
            smem[kWgArrive] = 0u;
            smem[kWgGo] = 0u;
        }
        if (threadIdx.x < 2u * kWgAccWords) smem[kWgAcc + threadIdx.x] = 0u;
        // the pose of this iteration, for the workgroup (a chained launch after the first gets it from the solving wave, below)
        if (threadIdx.x < 12u && !(P.chain && P.chain_iter > 0))
            reinterpret_cast<double *>(smem + kWgPose)[threadIdx.x] = threadIdx.x < 9u ? P.st->R[threadIdx.x] : P.st->T[4u + threadIdx.x - 9u];
        __syncthreads();
    }
    uint32_t *wl;
    if constexpr (PERSIST) wl = G->rows;
    else wl = smem + kWgHeaderWords + static_cast<unsigned>(wv) * icp_wave_words(LW);

    unsigned wave_id, stripe_id = 0u;          // wave-uniform
    if constexpr (PERSIST) wave_id = G->slot;  // (k_loop maps its workgroups to groups of queries itself)
    else wave_id = icp_wave_of_stripe(P, wv, stripe_id);

    const int qw = lane >> LW;                 // this lane's query within the wave
    const unsigned ci = static_cast<unsigned>(lane) & (W - 1u);
    // k_loop: a pass takes QW / 4 BLOCKS of four consecutive queries — not necessarily neighbours: the workgroup's
    // blocks are re-ordered every iteration by the work they were (a wave's pass lasts as long as its heaviest
    // query: blocks of like work share a wave).  The four queries of a block stay together, in order, on one
    // aligned group of lanes, which is all the exact block sums ask for (wave_terms_to_wgacc).
    unsigned q, qslot = 0u, bslot = 0u;
    if constexpr (PERSIST) {
        if constexpr (HALF == 1) {
            bslot = G->perm[G->unit * (QW / 4) + static_cast<unsigned>(qw >> 2)];
            qslot = bslot * 4u + (static_cast<unsigned>(qw) & 3u);
        } else {
            qslot = S->qslot;
        }
        q = G->q_first + qslot;
    } else {
        q = wave_id * QW + static_cast<unsigned>(qw);
    }
    const bool valid = q < static_cast<unsigned>(P.n);
    const unsigned qc = valid ? q : 0u;        // keeps the loads of idle lanes legal
    uint32_t *lrow = wl + (PERSIST ? qslot : static_cast<unsigned>(qw)) * kRowLdsStride;
    const uint32_t *grow = P.rows + static_cast<size_t>(qc) * kRowWords;

    // raw buffer resource over the point array (bounds-checked, 32-bit byte offsets)
    const __amdgpu_buffer_rsrc_t pts = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<Point4 *>(P.pts), 0, static_cast<int>(P.pts_bytes), 0x00020000);

    const __amdgpu_buffer_rsrc_t cands = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4 *>(P.cand), 0, static_cast<int>(P.cand_bytes), 0x00020000);
    constexpr int SHC = FILT ? 4 : 5;          // the scan's records (compact or full), by byte offset

    // ---- prologue: the query, its home voxel, its neighbourhood row ------------------------------
    // Everything the prologue needs is requested at once (one memory round trip): the row key, the
    // frame point, the previous iteration's record and — speculatively, before the key has been
    // checked — this lane's share of the cached row (words 0..27 in seven 16-B pieces).
    constexpr int NP = (7 + W - 1) / W;        // pieces per lane
    uint4 rk;                                  // key x, y, z | occupancy
    uint2 prev = make_uint2(0xFFFFFFFFu, 0u);     // the previous iteration's record of this query
    Point4 f;
    // (named registers, not an array: the compiler leaves a uint4 array in scratch memory)
    uint4 pc0 = make_uint4(0u, 0u, 0u, 0u), pc1 = pc0, pc2 = pc0, pc3 = pc0, pc4 = pc0, pc5 = pc0, pc6 = pc0;
    uint32_t *lst = nullptr;                   // k_loop: this query's state record (LDS)
    if constexpr (PERSIST) {
        // k_loop: everything is already here, in LDS — the state record and the row
        lst = G->state + qslot * kLoopStateWords;
        if constexpr (HALF == 1) {
            const uint4 fa = *reinterpret_cast<const uint4 *>(lst), fb = *reinterpret_cast<const uint4 *>(lst + 4);
            const uint4 pk = *reinterpret_cast<const uint4 *>(lst + kStPrev);
            const uint2 ko = *reinterpret_cast<const uint2 *>(lst + kStPrev + 4);
            S->qslot = qslot;
            S->fx = __hiloint2double(static_cast<int>(fa.y), static_cast<int>(fa.x));
            S->fy = __hiloint2double(static_cast<int>(fa.w), static_cast<int>(fa.z));
            S->fz = __hiloint2double(static_cast<int>(fb.y), static_cast<int>(fb.x));
            S->fl = __hiloint2double(static_cast<int>(fb.w), static_cast<int>(fb.z));
            S->prev_key = pk.x; S->prev_off = pk.y;
            S->kx = pk.z; S->ky = pk.w; S->kz = ko.x; S->occ = ko.y;
            S->pli = static_cast<int>(S->fl);
            return;
        }
        f.x = S->fx; f.y = S->fy; f.z = S->fz; f.l = S->fl;
        prev = make_uint2(S->prev_key, S->prev_off);
        rk = make_uint4(S->kx, S->ky, S->kz, S->occ);
    } else {
        rk = *reinterpret_cast<const uint4 *>(grow + kRowKey);
        if (FUSED) prev = P.nn_prev[qc];
        f = P.frame[qc];
        auto row_piece = [&](int k) {
            const unsigned p = min(ci + static_cast<unsigned>(W * k), 6u);
            return *reinterpret_cast<const uint4 *>(grow + 4u * p);
        };
        pc0 = row_piece(0); pc1 = pc0; pc2 = pc0; pc3 = pc0; pc4 = pc0; pc5 = pc0; pc6 = pc0;
        if (NP > 1) pc1 = row_piece(1);
        if (NP > 2) pc2 = row_piece(2);
        if (NP > 3) pc3 = row_piece(3);
        if (NP > 4) pc4 = row_piece(4);
        if (NP > 5) pc5 = row_piece(5);
        if (NP > 6) pc6 = row_piece(6);
    }
    PROBE_DELAY_WAIT(P, t0);
    if constexpr (FUSED && !PERSIST) {
        if (P.chain && P.chain_iter > 0) {
            // (the loads above are in flight while wave 0 waits for the pose: the launch started under the solve)
            if (wv == 0) chain_wait_pose(P, smem, lane);
            __syncthreads();
            if (smem[kWgGo]) return;
        }
    }
    PROBE_LOOP_POSE_USE(PERSIST, G);
    const Query s = [&]() {
        if constexpr (PERSIST) {
            return make_query<(W >= 4)>(f, pose, pose + 9, 1, P.voxel_size, P.inv_voxel_size, static_cast<unsigned>(lane));
        } else if constexpr (FUSED) {
            const double *lpose = reinterpret_cast<const double *>(smem + kWgPose);       // the workgroup's copy
            return make_query<(W >= 4)>(f, lpose, lpose + 9, P.apply_pose, P.voxel_size, P.inv_voxel_size, threadIdx.x);
        } else {
            return make_query<(W >= 4)>(f, P.st->R, P.st->T + 4, P.apply_pose, P.voxel_size, P.inv_voxel_size, threadIdx.x);
        }
    }();
    const bool stale = valid && (static_cast<uint32_t>(s.kx) != rk.x || static_cast<uint32_t>(s.ky) != rk.y ||
                                 static_cast<uint32_t>(s.kz) != rk.z);
    unsigned occ = rk.w;
    NN_T(np, 0);
    LP_T(PERSIST, G, 0);
    if constexpr (!PERSIST) {
        // stage the row in LDS (a stale one is overwritten below)
        auto stage = [&](int k, const uint4 &v) {
            const unsigned p = ci + static_cast<unsigned>(W * k);
            if (p < 7u) *reinterpret_cast<uint4 *>(lrow + 4u * p) = v;
        };
        stage(0, pc0);
        if (NP > 1) stage(1, pc1);
        if (NP > 2) stage(2, pc2);
        if (NP > 3) stage(3, pc3);
        if (NP > 4) stage(4, pc4);
        if (NP > 5) stage(5, pc5);
        if (NP > 6) stage(6, pc6);
    }
    if (__ballot(stale)) {
        // A query crossed a voxel face since its row was built (a few % of the queries per iteration
        // at the start of a cold registration, almost none near convergence; every query in the first
        // pass of k_loop): its lanes rebuild the row in LDS (and in the cache).  With eight or more
        // lanes per query (k_loop: four) a step into a NEIGHBOURING voxel keeps what the two neighbourhoods share —
        // 18 of the 27 voxels after a step through a face, 12 through an edge, 8 through a corner: the
        // words move inside the row, only the new layer is probed (one batch of loads instead of two or
        // three), and the previous answer, if it lies in the shared part, stays the seed under its new
        // enumeration key.  Otherwise all 27 voxels are probed, up to three / four in flight per lane.
        if (stale) {
            unsigned o = 0u, cq = 0u;
            constexpr int NV = (27 + W - 1) / W;          // voxels per lane
            constexpr bool kShift = NV <= (PERSIST ? 7 : 4);     // (k_icp with four lanes per query sits on its register edge)
            auto tally = [&](int v, uint32_t w) {
                const unsigned c = (w == kEmptySlot) ? 0u : (w & 255u);
                lrow[v] = w;
                if constexpr (!PERSIST) P.rows[static_cast<size_t>(q) * kRowWords + static_cast<unsigned>(v)] = w;
                o |= (c != 0u ? 1u : 0u) << v;
                cq += c;
            };
            // one probe: first slot load issued by `start`, resolved (and the row word stored) by `finish`
            auto start = [&](int v, uint32_t &sl, int4 &e) {
                const int vc = v < 27 ? v : 26;
                sl = voxel_hash(s.kx + vc / 9 - 1, s.ky + (vc / 3) % 3 - 1, s.kz + vc % 3 - 1) & P.mask;
                e = reinterpret_cast<const int4 *>(P.table)[sl];
            };
            auto finish = [&](int v, uint32_t sl, const int4 &e) {
                if (v >= 27) return;
                tally(v, probe_resolve(P.table, P.mask, sl, e, s.kx + v / 9 - 1, s.ky + (v / 3) % 3 - 1,
                                       s.kz + v % 3 - 1));
            };
            if constexpr (kShift) {
                // (unsigned differences: a row not built yet carries kNoVoxel = 0x7FFFFFFF, and a signed difference from
                // a negative index would overflow)
                const unsigned dxu = static_cast<unsigned>(s.kx) - rk.x, dyu = static_cast<unsigned>(s.ky) - rk.y,
                               dzu = static_cast<unsigned>(s.kz) - rk.z;
                const bool nearv = dxu + 1u <= 2u && dyu + 1u <= 2u && dzu + 1u <= 2u;
                const int dx = static_cast<int>(dxu), dy = static_cast<int>(dyu), dz = static_cast<int>(dzu);
                // k_loop at four lanes: a step into a neighbouring voxel costs what it needs (row_shift.h).  The kept
                // words move by ONE offset under one mask, the occupancy mask is the old one shifted, and the 9 / 15 / 19
                // new voxels are dealt over the query's lanes by rank: a lane has all its probes of a face crossing
                // (three at most) in flight at once, whatever the axis.  It repeats the walk's pattern below — old words,
                // `start`, `finish` — over its own, shorter lists.  (Eight and sixteen lanes keep the walk: SAGE_ROW_SHIFT_MAXW.)
                constexpr bool kLayer = SAGE_ROW_SHIFT_LAYER && PERSIST && W >= 4 && W <= SAGE_ROW_SHIFT_MAXW;
                bool shifted = false;
                if constexpr (kLayer) {
                    if (nearv && (SAGE_ROW_SHIFT_LAYER != 2 || P.n < 0)) {
                        shifted = true;
                        const uint32_t kept = rowshift::kept_mask(dx, dy, dz);
                        // the old words of this lane's kept voxels (LDS is in order within a wave: every read here
                        // precedes the writes below, also those of the query's other lanes)
                        // (`kept` has 27 bits: bit W * j of `kl` is never set for a v = ci + W * j >= 27, which so is
                        // neither read nor written)
                        const uint32_t kl = kept >> ci;
                        uint32_t ow[NV];
#pragma unroll
                        for (int j = 0; j < NV; ++j) {
                            const bool kp = (kl >> (W * j)) & 1u;
                            const int v = static_cast<int>(ci) + W * j;
                            ow[j] = lrow[kp ? rowshift::old_position(static_cast<uint32_t>(v), dx, dy, dz) : 0u];
                        }
                        if (ci == 0u) o = rowshift::shifted_mask(occ, dx, dy, dz);
                        uint32_t nm = rowshift::lane_first<W>(rowshift::new_mask(dx, dy, dz), ci);
                        constexpr int NL = (19 + W - 1) / W;      // new voxels per lane at most (a corner)
                        constexpr int NB = 3;                     // probes in flight per lane: a face crossing is one batch
#pragma unroll
                        for (int j0 = 0; j0 < NL; j0 += NB) {
                            if (j0 == 0 || nm != 0u) {          // (a later batch only for a lane with voxels left: edges, corners)
                                int nv[NB];
                                bool has[NB];
                                uint32_t sl[NB];
                                int4 e[NB];
#pragma unroll
                                for (int j = 0; j < NB && j0 + j < NL; ++j) {
                                    has[j] = nm != 0u;
                                    nv[j] = has[j] ? static_cast<int>(rowshift::lowest(nm)) : 0;     // (0: never probed, never stored)
                                    nm = rowshift::lane_next<W>(nm);
                                    sl[j] = 0u;
                                    e[j] = make_int4(0, 0, 0, 0);
                                    if (has[j]) start(nv[j], sl[j], e[j]);
                                }
                                if (j0 == 0) {
                                    // under the loads: the kept words take their new places, C_q is re-summed
#pragma unroll
                                    for (int j = 0; j < NV; ++j) {
                                        if ((kl >> (W * j)) & 1u) {
                                            lrow[static_cast<int>(ci) + W * j] = ow[j];
                                            cq += (ow[j] == kEmptySlot) ? 0u : (ow[j] & 255u);
                                        }
                                    }
                                }
#pragma unroll
                                for (int j = 0; j < NB && j0 + j < NL; ++j)
                                    if (has[j]) finish(nv[j], sl[j], e[j]);
                            }
                        }
                    }
                }
                if (!shifted) {
                    // the old words of this lane's voxels (LDS is in order within a wave: every read here
                    // precedes the writes below, also those of the query's other lanes)
                    uint32_t ow[NV];
                    bool reuse[NV];
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        const int v = static_cast<int>(ci) + W * j;
                        const unsigned a = static_cast<unsigned>(v / 9) + dxu, b = static_cast<unsigned>((v / 3) % 3) + dyu,
                                       c = static_cast<unsigned>(v % 3) + dzu;
                        reuse[j] = nearv && v < 27 && a <= 2u && b <= 2u && c <= 2u;
                        ow[j] = lrow[reuse[j] ? a * 9u + b * 3u + c : 0u];
                    }
                    uint32_t sl[NV];
                    int4 e[NV];
                    constexpr int NB = PERSIST ? 4 : 3;       // probes in flight per lane (k_icp: its register budget)
#pragma unroll
                    for (int j0 = 0; j0 < NV; j0 += NB) {
#pragma unroll
                        for (int j = j0; j < j0 + NB && j < NV; ++j) {
                            sl[j] = 0u;
                            e[j] = make_int4(0, 0, 0, 0);
                            if (!reuse[j]) start(static_cast<int>(ci) + W * j, sl[j], e[j]);
                        }
#pragma unroll
                        for (int j = j0; j < j0 + NB && j < NV; ++j) {
                            const int v = static_cast<int>(ci) + W * j;
                            if (reuse[j]) tally(v, ow[j]);
                            else finish(v, sl[j], e[j]);
                        }
                    }
                }
                // the previous answer under the new enumeration, if its voxel is still one of the 27
                if (nearv && prev.x != 0xFFFFFFFFu) {
                    const int vo = static_cast<int>(prev.x >> 8);
                    const int a = vo / 9 - dx, b = (vo / 3) % 3 - dy, c = vo % 3 - dz;
                    const bool in = static_cast<unsigned>(a) <= 2u && static_cast<unsigned>(b) <= 2u &&
                                    static_cast<unsigned>(c) <= 2u;
                    prev.x = in ? (static_cast<unsigned>(a * 9 + b * 3 + c) << 8) | (prev.x & 255u) : 0xFFFFFFFFu;
                } else {
                    prev.x = 0xFFFFFFFFu;
                }
            } else {
                prev.x = 0xFFFFFFFFu;          // (the key's meaning went with the old row)
#pragma unroll 1
                for (int k0 = 0; k0 < NV; k0 += 3) {
                    const int v0 = static_cast<int>(ci) + W * k0;
                    const int v1 = k0 + 1 < NV ? v0 + W : 27, v2 = k0 + 2 < NV ? v0 + 2 * W : 27;
                    uint32_t s0, s1, s2;
                    int4 e0, e1, e2;
                    start(v0, s0, e0);
                    start(v1, s1, e1);
                    start(v2, s2, e2);
                    finish(v0, s0, e0);
                    finish(v1, s1, e1);
                    finish(v2, s2, e2);
                }
            }
            o = seg_or_u32<W>(o);              // the lanes of a query are stale together
            cq = seg_add_u32<W>(cq);
            occ = o;
            if (ci == 0u) {
                lrow[kRowCq] = cq;
                if constexpr (!PERSIST) {
                    uint4 t;
                    t.x = static_cast<uint32_t>(s.kx); t.y = static_cast<uint32_t>(s.ky);
                    t.z = static_cast<uint32_t>(s.kz); t.w = o;
                    *reinterpret_cast<uint4 *>(P.rows + static_cast<size_t>(q) * kRowWords + kRowKey) = t;
                    P.rows[static_cast<size_t>(q) * kRowWords + kRowCq] = cq;
                }
            }
            if constexpr (PERSIST) {
                if (ci == 0u) {
                    *reinterpret_cast<uint2 *>(lst + kStKey) = make_uint2(static_cast<uint32_t>(s.kx), static_cast<uint32_t>(s.ky));
                    *reinterpret_cast<uint2 *>(lst + kStKey + 2) = make_uint2(static_cast<uint32_t>(s.kz), o);
                    lst[kStPrev] = prev.x;         // (re-keyed or dropped: read again below)
                }
            }
        }
    }
    if constexpr (PERSIST) {
        // k_loop: the previous answer's key is not carried through the rebuild and the scans in a register — the state
        // record has it (a rebuilt row's lanes have just stored theirs), and whoever needs it reads it there.
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        prev.x = lst[opaque_v(kStPrev)];
    }
    if (!valid) occ = 0u;

    // Squared gaps to the six faces of the home cell, pre-scaled by prune_scale.  The cell of voxel
    // index k on one axis (truncation toward zero: cell 0 is two voxels wide): [k vs, (k+1) vs)
    // for k > 0, (-vs, vs) for k = 0, ((k-1) vs, k vs] for k < 0.  Points stored in the voxel
    // below / above the home voxel therefore lie at or beyond `below_hi` / `above_lo`; the gaps are
    // shortened by an absolute slack that dwarfs the rounding of the divide, the product and the
    // subtraction (~1e-16 relative).
    double gx[3], gy[3], gz[3];
    {
        const double vs = P.voxel_size, sc = P.prune_scale;
        double fs = 0.0;
        // (k_loop's P is LoopArgs::P, the first member of its one argument: the product is read from the kernel-argument
        // segment here, beside vs and sc — handed down through G it sat in two scalar registers all through the rebuild)
        if constexpr (PERSIST) fs = reinterpret_cast<const LoopArgs *>(&P)->face_slack;
        axis_gaps<PERSIST>(s.x, s.kx, vs, sc, fs, gx);
        axis_gaps<PERSIST>(s.y, s.ky, vs, sc, fs, gy);
        axis_gaps<PERSIST>(s.z, s.kz, vs, sc, fs, gz);
    }
    NN_T(np, 1);
    LP_T(PERSIST, G, 1);

    // ---- search -----------------------------------------------------------------------------------
    // closest_distance2 starts at numeric_limits<double>::max() (VoxelHashMap.cpp:80); the value
    // travels as a kernel argument so that it sits in scalar registers
    double best = P.dist_init;                 // scaled squared distance
    unsigned bkey = 0xFFFFFFFFu;               // (voxel << 8) | slot: the enumeration order
    const int pli = HALF == 2 ? S->pli : static_cast<int>(s.l);
    const double th = P.sem_th;
    unsigned npairs = 0u;                      // points this query's lanes were handed

    // voxel cursor of this lane: it takes points ci, ci + W, ... of the open voxel.  k = (voxel <<
    // 8) | slot of its next point, kend = (voxel << 8) | points in the voxel, off = where the
    // compact record of point k lives (bytes).  Only the key of the winner is
    // tracked; its offset is rebuilt from the row once per query.
    unsigned k = ci, kend = 0u, off = 0u;
    unsigned pk = 0u, needs = 0u, wn = 0u;     // AHEAD (below): packed cursor, `need` with its end mark, the next voxel's row word
    // The reference's comparison, fp64, on a full record.  Branch-free: a lane that holds no
    // candidate here (`on` false) turns its distance into a NaN, which loses every comparison.
    auto evaluate = [&](const Point4 &nb, bool on, unsigned key) {
        const double dx = nb.x - s.x, dy = nb.y - s.y, dz = nb.z - s.z;
        double d = SAGE_SQNORM3_NN(dx * dx, dy * dy, dz * dz);
        // same label, or either side unlabelled (VoxelHashMap.cpp:87-88)
        // ((int)(a * b) == 0  <=>  |a * b| < 1 under truncation toward zero)
        const bool same = static_cast<int>(nb.l) == pli || fabs(nb.l * s.l) < 1.0;
        const double ds = d * th;
        d = same ? ds : d;
        d = __hiloint2double(on ? __double2hiint(d) : 0x7FF80000, __double2loint(d));
        // lexicographic (d, key): the home voxel is visited first, out of enumeration order;
        // a NaN distance never wins
        const bool lt = d < best, eq = d == best, kl = key < bkey;
        const bool take = lt | (eq & kl);
        best = min_f64(best, d);
        bkey = take ? key : bkey;
    };

    // ---- the fp32 filter in front of it ------------------------------------------------------
    // p, q: map point and query (fp64), p32, q32 their fp32 roundings, u = 2^-24.  Per axis
    // |fl(p32 - q32) - (p - q)| <= u(|p| + |q| + |p - q|) <= 2u(|q| + |p - q|) <= E_a with
    // E_a = 2^-22 (|q_a| + 4 voxel_size): a candidate lies within three voxels of the query.  The
    // fp32 sum of squares D32 is within (1 + u)^4 of the exact one of the rounded differences, so
    // |p - q| >= sqrt(D32 (1 - 5u)) - |E|.  A candidate whose scaled distance scale * |p - q|^2
    // can be <= b (no worse than what is held: it could win or tie) therefore has
    //     D32 <= (sqrt(b / scale) + |E|)^2 / (1 - 5u) <= (b / scale)(1 + 2^-10) k + |E|^2 (1 + 2^10) k
    // (2xy <= e x^2 + y^2 / e), k = 1 + 1e-6; the right-hand side, rounded up to fp32, is the
    // threshold: Ts for candidates of the query's label class (scale = sem_th), Td for the others
    // (scale = 1).  Anything at or under it is fetched as fp64 and compared by `evaluate`.  A label
    // that fp32 cannot classify (k_derive_cand's flag, or a query label that is no small integer)
    // gets the looser of the two.  Pruning off (sem_th negative or NaN): both infinite.
    // (FILT is off for small frames and sparse voxels, where a scan is a handful of points and the
    // filter's set-up and its occasional extra round trip cost more than the bytes it saves: the
    // scan then reads the full records and every point goes through `evaluate`.)
    const float qx = static_cast<float>(s.x), qy = static_cast<float>(s.y), qz = static_cast<float>(s.z);
    const float plab = static_cast<float>(pli);
    const bool q_zero = pli == 0;              // an unlabelled query: every candidate is of its class
    bool unknown = false;
    double slack = 0.0;
    if constexpr (FILT) {
        const bool q_exact = s.l == trunc(s.l) && fabs(s.l) < 16777216.0;
        unknown = !q_exact || (P.cand_flags[0] & 1u);
        const double ex = fabs(s.x) + 4.0 * P.voxel_size, ey = fabs(s.y) + 4.0 * P.voxel_size,
                     ez = fabs(s.z) + 4.0 * P.voxel_size;
        slack = (ex * ex + (ey * ey + ez * ez)) * P.filt_slack;     // 2^-44 (1 + 2^10) k
    }
    double fb = best;                          // what the thresholds were derived from (>= the query's final best)
    float Ts = 0.0f, Td = 0.0f, Tmax = 0.0f;   // Tmax: the looser of the two
    auto set_thresholds = [&]() {
        if constexpr (!FILT) return;
        float a = round_up_f32(fb * P.filt_inv_same + slack), b = round_up_f32(fb * P.filt_inv_diff + slack);
        float m = a > b ? a : b;               // the looser one; a NaN stands for an infinity
        if (a != a || b != b) m = __uint_as_float(0x7FC00000u);
        if (unknown) a = b = m;
        Ts = a; Td = b; Tmax = m;
    };
    // The filter in two steps.  Every scanned point pays for the fp32 distance and ONE comparison with the looser
    // threshold (packed arithmetic: x and y in one instruction, z and the label difference in another — six vector
    // instructions per point); only a step in which some lane holds a point under it looks at the label classes
    // (`tight`), and only a point under the threshold of ITS class is fetched.  (Any association, and fused: the
    // filter's bound assumes four roundings of relative size u — this sum rounds three times; the library is built
    // with -ffp-contract=off for the fp64 comparisons that decide.)
    typedef float f2 __attribute__((ext_vector_type(2)));
    auto dist32 = [&](const uint4 &c, float &dl) {
        const f2 u = f2{__uint_as_float(c.x), __uint_as_float(c.y)} - f2{qx, qy};
        const f2 v = f2{__uint_as_float(c.z), __uint_as_float(c.w)} - f2{qz, plab};
        const f2 sq = u * u;
        dl = v.y;                              // label - query label (exact: small integers; a NaN label stays a NaN)
        return __builtin_fmaf(v.x, v.x, sq.x) + sq.y;
    };
    auto tight = [&](const uint4 &c, float d, float dl) {
        const bool same = (dl == 0.0f) | (__uint_as_float(c.w) == 0.0f) | q_zero;
        return !(d > (same ? Ts : Td));
    };

    // Per-lane state machine over the voxels in `need` (and the one already open).  A step handles
    // two points of the open voxel (k and k + W); two register sets alternate, so while one pair
    // is filtered the loads of the next pair are in flight (no register copies across the loop
    // edge: the wait before a pair leaves the younger loads outstanding).
    // FLAT: the lanes of a query stride through the points of its open voxels as ONE sequence — lane c
    // takes points c, c + W, c + 2W, ... of the concatenation — instead of starting again at slot c in
    // every voxel.  With 16 lanes and ~10 points per voxel the restart leaves lanes 10..15 idle in every
    // voxel and gives lanes 0..9 one point per voxel: a query that must look at all 27 voxels is a chain
    // of 27 points per lane; in flat order it is 270 / 16 = 17.  (Which lane looks at a point changes
    // nothing: the answer is the lexicographic minimum over all of them, reduced across the lanes
    // afterwards.)  A launch ends with its slowest wave — the one holding the heaviest query
    // (profiles/r04/loop_times.txt) — and few points per voxel relative to the lanes per query make
    // the restart's chain the longer one: always with 8 and 16 lanes (k_loop c1 17.8 -> 13.4 us per
    // iteration, 15k-query shards 19.0 -> 15.8 with 16 lanes, the streamed sources' ICP 1.52 -> 1.44 ms),
    // with 2 and 4 lanes where the host finds fewer than 2 W points per voxel on average (P.flat: c5
    // 213 -> 223 frames/s; against c2's and c4's ~12 points per voxel the per-voxel restart is the faster
    // one by 1.5 and 5 %, profiles/r04/flat_where.txt).
    constexpr bool FLAT = PERSIST ? (W >= SAGE_LOOP_FLAT_MINW) : FLATQ;
    // AHEAD (per-voxel restart order only): the same points on the same lanes, with the cursor kept otherwise.
    //  - One register `pk` holds the key of the lane's next point in its low half and slot - points-in-the-voxel in its
    //    high half: negative while the lane has a point (`ha`), below -W while it has a second one (`hb`); one add
    //    advances both.  (Keys stay under 2^13, the steps of a scan add less than 2^13 more: no carry into the high half.)
    //  - The row word of the lane's NEXT voxel, `wn`, is read from LDS at the end of issue(), under the loads just sent
    //    and the other set's consume(); the step that finds the open voxel exhausted takes it in ONE divergent region (as
    //    selects it cost 48 B more scratch in k_loop): no LDS round trip and no loop inside the step.  A lane opens at most one voxel per step: one in which it has no point
    //    (fewer points than its lane index; `need` holds no empty voxel, it is masked by `occ`) costs it an idle step.
    //    Lane 0 of the query has a point in every voxel of `need` and at least as many as any other lane, so it takes
    //    the steps it took before and no lane takes more: the scan is as long as it was.
    //  - `needs` is `need` with bit 31 set: its lowest set bit is always defined, and an exhausted mask reads row word
    //    31 (kRowOcc, inside the row), which nothing takes.
    //  The descriptor read ahead lives inside one scan(): rows are rebuilt before the first.
    //  (Where the registers allow: not the plain nearest-neighbour query on full records, k_icp<*, false, false, false>,
    //  69 -> 76 registers, nor k_loop at two lanes per query, one more spilled register; profiles/r19/resource_usage.txt.)
    constexpr bool AHEAD = SAGE_SCAN_AHEAD != 0 && !FLAT && (PERSIST ? W >= 4 : (FUSED || FILT));
    constexpr unsigned kNeedEnd = 0x80000000u;
    using Pair = std::conditional_t<FLAT, std::conditional_t<FILT, PairCompactFlat, PairFullFlat>,
                                    std::conditional_t<FILT, PairCompact, PairFull>>;
    auto scan = [&](unsigned need, const Point4 *seed, bool seeded, unsigned seed_key) {
        // flat order: the next point of this lane — its key, where its record lives, whether there is one
        auto next = [&](bool &h, unsigned &key, unsigned &o) {
            while (k >= kend && need) {        // past the end of the open voxel by k - kend points: on into the next
                const unsigned e = k - kend;
                const unsigned v = static_cast<unsigned>(__builtin_ctz(need));
                need &= need - 1u;
                const uint32_t w = lrow[v];
                kend = (v << 8) | (w & 255u);
                k = (v << 8) + e;
                off = (((w >> 8) * kUnitPoints) + e) << SHC;
                npairs += w & 255u;
            }
            h = k < kend;
            key = k;
            o = off;
            k += h ? static_cast<unsigned>(W) : 0u;
            off += h ? static_cast<unsigned>(W) << SHC : 0u;
        };
        auto pair_hb = [&](unsigned p) { return static_cast<int>(p) < -static_cast<int>(static_cast<unsigned>(W) << 16); };
        auto issue = [&](Pair &n, bool &more) {
            if constexpr (FLAT) {
                unsigned oa, ob;
                next(n.ha, n.ka, oa);
                next(n.hb, n.kb, ob);
                if constexpr (FILT) {
                    n.oa = oa;
                    n.ob = ob;
                    n.a = load_cand(cands, n.ha ? oa : 0u);
                    n.b = load_cand(cands, n.hb ? ob : 0u);
                } else {
                    n.a = load_point(pts, n.ha ? oa : 0u);
                    n.b = load_point(pts, n.hb ? ob : 0u);
                }
                __builtin_amdgcn_sched_barrier(0);
                more = (k < kend) | (need != 0u);
                return;
            } else if constexpr (AHEAD) {
                // (one test, not two nested ones)
                const bool adv = (static_cast<int>(pk) >= 0) & (needs != kNeedEnd);
                if (adv) {                                       // exhausted, and another voxel to open: at most one
                    const unsigned v = static_cast<unsigned>(__builtin_ctz(needs));
                    const unsigned cnt = wn & 255u;
                    pk = ((ci - cnt) << 16) + ((v << 8) | ci);
                    off = (((wn >> 8) * kUnitPoints) + ci) << SHC;
                    npairs += cnt;
                    needs &= needs - 1u;
                }
                n.ka = pk;                                       // (consume() reads ha, hb and the key from it)
                if constexpr (FILT) n.oa = off;
                n.ha = static_cast<int>(pk) < 0;
                n.hb = pair_hb(pk);
                const unsigned oa = n.ha ? off : 0u;             // (idle lanes re-read record 0, as below)
                if constexpr (FILT) {
                    n.a = load_cand(cands, oa);
                    n.b = load_cand(cands, oa, W << SHC);
                } else {
                    const unsigned ob = n.hb ? off + (static_cast<unsigned>(W) << SHC) : 0u;
                    n.a = load_point(pts, oa);
                    n.b = load_point(pts, ob);
                }
                __builtin_amdgcn_sched_barrier(0);
                pk += 2u * W * 0x10001u;
                off += (2u * W) << SHC;
                wn = lrow[__builtin_ctz(needs)];                 // the voxel after: in flight until the next issue()
                more = (static_cast<int>(pk) < 0) | (needs != kNeedEnd);
            } else {
            while (k >= kend && need) {        // open this lane's next voxel
                const unsigned v = static_cast<unsigned>(__builtin_ctz(need));
                need &= need - 1u;
                const uint32_t w = lrow[v];
                kend = (v << 8) | (w & 255u);
                k = (v << 8) | ci;
                off = (((w >> 8) * kUnitPoints) + ci) << SHC;
                npairs += w & 255u;
            }
            n.ha = k < kend;
            n.hb = k + W < kend;
            n.ka = k;
            if constexpr (FILT) n.oa = off;
            // issued by every lane (idle lanes re-read record 0): a load behind a branch would make
            // the compiler drain the whole queue before the other set is looked at
            const unsigned oa = n.ha ? off : 0u;
            if constexpr (FILT) {
                // (b lies W records behind a — a constant in the instruction; a lane without a b reads whatever
                // lies there, under the buffer's bounds check, and its `hb` drops it)
                n.a = load_cand(cands, oa);
                n.b = load_cand(cands, oa, W << SHC);
            } else {
                const unsigned ob = n.hb ? off + (static_cast<unsigned>(W) << SHC) : 0u;
                n.a = load_point(pts, oa);
                n.b = load_point(pts, ob);
            }
            // the filtering of the other set stays below these loads (the scheduler would
            // otherwise sink them under the arithmetic it believes is ready)
            __builtin_amdgcn_sched_barrier(0);
            // (a lane past the end of its voxel keeps counting: the next voxel it opens sets k and off afresh)
            k += 2u * W;
            off += (2u * W) << SHC;
            more = (k < kend) | (need != 0u);
            }
        };
        auto consume = [&](const Pair &n) {
            unsigned kb;                        // b's key: W points on in a's voxel, or its own (flat order)
            const unsigned ka = AHEAD ? n.ka & 0xFFFFu : n.ka;
            const bool ha = AHEAD ? static_cast<int>(n.ka) < 0 : n.ha, hb = AHEAD ? pair_hb(n.ka) : n.hb;
            if constexpr (FLAT) kb = n.kb; else kb = ka + W;
            if constexpr (!FILT) {
                evaluate(n.a, ha, ka);
                evaluate(n.b, hb, kb);
            } else {
            // (the candidate already held — the seed met again in its voxel — needs no second look)
            float dla, dlb;
            const float da = dist32(n.a, dla), db = dist32(n.b, dlb);
            const bool la = ha & !(da > Tmax) & (ka != bkey), lb = hb & !(db > Tmax) & (kb != bkey);
            PROBE_NN_CONSUME(np);
            if (__ballot(la | lb)) {
            const bool pa = la & tight(n.a, da, dla), pb = lb & tight(n.b, db, dlb);
            if (__ballot(pa | pb)) {
                // rarer and rarer as the registration settles (a fifth of the pair steps at the
                // start of a cold one, 2 % near convergence): the full records of the candidates
                // that passed (a compact offset is half the byte offset of the full record).
                // (Parking them and fetching in batches was tried: more registers, no fewer trips.)
                PROBE_NN_EXACT(np, pa, pb);
                unsigned ob;
                if constexpr (FLAT) ob = n.ob; else ob = n.oa + (static_cast<unsigned>(W) << SHC);
                const Point4 ea = load_point(pts, pa ? n.oa << 1 : 0u);
                const Point4 eb = load_point(pts, pb ? ob << 1 : 0u);
                evaluate(ea, pa, ka);
                evaluate(eb, pb, kb);
                fb = min_f64(fb, best);
                set_thresholds();
            }
            }
            }
        };
        // (k_loop has registers to spare — a few waves per SIMD, 128 registers each — and an iteration
        // of it ends with its SLOWEST wave, so three / four sets in flight were tried there:
        // 15k queries 18.8 -> 19.9 us per iteration with three sets
        // of full records, 20.6 -> 22.0 with four of compact ones (profiles/r04/loop_depth.txt) — the
        // slow waves are not waiting for their loads.  Two sets everywhere; the switch is gone.)
        Pair A, B;
        bool more = false;
        if constexpr (AHEAD) {
            pk = 0u;                            // no voxel open
            off = 0u;
            needs = need | kNeedEnd;
            wn = lrow[__builtin_ctz(needs)];
        }
        issue(A, more);
        // the seed's load is older than A's: waiting for it leaves A's loads in flight
        if (seed) evaluate(*seed, seeded, seed_key);
        fb = min_f64(fb, best);
        set_thresholds();
        // One exit per double step: an exit between the two halves gives the loop header a
        // predecessor with B's loads pending, and the compiler then drains the queue (vmcnt(0))
        // before every issue(B) — the overlap this loop exists for.  A scan that ends after the
        // first half pays one idle half step instead.
        // (Peeling short scans out of the loop — one pair step, or none — was tried: the extra
        // paths cost 10 registers and spills, every workload lost 5-10 %.)
        for (;;) {
            issue(B, more);
            consume(A);
            issue(A, more);
            consume(B);
            if (!__ballot((AHEAD ? static_cast<int>(A.ka) < 0 : A.ha) | more)) break;
        }
    };

    // The previous iteration's nearest neighbour is still a point of this neighbourhood as long as
    // the home voxel has not changed (the row, and with it the meaning of `key`, is the same; the
    // map is constant during a call): evaluated first, it gives every query — also one whose
    // home voxel is empty — a tight bound before anything is scanned.  It is an ordinary
    // candidate: meeting it again in the scan changes nothing.
    constexpr unsigned kHome = 13u;
    bool merged = false;                       // this query's home voxel is scanned with its neighbours
    if constexpr (PERSIST) {
        // k_loop holds the seed's record in registers: a seeded query takes its bound from the seed
        // alone — no memory — and scans its home voxel together with the neighbours that survive
        // that bound, in ONE pass (any bound at or above the final best prunes exactly; after the
        // first iterations the seed IS the answer for most queries and the bound is the final
        // one).  Only queries without a seed (the first pass of a call, a rebuilt row) scan their
        // home voxel first; a wave without such a query skips that pass altogether.
        const bool seeded = valid && prev.x != 0xFFFFFFFFu;          // (a rebuilt row re-keyed or dropped it)
        const Point4 pp = *reinterpret_cast<const Point4 *>(lst + 8);
        evaluate(pp, seeded, prev.x);
        merged = seeded;
        const unsigned first = seeded ? 0u : (occ & (1u << kHome));
        if (__ballot(first != 0u)) scan(first, nullptr, false, 0u);
    } else if (FUSED) {
        const bool seeded = valid && prev.x != 0xFFFFFFFFu;          // (a rebuilt row re-keyed or dropped it)
        const Point4 pp = load_point(pts, seeded ? prev.y : 0u);      // the full record
        scan(occ & (1u << kHome), &pp, seeded, prev.x);
    } else {
        scan(occ & (1u << kHome), nullptr, false, 0u);
    }
    NN_T(np, 2);
    LP_T(PERSIST, G, 2);
    // what the query holds after its home voxel (or its seed) bounds the rest of its search
    const double bound = seg_min_f64<W>(best);
    fb = bound;                                // (set_thresholds runs at the start of the scan)
    unsigned need = P.keep_all;
    if constexpr (W >= 4) {
        // The 26 bound tests are the same for every lane of the query: lane a < 3 takes the x-layer
        // a (nine voxels, one add and one compare each on top of the shared gy + gz sums), the
        // layers meet in two DPP exchanges.  Same operands, same association: the same mask as
        // the loop below, in 40 instructions instead of 100.
        // (k_loop: from the lane index anew — make_query's copy of these two bits otherwise lives through the first scan)
        const unsigned a = (PERSIST ? static_cast<unsigned>(lane_now()) : ci) & 3u;
        const double ga = a == 0u ? gx[0] : (a == 2u ? gx[2] : 0.0);
        unsigned layer = 0u;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double lb = ga + (gy[b] + gz[c]);
                layer |= (lb <= bound) ? (1u << (3 * b + c)) : 0u;
            }
        }
        layer = (a < 3u && ci < 4u) ? layer << (9u * a) : 0u;
        layer |= dpp_u32<kDppXor1>(layer);
        layer |= dpp_u32<kDppXor2>(layer);          // lanes 0..3 of the query now hold all three layers
        if (W >= 8) layer |= dpp_u32<kDppHalfMirror>(layer);
        if (W >= 16) layer |= dpp_u32<kDppMirror>(layer);
        need |= layer & ~(1u << kHome);
    } else {
#pragma unroll
        for (int v = 0; v < 27; ++v) {
            if (v == static_cast<int>(kHome)) continue;
            const double lb = gx[v / 9] + (gy[(v / 3) % 3] + gz[v % 3]);
            need |= (lb <= bound) ? (1u << v) : 0u;
        }
    }
    LP_T(PERSIST, G, 3);
    scan((merged ? (need | (1u << kHome)) : (need & ~(1u << kHome))) & occ, nullptr, false, 0u);
    LP_T(PERSIST, G, 4);
    if constexpr (PERSIST) {
        // what this block cost: the most points one of its queries was handed (a rebuilt row counts as a few more) —
        // next iteration's order of the workgroup's blocks (k_loop)
        // (the lane index anew, from it the block's slot in this iteration's order again, and with that where the
        // query's state record lies: none of them is kept across the scans)
        lane = lane_now();
        const unsigned qe = static_cast<unsigned>(lane) >> LW;
        const unsigned bs = G->perm[G->unit * (QW / 4) + (qe >> 2)];
        lst = G->state + (bs * 4u + (qe & 3u)) * kLoopStateWords;
        if (valid && ci == 0u)
            (void)__hip_atomic_fetch_max(G->work + bs, npairs + (stale ? 48u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }

    unsigned mkey, woff;
    const bool found = reduce_argmin<LW>(best, bkey, valid, lrow, mkey, woff);
    NN_T(np, 3);
    LP_T(PERSIST, G, 5);

    if (P.counters) {                          // C_q and pairs handed out, summed over the wave
        // (both fit 16 bits per query: one packed value goes through the four DPP exchanges inside
        // the rows of 16 lanes, four v_readlane collect the rows; the wave's private slot takes the
        // sums as fire-and-forget atomics — a read-modify-write would hold the wave for a round trip)
        const unsigned long long ab = (valid && ci == 0u)
                                          ? (static_cast<unsigned long long>(lrow[kRowCq]) << 32) | npairs : 0ull;
        unsigned lo = static_cast<unsigned>(ab), hi = static_cast<unsigned>(ab >> 32);
        lo += dpp_u32<kDppXor1>(lo);        hi += dpp_u32<kDppXor1>(hi);
        lo += dpp_u32<kDppXor2>(lo);        hi += dpp_u32<kDppXor2>(hi);
        lo += dpp_u32<kDppHalfMirror>(lo);  hi += dpp_u32<kDppHalfMirror>(hi);
        lo += dpp_u32<kDppMirror>(lo);      hi += dpp_u32<kDppMirror>(hi);
        unsigned b = 0u, a = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            b += static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(lo), 16 * r));
            a += static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(hi), 16 * r));
        }
        if (lane == 0 && wave_id < P.nwaves) {
            (void)__hip_atomic_fetch_add(&P.counters[2u * wave_id], static_cast<unsigned long long>(a),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(&P.counters[2u * wave_id + 1u], static_cast<unsigned long long>(b),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    if (!FUSED) {
        if (valid && ci == 0u) P.nn_idx[q] = found ? static_cast<int>(woff >> SH) : -1;
    } else {
        // ---- fused epilogue: acceptance + Gauss-Newton terms of this query's pair -----------------
        if constexpr (!PERSIST) {
            if (valid && ci == 0u) P.nn_prev[q] = make_uint2(found ? mkey : 0xFFFFFFFFu, woff);
        }
        Point4 g;
        if constexpr (PERSIST) {
            // The answer of most queries is the previous iteration's (and then so is its record: the
            // map is constant during a call, and the key was carried over if the row was rebuilt):
            // only a query whose answer changed fetches a record, on all of its lanes (one request:
            // the same address), since every lane evaluates the seed.
            const bool changed = found && mkey != lst[opaque_v(kStPrev)];
            g = *reinterpret_cast<const Point4 *>(lst + 8);
            if (__ballot(changed)) {
                const Point4 t = load_point(pts, changed ? woff : 0u);
                if (changed) {
                    g = t;
                    if (ci == 0u) *reinterpret_cast<Point4 *>(lst + 8) = t;
                }
            }
            if (ci == 0u) *reinterpret_cast<uint2 *>(lst + kStPrev) = make_uint2(found ? mkey : 0xFFFFFFFFu, woff);
            LP_T(PERSIST, G, 6);
        }
        PROBE_NN_WORK(P, q, valid && ci == 0u, npairs);
        // Branch-free: every lane of a query computes the terms of the query's pair and keeps the K = 16 / W of
        // them wave_terms_to_wgacc takes from it (components ci K .. ci K + K - 1), zeroed unless the query has an
        // accepted answer (exact zeros of either sign, which the block sums and their digits do not tell apart).
        // One lane per query (W = 1) zeroes the operands instead: clearing sixteen fp64 registers twice around
        // two nested branches cost more than the selects.
        constexpr int K = kCount >> LW;
        double t[K];
        if constexpr (!PERSIST) g = load_point(pts, found ? woff : 0u);     // (a query without an answer re-reads record 0: no branch)
        const double rx0 = s.x - g.x, ry0 = s.y - g.y, rz0 = s.z - g.z;
        // (closest_neighboor - point).head<3>().norm() < max_correspondance_distance (VoxelHashMap.cpp:111)
        const bool use = found && SAGE_SQNORM3_ACCEPT(rx0 * rx0, ry0 * ry0, rz0 * rz0) <= P.accept_r2;
        {
            // residual.squaredNorm() (Registration.cpp:79): its own reduction (sageicp_types.h)
            const double r2 = SAGE_SQNORM3_RESID(rx0 * rx0, ry0 * ry0, rz0 * rz0);
            const double k = P.kernel;
            const double den = k + r2;
            const double wq = (k * k) / (den * den);   // square(th) / square(th + residual2)
            const bool z = W == 1;                     // zero the operands (W = 1) or the kept terms
            const double w = !z || use ? wq : 0.0;
            const double sx = !z || use ? s.x : 0.0, sy = !z || use ? s.y : 0.0, sz = !z || use ? s.z : 0.0;
            const double rx = !z || use ? rx0 : 0.0, ry = !z || use ? ry0 : 0.0, rz = !z || use ? rz0 : 0.0;
            const double wsx = w * sx, wsy = w * sy, wsz = w * sz;
            double u[kCount];
            u[kW] = w;
            u[kWsx] = wsx; u[kWsy] = wsy; u[kWsz] = wsz;
            u[kWxx] = wsx * sx; u[kWxy] = wsx * sy; u[kWxz] = wsx * sz;
            u[kWyy] = wsy * sy; u[kWyz] = wsy * sz; u[kWzz] = wsz * sz;
            u[kWrx] = w * rx; u[kWry] = w * ry; u[kWrz] = w * rz;
            u[kWcx] = w * (sy * rz - sz * ry);
            u[kWcy] = w * (sz * rx - sx * rz);
            u[kWcz] = w * (sx * ry - sy * rx);
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
                double v = u[kk];
#pragma unroll
                for (int l = 1; l < W; ++l) v = ci == static_cast<unsigned>(l) ? u[l * K + kk] : v;
                t[kk] = z || use ? v : 0.0;
            }
        }
        const unsigned pairs = static_cast<unsigned>(__popcll(__ballot(use && ci == 0u)));
        if constexpr (PERSIST) {
            // k_loop: block sums -> exact digits -> the workgroup's accumulators (the rows stay: the scratch
            // is the running wave's own)
            wave_terms_to_wgacc<LW, true>(t, pairs, lane, G->red, G->wgacc, kDigitLimitCounted, P.acc_scale);
            PROBE_LOOP_WAVE_STATS(smem, valid, ci, npairs, stale, lane);
            LP_T(PERSIST, G, 7);
            return;                             // (k_loop closes the workgroup's iteration itself)
        }
        if (P.stripe_work) {
            // (an iteration that measures: the most points one of this wave's queries was handed -> the stripe's heaviest wave)
            unsigned mx = valid ? npairs : 0u;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) mx = max(mx, static_cast<unsigned>(__shfl_xor(mx, d, 64)));
            if (lane == 0) (void)__hip_atomic_fetch_max(&P.stripe_work[stripe_id], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        {
            // k_icp: the same, into this workgroup's accumulators; the last wave to arrive sends them on
            // (what the ticket orders lives in LDS, which serves a CU's waves in order: the ticket is a
            // relaxed LDS atomic between compiler barriers)
            unsigned long long *wgacc = reinterpret_cast<unsigned long long *>(smem + kWgAcc);
            wave_terms_to_wgacc<LW>(t, pairs, lane, reinterpret_cast<double *>(wl), wgacc, P.digit_limit, P.acc_scale);
            unsigned prior = 0u;
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            if (lane == 0)
                prior = __hip_atomic_fetch_add(&smem[kWgArrive], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            prior = __builtin_amdgcn_readfirstlane(prior);
            if (prior == kIcpWavesPerBlock - 1u) {
                if (P.chain)
                    wgacc_flush<true>(wgacc, &P.chain->acc32[P.chain_iter & 1][blockIdx.x & (kChainReplicas - 1)][0], nullptr);
                else
                    wgacc_flush(wgacc, P.acc + static_cast<size_t>(blockIdx.x & (kAccReplicas - 1)) * kAccWords,
                                P.acc + kAccWords - 1);
            }
        }
    }
    PROBE_NN_END(np, P, valid, ci, npairs, lane, wave_id);
}

}  // namespace sageicp
