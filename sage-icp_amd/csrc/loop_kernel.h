// The one-launch ICP loop: k_loop, the grid of query workgroups, and k_loop_solve, the solving wave beside it.  Included by
// kernels.hip only, inside its translation unit, after icp_body.h (what the body and the loop share — LoopGroup, the kLp*
// words of the LDS header, LoopLds — is defined in kernels.hip ahead of both).
#pragma once

#include "loop_deal.h"

namespace sageicp {

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
//   every wave        behind a barrier (the closing wave has written the next order of the blocks): runs the front of
//                     its first pass of the next iteration, the part that does not need the pose (icp_body, HALF 1);
//   wave 0 of every   polls its XCD's granules (one relaxed agent-scope load per lane and pass), hands the
//   workgroup         pose to its workgroup through LDS;  __syncthreads();  the staged passes go on with the pose.
// Every word the workgroups share is accessed with agent-scope atomics only.  Every wait is bounded:
// a timeout raises LoopShared::abort_word and IcpState::loop_aborted, everybody leaves, and the host
// registers the frame through the launch-per-iteration loop instead (a grid that is not fully
// resident — another process or stream holding CUs — ends this way, not in a hang).

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
// The solving wave gives the loop up at iteration `it` (tag = it + 1: its own wait timed out, somebody raised the abort
// word, or — `peer` — a peer GPU gave up at this exchange).  `sh`, `st`: L.sh and L.st as the caller holds them (read
// from L again they cost the solving kernels scalar loads).  Writes: the abort word, which every workgroup's wait looks at;
// IcpState::loop_aborted [and peer_aborted], for the host; the progress word (chained launches: the host stops
// enqueuing); and every pose copy's done word with this iteration's tag and the value 2.
__device__ __forceinline__ void loop_give_up(const LoopParams &L, LoopShared *sh, IcpState *st, int it, unsigned long long tag, int lane,
                                             bool peer) {
    if (lane == 0) {
        st_agent(&sh->abort_word[0], 1ull);
        st->loop_aborted = 1;
        if (peer) st->peer_aborted = 1;
        if (L.progress)
            __hip_atomic_store(&L.progress->word, (1ull << 32) | static_cast<unsigned long long>(it), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (const int al = lane_now(); al < kLoopPoseCopies) st_agent(&sh->pose[al][24], (tag << 32) | 2ull);
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
                loop_give_up(L, sh, st, it, tag, lane, false);
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
            loop_give_up(L, sh, st, it, tag, lane, true);
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

// A SIMD's issue slots go to its waves by priority: the wave with the heaviest unit of its workgroup (the
// units are ordered by last iteration's work) runs at the highest, the lightest at the lowest, a unit beyond
// one per wave — it starts late — at `prio` (3 by default).  The work of a SIMD does not change with the order, but
// its END does: the long chains run while there is other work to fill their stalls with, and what
// is left to run alone at the end of an iteration are the short ones (c2: 31.2 -> 28.2 us per iteration,
// profiles/r06/deal_ab.txt).
// Reads: the unit `gi` this wave has taken, the waves per workgroup, LoopParams::prio.  Writes: the wave's priority.
__device__ __forceinline__ void loop_set_priority(unsigned gi, int nw, int prio) {
    const unsigned rk = gi >= static_cast<unsigned>(nw) ? static_cast<unsigned>(prio) : 3u - min(gi, 3u);
    switch (rk) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

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
    // (set-up only; the iteration loop below takes what it needs of this from its arguments and through opaque_s)
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
    constexpr unsigned BPW = QW / 4;                                  // blocks of four queries per pass
    // (set-up only, like nw and gpw: the iteration loop lays the LDS out again from its arguments)
    const unsigned nblk_max = gpw * BPW;
    const LoopLds<unsigned> lds0(LW, static_cast<unsigned>(nw), gpw); // (kernels.hip: the one description of this LDS)
    uint32_t *perm0 = smem + lds0.perm;
    uint32_t *work0 = smem + lds0.work;
    uint32_t *state0 = smem + lds0.state;

    // ---- set-up: the initial pose, the state records of the groups' queries --------------------------
    if (threadIdx.x < 9) s_pose[threadIdx.x] = P.st->R[threadIdx.x];
    else if (threadIdx.x < 12) s_pose[threadIdx.x] = P.st->T[4 + threadIdx.x - 9];
    if (threadIdx.x == 0) {
        smem[kLpArrive] = 0u;
        smem[kLpNext] = 0u;
        smem[kLpDone] = 0u;
        smem[kLpIter] = 0u;
        PROBE_LOOP_CLEAR_STATS(smem);
    }
    if (L.deal && (threadIdx.x & 63u) == 0u) {
        // The heaviest unit of a workgroup (its blocks are ordered by work) should not meet the heaviest units of the
        // other workgroups of its CU on one SIMD: a workgroup's four waves sit on the four SIMDs, one wave of every
        // workgroup of the CU per SIMD, and a SIMD's issue slots are what its waves share.  Workgroup r of the CU
        // (its waves' slot number) hands unit (s + r) mod waves to its wave on SIMD s: every SIMD gets the same mix.
        // That holds for the first four workgroups of a CU; the rows of the fifth to the seventh come from a table that
        // levels what goes WITH the second heaviest unit two or three SIMDs then hold (loop_deal.h; L.deal == 2: the
        // formula for every row).
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        const unsigned simd = (hw >> 4) & 3u, slot = hw & 15u;
        smem[kLpFirst + static_cast<unsigned>(wv)] = L.deal == 2 ? loopdeal::formula(simd, slot, static_cast<unsigned>(nw))
                                                                 : loopdeal::loop_deal_unit(simd, slot, static_cast<unsigned>(nw));
    }
    for (unsigned i = threadIdx.x; i < 2u * kWgAccWords; i += blockDim.x) smem[kLpAcc + i] = 0u;
    for (unsigned i = threadIdx.x; i < nblk_max; i += blockDim.x) {
        perm0[i] = i;                          // the order of the frame, until the blocks' work is known
        work0[i] = 0u;
    }
    for (unsigned sl = threadIdx.x; sl < gcnt * QW; sl += blockDim.x) {
        const unsigned q = g0 * QW + sl;       // slot sl of this workgroup
        const Point4 f = P.frame[q < static_cast<unsigned>(P.n) ? q : 0u];
        {
            uint32_t *lst = state0 + sl * kLoopStateWords;
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
    // who this wave is, in ONE scalar for the loop below: the workgroup's index and, in the low three bits, its wave
    static_assert(kLoopMaxWaves <= 8, "k_loop keeps the wave's index in three bits");
    const unsigned who = (blockIdx.x << 3) | static_cast<unsigned>(wv);
    PROBE_LOOP_BEGIN(lp);

    // THE RULE of the iteration loop: nothing derived from threadIdx or blockIdx, and no predicate, offset or pointer
    // derived from the set-up's scalars, is used inside it.  Three scalars cross it as VALUES — `who`, `g0` and `gcnt`,
    // each read through opaque_s where it is used —; the lane index is lane_now() at every use; nw, gpw and the LDS
    // layout come from the arguments, re-read where they are needed (scalar loads from the constant cache, as a wave of
    // k_icp does at its start).  What the compiler can prove invariant it hoists in front of the loop and keeps alive
    // across the pass: at 72 registers that meant 48 B of scratch and 32 scalars parked in a register's lanes, reloaded
    // inside the pass or not as the allocation fell (5 % of c2, profiles/r20/README.md).  tests/test_loop_resources.py
    // holds the kernels at no scratch.  (icp_body follows the same rule for the values of a pass: icp_body.h.)  The
    // iteration's number is not among them: the workgroup's LDS header has it (kLpIter, counted by the closing wave), and
    // the two places that need it — the poll's tag, the close's accumulator set — read it there.

    for (;;) {
        PROBE_LOOP_IT(it, smem);
        // The workgroup's units.  A pass is cut in two (icp_body, HALF): the half that does not need the pose — arguments,
        // unit, priority, LDS layout, `perm`, the query's state record — and the rest.  A wave's FIRST pass of an iteration
        // is staged in front of the wait for that pose: the wave leaves the barrier behind the wait with its query in
        // registers, and the next thing it does is read the pose.  The units beyond one per wave go first come first
        // served, staged behind the run before: a wave held up by a heavy query takes fewer.  (One copy of the run half
        // in the code; the stage half, some forty instructions, stands twice.)
        // ("no unit" is a value of `gi`, and the staged values are set on every path, also the one that stages nothing: a
        // flag sat in a register pair all through the run half, and a value left open on one path into the wait is, to the
        // register allocator, one that lives round the loop)
        constexpr unsigned kNoUnit = 0xFFFFFFFFu;
        LoopStaged S{};
        PROBE_LOOP_UNIT_VAR(t_unit);
        // where unit `u` of the workgroup lies, from the arguments `B` (the LDS layout is not carried from the stage half
        // to the run half: each lays it out for itself, beside its other scalar work and under its LDS reads — carried, it
        // was eight more scalars to hold through the run half, and k_loop<2, true> spilled four)
        auto group_of = [&](unsigned u, const LoopArgs &B) {
            const LoopLds<unsigned> lds(LW, static_cast<unsigned>(B.L.nw), static_cast<unsigned>(B.L.gpw));
            const unsigned first_unit = opaque_s(g0);
            LoopGroup G;
            G.rows = smem + lds.rows;
            G.state = smem + lds.state;
            G.perm = smem + lds.perm;
            G.work = smem + lds.work;
            G.unit = u;
            G.red = reinterpret_cast<double *>(smem + lds.red + (opaque_s(who) & 7u) * loop_red_words());
            G.wgacc = reinterpret_cast<unsigned long long *>(smem + kLpAcc);
            G.q_first = first_unit * QW;
            G.slot = first_unit + u;
            return G;
        };
        // takes unit `u`: the wave's priority, the stage half of the pass
        auto stage = [&](unsigned u) {
            // (the pass's arguments, and where the workgroup's LDS lies, from the kernel-argument segment: see above)
            auto kb = __builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(kb));
            const LoopArgs &B = *(const LoopArgs *)(kb);
            if (B.L.prio) loop_set_priority(u, B.L.nw, B.L.prio);
            PROBE_LOOP_UNIT_BEGIN(it, u, B.L.nw, t_unit);
            LoopGroup G = group_of(u, B);
            icp_body<LW, true, FILT, true, false, 1>(B.P, smem, &G, nullptr, &S);
        };
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        unsigned gi = kNoUnit;
        // (this wave's first unit is fixed by where it sits; without the deal, or with more waves than units, it stages
        // nothing and goes to the counter behind the barrier)
        if (((const LoopArgs *)(ka))->L.deal) {
            gi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(smem[kLpFirst + (opaque_s(who) & 7u)])));
            if (gi >= opaque_s(gcnt)) gi = kNoUnit;
        }
        if (gi != kNoUnit) stage(gi);
        {
            const LoopParams &L = ((const LoopArgs *)(ka))->L;
            // the pose of this iteration, for this workgroup (the first iteration's is the set-up's)
            // (the iteration's number, as the wait needs it — test, tag —, from the workgroup's header)
            const unsigned itn = (opaque_s(who) & 7u) == 0u ? static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(smem[kLpIter]))) : 0u;
            if (itn != 0u) {
                LoopShared *sh = L.sh;
                const int lane = lane_now();
                const unsigned wg = opaque_s(who) >> 3;
                const unsigned long long tag = static_cast<unsigned long long>(itn);
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                unsigned long long g = tag << 32;
                bool aborted = false;
                for (;;) {
                    if (lane < kLoopPoseGranules) g = ld_agent(&sh->pose[loop_pose_copy(L.pose_map, wg)][lane]);
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
                    if (lane < 24) smem[kLpPose + static_cast<unsigned>(lane)] = static_cast<uint32_t>(g);
                    if (lane == 24) smem[kLpDone] = static_cast<uint32_t>(g);
                }
                LOOP_STAMP_WG(itn - 1u, 1);
            }
        }
        PROBE_LOOP_WAIT_BEGIN(t_b);
        __syncthreads();
        PROBE_LOOP_WAITED(lp, t_b);
        // (a wave that leaves here has staged and written nothing)
        if (smem[kLpDone]) break;
        for (;;) {
            if (gi != kNoUnit) {
                auto kb = __builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(kb));
                const LoopArgs &B = *(const LoopArgs *)(kb);
                LoopGroup G = group_of(opaque_s(gi), B);
                PROBE_LOOP_PASS_BEGIN(lp, G);
                icp_body<LW, true, FILT, true, false, 2>(B.P, smem, &G, reinterpret_cast<const double *>(smem + kLpPose), &S);
                PROBE_LOOP_UNIT_END(lp, G, it, gi, B.L.nw, static_cast<int>(opaque_s(who) & 7u), lane_now(), t_unit);
                PROBE_LOOP_UNIT_WORK(G, it, gi, BPW, lane_now());
            }
            gi = 0u;
            if (lane_now() == 0)
                gi = __hip_atomic_fetch_add(&smem[kLpNext], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            gi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(gi)));
            if (gi >= opaque_s(gcnt)) break;
            stage(gi);
        }
        PROBE_LOOP_MARK(t_a);
        // the close: its arguments and its lane index anew (nothing of the passes' is kept for it)
        auto kc = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kc));
        const LoopParams &L = ((const LoopArgs *)(kc))->L;
        LoopShared *sh = L.sh;
        const int lane = lane_now();
        const unsigned me = opaque_s(who), wg = me >> 3;
        // (what the ticket orders — the groups' sums — lives in LDS, which serves a CU's waves in order)
        unsigned prior = 0u;
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if (lane == 0)
            prior = __hip_atomic_fetch_add(&smem[kLpArrive], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        prior = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(prior)));
        const bool last = prior == static_cast<unsigned>(L.nw) - 1u;
        if (last) {
            // this wave closes the workgroup's iteration, and counts it
            const int it = __builtin_amdgcn_readfirstlane(static_cast<int>(smem[kLpIter]));
            wgacc_flush<true, true>(reinterpret_cast<unsigned long long *>(smem + kLpAcc), &sh->acc[it & 1][wg & (kLoopReplicas - 1)][0],
                                    &sh->acc[it & 1][0][kAccWords - 1]);
            if (lane == 0) {                   // everybody is in: ready for the next iteration
                smem[kLpArrive] = 0u;
                smem[kLpIter] = static_cast<unsigned>(it) + 1u;
                smem[kLpNext] = L.deal ? static_cast<unsigned>(L.nw) : 0u;
            }
            // The next iteration's order of the workgroup's blocks: heaviest first, by what they cost in this one (a
            // rank sort on one wave: lane i counts the blocks that go before block i).  Blocks of like work then
            // share a wave — whose pass lasts as long as its heaviest query — and the heaviest waves start first.
            // (Which blocks share a wave does not reach the sums: they are exact from the block on.)
            const unsigned nblk = opaque_s(gcnt) * BPW;
            if (nblk <= 64u && nblk > BPW) {
                const LoopLds<unsigned> lds(LW, static_cast<unsigned>(L.nw), static_cast<unsigned>(L.gpw));
                uint32_t *perm = smem + lds.perm, *work = smem + lds.work;
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
            PROBE_LOOP_WG_INFO(smem, it, lane);
            LOOP_STAMP_WG(it, 0);
        }
        PROBE_LOOP_CLOSED(lp, last, t_a);
        PROBE_LOOP_WAIT_BEGIN(t_c);
        // the closing wave has written the next iteration's `perm`, unit counter and arrival count: nobody stages before
        // (the waves waited at the barrier behind the poll for just as long before: the pose cannot come before the close)
        __syncthreads();
        PROBE_LOOP_WAITED(lp, t_c);
    }
    PROBE_LOOP_END(lp);
}

}  // namespace sageicp
