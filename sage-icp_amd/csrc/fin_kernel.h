// The launch-per-iteration finish: k_fin, one workgroup that turns an iteration's sums into the next pose, and what it is
// made of.  Included by kernels.hip only, inside its translation unit (it calls the lane helpers defined there).
#pragma once

namespace sageicp {

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
// Executed by ONE workgroup of 1024 threads once per ICP iteration (k_fin): the sums — from the fixed-point
// accumulators k_icp's workgroups added into (reduce_accumulators; exact, so bit-reproducible), or, for the
// stand-alone k_gn entry, from its per-workgroup partials in a fixed order —, then the first wave solves the normal
// equations from the 16 closed-form sums (se3_math.h solve_normal_equations_t: the block-structured
// solve, the register-resident pivoted 6x6 LDL^T where its guard refuses), applies SE3 exp, composes
// the pose and tests convergence (Registration.cpp:92-93,135-137).
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
    PROBE_FIN_BEGIN(fin_t);
    FIN_STAMP(fin_t, 1);
    const int lane = static_cast<int>(threadIdx.x);
    double x[6], est[7], nrm;
    solve_normal_equations_t<WaveLanes>(S, x);
    FIN_STAMP(fin_t, 2);
    se3_exp_sqrt_t<WaveLanes>(x, est, SAGE_SQNORM6(x), nrm);        // nrm = |x|, beside the exponential's sqrt
    FIN_STAMP(fin_t, 3);

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
    PROBE_FIN_END(fin_t);
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
    PROBE_FIN_START(t_start);
    FinState pre{};
    if (threadIdx.x < 64) pre = prefetch_state(st);
    if (P.mode != 2) {
        if (P.acc) {
            if (!reduce_accumulators(P.acc, S, P.standalone ? nullptr : &st->done, &st->acc_overflow, P.acc_unscale)) return;
        } else if (!reduce_partials(P.partials, P.nparts, S, P.standalone ? nullptr : &st->done)) return;
        PROBE_FIN_REDUCED(t_start);
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

}  // namespace sageicp
