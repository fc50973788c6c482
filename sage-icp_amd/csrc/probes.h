// Instrumentation of the search body (icp_body.h, icp_body) for the probe builds under profiles/ — none of it is in the
// product: every macro below is empty unless its switch is defined when the library is built
// (python sage-icp_amd/build.py <out.so> -DSAGE_NN_TIMING ...; tests/test_probe_variants.py compiles each so they do not rot).
//
//   SAGE_NN_TIMING        k_icp: shader cycles per phase of a wave, its lifetime, the span of one chosen launch per wave
//                         (profiles/icp_tail.py, phase_probe.py); sageicp_debug_nn_phases / _nn_raw / _nn_spans
//   SAGE_LOOP_TIMING      k_loop: cycles per phase of a pass, per-workgroup / per-wave / solver stamps (profiles/loop_tail.py,
//                         loop_times.py, solve_split.py) — the stamps of the loop itself stay in kernels.hip beside the loop
//   SAGE_ICP_DELAY_PROBE  k_icp: the pose arrives `dbg_delay` ticks after a wave's start / the pass repeated inside the launch
//
// A probe is one line in the body and takes what it reads as arguments: the kernel's parameters, the pass's LoopGroup,
// the body's own values, and `np` / `t0` — the probe's state, a local that PROBE_NN_BEGIN / PROBE_DELAY_BEGIN declare
// under the name they are given (nothing in the product).
#pragma once

namespace sageicp {

// ---------------------------------------------------------------------------------------------- SAGE_NN_TIMING
#ifdef SAGE_NN_TIMING
constexpr unsigned kNnTimingSlots = 1u << 17;
__device__ unsigned long long g_nn_phase[8ull * kNnTimingSlots];   // per wave: 5 phases, lifetime, realtime, count
__device__ unsigned long long g_nn_span[4ull * kNnTimingSlots];    // per wave, iteration g_nn_span_iter: start, end (100-MHz ticks), HW_ID, pairs
__device__ int g_nn_span_iter;
// what a wave's probes keep from one call to the next
struct NnProbe {
    unsigned long long tph[5] = {0, 0, 0, 0, 0};                            // cycles per phase (NN_T)
    unsigned long long tprev = __builtin_amdgcn_s_memtime();                // the last stamp
    unsigned long long tstart = tprev;
    unsigned long long rstart = __builtin_amdgcn_s_memrealtime();
    unsigned n_consume = 0u, n_exact = 0u, n_exact_lanes = 0u;              // pair steps | with a fetch of full records | lanes that fetched
};
#define PROBE_NN_BEGIN(np) NnProbe np
#define NN_T(np, i) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); (np).tph[i] += _t - (np).tprev; (np).tprev = _t; } while (0)
#define PROBE_NN_CONSUME(np) ++(np).n_consume
#define PROBE_NN_EXACT(np, pa, pb) do { ++(np).n_exact; (np).n_exact_lanes += static_cast<unsigned>(__popcll(__ballot(pa)) + __popcll(__ballot(pb))); } while (0)
#define PROBE_NN_WORK(P, q, first_lane, npairs) do { if ((first_lane) && (P).work) (P).work[q] = (npairs); } while (0)
// private slot per wave (no contended atomics: they would stall the very loads being timed)
#define PROBE_NN_END(np, P, valid, ci, npairs, lane, wave_id)                                                              \
    do {                                                                                                                   \
        NN_T(np, 4);                                                                                                       \
        unsigned long long np_packed, xp_packed;                                                                           \
        {   /* points handed to the queries of this wave: max over the queries | sum */                                    \
            unsigned mx = (valid) ? (npairs) : 0u, sm = ((valid) && (ci) == 0u) ? (npairs) : 0u;                           \
            for (int d = 1; d < 64; d <<= 1) {                                                                             \
                mx = max(mx, static_cast<unsigned>(__shfl_xor(mx, d, 64)));                                                \
                sm += __shfl_xor(sm, d, 64);                                                                               \
            }                                                                                                              \
            np_packed = (static_cast<unsigned long long>(mx) << 32) | sm;                                                  \
            /* pair steps of this wave | of them with a fetch of full records | lanes that fetched */                      \
            xp_packed = (static_cast<unsigned long long>((np).n_consume) << 40) | (static_cast<unsigned long long>((np).n_exact) << 20) | (np).n_exact_lanes; \
        }                                                                                                                  \
        if ((lane) == 0 && (wave_id) < kNnTimingSlots && (wave_id) < (P).nwaves) {                                         \
            unsigned long long *tt = g_nn_phase + 8ull * (wave_id);                                                        \
            for (int k = 0; k < 5; ++k) tt[k] += (np).tph[k];                                                              \
            tt[5] += __builtin_amdgcn_s_memtime() - (np).tstart;                                                           \
            tt[6] += __builtin_amdgcn_s_memrealtime() - (np).rstart;                                                       \
            tt[7] += 1ull;                                                                                                 \
            unsigned long long *sp = g_nn_span + 4ull * (wave_id);                                                         \
            if ((P).st->iter == g_nn_span_iter) {                                                                          \
                sp[0] = (np).rstart;                                                                                       \
                sp[1] = __builtin_amdgcn_s_memrealtime();                                                                  \
                sp[2] = xp_packed;                                                                                         \
                sp[3] = np_packed;                                                                                         \
            }                                                                                                              \
        }                                                                                                                  \
    } while (0)
#else
#define NN_T(np, i) do { } while (0)
#define PROBE_NN_BEGIN(np) do { } while (0)
#define PROBE_NN_CONSUME(np) do { } while (0)
#define PROBE_NN_EXACT(np, pa, pb) do { } while (0)
#define PROBE_NN_WORK(P, q, first_lane, npairs) do { } while (0)
#define PROBE_NN_END(np, P, valid, ci, npairs, lane, wave_id) do { } while (0)
#endif

// -------------------------------------------------------------------------------------------- SAGE_LOOP_TIMING
#ifdef SAGE_LOOP_TIMING
// (icp_body<PERSIST>: cycles per phase into the pass's LoopGroup `G`, summed by k_loop; `persist`: a constant expression)
#define LP_T(persist, G, i) do { if constexpr (persist) { const unsigned long long _t = __builtin_amdgcn_s_memtime(); (G)->ph[i] += _t - (G)->tprev; (G)->tprev = _t; } } while (0)
// per workgroup and iteration: max points of a query | stale queries | points (LDS words kLpDbg ..)
#define PROBE_LOOP_WAVE_STATS(smem, valid, ci, npairs, stale, lane)                                                        \
    do {                                                                                                                   \
        unsigned mx = (valid) ? (npairs) : 0u, sm = ((valid) && (ci) == 0u) ? (npairs) : 0u, stl = ((stale) && (ci) == 0u) ? 1u : 0u; \
        for (int d = 1; d < 64; d <<= 1) {                                                                                 \
            mx = max(mx, static_cast<unsigned>(__shfl_xor(mx, d, 64)));                                                    \
            sm += __shfl_xor(sm, d, 64);                                                                                   \
            stl += __shfl_xor(stl, d, 64);                                                                                 \
        }                                                                                                                  \
        if ((lane) == 0) {                                                                                                 \
            atomicMax(&(smem)[kLpDbg], mx);                                                                                \
            atomicAdd(&(smem)[kLpDbg + 1], stl);                                                                           \
            atomicAdd(&(smem)[kLpDbg + 2], sm);                                                                            \
        }                                                                                                                  \
    } while (0)
#else
#define LP_T(persist, G, i) do { } while (0)
#define PROBE_LOOP_WAVE_STATS(smem, valid, ci, npairs, stale, lane) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------- SAGE_ICP_DELAY_PROBE
#ifdef SAGE_ICP_DELAY_PROBE
#define PROBE_DELAY_BEGIN(t0) const unsigned long long t0 = __builtin_amdgcn_s_memrealtime()
// the pose becomes available `dbg_delay` ticks (100 MHz) after this wave started, with the prologue loads already in
// flight — what hiding k_fin under the prologue would cost
#define PROBE_DELAY_WAIT(P, t0)                                                                                            \
    do {                                                                                                                   \
        if ((P).dbg_delay) {                                                                                               \
            __builtin_amdgcn_sched_barrier(0);                                                                             \
            while (__builtin_amdgcn_s_memrealtime() - (t0) < (P).dbg_delay) __builtin_amdgcn_s_sleep(8);                  \
            __builtin_amdgcn_sched_barrier(0);                                                                             \
        }                                                                                                                  \
    } while (0)
// the same pass again inside the launch — what an iteration costs on L2s that were not emptied by a kernel boundary (its
// sums are added a second time: the solve does not care)
#define PROBE_DELAY_REPEAT(P, pass)                                                                                        \
    do {                                                                                                                   \
        for (unsigned r = 0; r < (P).dbg_repeat; ++r) {                                                                    \
            __syncthreads();                                                                                               \
            pass;                                                                                                          \
        }                                                                                                                  \
    } while (0)
#else
#define PROBE_DELAY_BEGIN(t0) do { } while (0)
#define PROBE_DELAY_WAIT(P, t0) do { } while (0)
#define PROBE_DELAY_REPEAT(P, pass) do { } while (0)
#endif

}  // namespace sageicp
