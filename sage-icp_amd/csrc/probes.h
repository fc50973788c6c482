// Instrumentation of the kernels of kernels.hip (the search body, icp_body.h; the finish, fin_kernel.h; the one-launch loop,
// loop_kernel.h) for the probe builds under profiles/: the globals the stamps go to, the macros that write them and the
// sageicp_debug_* entries that read them back.  None of it is in the product: every macro below is empty, and nothing
// else is declared, unless its switch is defined when the library is built
// (python sage-icp_amd/build.py <out.so> -DSAGE_NN_TIMING ...; tests/test_probe_variants.py compiles each so they do not rot).
//
//   SAGE_NN_TIMING        k_icp: shader cycles per phase of a wave, its lifetime, the span of one chosen launch per wave
//                         (profiles/icp_tail.py, phase_probe.py); sageicp_debug_nn_phases / _nn_raw / _nn_spans
//   SAGE_LOOP_TIMING      k_loop: cycles per phase of a pass, per-workgroup / per-wave / solver stamps (profiles/loop_tail.py,
//                         loop_times.py, solve_split.py); sageicp_debug_loop_*
//   SAGE_GN_TIMING        k_fin: 100-MHz ticks of the reduction, the solve, the exponential, the rest (profiles/fin_phases.py);
//                         sageicp_debug_gn_phases
//   SAGE_ICP_DELAY_PROBE  k_icp: the pose arrives `dbg_delay` ticks after a wave's start / the pass repeated inside the launch
//
// (SAGE_LOOP_INGRID is not here: it changes the protocol of k_loop, not its instrumentation.)
//
// A probe is one line at its site and takes what it reads as arguments: the kernel's parameters, the pass's LoopGroup,
// the site's own values (`it`, `gi`, `nw`, `wv`, `lane`, `smem`), and the probe's state — a local that a PROBE_*_BEGIN
// (or the probe that takes the first of two stamps) declares under the name it is given; nothing in the product.
#pragma once

#include <algorithm>
#include <vector>

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
#define PROBE_LOOP_GROUP_FIELDS unsigned long long ph[8], tprev, tpose;      /* LoopGroup: cycles per phase of the body in this pass | the last stamp | 100-MHz stamp of the pass's first use of the pose */
// (icp_body<PERSIST>, in front of make_query: the first instruction of the pass that needs the pose)
#define PROBE_LOOP_POSE_USE(persist, G) do { if constexpr (persist) (G)->tpose = __builtin_amdgcn_s_memrealtime(); } while (0)
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
// 100-MHz stamps of the first kLoopTimedIters iterations — per workgroup when it counted itself in and when it had
// the next pose; for the solving wave when all counts were in, the sums read, the step solved, the pose published
constexpr int kLoopTimedIters = 32, kLoopTimedWgs = 2048;
__device__ unsigned long long g_loop_wg[kLoopTimedIters][kLoopTimedWgs][4];     // counted in | pose held | a wave took a unit beyond one per wave | ... finished it
__device__ unsigned g_loop_wginfo[kLoopTimedIters][kLoopTimedWgs][4];     // HW_ID | max points of a query | stale queries | points
__device__ unsigned long long g_loop_solver[kLoopTimedIters][4];
__device__ unsigned long long g_loop_solver2[kLoopTimedIters][4];      // inside the solve: after the solve | the exponential (and the sqrt of the step norm) | the composition | the norm test
__device__ unsigned long long g_loop_wave[kLoopTimedIters][kLoopTimedWgs][8][2];      // per wave: its FIRST unit of the iteration: end stamp | start stamp (low 32) << 32 ... see PROBE_LOOP_UNIT_END
__device__ unsigned long long g_loop_wave_pose[kLoopTimedIters][kLoopTimedWgs][8];    // ... and when that pass first used the pose (PROBE_LOOP_POSE_USE)
__device__ unsigned g_loop_unit_work[kLoopTimedIters][kLoopTimedWgs][8];       // per unit of a workgroup, in the iteration's order (0 = heaviest by the iteration before): see PROBE_LOOP_UNIT_WORK
__device__ unsigned long long g_loop_phase[16];     // [0..7] cycles per body phase, [8] wait for the pose, [9] closing a workgroup, [10] group passes
#define LOOP_STAMP_SOLVER(it, k) do { if ((it) < kLoopTimedIters && (threadIdx.x & 63u) == 0u) g_loop_solver[it][k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define LOOP_STAMP_SOLVER2(it, k) do { if ((it) < kLoopTimedIters && (threadIdx.x & 63u) == 0u) g_loop_solver2[it][k] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define LOOP_STAMP_WG(it, k) do { if ((it) < kLoopTimedIters && blockIdx.x < kLoopTimedWgs && (threadIdx.x & 63u) == 0u) g_loop_wg[it][blockIdx.x][k] = __builtin_amdgcn_s_memrealtime(); } while (0)
// what a wave of k_loop keeps over the call: cycles per phase of the body | waiting at the barrier | closing the
// workgroup's iteration | passes
#define PROBE_LOOP_BEGIN(lp)                                                                                               \
    unsigned long long lp##_ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                                              \
    unsigned long long lp##_t_wait = 0, lp##_t_close = 0, lp##_n_pass = 0
#define PROBE_LOOP_CLEAR_STATS(smem) { (smem)[kLpDbg] = 0u; (smem)[kLpDbg + 1] = 0u; (smem)[kLpDbg + 2] = 0u; }
// the iteration's number under the name given, for the stamps of the passes (k_loop keeps it in its LDS header)
#define PROBE_LOOP_IT(it, smem) const int it = __builtin_amdgcn_readfirstlane(static_cast<int>((smem)[kLpIter]))
// the stamp `t_unit` | a wave has taken unit `gi` (sets it; the stage half follows) | the run half of the pass on it starts | ... is over
#define PROBE_LOOP_UNIT_VAR(t_unit) unsigned long long t_unit = 0
#define PROBE_LOOP_UNIT_BEGIN(it, gi, nw, t_unit)                                                                          \
    if ((gi) >= static_cast<unsigned>(nw)) LOOP_STAMP_WG(it, 2);                                                           \
    t_unit = __builtin_amdgcn_s_memrealtime()
#define PROBE_LOOP_PASS_BEGIN(lp, G)                                                                                       \
    {                                                                                                                      \
        for (int i = 0; i < 8; ++i) (G).ph[i] = 0;                                                                         \
        (G).tprev = __builtin_amdgcn_s_memtime();                                                                          \
        ++lp##_n_pass;                                                                                                     \
    }
#define PROBE_LOOP_UNIT_END(lp, G, it, gi, nw, wv, lane, t_unit)                                                           \
    {                                                                                                                      \
        if ((gi) >= static_cast<unsigned>(nw)) LOOP_STAMP_WG(it, 3);                                                       \
        if ((it) < kLoopTimedIters && blockIdx.x < kLoopTimedWgs && (lane) == 0 && (wv) < 8 && (gi) < static_cast<unsigned>(nw)) { \
            unsigned hw;                                                                                                   \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                               \
            g_loop_wave[it][blockIdx.x][wv][0] = __builtin_amdgcn_s_memrealtime();                                         \
            g_loop_wave[it][blockIdx.x][wv][1] = ((t_unit) << 24) | (static_cast<unsigned long long>((gi) & 0xFFu) << 16) | (hw & 0xFFFFu); \
            g_loop_wave_pose[it][blockIdx.x][wv] = (G).tpose;                                                              \
        }                                                                                                                  \
        for (int i = 0; i < 8; ++i) lp##_ph[i] += (G).ph[i];                                                               \
    }
// ... and what the unit cost by the kernel's own measure: the most points one of its queries was handed (+ 48 for a stale
// row), the maximum of LoopGroup::work over the unit's blocks of four queries — for the first units and the ones beyond
#define PROBE_LOOP_UNIT_WORK(G, it, gi, bpw, lane)                                                                         \
    {                                                                                                                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                                                             \
        if ((it) < kLoopTimedIters && blockIdx.x < kLoopTimedWgs && (lane) == 0 && (gi) < 8u) {                            \
            unsigned mx = 0u;                                                                                              \
            for (unsigned b = 0; b < (bpw); ++b) mx = max(mx, (G).work[(G).perm[(gi) * (bpw) + b]]);                       \
            g_loop_unit_work[it][blockIdx.x][gi] = mx;                                                                     \
        }                                                                                                                  \
    }
// a stamp in shader cycles under the name given
#define PROBE_LOOP_MARK(t) const unsigned long long t = __builtin_amdgcn_s_memtime()
// the wave that closed the workgroup's iteration: where it ran and what the iteration's passes counted (PROBE_LOOP_WAVE_STATS)
#define PROBE_LOOP_WG_INFO(smem, it, lane)                                                                                 \
    {                                                                                                                      \
        if ((lane) == 0 && (it) < kLoopTimedIters && blockIdx.x < kLoopTimedWgs) {                                         \
            unsigned hw;                                                                                                   \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                               \
            unsigned xcc;                                                                                                  \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                                             \
            unsigned *o = g_loop_wginfo[it][blockIdx.x];                                                                   \
            o[0] = (xcc << 28) | (hw & 0x0FFFFFFFu);                                                                       \
            o[1] = (smem)[kLpDbg]; o[2] = (smem)[kLpDbg + 1]; o[3] = (smem)[kLpDbg + 2];                                   \
            (smem)[kLpDbg] = 0u; (smem)[kLpDbg + 1] = 0u; (smem)[kLpDbg + 2] = 0u;                                         \
        }                                                                                                                  \
    }
// behind the close (`t_a`: the mark after the wave's last pass) | before a barrier (declares `t_b`) | after it
#define PROBE_LOOP_CLOSED(lp, last, t_a)                                                                                   \
    if (last) lp##_t_close += __builtin_amdgcn_s_memtime() - (t_a)
#define PROBE_LOOP_WAIT_BEGIN(t_b) const unsigned long long t_b = __builtin_amdgcn_s_memtime()
#define PROBE_LOOP_WAITED(lp, t_b) lp##_t_wait += __builtin_amdgcn_s_memtime() - (t_b)
#define PROBE_LOOP_END(lp)                                                                                                 \
    {                                                                                                                      \
        if ((threadIdx.x & 63u) == 0u) {                                                                                   \
            for (int i = 0; i < 8; ++i) atomicAdd(&g_loop_phase[i], lp##_ph[i]);                                           \
            atomicAdd(&g_loop_phase[8], lp##_t_wait);                                                                      \
            atomicAdd(&g_loop_phase[9], lp##_t_close);                                                                     \
            atomicAdd(&g_loop_phase[10], lp##_n_pass);                                                                     \
        }                                                                                                                  \
    }
extern "C" void sageicp_debug_loop_solver2(unsigned long long *out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_solver2), sizeof(unsigned long long) * kLoopTimedIters * 4);
}
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
extern "C" void sageicp_debug_loop_wave_pose(unsigned long long *out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_wave_pose), sizeof(unsigned long long) * kLoopTimedIters * kLoopTimedWgs * 8);
}
extern "C" void sageicp_debug_loop_unit_work(unsigned *out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_loop_unit_work), sizeof(unsigned) * kLoopTimedIters * kLoopTimedWgs * 8);
}
extern "C" void sageicp_debug_loop_info(unsigned *info) {
    (void)hipMemcpyFromSymbol(info, HIP_SYMBOL(g_loop_wginfo), sizeof(unsigned) * kLoopTimedIters * kLoopTimedWgs * 4);
}
extern "C" void sageicp_debug_loop_times(unsigned long long *wg, unsigned long long *solver) {
    (void)hipMemcpyFromSymbol(wg, HIP_SYMBOL(g_loop_wg), sizeof(unsigned long long) * kLoopTimedIters * kLoopTimedWgs * 4);
    (void)hipMemcpyFromSymbol(solver, HIP_SYMBOL(g_loop_solver), sizeof(unsigned long long) * kLoopTimedIters * 4);
}
#else
#define LP_T(persist, G, i) do { } while (0)
#define PROBE_LOOP_GROUP_FIELDS
#define LOOP_STAMP_SOLVER(it, k) do { } while (0)
#define LOOP_STAMP_SOLVER2(it, k) do { } while (0)
#define LOOP_STAMP_WG(it, k) do { } while (0)
#define PROBE_LOOP_BEGIN(lp) ((void)0)
#define PROBE_LOOP_CLEAR_STATS(smem) ((void)0)
#define PROBE_LOOP_POSE_USE(persist, G) do { } while (0)
#define PROBE_LOOP_UNIT_VAR(t_unit) ((void)0)
#define PROBE_LOOP_IT(it, smem) ((void)0)
#define PROBE_LOOP_UNIT_BEGIN(it, gi, nw, t_unit) ((void)0)
#define PROBE_LOOP_PASS_BEGIN(lp, G) ((void)0)
#define PROBE_LOOP_UNIT_END(lp, G, it, gi, nw, wv, lane, t_unit) ((void)0)
#define PROBE_LOOP_UNIT_WORK(G, it, gi, bpw, lane) ((void)0)
#define PROBE_LOOP_MARK(t) ((void)0)
#define PROBE_LOOP_WG_INFO(smem, it, lane) ((void)0)
#define PROBE_LOOP_CLOSED(lp, last, t_a) ((void)0)
#define PROBE_LOOP_WAIT_BEGIN(t_b) ((void)0)
#define PROBE_LOOP_WAITED(lp, t_b) ((void)0)
#define PROBE_LOOP_END(lp) ((void)0)
#define PROBE_LOOP_WAVE_STATS(smem, valid, ci, npairs, stale, lane) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------- SAGE_GN_TIMING
#ifdef SAGE_GN_TIMING
__device__ unsigned long long g_gn_phase[16];       // [4] solves | [8] ticks of the reduction | [9..11] the solve, the exponential, the rest
// k_fin: from its start (declares `t_start`) to the sums
#define PROBE_FIN_START(t_start) const unsigned long long t_start = __builtin_amdgcn_s_memrealtime()
#define PROBE_FIN_REDUCED(t_start) do { if (threadIdx.x == 0) atomicAdd(&g_gn_phase[8], __builtin_amdgcn_s_memrealtime() - (t_start)); } while (0)
// solve_and_publish: `ft`, the stamps of thread 0
#define PROBE_FIN_BEGIN(ft) unsigned long long ft[8]
#define FIN_STAMP(ft, i) do { if (threadIdx.x == 0) (ft)[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define PROBE_FIN_END(ft)                                                                                                  \
    do {                                                                                                                   \
        (ft)[4] = __builtin_amdgcn_s_memrealtime();                                                                        \
        for (int i = 1; i < 4; ++i) atomicAdd(&g_gn_phase[8 + i], (ft)[i + 1] - (ft)[i]);                                  \
        atomicAdd(&g_gn_phase[4], 1ull);                                                                                   \
    } while (0)
extern "C" void sageicp_debug_gn_phases(unsigned long long out[16], int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gn_phase), sizeof(unsigned long long) * 16);
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_gn_phase), z, sizeof(z));
    }
}
#else
#define PROBE_FIN_START(t_start) ((void)0)
#define PROBE_FIN_REDUCED(t_start) ((void)0)
#define PROBE_FIN_BEGIN(ft) ((void)0)
#define FIN_STAMP(ft, i) do { } while (0)
#define PROBE_FIN_END(ft) ((void)0)
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
