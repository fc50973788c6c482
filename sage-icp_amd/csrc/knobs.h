// The SAGEICP_* knobs of the process environment: one typed struct, one table that names every knob once, one loader
// and one accessor.  The environment is read when the first knob is asked for and again only by sageicp_reload_env()
// (a registration asks for ~35 knobs, and a ROS node's environment does not change under it; tests and probes that flip
// knobs between calls go through the Python binding, which reloads whenever the SAGEICP_* part of os.environ changed).
// A load is a SNAPSHOT: a call takes `const Knobs &k = knobs()` once and sees one value of every knob, whatever is
// reloaded beside it, and the reference stays valid for the rest of the process.  What a knob is for is said where it
// is used; the table says what exists, the default and the clamp where neither depends on the frame or the map.
// No HIP and no other header of the project: tests/knobs_check.cpp includes this file alone.
#pragma once

#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>

namespace sageicp {

// An integer knob.  `value` is the environment's number (atoi) inside the table's clamp, or the table's default where
// the knob is unset; a knob whose default depends on the frame or the map has none in the table and is asked with
// get(dflt).
struct IntKnob {
    int value = 0;
    bool set = false;
    int get() const { return value; }
    int get(int dflt) const { return set ? value : dflt; }
    bool operator==(const IntKnob &o) const { return value == o.value && set == o.set; }
};

constexpr int kMaxKnobDevices = 16;     // (sageicp_map_set_devices refuses more than 8: a longer list is still refused)

struct Knobs {
    // lanes, scan and sums of a search (capi_run.hip: icp_lw, wants_filter, wants_flat, icp_params)
    IntKnob lw, filter, flat, exact_divide, no_filter, no_prune, acc_shift, dbg_delay, dbg_repeat;
    // the one-launch loop: whether, its shape, its patience (plan_loop, solver_params, run_one_launch)
    IntKnob loop, loop_waves, loop_gpw, loop_max_wgs, loop_debug, loop_contiguous, loop_prio, loop_deal, loop_pose_map;
    IntKnob loop_timeout_ms, loop_timeout_ticks, loop_count_timeout_rank, loop_count_timeout_ticks, loop_cooldown;
    // the launch-per-iteration forms and the direct exchange (IcpCall::constants, plan_attempt, Iterations)
    IntKnob chunked, max_iter, depth, sort_from, lpt, chain, chain_comm, p2p_timeout_s, p2p_timeout_ticks, quiet;
    // read when a map is created (capi.hip) or its archive first grows (capi_archive.hip)
    IntKnob map_reference_order, map_archive, archive_initial_rows;
    // frame preparation, outputs, scores, places
    IntKnob source_reference_order, replay_threads, debug_order, occ_global, egress_two_pass, touch_threads, hugepages;
    IntKnob score_chunk_rows, place_doubled;
    // the knobs that are text, parsed at the load
    int devices[kMaxKnobDevices] = {};  // SAGEICP_DEVICES=0,1,...: the ordinals up to the first that is no number
    int n_devices = 0;
    int cu_share_i = 0, cu_share_k = 1; // SAGEICP_CU_SHARE=i/k with 1 <= k <= 16 and 0 <= i < k, else unset
    bool cu_share_set = false;
    uint64_t map_archive_max_rows = 0;  // decimal, 64 bits; unset or a leading '-': 0 (no limit)
    bool size_classes = true;           // off only for a value that begins with '0'
};

inline void parse_devices(Knobs &k, const char *v) {
    k.n_devices = 0;
    for (const char *q = v ? v : ""; *q && k.n_devices < kMaxKnobDevices;) {
        char *end = nullptr;
        const long d = std::strtol(q, &end, 10);
        if (end == q) break;
        k.devices[k.n_devices++] = static_cast<int>(d);
        q = (*end == ',') ? end + 1 : end;
    }
}
inline void parse_cu_share(Knobs &k, const char *v) {
    int i = 0, n = 1;
    k.cu_share_set = v && std::sscanf(v, "%d/%d", &i, &n) == 2 && n >= 1 && n <= 16 && i >= 0 && i < n;
    k.cu_share_i = k.cu_share_set ? i : 0;
    k.cu_share_k = k.cu_share_set ? n : 1;
}
inline void parse_archive_max_rows(Knobs &k, const char *v) {
    k.map_archive_max_rows = (v && v[0] != '-') ? std::strtoull(v, nullptr, 10) : 0;
}
inline void parse_size_classes(Knobs &k, const char *v) { k.size_classes = !(v && v[0] == '0'); }

// One line per knob: an integer (`field`; `has_default`, `dflt`, and the clamp [lo, hi] a set value is brought into) or
// a text knob (`parse`, given the environment's value or nullptr).
struct KnobDesc {
    const char *name;
    IntKnob Knobs::*field;
    void (*parse)(Knobs &, const char *);
    bool has_default;
    int dflt, lo, hi;
};
constexpr int kNoMin = INT_MIN, kNoMax = INT_MAX;
constexpr KnobDesc kKnobTable[] = {
    {"SAGEICP_LW", &Knobs::lw, nullptr, true, -1, -1, 4},                    // log2 lanes per query; negative: not forced
    {"SAGEICP_FILTER", &Knobs::filter, nullptr, false, 0, kNoMin, kNoMax},   // compact scan; default by frame and map
    {"SAGEICP_FLAT", &Knobs::flat, nullptr, false, 0, kNoMin, kNoMax},       // flat order at 2 / 4 lanes; default by the map
    {"SAGEICP_EXACT_DIVIDE", &Knobs::exact_divide, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_NO_FILTER", &Knobs::no_filter, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_NO_PRUNE", &Knobs::no_prune, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_ACC_SHIFT", &Knobs::acc_shift, nullptr, true, 0, 0, 2},
    {"SAGEICP_DBG_DELAY", &Knobs::dbg_delay, nullptr, true, 0, kNoMin, kNoMax},     // (used by the delay-probe build only)
    {"SAGEICP_DBG_REPEAT", &Knobs::dbg_repeat, nullptr, true, 0, kNoMin, kNoMax},   // (likewise)
    {"SAGEICP_LOOP", &Knobs::loop, nullptr, true, 1, kNoMin, kNoMax},
    {"SAGEICP_LOOP_WAVES", &Knobs::loop_waves, nullptr, true, 0, 0, kNoMax},        // (at most kLoopMaxWavesHost: at its use)
    {"SAGEICP_LOOP_GPW", &Knobs::loop_gpw, nullptr, true, 0, 0, kNoMax},
    {"SAGEICP_LOOP_MAX_WGS", &Knobs::loop_max_wgs, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_LOOP_DEBUG", &Knobs::loop_debug, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_LOOP_CONTIGUOUS", &Knobs::loop_contiguous, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_LOOP_PRIO", &Knobs::loop_prio, nullptr, true, 3, 0, 3},
    {"SAGEICP_LOOP_DEAL", &Knobs::loop_deal, nullptr, true, 1, 0, 2},
    {"SAGEICP_LOOP_POSE_MAP", &Knobs::loop_pose_map, nullptr, true, 0, 0, 2},
    {"SAGEICP_LOOP_TIMEOUT_MS", &Knobs::loop_timeout_ms, nullptr, true, 50, 1, kNoMax},
    {"SAGEICP_LOOP_TIMEOUT_TICKS", &Knobs::loop_timeout_ticks, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_LOOP_COUNT_TIMEOUT_RANK", &Knobs::loop_count_timeout_rank, nullptr, true, -1, kNoMin, kNoMax},
    {"SAGEICP_LOOP_COUNT_TIMEOUT_TICKS", &Knobs::loop_count_timeout_ticks, nullptr, true, 1, 1, kNoMax},
    {"SAGEICP_LOOP_COOLDOWN", &Knobs::loop_cooldown, nullptr, true, 256, 0, kNoMax},
    {"SAGEICP_CHUNKED", &Knobs::chunked, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_MAX_ITER", &Knobs::max_iter, nullptr, false, 0, 1, kNoMax},           // default and ceiling: kMaxIterations
    {"SAGEICP_DEPTH", &Knobs::depth, nullptr, true, 4, 1, 8},
    {"SAGEICP_SORT_FROM", &Knobs::sort_from, nullptr, false, 0, 0, kNoMax},         // default: kSortFrameFrom
    {"SAGEICP_LPT", &Knobs::lpt, nullptr, false, 0, kNoMin, kNoMax},                // default by the frame's size
    {"SAGEICP_CHAIN", &Knobs::chain, nullptr, true, 1, kNoMin, kNoMax},
    {"SAGEICP_CHAIN_COMM", &Knobs::chain_comm, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_P2P_TIMEOUT_S", &Knobs::p2p_timeout_s, nullptr, true, 5, 1, kNoMax},
    {"SAGEICP_P2P_TIMEOUT_TICKS", &Knobs::p2p_timeout_ticks, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_QUIET", &Knobs::quiet, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_DEVICES", nullptr, parse_devices, false, 0, 0, 0},
    {"SAGEICP_CU_SHARE", nullptr, parse_cu_share, false, 0, 0, 0},
    {"SAGEICP_SIZE_CLASSES", nullptr, parse_size_classes, false, 0, 0, 0},
    {"SAGEICP_MAP_REFERENCE_ORDER", &Knobs::map_reference_order, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_MAP_ARCHIVE", &Knobs::map_archive, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_MAP_ARCHIVE_MAX_ROWS", nullptr, parse_archive_max_rows, false, 0, 0, 0},
    {"SAGEICP_ARCHIVE_INITIAL_ROWS", &Knobs::archive_initial_rows, nullptr, true, 1 << 16, 1, kNoMax},
    {"SAGEICP_SOURCE_REFERENCE_ORDER", &Knobs::source_reference_order, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_REPLAY_THREADS", &Knobs::replay_threads, nullptr, true, 8, 1, kNoMax},
    {"SAGEICP_DEBUG_ORDER", &Knobs::debug_order, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_OCC_GLOBAL", &Knobs::occ_global, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_EGRESS_TWO_PASS", &Knobs::egress_two_pass, nullptr, true, 0, kNoMin, kNoMax},
    {"SAGEICP_TOUCH_THREADS", &Knobs::touch_threads, nullptr, true, 4, kNoMin, kNoMax},   // (<= 0: off; the pool's size: at its use)
    {"SAGEICP_HUGEPAGES", &Knobs::hugepages, nullptr, true, 1, kNoMin, kNoMax},
    {"SAGEICP_SCORE_CHUNK_ROWS", &Knobs::score_chunk_rows, nullptr, true, 1 << 20, 1, kNoMax},
    {"SAGEICP_PLACE_DOUBLED", &Knobs::place_doubled, nullptr, true, 0, kNoMin, kNoMax},
};

inline bool operator==(const Knobs &a, const Knobs &b) {
    for (const KnobDesc &d : kKnobTable)
        if (d.field && !(a.*d.field == b.*d.field)) return false;
    if (a.n_devices != b.n_devices) return false;
    for (int i = 0; i < a.n_devices; ++i)
        if (a.devices[i] != b.devices[i]) return false;
    return a.cu_share_set == b.cu_share_set && a.cu_share_i == b.cu_share_i && a.cu_share_k == b.cu_share_k &&
           a.map_archive_max_rows == b.map_archive_max_rows && a.size_classes == b.size_classes;
}

inline Knobs load_from_environment() {
    Knobs k;
    for (const KnobDesc &d : kKnobTable) {
        const char *v = std::getenv(d.name);
        if (d.parse) {
            d.parse(k, v);
            continue;
        }
        IntKnob &f = k.*d.field;
        f.set = v != nullptr;
        const int e = v ? std::atoi(v) : d.dflt;
        f.value = !v ? e : (e < d.lo ? d.lo : (e > d.hi ? d.hi : e));
    }
    return k;
}

// The snapshots of the process: never shrunk, so a reference handed out stays good; `current` is the one knobs() gives
// (null: nothing loaded yet).  Leaked on purpose: calls may still be running when the process's statics go.
struct KnobStore {
    std::mutex mu;
    std::deque<Knobs> snapshots;
    std::atomic<const Knobs *> current{nullptr};
};
inline KnobStore &knob_store() {
    static KnobStore &s = *new KnobStore;
    return s;
}
// Reads the environment and publishes what it found, unless that equals the current snapshot.  (Not beside a setenv of
// another thread: that is a race of the C library's.)
inline const Knobs &reload_knobs() {
    KnobStore &s = knob_store();
    const Knobs fresh = load_from_environment();
    std::lock_guard<std::mutex> lk(s.mu);
    const Knobs *cur = s.current.load(std::memory_order_relaxed);
    if (cur && *cur == fresh) return *cur;
    s.snapshots.push_back(fresh);
    s.current.store(&s.snapshots.back(), std::memory_order_release);
    return s.snapshots.back();
}
inline const Knobs &knobs() {
    const Knobs *k = knob_store().current.load(std::memory_order_acquire);
    return k ? *k : reload_knobs();
}

}  // namespace sageicp
