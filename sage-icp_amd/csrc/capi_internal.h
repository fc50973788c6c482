// Internals shared by the translation units of libsageicp_hip.so's host side (capi.hip, capi_pipeline.hip,
// capi_outputs.hip, caller_mem.hip, capi_mirror.hip, capi_run.hip, prep.hip): error channel, tuning knobs, the
// per-handle device scratch, the pipeline's frame source and buffers (prep.h) and its prefetch state (prefetch.h), the
// checks of a caller's device memory (caller_mem.h), the way out (outputs.h), the opaque handles of include/sageicp.h
// except the pipeline's (capi_pipeline.hip).  Not part of the C ABI.
#pragma once

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cfloat>
#include <limits>
#include <memory>
#include <cstring>
#include <map>
#include <mutex>
#include <array>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/sageicp.h"
#include "dev_buffer.h"
#include "dyn_rules.h"
#include "host_map.hpp"
#include "kernels.h"
#include "egress.h"
#include "msg.h"
#include "map_update.h"
#include "metrics.hpp"
#include "pipeline.hpp"
#include "prefetch.h"
#include "robin_order.hpp"
#include "se3_math.h"
#include "sageicp_types.h"

namespace sageicp {

// ---- errors --------------------------------------------------------------------------
extern thread_local std::string g_err;
// (switches set through the C ABI, read by every call: several host threads may be inside the library)
extern std::atomic<int> g_profiling;
extern std::atomic<int> g_counting;                // sageicp_set_counting: the per-wave candidate / pair counters behind sageicp_stats
// VoxelDownsample emits its survivors in the reference's order (the bucket order of its
// tsl::robin_map, replayed on the host: robin_order.hpp) unless switched to arrival order
extern std::atomic<int> g_reference_order;

// tuning knobs (defaults chosen by measurement on MI355X; the environment overrides are for
// experiments only)
// The process environment is read ONCE per knob and call site (the first time it is asked for) and again only after
// sageicp_reload_env(): a registration asks for ~35 knobs, and a ROS node's environment does not change under it.
// (Tests and probes that flip knobs between calls go through the Python binding, which calls sageicp_reload_env()
// whenever the SAGEICP_* part of os.environ changed.)
extern std::atomic<unsigned> g_env_epoch;          // bumped by sageicp_reload_env()
struct EnvKnob {
    const char *name;
    std::atomic<unsigned> epoch{0xFFFFFFFFu};
    std::atomic<int> has{0}, val{0};
};
inline int env_knob(EnvKnob &k, int dflt) {
    const unsigned e = g_env_epoch.load(std::memory_order_relaxed);
    if (k.epoch.load(std::memory_order_acquire) != e) {
        const char *v = std::getenv(k.name);
        k.val.store(v ? std::atoi(v) : 0, std::memory_order_relaxed);
        k.has.store(v ? 1 : 0, std::memory_order_relaxed);
        k.epoch.store(e, std::memory_order_release);
    }
    return k.has.load(std::memory_order_relaxed) ? k.val.load(std::memory_order_relaxed) : dflt;
}
#define env_int(name, dflt) ([&]() -> int { static ::sageicp::EnvKnob _knob{name}; return ::sageicp::env_knob(_knob, (dflt)); }())
// a knob that is text: the value at the last (re)load (capi.hip), or nullptr
const char *env_cached(const char *name);
// Lanes per query in k_icp (log2).  One lane per query needs the fewest instructions per query
// but gives a frame of n points only n / 64 waves with long dependent chains; small frames and
// shards spread each query over more lanes.  Thresholds measured on MI355X (profiles/README.md);
// SAGEICP_LW overrides for experiments.
inline int icp_lw(uint64_t n, bool sparse_voxels) {
    const int e = env_int("SAGEICP_LW", -1);
    if (e >= 0) return e > 4 ? 4 : e;
    // (all of this re-measured after the flat-order scan, profiles/r04/lanes_probe2.txt (dense voxels) and
    // lanes_probe3.txt (sparse ones); us per iteration)
    // the biggest frames are bound by instruction issue, not by the length of a wave's chain: two
    // lanes per query halve the per-query share of the fixed work (prologue, bounds, epilogue) — against
    // dense voxels only at c4's size (500k: 90.7 against 92.9 with four, 400k a tie), against sparse ones
    // from ~150k (c5, 200k: 42.8 / 43.2; 100k: 33.3 / 31.6)
    if (n >= (sparse_voxels ? 150000u : 400000u)) return 1;
    // eight lanes stride through a query's voxels in flat order (kernels.hip) and hold against dense voxels
    // up to ~110k queries (50k: 25.7 against 31.1 with four; 60k: 28.0 / 31.5; 80k: 32.3 / 34.5; 100k: 36.2 /
    // 37.1; 120k: 40.8 / 40.6), against sparse ones up to ~60k (25k: 19.8 / 22.9; 50k: 24.7 / 25.1; 100k:
    // 34.9 / 31.6); until late round 4 the switch to four sat at 50k and, for sparse voxels, at 4k
    if (n >= (sparse_voxels ? 60000u : 110000u)) return 2;
    // sixteen lanes only for small frames against dense voxels (in flat order they hold up to ~20k queries:
    // 10k 17.8 against 18.9 with eight, 15k 19.1 / 20.0, 30k 24.7 / 22.6 — lanes_probe4.txt; the switch used
    // to sit at 10k): a scan against sparse ones is a handful of points whatever the split (c1, 10k: 17.6
    // with eight, 20.7 with four)
    if (n >= (sparse_voxels ? 4096u : 20000u)) return 3;
    return 4;
}


inline int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                      \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(SAGEICP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// There is no CPU fallback: an entry that needs the device fails without one, and one that names a device needs the
// ordinal of a visible one.
inline int require_device() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(SAGEICP_ERR_NO_DEVICE, "no HIP device visible (gfx950 required; no CPU fallback)");
    return SAGEICP_OK;
}
inline int require_device(int device) {
    if (int rc = require_device()) return rc;
    if (device < 0 || device >= sageicp_device_count()) return fail(SAGEICP_ERR_INVALID, "device ordinal out of range");
    return SAGEICP_OK;
}

// The work the caller enqueued on its stream before this call goes before whatever `ours` runs from here on (`ev`:
// created with the first use, on the current device).
inline int stream_after_caller(OwnedEvent &ev, hipStream_t caller, hipStream_t ours) {
    if (!ev) HIPCHK(ev.create(hipEventDisableTiming));
    HIPCHK(hipEventRecord(ev.get(), caller));
    HIPCHK(hipStreamWaitEvent(ours, ev.get(), 0));
    return SAGEICP_OK;
}

inline bool finite_n(const double *v, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

inline double now_us() {
    using namespace std::chrono;
    return duration<double, std::micro>(steady_clock::now().time_since_epoch()).count();
}

// ---- per-handle device scratch -----------------------------------------------------------
constexpr int kChunkMax = 16;

struct Scratch {
    int device = -1;
    OwnedStream stream;
    DevBuf<Point4> d_frame, d_tgt;
    DevBuf<int32_t> d_nn;
    // Morton re-ordering of the frame (sort.hip)
    DevBuf<Point4> d_sorted;
    DevBuf<uint32_t> d_keys, d_vals;
    DevBuf<unsigned char> d_sort_temp;
    size_t sort_cap = 0;           // points the buffers of reserve_sort hold (all of them: 0 after a failed reserve)
    // per-call work buffers: the queries' cached neighbourhood rows, the workgroup partials
    DevBuf<uint32_t> d_rows;
    DevBuf<uint2> d_prev;          // every query's record of the previous iteration (kernels.h)
    DevBuf<uint32_t> d_work;       // instrumented builds: points handed to each query
    DevBuf<double> d_partials;
    DevBuf<long long> d_acc;       // fixed-point accumulators of the Gauss-Newton sums (kernels.h, kAcc*)
    DevBuf<LoopShared> d_loop;     // what the workgroups of k_loop share inside its launch (kernels.h)
    unsigned long long go_word = 0; // (host source of a `go` word sent by a copy: SolverGuard)
    OwnedStream stream2;           // the solving wave of the one-launch loop runs here, beside the grid on `stream`
                                   // (created with the first such launch: a process has few hardware queues, and
                                   // streams that never run anything still take their turn on them)
    std::vector<uint32_t> cu_mask; // of both streams (empty: the whole device)
    OwnedEvent ev_solve;           // ... and this says that it has finished
    unsigned long long loop_epoch = 0;
    int num_cus = 0;               // CUs the streams of this handle may use (the whole device, or its share: below)
    int cu_share_i = 0, cu_share_k = 1;   // SAGEICP_CU_SHARE=i/k: the i-th of k equal parts of the device's CUs (several
                                   // ranks on ONE GPU — tests, or a small node — each keep a persistent grid resident)
    int loop_cooldown = 0;         // calls that stay away from k_loop after one of its launches timed out
    int loop_derate = 0;           // x 32 workgroups fewer than the residency rule allows: one more after every time-out
    // what sageicp_map_loop_status reports
    uint64_t calls_single_launch = 0, calls_per_iteration = 0, calls_chained = 0;
    uint32_t loop_timeouts = 0;
    int last_fallback = 0;
    DevBuf<unsigned long long> d_cand;         // per-wave counters of k_icp [2 x sort_cap]
    DevBuf<IcpState> d_state;
    PinnedBuf<IcpState> h_state;
    PinnedBuf<IcpProgress, hipHostMallocMapped | hipHostMallocCoherent> h_prog;   // written by the device every iteration
    IcpProgress *d_prog = nullptr; // its device address
    std::vector<OwnedEvent> events;  // 5 per profiled iteration

    ~Scratch() { wait(); }          // (then the members go: nothing runs on the streams any more)
    // waits for both streams, with the device current (a scratch that never created a stream calls nothing)
    void wait() const {
        if (!stream) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream.get());
        if (stream2) (void)hipStreamSynchronize(stream2.get());
    }

    int init(int dev) {
        if (stream) return SAGEICP_OK;
        if (int rc = require_device(dev)) return rc;
        device = dev;
        HIPCHK(hipSetDevice(device));
        {
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess) num_cus = cus;
        }
        if (cu_share_k <= 1) {
            if (const char *e = env_cached("SAGEICP_CU_SHARE")) {
                int i = 0, k = 1;
                if (std::sscanf(e, "%d/%d", &i, &k) == 2 && k >= 1 && k <= 16 && i >= 0 && i < k) {
                    cu_share_i = i;
                    cu_share_k = k;
                }
            }
        }
        if (cu_share_k > 1 && num_cus >= 8 * cu_share_k) {
            // this handle's kernels run on CUs [i, i + 1) * num_cus / k only: the persistent grids of k ranks
            // that share one GPU are then resident side by side instead of waiting for each other
            const int per = num_cus / cu_share_k, lo = cu_share_i * per;
            std::vector<uint32_t> mask((num_cus + 31) / 32, 0u);
            for (int c = lo; c < lo + per; ++c) mask[c / 32] |= 1u << (c % 32);
            HIPCHK(stream.create(static_cast<uint32_t>(mask.size()), mask.data()));
            cu_mask = mask;
            num_cus = per;
        } else {
            cu_share_i = 0;
            cu_share_k = 1;
            HIPCHK(stream.create());
        }
        HIPCHK(d_state.reserve(1));
        HIPCHK(d_acc.reserve(kAccReplicas * kAccWords));
        HIPCHK(d_loop.reserve(1));
        HIPCHK(hipMemset(d_loop.data(), 0, sizeof(LoopShared)));

        HIPCHK(h_state.reserve(1));
        HIPCHK(h_prog.reserve(1));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&d_prog), h_prog.data(), 0));
        return SAGEICP_OK;
    }
    int loop_streams() {
        if (stream2) return SAGEICP_OK;
        HIPCHK(hipSetDevice(device));
        if (!cu_mask.empty()) HIPCHK(stream2.create(static_cast<uint32_t>(cu_mask.size()), cu_mask.data()));
        else {
            // a stream of its own priority gets a hardware queue of its own: the solving wave runs for the whole
            // loop, and whatever shared its queue (a process has four) would wait behind it — the pipeline's
            // prefetch stream did (2.74 against 2.17 ms per streamed frame, profiles/r05/stream.txt)
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (stream2.create(greatest) != hipSuccess) {
                (void)hipGetLastError();
                HIPCHK(stream2.create());
            }
        }
        // (if this fails, stream2 exists and the next call returns above: ev_solve stays empty)
        HIPCHK(ev_solve.create(hipEventDisableTiming));
        return SAGEICP_OK;
    }
    int reserve_frame(size_t n) {
        if (n > d_frame.capacity()) HIPCHK(d_frame.reserve(n + n / 4 + 1024));
        return SAGEICP_OK;
    }
    int reserve_tgt(size_t n) {
        if (n > d_tgt.capacity()) HIPCHK(d_tgt.reserve(n + n / 4 + 1024));
        return SAGEICP_OK;
    }
    int reserve_nn(size_t n) {
        if (n > d_nn.capacity()) HIPCHK(d_nn.reserve(n + n / 4 + 1024));
        return SAGEICP_OK;
    }
    int reserve_sort(size_t n) {
        if (n <= sort_cap) return SAGEICP_OK;
        sort_cap = 0;
        const size_t cap = n + n / 4 + 1024;
        HIPCHK(d_sorted.reserve(cap));
        HIPCHK(d_rows.reserve(cap * kRowWords));
        HIPCHK(d_prev.reserve(cap));
#ifdef SAGE_NN_TIMING
        HIPCHK(d_work.reserve(cap));
#endif
        HIPCHK(d_cand.reserve(2 * cap));
        HIPCHK(d_keys.reserve(2 * cap));
        HIPCHK(d_vals.reserve(2 * cap));
        HIPCHK(d_sort_temp.reserve(sort_temp_bytes(static_cast<int>(cap))));
        sort_cap = cap;
        return SAGEICP_OK;
    }
    int reserve_partials(size_t blocks) {
        if (blocks > d_partials.capacity() / kNumSums) HIPCHK(d_partials.reserve((blocks + blocks / 4 + 256) * kNumSums));
        return SAGEICP_OK;
    }
    int reserve_events(size_t iterations) {
        while (events.size() < 5 * iterations) {
            OwnedEvent e;
            HIPCHK(e.create(hipEventDefault));
            events.push_back(std::move(e));
        }
        return SAGEICP_OK;
    }
};


// A few parked host threads for the order replays of one Prep (one per label group at most): a
// replay of a few thousand keys costs no more than starting a thread does, and the replays of a
// level are the critical path of a streamed frame.  run(count, f) executes f(0..count-1), each index
// once, on the workers and the calling thread; indices are handed out in order (largest job first
// if the caller sorted them so).
class ReplayPool {
public:
    ~ReplayPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void run(size_t count, const std::function<void(size_t)> &f, size_t want_threads) {
        if (count <= 1 || want_threads <= 1) {
            for (size_t i = 0; i < count; ++i) f(i);
            return;
        }
        while (th_.size() + 1 < std::min(want_threads, count)) th_.emplace_back([this] { worker(); });
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f;
            total_ = count;
            next_ = 0;
            pending_ = count;
            ++epoch_;
        }
        cv_.notify_all();
        drain();
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
        job_ = nullptr;
        total_ = next_ = 0;
    }

private:
    void drain() {
        for (;;) {
            size_t i;
            const std::function<void(size_t)> *job;
            {   // (a handful of jobs per level: the lock is not contended, and a worker still between
                // two jobs when the next run() starts sees that run's state consistently)
                std::lock_guard<std::mutex> lk(mu_);
                if (next_ >= total_) return;
                i = next_++;
                job = job_;
            }
            (*job)(i);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void worker() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || (epoch_ != seen && job_); });
                if (stop_) return;
                seen = epoch_;
            }
            drain();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t)> *job_ = nullptr;
    size_t total_ = 0, pending_ = 0, next_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
};

// ---- dynamic vehicle filter (dyn_filter.hip; core/Preprocessing.cpp:95-172) -----------------------
// PCL's cluster order: EuclideanClusterExtraction finds the clusters in order of their smallest index, then
// std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters) orders them by size, largest first — not stably.
// std::sort permutes by comparisons only, so the same call on (size, index) records with the same comparator gives
// PCL's permutation under the same standard library (libstdc++).  order[j] = index of the j-th cluster emitted.
inline void cluster_emission_order(const uint32_t *sizes, size_t n, uint32_t *order) {
    struct Rec {
        uint32_t size, index;
    };
    std::vector<Rec> v(n);
    for (size_t k = 0; k < n; ++k) v[k] = Rec{sizes[k], static_cast<uint32_t>(k)};
    std::sort(v.rbegin(), v.rend(), [](const Rec &a, const Rec &b) { return a.size < b.size; });
    for (size_t k = 0; k < n; ++k) order[k] = v[k].index;
}
// cluster_is_static (Preprocessing.cpp:141-158): dyn_rules.h

}  // namespace sageicp

// the frame-preparation driver in front of registration (prep.hip): DynFilter, FrameSource, PrepJob, Prep
#include "prep.h"

using namespace sageicp;

#include "caller_mem.h"
#include "outputs.h"

// ---- opaque handles -----------------------------------------------------------------------
struct sageicp_map {
    HostMap host;
    int device = 0;
    // device mirror + scratch: logically a cache of `host`, refreshed lazily by const searches
    mutable Scratch sc;
    mutable DevBuf<Slot> d_table;
    mutable DevBuf<Point4> d_pts;                // units of 4 points, + one NaN point after them (reserve_device_points)
    mutable DevBuf<uint32_t> d_regions;          // per block: (class << 28) | first unit of its region
    mutable DevBuf<uint32_t> d_free_units[kMaxClasses];   // device-side update: per-class stacks of free regions
    mutable DevBuf<uint32_t> d_freed;            // regions released by one insertion pass
    mutable DevBuf<uint32_t> d_block_of;         // device-side update: unit -> block (slot words carry units)
    mutable bool mirror_stale_all = true;
    // compact copy of d_pts for k_icp's scan (fp32 x, y, z, label), derived on the device whenever
    // the HBM copy of the map has changed since the last search: a record per point slot, one more, and
    // kCandSlack records nothing reads (k_icp loads a record's neighbour at a constant offset that the
    // buffer load's range check does not cover)
    static constexpr size_t kCandSlack = 64;
    mutable DevBuf<uint4> d_cand;
    mutable DevBuf<uint32_t> d_cand_flags;
    mutable bool cand_stale = true;
    // pinned staging + device landing buffers for the scattered refresh of changed records
    mutable PinnedBuf<char> h_stage;
    mutable DevBuf<char> d_stage;
    mutable size_t stage_bytes = 0;              // what both hold (0 after a failed reserve)
    // Device-side Update() (map_update.hip).  After one the HBM copy is the authority
    // (`on_device`) and `host` is stale until ensure_host() downloads it; `ctr` is the host's
    // shadow of the device counters.  The auxiliary arrays are valid for the host generation
    // they were uploaded at.
    mutable bool on_device = false;
    // the update's per-block arrays: as many blocks as d_zeros holds (d_regions holds at least as many)
    mutable DevBuf<uint8_t> d_zeros;
    mutable DevBuf<uint32_t> d_slot_of;
    mutable DevBuf<uint32_t> d_free;
    mutable DevBuf<MapCounters> d_ctr;
    mutable PinnedBuf<MapCounters> h_ctr;
    mutable PinnedBuf<uint32_t> h_ctr_aux;       // 16 words: what else a device update hands back (far voxels found)
    // reference-order maps: the lists a device update exchanges with the host's bucket array (pinned)
    mutable PinnedBuf<uint2> h_lists;
    int reserve_lists(size_t n) const {
        if (n + 2 > h_lists.capacity()) HIPCHK(h_lists.reserve(n + n / 2 + 4096));
        return SAGEICP_OK;
    }
    mutable bool aux_valid = false;
    mutable uint64_t aux_generation = 0;
    mutable MapCounters ctr{};
    // the update's scratch (reserve_update_scratch); map_update.hip gets the view
    struct UpdateBuffers {
        DevBuf<Point4> raw, w;
        DevBuf<unsigned long long> keys, keys_alt;
        DevBuf<uint32_t> idx, idx_alt, head_slot;
        DevBuf<UpdateEvents> flag, rank;
        DevBuf<int8_t> want;
        DevBuf<uint2> new_list;
        size_t n = 0;                            // points the buffers above hold (0 after a failed reserve)
        DevBuf<uint32_t> far_flag, far_sel;
        DevBuf<uint2> far_list;
        size_t nb = 0;                           // blocks the three above hold (0 after a failed reserve)
        DevBuf<uint32_t> n_sel;
        DevBuf<unsigned char> temp;
        UpdateScratch view() const {
            UpdateScratch v{};
            v.raw = raw.data(); v.w = w.data();
            v.keys = keys.data(); v.keys_alt = keys_alt.data();
            v.idx = idx.data(); v.idx_alt = idx_alt.data(); v.head_slot = head_slot.data();
            v.flag = flag.data(); v.rank = rank.data(); v.want = want.data();
            v.far_flag = far_flag.data(); v.far_sel = far_sel.data(); v.n_sel = n_sel.data();
            v.new_list = new_list.data(); v.far_list = far_list.data();
            v.temp = temp.data(); v.temp_bytes = temp.capacity();
            return v;
        }
    };
    mutable UpdateBuffers up;
    mutable sageicp_impl::OutputBuffers out;     // sageicp_map_pointcloud*: the exports work in these (outputs.h)
    size_t units_cap() const { return d_pts.capacity() / kUnitPoints; }       // units the point array holds
    size_t blocks_cap() const { return d_zeros.capacity(); }
    size_t cand_slots() const { return d_cand.capacity() ? d_cand.capacity() - 1 - kCandSlack : 0; }
    // Single-process multi-GPU mode (SAGEICP_DEVICES / sageicp_map_set_devices): one more complete
    // copy of the map per extra device.  Every mutation is applied to all of them, RegisterFrame
    // shards the frame over them (one host thread and one stream per device) and the ranks'
    // Gauss-Newton sums meet in peer-mapped exchange blocks.  `this` is rank 0.
    std::vector<sageicp_map *> replicas;
    mutable std::vector<struct sageicp_comm *> ranks;   // created at the first sharded registration
    // a mutation reached some copies of the map but not all (a device ran out of memory, ...): the
    // ranks would sum Gauss-Newton terms computed against different maps, so every later entry
    // refuses the handle until Clear() has emptied all copies
    bool replicas_diverged = false;
    // the buffers above are used on sc's streams and go before sc does: the streams are waited for first
    ~sageicp_map() { sc.wait(); }
};

struct sageicp_frame {
    int device = 0;
    DevBuf<Point4> d;
    uint64_t n = 0;
};

struct sageicp_comm {
    ncclComm_t comm = nullptr;           // RCCL (may be absent when only the direct exchange is used)
    int rank = 0, nranks = 1, device = 0;
    // direct exchange of the sums over xGMI (P2pBlock, sageicp_types.h)
    bool p2p = false;
    bool poisoned = false;               // an exchange timed out: the ranks' exchange counters may
                                         // differ, so the blocks must not be used again
    P2pBlock *my_block = nullptr;        // fine-grained device memory, exported through HIP IPC
    P2pBlock *blocks[kMaxRanks] = {};    // every rank's block as mapped here (blocks[rank] == my_block)
    DevBuf<unsigned long long> d_exchanges;
    bool peer_mapped = false;            // blocks[] are plain peer pointers of this process (no IPC handles to close)
    bool device_shared = false;          // several ranks of ONE process run on this device (tests on a 1-GPU box): their
                                         // streams share the process's few hardware queues, where a solving wave that
                                         // waits for its peer can sit in front of that very peer's grid — such ranks
                                         // stay with the launch-per-iteration loop
};

// ---- the library's translation units call each other through these --------------------------------------
// capi.hip: the C ABI of maps, frames, communicators and the stand-alone entries.  capi_pipeline.hip: the pipeline
// handle and its entries.  capi_outputs.hip: rows, records and grids out (outputs.h).  caller_mem.hip: the checks of a
// caller's device memory (caller_mem.h).  capi_mirror.hip: the HBM mirror of a map and Update() on the device.
// capi_run.hip: the ICP loop (plan_loop, run_icp and its attempts), the RCCL binding and the single-process multi-GPU
// mode.
namespace sageicp_impl {
struct Rccl {
    void *h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                              hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;        // optional: what RCCL itself reports
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
};
extern Rccl g_rccl;
int load_rccl();
// capi.hip
int register_resident(const sageicp_map *m, const Point4 *d_frame, uint64_t n, int device, const double init[7],
                      double max_dist, double kernel, double sem_th, sageicp_comm *comm, double pose_out[7],
                      sageicp_stats *stats);
// capi_mirror.hip
int reserve_device_points(const sageicp_map *m, size_t units, size_t keep);
int sync_mirror(const sageicp_map *m);
int ensure_cand(const sageicp_map *m, bool derive = true);
bool map_is_empty(const sageicp_map *m);
int ensure_host(const sageicp_map *m);
int reserve_update_scratch(const sageicp_map *m, size_t n, size_t nb);
int grow_device_blocks(const sageicp_map *m, size_t blocks, size_t keep);
int reserve_unit_stacks(const sageicp_map *m, size_t n);
DevMap dev_map(const sageicp_map *m);
int device_update(sageicp_map *m, const double *xyzl, uint64_t n, const double pose[7], const Point4 *d_points = nullptr);
bool all_finite(const double *xyzl, uint64_t n);
// capi_run.hip
void identity_pose(double T[7]);
void fill_state(IcpState *st, const double init[7]);
bool sparse_voxels(const sageicp_map *m);
bool wants_filter(const sageicp_map *m, uint64_t n, double sem_th);
IcpParams icp_params(const sageicp_map *m, const Point4 *d_queries, uint64_t n, double sem_th, int lw, int acc_shift);
int run_icp(const sageicp_map *m, const Point4 *d_frame, uint64_t n, const double init[7], double max_dist, double kernel,
            double sem_th, sageicp_comm *comm, double out[7], sageicp_stats *stats, double us_upload, double t_begin);
int device_update_all(sageicp_map *m, const double *xyzl, uint64_t n, const double pose[7], const Point4 *d_points);
int register_sharded(const sageicp_map *m, const double *h_frame, const Point4 *d_frame, uint64_t n, const double init[7],
                     double max_dist, double kernel, double sem_th, double pose_out[7], sageicp_stats *stats, double t0);
}  // namespace sageicp_impl
using namespace sageicp_impl;
