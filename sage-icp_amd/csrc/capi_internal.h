// Internals shared by the translation units of libsageicp_hip.so's host side (capi.hip, capi_mirror.hip,
// capi_run.hip): error channel, tuning knobs, the per-handle device scratch, the pipeline's buffers, the opaque
// handles of include/sageicp.h.  Not part of the C ABI.
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

struct DynFilterConfig {
    double dy_th = 0.5;
    std::vector<uint32_t> dynamic_labels;      // the reference's std::vector<int>, compared as uint32_t
    std::vector<uint32_t> landmark_labels;
};

// buffers of one Prep; run() filters a frame already on the device (n points at `in`) into `out` (may be `in`),
// passing the cropped points through `tmp` (n points)
struct DynFilter {
    size_t cap = 0;                            // points the buffers of reserve() hold (all of them: 0 after a failed reserve)
    DevBuf<uint32_t> d_labels, d_ctr;
    PinnedBuf<uint32_t> h_ctr;                 // [0..3] counters, [4] flags
    DevBuf<unsigned long long> d_cnt, d_pos, d_vkey, d_lkey, d_count;
    DevBuf<float4> d_vp, d_vs, d_lp, d_ls;
    DevBuf<uint32_t> d_vval, d_lval, d_vframe, d_parent, d_root, d_size, d_rec_of_root, d_start, d_rkv, d_off;
    DevBuf<uint4> d_rec;
    DevBuf<unsigned char> d_temp;
    PinnedBuf<uint4> h_rec;                    // the component table
    PinnedBuf<uint32_t> h_off;                 // output offset per component (~0: dropped)
    OwnedEvent ev[6];                          // device time of the three launch batches (sageicp_set_profiling)
    OwnedEvent ev_table;
    std::vector<uint32_t> order_scratch, size_scratch;
    sageicp_dynfilter_info info{};             // of the last run

    int reserve(size_t n, size_t nlabels);
    int run(const Point4 *in, uint64_t n, double max_range, double min_range, double label_max_range,
            const DynFilterConfig &cfg, Point4 *tmp, Point4 *out, int *d_ovf, uint64_t &n_out, hipStream_t s);
};

// ---- deskew of a frame before it is preprocessed (deskew.hip; core/Deskew.cpp:36-50) ---------------------------
struct DeskewArgs {
    const double *timestamps;           // host, one per point, all finite (checked by the caller); a device frame's are in
                                        // its DeviceSource
    DeskewTangent delta;                // (start.inverse() * finish).log()
};

// A raw frame in the caller's device memory (sageicp_device_frame, validated by capi.hip): the ingest kernel reads it
// into d_in on Prep::stream once that stream has waited for the caller's.  timestamps: device, n of them, or nullptr
// (not asked for); they are copied to d_ts and checked in the same pass.
struct MsgSource;
struct DeviceSource {
    const sageicp_device_frame *frame;
    const double *timestamps;
    hipStream_t stream;
    const MsgSource *msg = nullptr;     // the frame is a message's payload instead (frame and timestamps are not read)
};
// A sensor_msgs/PointCloud2 payload (sageicp_msg_layout, validated by capi.hip): n records in host memory, which are
// uploaded as they are, or in the caller's device memory, read in place behind DeviceSource::stream.  k_msg_unpack
// (msg.hip) writes the rows into d_in and, with want_time, the stamps into d_ts.
struct MsgSource {
    const unsigned char *host;          // one of the two is set
    const unsigned char *device;
    sageicp_msg_layout layout;
    bool want_time;                     // deskew is on: the time field is read and checked (layout.time_kind != 0)
};
inline IngestArgs ingest_args(const sageicp_device_frame &f) {
    IngestArgs a{};
    a.xyz = static_cast<const unsigned char *>(f.xyz);
    a.xyz_stride = f.xyz_stride;
    a.xyz_dtype = f.xyz_dtype;
    a.label = static_cast<const unsigned char *>(f.label);
    a.label_stride = f.label_stride;
    a.label_dtype = f.label_dtype;
    a.n = static_cast<int>(f.n);
    return a;
}

// ---- device preprocessing (preprocess.hip): buffers of one pipeline ------------------------------
struct Prep {
    int device = -1;
    OwnedStream stream;
    size_t cap = 0;                     // points the buffers of reserve() hold (all of them: 0 after a failed reserve)
    DevBuf<Point4> d_in, d_tmp, d_fd, d_src;
    DevBuf<uint32_t> d_slot, d_skey, d_sval, d_winner;
    DevBuf<unsigned long long> d_keys;
    DevBuf<unsigned char> d_sort_temp;
    DevBuf<unsigned long long> d_okeys;      // survivors' voxel keys (reference-order emission)
    DevBuf<uint32_t> d_perm;
    PinnedBuf<unsigned long long> h_keys;
    PinnedBuf<uint32_t> h_perm;
    std::vector<uint32_t> h_hash;
    RobinScratch rscratch[8];                // bucket arrays of the order replay, one pair per label group
    std::unique_ptr<ReplayPool> pool;        // parked helper threads of the order replays
    double us_order = 0;                // host time of the last run's order replays
    // levels whose survivors are emitted in arrival order even under g_reference_order (bit l): the
    // pipeline's second level — its cloud is only registered, and registration sorts its frame
    // spatially first, so its emission order reaches nothing but the order of fp64 summation
    unsigned arrival_order_levels = 0;
    DevBuf<uint32_t> d_nkept;           // [2]
    DevBuf<int> d_overflow;
    DevBuf<int> d_gcounts, d_glabels;
    PinnedBuf<Point4> h_pin;            // staging for the raw frame and the results
    uint32_t kept_levels[2] = {0, 0};   // points the last run left in d_fd / d_src
    DynFilter dyn;                      // the dynamic vehicle filter's buffers (allocated with its first use)
    bool dyn_ran = false;               // the last run filtered (dyn.info describes its frame)
    // the timestamps of a frame that is deskewed (allocated with the first such frame): pinned staging, device copy
    PinnedBuf<double> h_ts;
    DevBuf<double> d_ts;
    OwnedEvent ev_caller;               // a device frame: orders the caller's stream before `stream` (created with the first)
    // key-frame selection (keyframe.hip): the raw frame copied aside before deskew and the dynamic filter rewrite d_in
    // in place — its coordinates checked — for the pass that follows the registration (allocated with the first use)
    bool keep_raw = false;
    DevBuf<Point4> d_raw;
    // a message's payload (MsgSource): pinned staging and device copy of host bytes, the maximum of uint32 stamps
    // (allocated with the first such frame)
    PinnedBuf<unsigned char> h_blob;
    DevBuf<unsigned char> d_blob;
    DevBuf<uint32_t> d_tmax;

    // waits for the stream with the device current, then the members go, dyn's among them: nothing runs on the stream
    // any more (a Prep that never created its stream calls nothing)
    ~Prep() {
        if (!stream) return;
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream.get());
    }

    int init(int dev) {
        if (stream) return SAGEICP_OK;
        if (int rc = require_device(dev)) return rc;
        device = dev;
        HIPCHK(hipSetDevice(device));
        HIPCHK(stream.create());
        HIPCHK(d_nkept.reserve(2));
        HIPCHK(d_overflow.reserve(1));
        HIPCHK(d_gcounts.reserve(8));
        return SAGEICP_OK;
    }
    int reserve(size_t n, size_t nlabels) {
        if (nlabels > d_glabels.capacity()) HIPCHK(d_glabels.reserve(nlabels + 16));
        if (n <= cap) return SAGEICP_OK;
        cap = 0;
        const size_t c = n + n / 4 + 1024;
        uint32_t t = 1024;
        while (t < 2 * c) t <<= 1;
        HIPCHK(d_in.reserve(c));
        HIPCHK(d_tmp.reserve(c));
        HIPCHK(d_fd.reserve(c));
        HIPCHK(d_src.reserve(c));
        HIPCHK(d_slot.reserve(c));
        HIPCHK(d_skey.reserve(2 * c));
        HIPCHK(d_sval.reserve(2 * c));
        HIPCHK(d_keys.reserve(t));
        HIPCHK(d_winner.reserve(t));
        HIPCHK(d_okeys.reserve(c));
        HIPCHK(d_perm.reserve(c));
        HIPCHK(h_keys.reserve(c));
        HIPCHK(h_perm.reserve(c));
        HIPCHK(d_sort_temp.reserve(vds_sort_temp_bytes(static_cast<int>(c))));
        HIPCHK(h_pin.reserve(3 * c));
        cap = c;
        return SAGEICP_OK;
    }
    // (the staging copy goes first and comes back last: after a failed reserve it is empty)
    int reserve_timestamps(size_t n) {
        if (n <= h_ts.capacity()) return SAGEICP_OK;
        const size_t c = n + n / 4 + 1024;
        h_ts.reset();
        HIPCHK(d_ts.reserve(c));
        HIPCHK(h_ts.reserve(c));
        return SAGEICP_OK;
    }

    // The raw frame of a device source into d_in (and its timestamps into d_ts), after the work the caller enqueued on
    // its stream.  Timestamps are checked here, before anything reads them: a non-finite one refuses the frame (the
    // host entry's check, sageicp_pipeline_register_frame_timestamps).  The caller's buffers are last read by this
    // launch, which the first level's synchronisation waits for: run() returns with them released.
    int ingest(const DeviceSource &src, uint64_t n) {
        if (src.msg) return ingest_msg(*src.msg, src.stream, n);
        if (!ev_caller) HIPCHK(ev_caller.create(hipEventDisableTiming));
        HIPCHK(hipEventRecord(ev_caller.get(), src.stream));
        HIPCHK(hipStreamWaitEvent(stream.get(), ev_caller.get(), 0));
        IngestArgs a = ingest_args(*src.frame);
        a.n = static_cast<int>(n);
        a.ts = src.timestamps;
        a.ts_out = src.timestamps ? d_ts.data() : nullptr;
        a.flags = d_overflow.data();
        launch_ingest(a, d_in.data(), stream.get());
        HIPCHK(hipGetLastError());
        if (src.timestamps) {
            int flags = 0;
            HIPCHK(hipMemcpyAsync(&flags, d_overflow.data(), sizeof(int), hipMemcpyDeviceToHost, stream.get()));
            HIPCHK(hipStreamSynchronize(stream.get()));
            if (flags & kIngestBadTimestamp) return fail(SAGEICP_ERR_INVALID, "deskew is on and a timestamp is not finite");
        }
        return SAGEICP_OK;
    }

    // The same of a message's payload: host bytes cross PCIe as they are (through the pinned staging copy), device bytes
    // are read in place behind the caller's stream.  uint32 stamps are normalised by their maximum in a second small
    // pass (NormalizeTimestamps); float64 stamps are checked like a device frame's.
    int ingest_msg(const MsgSource &m, hipStream_t caller, uint64_t n) {
        const size_t bytes = static_cast<size_t>(n) * m.layout.point_step;
        const unsigned char *d = m.device;
        if (m.host) {
            if (bytes > h_blob.capacity()) {
                const size_t c = bytes + bytes / 4 + 4096;
                h_blob.reset();
                HIPCHK(d_blob.reserve(c));
                HIPCHK(h_blob.reserve(c));
            }
            std::memcpy(h_blob.data(), m.host, bytes);
            HIPCHK(hipMemcpyAsync(d_blob.data(), h_blob.data(), bytes, hipMemcpyHostToDevice, stream.get()));
            d = d_blob.data();
        } else {
            if (!ev_caller) HIPCHK(ev_caller.create(hipEventDisableTiming));
            HIPCHK(hipEventRecord(ev_caller.get(), caller));
            HIPCHK(hipStreamWaitEvent(stream.get(), ev_caller.get(), 0));
        }
        MsgUnpackArgs a{};
        a.data = d;
        a.point_step = m.layout.point_step;
        a.x_offset = m.layout.x_offset; a.y_offset = m.layout.y_offset; a.z_offset = m.layout.z_offset;
        a.label_offset = m.layout.label_offset;
        a.label_dtype = m.layout.label_dtype;
        a.time_kind = m.want_time ? m.layout.time_kind : 0;
        a.time_offset = m.layout.time_offset;
        a.n = static_cast<int>(n);
        a.ts_out = a.time_kind ? d_ts.data() : nullptr;
        a.flags = d_overflow.data();
        if (a.time_kind == 1) {
            if (!d_tmax) HIPCHK(d_tmax.reserve(1));
            HIPCHK(hipMemsetAsync(d_tmax.data(), 0, sizeof(uint32_t), stream.get()));
            a.ts_max = d_tmax.data();
        }
        launch_msg_unpack(a, d_in.data(), stream.get());
        HIPCHK(hipGetLastError());
        if (a.time_kind == 1) {
            launch_msg_normalize(d_ts.data(), a.n, d_tmax.data(), stream.get());
            HIPCHK(hipGetLastError());
        }
        if (a.time_kind == 2) {
            int flags = 0;
            HIPCHK(hipMemcpyAsync(&flags, d_overflow.data(), sizeof(int), hipMemcpyDeviceToHost, stream.get()));
            HIPCHK(hipStreamSynchronize(stream.get()));
            if (flags & kIngestBadTimestamp) return fail(SAGEICP_ERR_INVALID, "deskew is on and a timestamp is not finite");
        }
        return SAGEICP_OK;
    }

    // levels: each {do_crop, scale}; a scale <= 0 means "crop only" (no voxel test).  Runs the
    // levels in sequence on the device, each feeding the next, and returns every level's cloud.
    // With `dyn_cfg` the frame first goes through Preprocess()'s dynamic vehicle filter (dyn_filter.hip), which
    // crops it itself: the levels then start from the filtered cloud with the crop off.
    // With `deskew` the uploaded frame is deskewed in place before anything else reads it (the reference's order:
    // DeSkewScan, then Preprocess, then Voxelize; pipeline/sageICP.cpp:36-52).
    // With `dev` the raw frame comes from the caller's device memory instead of `frame` (ingest()); everything after
    // it reaches d_in is the same.
    int run(const double *frame, uint64_t n, double max_range, double min_range,
            double label_max_range, int n_groups, const int *gcounts, const int *glabels,
            const double *gvs, const int *crop, const double *scales, int n_levels,
            std::vector<std::vector<double>> &out, bool download = true,
            const DynFilterConfig *dyn_cfg = nullptr, const DeskewArgs *deskew = nullptr,
            const DeviceSource *dev = nullptr) {
        kept_levels[0] = kept_levels[1] = 0;
        us_order = 0;
        dyn_ran = dyn_cfg != nullptr;
        dyn.info = sageicp_dynfilter_info{};
        if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "frame too large (2^26 - 4 points max)");
        if (n_groups > 8) return fail(SAGEICP_ERR_INVALID, "at most 8 label groups");
        size_t nlabels = 0;
        for (int g = 0; g < n_groups; ++g) nlabels += static_cast<size_t>(gcounts[g]);
        int rc = reserve(n, nlabels);
        if (rc) return rc;
        if (deskew || (dev && (dev->timestamps || (dev->msg && dev->msg->want_time)))) {
            rc = reserve_timestamps(n);
            if (rc) return rc;
        }
        HIPCHK(hipSetDevice(device));
        out.assign(n_levels, std::vector<double>());
        if (n == 0) return SAGEICP_OK;
        if (n_groups > 0) {
            HIPCHK(hipMemcpyAsync(d_gcounts.data(), gcounts, n_groups * sizeof(int), hipMemcpyHostToDevice, stream.get()));
            HIPCHK(hipMemcpyAsync(d_glabels.data(), glabels, nlabels * sizeof(int), hipMemcpyHostToDevice, stream.get()));
        }
        HIPCHK(hipMemsetAsync(d_overflow.data(), 0, sizeof(int), stream.get()));
        if (keep_raw && d_raw.capacity() < n) HIPCHK(d_raw.reserve(n + n / 4 + 1024));
        if (dev) {
            rc = ingest(*dev, n);
            if (rc) return rc;
            if (keep_raw) launch_occ_keep(d_in.data(), d_raw.data(), static_cast<int>(n), d_overflow.data(), stream.get());
            if (deskew) {
                launch_deskew(d_in.data(), d_in.data(), d_ts.data(), static_cast<int>(n), deskew->delta, stream.get());
                HIPCHK(hipGetLastError());
            }
        } else {
            std::memcpy(h_pin.data(), frame, n * sizeof(Point4));
            HIPCHK(hipMemcpyAsync(d_in.data(), h_pin.data(), n * sizeof(Point4), hipMemcpyHostToDevice, stream.get()));
            if (keep_raw) launch_occ_keep(d_in.data(), d_raw.data(), static_cast<int>(n), d_overflow.data(), stream.get());
            if (deskew) {
                std::memcpy(h_ts.data(), deskew->timestamps, n * sizeof(double));
                HIPCHK(hipMemcpyAsync(d_ts.data(), h_ts.data(), n * sizeof(double), hipMemcpyHostToDevice, stream.get()));
                launch_deskew(d_in.data(), d_in.data(), d_ts.data(), static_cast<int>(n), deskew->delta, stream.get());
                HIPCHK(hipGetLastError());
            }
        }
        const Point4 *in = d_in.data();
        Point4 *outs[2] = {d_fd.data(), d_src.data()};
        uint64_t cur = n;
        if (dyn_cfg) {      // the filtered cloud replaces the frame in d_in (the filter has read it by then)
            int r = dyn.run(d_in.data(), n, max_range, min_range, label_max_range, *dyn_cfg, d_tmp.data(), d_in.data(), d_overflow.data(), cur,
                            stream.get());
            if (r) return r;
        }
        for (int l = 0; l < n_levels; ++l) {
            VdsParams P{};
            P.in = in; P.n = static_cast<int>(cur); P.do_crop = dyn_cfg ? 0 : crop[l];
            P.max_range = max_range; P.min_range = min_range; P.label_max_range = label_max_range;
            P.n_groups = scales[l] > 0.0 ? n_groups : -1;
            P.group_counts = d_gcounts.data(); P.group_labels = d_glabels.data();
            for (int g = 0; g < n_groups; ++g) P.group_vs[g] = gvs[g];
            P.scale = scales[l];
            P.keys = d_keys.data(); P.winner = d_winner.data(); P.mask = static_cast<uint32_t>(d_keys.capacity() - 1);
            P.tmp = d_tmp.data(); P.slot_of = d_slot.data(); P.sort_key = d_skey.data(); P.sort_val = d_sval.data();
            P.overflow = d_overflow.data();
            const bool reorder = g_reference_order && P.n_groups > 0 && !((arrival_order_levels >> l) & 1u);
            P.out_keys = reorder ? d_okeys.data() : nullptr;
            Point4 *dst = outs[l & 1];
            HIPCHK(voxel_downsample_device(P, d_sort_temp.data(), d_sort_temp.capacity(), d_nkept.data() + (l & 1), dst, stream.get()));
            uint32_t kept = 0;
            HIPCHK(hipMemcpyAsync(&kept, d_nkept.data() + (l & 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream.get()));
            HIPCHK(hipStreamSynchronize(stream.get()));
            kept_levels[l & 1] = kept;
            if (reorder && kept) {
                // the reference's emission order (Preprocessing.cpp:76-82): replay, group by
                // group, the insertions into its robin_map and permute the survivors
                const double t0 = now_us();
                HIPCHK(hipMemcpyAsync(h_keys.data(), d_okeys.data(), kept * sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, stream.get()));
                HIPCHK(hipStreamSynchronize(stream.get()));
                const double t1 = now_us();
                h_hash.resize(kept);
                // survivors are grouped (stable sort by group); the groups' tables are independent:
                // one host thread per group hashes and replays its run and writes its part of the
                // permutation in place
                std::vector<std::pair<uint32_t, uint32_t>> runs;
                for (uint32_t a = 0; a < kept;) {
                    const unsigned long long g = h_keys.data()[a] >> 60;
                    uint32_t lo = a, hi = kept;            // first index of another group (binary search: the runs are long)
                    while (hi - lo > 1) {
                        const uint32_t mid = lo + (hi - lo) / 2;
                        if ((h_keys.data()[mid] >> 60) == g) lo = mid; else hi = mid;
                    }
                    runs.emplace_back(a, hi);
                    a = hi;
                }
                auto replay = [&](size_t r) {
                    const uint32_t a = runs[r].first, b = runs[r].second;
                    for (uint32_t i = a; i < b; ++i) h_hash[i] = static_cast<uint32_t>(h_keys.data()[i] & 0xFFFFFu);   // hashed on the device
                    std::vector<uint32_t> part;
                    part.reserve(b - a);
                    if (!RobinOrderReplay::iteration_order(h_hash.data() + a, b - a, a, part, &rscratch[r & 7])) {
                        // a probe distance the replay does not model (robin_order.hpp): this group keeps
                        // its arrival order — said once, loudly, because the poses of a stream then
                        // differ from the reference's by centimetres
                        static std::atomic<bool> told{false};
                        if (!told.exchange(true))
                            std::fprintf(stderr, "sageicp: VoxelDownsample: a label group of %u voxels exceeds the probe "
                                                 "distance the tsl::robin_map replay models; it is emitted in arrival order\n",
                                         b - a);
                        part.resize(b - a);
                        for (uint32_t i = a; i < b; ++i) part[i - a] = i;
                    }
                    std::memcpy(h_perm.data() + a, part.data(), (b - a) * sizeof(uint32_t));
                };
                // The groups' replays are independent and the largest (half of the survivors on street
                // scenes) is the critical path: every group gets its own thread — parked helpers of
                // this Prep, woken per level (starting threads costs what a small replay does) —
                // largest first, the calling thread takes part.
                std::vector<size_t> by_size(runs.size());
                for (size_t r = 0; r < runs.size(); ++r) by_size[r] = r;
                std::sort(by_size.begin(), by_size.end(), [&](size_t x, size_t y) {
                    return runs[x].second - runs[x].first > runs[y].second - runs[y].first;
                });
                if (kept > 8192 && runs.size() > 1) {
                    if (!pool) pool.reset(new ReplayPool);
                    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
                    pool->run(runs.size(), [&](size_t k) { replay(by_size[k]); },
                              std::min<size_t>(hw, static_cast<size_t>(std::max(1, env_int("SAGEICP_REPLAY_THREADS", 8)))));
                } else {
                    for (size_t r = 0; r < runs.size(); ++r) replay(r);
                }
                const double t2 = now_us();
                HIPCHK(hipMemcpyAsync(d_perm.data(), h_perm.data(), kept * sizeof(uint32_t), hipMemcpyHostToDevice, stream.get()));
                launch_vds_permute(dst, d_perm.data(), kept, d_tmp.data(), stream.get());
                HIPCHK(hipMemcpyAsync(dst, d_tmp.data(), kept * sizeof(Point4), hipMemcpyDeviceToDevice, stream.get()));
                us_order += now_us() - t0;
                if (env_int("SAGEICP_DEBUG_ORDER", 0)) {
                    std::string rs;
                    for (auto &r : runs) rs += " " + std::to_string(r.second - r.first);
                    std::fprintf(stderr, "order level %d: kept %u, fetch keys %.0f us, replay %.0f us (runs:%s), rest %.0f us\n",
                                 l, kept, t1 - t0, t2 - t1, rs.c_str(), now_us() - t2);
                }
            }
            if (download) {       // otherwise the level's cloud stays in d_fd / d_src for the caller
                Point4 *hp = h_pin.data() + static_cast<size_t>(1 + (l & 1)) * cap;
                if (kept) HIPCHK(hipMemcpyAsync(hp, dst, kept * sizeof(Point4), hipMemcpyDeviceToHost, stream.get()));
                HIPCHK(hipStreamSynchronize(stream.get()));
                out[l].resize(4 * static_cast<size_t>(kept));
                if (kept) std::memcpy(out[l].data(), hp, kept * sizeof(Point4));
            }
            in = dst;
            cur = kept;
        }
        int ovf = 0;
        HIPCHK(hipMemcpy(&ovf, d_overflow.data(), sizeof(int), hipMemcpyDeviceToHost));
        if (ovf & kOccNonFinite)
            return fail(SAGEICP_ERR_INVALID, "key-frame selection is on and a coordinate is not finite (NaN / Inf)");
        if (ovf & 2) return fail(SAGEICP_ERR_INVALID, "a label (or, without the range crop, a coordinate) is not finite (NaN / Inf)");
        if (ovf) return fail(SAGEICP_ERR_CAPACITY, "voxel index beyond +-2^19 in VoxelDownsample");
        return SAGEICP_OK;
    }
};

}  // namespace sageicp

using namespace sageicp;

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
    // Pointcloud() served from the HBM copy: the packed points before they cross PCIe
    mutable DevBuf<Point4> d_pc;
    // sageicp_map_pointcloud_msg: the 21-byte records before they cross PCIe
    mutable DevBuf<unsigned char> d_msg;
    // sageicp_map_pointcloud_device: the label-range flag (egress.h) and the event that orders the caller's stream
    // before the map's (created with the first call)
    mutable DevBuf<int> d_egress_flag;
    mutable OwnedEvent ev_caller;
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
// capi.hip: the C ABI.  capi_mirror.hip: the HBM mirror of a map and Update() on the device.  capi_run.hip: the ICP
// loop (plan_loop, run_icp and its attempts), the RCCL binding and the single-process multi-GPU mode.
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
