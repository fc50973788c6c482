// Internals shared by the translation units of libsageicp_hip.so's host side (capi.hip, capi_pipeline.hip,
// capi_outputs.hip, capi_query.hip, capi_relocalize.hip, caller_mem.hip, map_device.hip, capi_run.hip, prep.hip): error channel, tuning knobs (knobs.h), the
// per-handle device scratch, the pipeline's frame source and buffers (prep.h) and its prefetch state (prefetch.h), the
// checks of a caller's device memory (caller_mem.h), the HBM copy of a map (map_device.h), the way out (outputs.h), what
// follows the search of GetCorrespondences on the device (correspond.h), the registration quality pass (quality.h), the
// batch score of candidate poses (score.h), the opaque handles of include/sageicp.h except the pipeline's (capi_pipeline.hip) and the one place where the ABI's
// `const sageicp_map *` becomes the reference the internals take (internal()).  Not part of the C ABI.
#pragma once

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cfloat>
#include <limits>
#include <memory>
#include <cstring>
#include <map>
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sageicp.h"
#include "dev_buffer.h"
#include "dyn_rules.h"
#include "host_map.hpp"
#include "kernels.h"
#include "knobs.h"
#include "egress.h"
#include "correspond.h"
#include "quality.h"
#include "score.h"
#include "place.h"
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

// tuning knobs (defaults chosen by measurement on MI355X; the environment overrides are for experiments only): knobs.h —
// knobs() is the snapshot of the last (re)load, and an entry that reads more than one knob takes it once

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
    // GetCorrespondences on the device (correspond.h): every query's accepted answer, the workgroups' counts and their
    // scan, the words the kernels leave (pairs, refusal flags) and their pinned landing place
    DevBuf<int32_t> d_by_query;
    DevBuf<uint32_t> d_corr_counts;
    DevBuf<unsigned long long> d_corr_words;
    PinnedBuf<unsigned long long> h_corr_words;
    // registration quality (quality.h): the workgroups' slabs, what the kernels leave and its pinned landing place
    DevBuf<double> d_qual_slabs;
    DevBuf<QualityRaw> d_qual_raw;
    PinnedBuf<QualityRaw> h_qual_raw;
    // the batch score of candidate poses (score.h): the frame's pristine rows, and per chunk the candidates as the
    // device applies them, the moved rows, their accepted answers, the workgroups' slabs, what the kernels leave and its
    // pinned landing place.  They grow to the largest chunk a call needed (SAGEICP_SCORE_CHUNK_ROWS rows) and stay
    // reserved on the handle, like every buffer here.
    DevBuf<Point4> d_score_frame, d_score_rows;
    DevBuf<int32_t> d_score_by_query;
    DevBuf<double> d_score_slabs;
    DevBuf<ScorePose> d_score_poses;
    PinnedBuf<ScorePose> h_score_poses;
    DevBuf<ScoreRaw> d_score_raw;
    PinnedBuf<ScoreRaw> h_score_raw;

    ~Scratch() { wait(); }         // (then the members go: nothing runs on the streams any more)
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
        if (const Knobs &k = knobs(); cu_share_k <= 1 && k.cu_share_set) {
            cu_share_i = k.cu_share_i;
            cu_share_k = k.cu_share_k;
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
    int reserve_correspond(size_t n) {
        if (n > d_by_query.capacity()) HIPCHK(d_by_query.reserve(n + n / 4 + 1024));
        const size_t words = 2 * static_cast<size_t>(correspond_blocks(static_cast<int>(n)));
        if (words > d_corr_counts.capacity()) HIPCHK(d_corr_counts.reserve(words + words / 4 + 16));
        if (!d_corr_words) HIPCHK(d_corr_words.reserve(2));
        if (!h_corr_words) HIPCHK(h_corr_words.reserve(2));
        return SAGEICP_OK;
    }
    int reserve_quality(size_t n) {
        if (n > d_by_query.capacity()) HIPCHK(d_by_query.reserve(n + n / 4 + 1024));
        if (!d_qual_slabs) HIPCHK(d_qual_slabs.reserve(kQualSlabDoubles));
        if (!d_qual_raw) HIPCHK(d_qual_raw.reserve(1));
        if (!h_qual_raw) HIPCHK(h_qual_raw.reserve(1));
        return SAGEICP_OK;
    }
    int reserve_score_frame(size_t n) {
        if (n > d_score_frame.capacity()) HIPCHK(d_score_frame.reserve(n + n / 4 + 1024));
        return SAGEICP_OK;
    }
    // a chunk of kc candidates of a frame of n rows
    int reserve_score(size_t n, size_t kc) {
        const size_t rows = n * kc, slabs = score_slab_doubles(static_cast<int>(n), static_cast<uint32_t>(kc));
        if (rows > d_score_rows.capacity()) HIPCHK(d_score_rows.reserve(rows + rows / 4 + 1024));
        if (rows > d_score_by_query.capacity()) HIPCHK(d_score_by_query.reserve(rows + rows / 4 + 1024));
        if (slabs > d_score_slabs.capacity()) HIPCHK(d_score_slabs.reserve(slabs + slabs / 4 + 1024));
        if (kc > d_score_poses.capacity()) HIPCHK(d_score_poses.reserve(kc + kc / 4 + 16));
        if (kc > h_score_poses.capacity()) HIPCHK(h_score_poses.reserve(kc + kc / 4 + 16));
        if (kc > d_score_raw.capacity()) HIPCHK(d_score_raw.reserve(kc + kc / 4 + 16));
        if (kc > h_score_raw.capacity()) HIPCHK(h_score_raw.reserve(kc + kc / 4 + 16));
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


}  // namespace sageicp

// the frame-preparation driver in front of registration (prep.hip): DynFilter, FrameSource, PrepJob, Prep
#include "prep.h"

using namespace sageicp;

#include "caller_mem.h"
#include "map_device.h"
#include "archive.h"
#include "recall.h"
#include "outputs.h"

// ---- opaque handles -----------------------------------------------------------------------
struct sageicp_map {
    HostMap host;
    int device = 0;
    Scratch sc;                                  // the ICP loop's buffers and streams
    sageicp_impl::MapDevice dev;                            // the copy in HBM, and which of the two copies counts (map_device.h)
    sageicp_impl::OutputBuffers out;             // sageicp_map_pointcloud*: the exports work in these (outputs.h)
    sageicp_impl::MapArchive arc;                // the log of evicted voxels (archive.h): off by default; replicas never archive
    // Single-process multi-GPU mode (SAGEICP_DEVICES / sageicp_map_set_devices): one more complete
    // copy of the map per extra device.  Every mutation is applied to all of them, RegisterFrame
    // shards the frame over them (one host thread and one stream per device) and the ranks'
    // Gauss-Newton sums meet in peer-mapped exchange blocks.  `this` is rank 0.
    std::vector<sageicp_map *> replicas;
    std::vector<struct sageicp_comm *> ranks;    // created at the first sharded registration
    // a mutation reached some copies of the map but not all (a device ran out of memory, ...): the
    // ranks would sum Gauss-Newton terms computed against different maps, so every later entry
    // refuses the handle until Clear() has emptied all copies
    bool replicas_diverged = false;

    bool resident() const { return dev.authority(); }
    bool empty() const { return counts().voxels == 0; }
    // what the map holds, read from the copy that counts: the one place that chooses between the two
    sageicp_impl::MapCounts counts() const {
        const bool on_device = dev.authority();
        const MapCounters &c = dev.ctr;
        sageicp_impl::MapCounts n;
        n.points = on_device ? c.total_points : host.total_points;
        n.voxels = on_device ? c.num_voxels : host.num_voxels;
        n.units_hi = on_device ? c.units_hi : host.units_hi;
        n.table_capacity = on_device ? dev.d_table.capacity() : host.table.size();
        n.used_slots = on_device ? c.used_slots : host.num_voxels;
        return n;
    }
    // the buffers above are used on sc's streams and go before sc does: the streams are waited for first
    ~sageicp_map() { sc.wait(); }
};

// The ABI's `const sageicp_map *` says that the map as a set of points is unchanged by the call.  Its representation
// changes under it — the HBM mirror is refreshed lazily by a search, the host copy is downloaded on demand, the scratch
// is used — so the extern "C" entries, and only they, turn their pointer into the reference the internals take here.
// (Handles are created with `new sageicp_map`, never as const objects: the cast is defined.)
inline sageicp_map &internal(const sageicp_map *m) { return *const_cast<sageicp_map *>(m); }

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
// capi.hip: the C ABI of maps, frames, communicators and the stand-alone entries that ask a map nothing.
// capi_pipeline.hip: the pipeline handle and its entries.  capi_outputs.hip: rows, records and grids out (outputs.h).
// caller_mem.hip: the checks of a caller's device memory (caller_mem.h).  map_device.hip: the HBM copy of a map
// (MapDevice): mirror refresh, download, copy, Update() on the device.
// capi_query.hip: the one path of the entries that ask a map about a frame — stage, move, sort and search, accept
// (query.h) — with GetCorrespondences, RegistrationQuality and the host side of the quality report.
// capi_relocalize.hip: the candidate grid, the chunked batch score of candidate poses and Relocalize, on that path.
// capi_run.hip: the ICP loop (plan_loop, run_icp and its attempts), the RCCL binding and the single-process multi-GPU
// mode.  capi_recall.hip: recall (recall.h) — a place of a session's map into a second handle, on the device.
// capi_closure.hip: loop closure (closure.h) — the corrections of a trajectory, the stays, the session's map re-posed.
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
int register_resident(sageicp_map &m, const Point4 *d_frame, uint64_t n, int device, const double init[7],
                      double max_dist, double kernel, double sem_th, sageicp_comm *comm, double pose_out[7],
                      sageicp_stats *stats);
// (capi_query.hip: query.h)
// map_device.hip: the handle's device made current, its stream and host copy handed to MapDevice
int refresh_mirror(sageicp_map &m);
int ensure_host(sageicp_map &m);
int device_update(sageicp_map &m, const double *xyzl, uint64_t n, const double pose[7], const Point4 *d_points = nullptr);
bool all_finite(const double *xyzl, uint64_t n);
// capi_place.hip: place recognition (place.h) — the checks of its parameter structs, a database for the pipeline, and the
// pipeline's step for a key frame: describe the n raw rows at d_rows, match against the database as it is, append
int place_check_params(const sageicp_place_params *p);
int place_check_query(const sageicp_place_query *q);
sageicp_place_db *place_db_new(const sageicp_place_params &p, int device);
void place_db_clear(sageicp_place_db &db);
int place_db_step(sageicp_place_db &db, const Point4 *d_rows, uint64_t n, const sageicp_place_query &q, uint64_t tag,
                  const double pose[7], hipStream_t s, sageicp_place_match *out, uint32_t *n_out);
// capi_recall.hip: a session's map as two RecallParts (recall.h) — the records of a handle's archive in log order, its live
// voxels in Pointcloud() order — and what they point into, for one call (nothing is cached between calls): what recall
// selects from and the closure entries (capi_closure.hip) enumerate
struct LatestBuffers {               // what archive_latest works in
    DevBuf<unsigned long long> keys, keys_alt;
    DevBuf<uint32_t> idx, idx_alt, flag, sel, counts, offsets, n_sel;
    DevBuf<unsigned char> temp;
    LatestScratch view() const {
        return LatestScratch{keys.data(), keys_alt.data(), idx.data(), idx_alt.data(), flag.data(), sel.data(), counts.data(),
                             offsets.data(), n_sel.data(), temp.data(), temp.capacity()};
    }
    int reserve(size_t nv) {
        HIPCHK(keys.reserve(nv)); HIPCHK(keys_alt.reserve(nv));
        HIPCHK(idx.reserve(nv)); HIPCHK(idx_alt.reserve(nv)); HIPCHK(flag.reserve(nv)); HIPCHK(sel.reserve(nv));
        HIPCHK(counts.reserve(nv + 1)); HIPCHK(offsets.reserve(nv + 1)); HIPCHK(n_sel.reserve(1));
        HIPCHK(temp.reserve(archive_latest_temp_bytes(nv)));
        return SAGEICP_OK;
    }
};
struct SessionParts {
    LatestBuffers lb;
    RecallPart part[2]{};            // the records, the live voxels (scratch pointers: the user's)
    DevBuf<Slot> d_cand;             // the live voxels of a host-authoritative source
    DevBuf<uint32_t> d_list;         // the bucket order of a resident source in reference-order mode
    std::vector<Slot> h_cand;        // (pageable: they live until the stream has been waited for)
    std::vector<uint32_t> h_list;
};
// on s, the map's stream; a pending host tail of the archive is moved to the device first.  latest_only: the LATEST
// verdicts decide (the mirror refreshed for them, as before any search); otherwise every record is a candidate
int session_archive_part(sageicp_map &src, hipStream_t s, bool latest_only, SessionParts &sp);
int session_live_part(sageicp_map &src, hipStream_t s, SessionParts &sp);   // (after session_archive_part(.., true, ..): it reads the mirror)
bool same_policy(const HostMap &a, const HostMap &b);      // capi_recall.hip: voxel size, points per voxel, basic labels
// capi_closure.hip: the argument checks of the closure entries (`who`: the entry, for the message), and a pipeline's
// positions (and poses) where serial s of its archive is pose s — shared with the rebuild's entries (capi_rebuild.hip)
int check_selection(const sageicp_map *m, int which, const double *positions, uint64_t n, const uint64_t *n_out, const char *who);
int check_corrections(const double *corr, uint64_t n, const char *who);
int pipeline_positions(const sageicp_pipeline *p, const char *who, std::vector<double> &pos, std::vector<double> *poses);
// capi_archive.hip: RemovePointsFarFromLocation on the host copy of one handle, the evicted voxels into its archive while on
void host_remove_far(sageicp_map &m, const double origin[3]);
// capi_run.hip
void identity_pose(double T[7]);
void fill_state(IcpState *st, const double init[7]);
double accept_threshold(double max_dist);
bool sparse_voxels(const sageicp_map &m);
int icp_lw(const Knobs &k, uint64_t n, bool sparse_voxels);
bool wants_filter(const Knobs &k, const sageicp_map &m, uint64_t n, double sem_th);
IcpParams icp_params(const Knobs &k, const sageicp_map &m, const Point4 *d_queries, uint64_t n, double sem_th, int lw, int acc_shift);
int run_icp(sageicp_map &m, const Point4 *d_frame, uint64_t n, const double init[7], double max_dist, double kernel,
            double sem_th, sageicp_comm *comm, double out[7], sageicp_stats *stats, double us_upload, double t_begin);
int device_update_all(sageicp_map &m, const double *xyzl, uint64_t n, const double pose[7], const Point4 *d_points);
int register_sharded(sageicp_map &m, const double *h_frame, const Point4 *d_frame, uint64_t n, const double init[7],
                     double max_dist, double kernel, double sem_th, double pose_out[7], sageicp_stats *stats, double t0);
}  // namespace sageicp_impl
using namespace sageicp_impl;
