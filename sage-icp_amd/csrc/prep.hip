// Prep (prep.h): one frame from where it arrives — host rows, the caller's device memory, a message's payload — through
// keep-raw, deskew, the dynamic vehicle filter and the VoxelDownsample levels, in the reference's emission order, all
// on Prep::stream.  Host code only; the kernels are preprocess.hip's, deskew.hip's, ingest.hip's, msg.hip's,
// keyframe.hip's and dyn_filter.hip's.  Part of libsageicp_hip.so's host side: capi_internal.h.
#include "capi_internal.h"

#include <cassert>
#include <thread>

namespace sageicp {

Prep::~Prep() {
    if (!stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream.get());
}

int Prep::init(int dev) {
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

int Prep::reserve(size_t n, size_t nlabels) {
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
int Prep::reserve_timestamps(size_t n) {
    if (n <= h_ts.capacity()) return SAGEICP_OK;
    const size_t c = n + n / 4 + 1024;
    h_ts.reset();
    HIPCHK(d_ts.reserve(c));
    HIPCHK(h_ts.reserve(c));
    return SAGEICP_OK;
}

int Prep::run(const FrameSource &src, const PrepJob &job) {
    assert(job.n_levels <= 2);
    const uint64_t n = src.n;
    int rc = reset_and_reserve(src, job);
    if (rc || n == 0) return rc;
    if ((rc = load(src, src.stamps_to_device(job.deskew != nullptr)))) return rc;
    if ((rc = keep_raw_and_deskew(n, job.deskew))) return rc;
    const Point4 *in = d_in.data();
    Point4 *const outs[2] = {d_fd.data(), d_src.data()};
    uint64_t cur = n;
    // the filtered cloud replaces the frame in d_in (the filter has read it by then)
    if (job.dyn && (rc = dyn.run(d_in.data(), n, job.max_range, job.min_range, job.label_max_range, *job.dyn, d_tmp.data(),
                                 d_in.data(), d_overflow.data(), cur, stream.get())))
        return rc;
    for (int l = 0; l < job.n_levels; ++l) {
        const bool reorder = g_reference_order && job.levels[l].scale > 0.0 && job.n_groups > 0 &&
                             !((arrival_order_levels >> l) & 1u);
        uint32_t kept = 0;
        if ((rc = downsample(l, in, cur, job, reorder, outs[l], kept))) return rc;
        if (reorder && kept && (rc = restore_reference_order(l, outs[l], kept))) return rc;
        in = outs[l];
        cur = kept;
    }
    return refuse_flags();
}

// What the last run left is forgotten, the buffers hold n points, and — for a frame that has points — the group tables
// are on the device and the flag word is clear.
int Prep::reset_and_reserve(const FrameSource &src, const PrepJob &job) {
    const uint64_t n = src.n;
    kept_levels[0] = kept_levels[1] = 0;
    dyn_ran = job.dyn != nullptr;
    dyn.info = sageicp_dynfilter_info{};
    if (n > kMaxQueries) return fail(SAGEICP_ERR_INVALID, "frame too large (2^26 - 4 points max)");
    if (job.n_groups > 8) return fail(SAGEICP_ERR_INVALID, "at most 8 label groups");
    size_t nlabels = 0;
    for (int g = 0; g < job.n_groups; ++g) nlabels += static_cast<size_t>(job.group_counts[g]);
    if (int rc = reserve(n, nlabels)) return rc;
    if (job.deskew || src.stamps_to_device(false))
        if (int rc = reserve_timestamps(n)) return rc;
    HIPCHK(hipSetDevice(device));
    if (n == 0) return SAGEICP_OK;
    if (job.n_groups > 0) {
        HIPCHK(hipMemcpyAsync(d_gcounts.data(), job.group_counts, job.n_groups * sizeof(int), hipMemcpyHostToDevice, stream.get()));
        HIPCHK(hipMemcpyAsync(d_glabels.data(), job.group_labels, nlabels * sizeof(int), hipMemcpyHostToDevice, stream.get()));
    }
    HIPCHK(hipMemsetAsync(d_overflow.data(), 0, sizeof(int), stream.get()));
    if (keep_raw && d_raw.capacity() < n) HIPCHK(d_raw.reserve(n + n / 4 + 1024));
    return SAGEICP_OK;
}

// The raw frame into d_in and, with `stamps` (FrameSource::stamps_to_device), its stamps into d_ts.  What follows does
// not know where from.
int Prep::load(const FrameSource &src, bool stamps) {
    if (src.kind == FrameSource::kDeviceFrame) return ingest(src, stamps);
    if (src.kind == FrameSource::kMessage) return ingest_msg(src, stamps);
    const uint64_t n = src.n;
    std::memcpy(h_pin.data(), src.rows, n * sizeof(Point4));
    HIPCHK(hipMemcpyAsync(d_in.data(), h_pin.data(), n * sizeof(Point4), hipMemcpyHostToDevice, stream.get()));
    if (stamps) {
        std::memcpy(h_ts.data(), src.stamps, n * sizeof(double));
        HIPCHK(hipMemcpyAsync(d_ts.data(), h_ts.data(), n * sizeof(double), hipMemcpyHostToDevice, stream.get()));
    }
    return SAGEICP_OK;
}

// The raw frame of a device frame into d_in (and its timestamps into d_ts), after the work the caller enqueued on
// its stream.  Timestamps are checked here, before anything reads them: a non-finite one refuses the frame (the
// host entry's check, sageicp_pipeline_register_frame_timestamps).  The caller's buffers are last read by this
// launch, which the first level's synchronisation waits for: run() returns with them released.
int Prep::ingest(const FrameSource &src, bool stamps) {
    if (int rc = stream_after_caller(ev_caller, src.stream, stream.get())) return rc;
    IngestArgs a = ingest_args(*src.frame);
    a.ts = stamps ? src.stamps : nullptr;
    a.ts_out = stamps ? d_ts.data() : nullptr;
    a.flags = d_overflow.data();
    launch_ingest(a, d_in.data(), stream.get());
    HIPCHK(hipGetLastError());
    return stamps ? refuse_bad_timestamp() : SAGEICP_OK;
}

// The same of a message's payload: host bytes cross PCIe as they are (through the pinned staging copy), device bytes
// are read in place behind the caller's stream.  uint32 stamps are normalised by their maximum in a second small
// pass (NormalizeTimestamps); float64 stamps are checked like a device frame's.
int Prep::ingest_msg(const FrameSource &m, bool stamps) {
    const size_t bytes = static_cast<size_t>(m.n) * m.layout.point_step;
    const unsigned char *d = m.payload;
    if (!m.payload_on_device) {
        if (bytes > h_blob.capacity()) {
            const size_t c = bytes + bytes / 4 + 4096;
            h_blob.reset();
            HIPCHK(d_blob.reserve(c));
            HIPCHK(h_blob.reserve(c));
        }
        std::memcpy(h_blob.data(), m.payload, bytes);
        HIPCHK(hipMemcpyAsync(d_blob.data(), h_blob.data(), bytes, hipMemcpyHostToDevice, stream.get()));
        d = d_blob.data();
    } else if (int rc = stream_after_caller(ev_caller, m.stream, stream.get())) {
        return rc;
    }
    MsgUnpackArgs a{};
    a.data = d;
    a.point_step = m.layout.point_step;
    a.x_offset = m.layout.x_offset; a.y_offset = m.layout.y_offset; a.z_offset = m.layout.z_offset;
    a.label_offset = m.layout.label_offset;
    a.label_dtype = m.layout.label_dtype;
    a.time_kind = stamps ? m.layout.time_kind : 0;
    a.time_offset = m.layout.time_offset;
    a.n = static_cast<int>(m.n);
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
    return a.time_kind == 2 ? refuse_bad_timestamp() : SAGEICP_OK;
}

// the flag word so far, read back: a stamp the load found not finite refuses the frame before deskew reads it
int Prep::refuse_bad_timestamp() {
    int flags = 0;
    HIPCHK(hipMemcpyAsync(&flags, d_overflow.data(), sizeof(int), hipMemcpyDeviceToHost, stream.get()));
    HIPCHK(hipStreamSynchronize(stream.get()));
    if (flags & kIngestBadTimestamp) return fail(SAGEICP_ERR_INVALID, "deskew is on and a timestamp is not finite");
    return SAGEICP_OK;
}

// the raw frame aside for the key-frame pass (its coordinates checked), then deskew in place
int Prep::keep_raw_and_deskew(uint64_t n, const DeskewTangent *deskew) {
    if (keep_raw) launch_occ_keep(d_in.data(), d_raw.data(), static_cast<int>(n), d_overflow.data(), stream.get());
    if (deskew) {
        launch_deskew(d_in.data(), d_in.data(), d_ts.data(), static_cast<int>(n), *deskew, stream.get());
        HIPCHK(hipGetLastError());
    }
    return SAGEICP_OK;
}

// One VoxelDownsample level: n points at `in` into dst, `kept` of them (the stream is idle after this).  With `reorder`
// the survivors' voxel keys are left in d_okeys for restore_reference_order.
int Prep::downsample(int level, const Point4 *in, uint64_t n, const PrepJob &job, bool reorder, Point4 *dst, uint32_t &kept) {
    VdsParams P{};
    P.in = in; P.n = static_cast<int>(n); P.do_crop = job.dyn ? 0 : job.levels[level].crop;
    P.max_range = job.max_range; P.min_range = job.min_range; P.label_max_range = job.label_max_range;
    P.n_groups = job.levels[level].scale > 0.0 ? job.n_groups : -1;
    P.group_counts = d_gcounts.data(); P.group_labels = d_glabels.data();
    for (int g = 0; g < job.n_groups; ++g) P.group_vs[g] = job.group_voxel_size[g];
    P.scale = job.levels[level].scale;
    P.keys = d_keys.data(); P.winner = d_winner.data(); P.mask = static_cast<uint32_t>(d_keys.capacity() - 1);
    P.tmp = d_tmp.data(); P.slot_of = d_slot.data(); P.sort_key = d_skey.data(); P.sort_val = d_sval.data();
    P.overflow = d_overflow.data();
    P.out_keys = reorder ? d_okeys.data() : nullptr;
    uint32_t *d_kept = d_nkept.data() + level;
    HIPCHK(voxel_downsample_device(P, d_sort_temp.data(), d_sort_temp.capacity(), d_kept, dst, stream.get()));
    HIPCHK(hipMemcpyAsync(&kept, d_kept, sizeof(uint32_t), hipMemcpyDeviceToHost, stream.get()));
    HIPCHK(hipStreamSynchronize(stream.get()));
    kept_levels[level] = kept;
    return SAGEICP_OK;
}

// The reference's emission order (Preprocessing.cpp:76-82): replay, group by group, the insertions into its robin_map
// and permute the `kept` survivors at dst (their keys are in d_okeys).
int Prep::restore_reference_order(int level, Point4 *dst, uint32_t kept) {
    const double t0 = now_us();
    HIPCHK(hipMemcpyAsync(h_keys.data(), d_okeys.data(), kept * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream.get()));
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
                  std::min<size_t>(hw, static_cast<size_t>(knobs().replay_threads.get())));
    } else {
        for (size_t r = 0; r < runs.size(); ++r) replay(r);
    }
    const double t2 = now_us();
    HIPCHK(hipMemcpyAsync(d_perm.data(), h_perm.data(), kept * sizeof(uint32_t), hipMemcpyHostToDevice, stream.get()));
    launch_vds_permute(dst, d_perm.data(), kept, d_tmp.data(), stream.get());
    HIPCHK(hipMemcpyAsync(dst, d_tmp.data(), kept * sizeof(Point4), hipMemcpyDeviceToDevice, stream.get()));
    if (knobs().debug_order.get()) {
        std::string rs;
        for (auto &r : runs) rs += " " + std::to_string(r.second - r.first);
        std::fprintf(stderr, "order level %d: kept %u, fetch keys %.0f us, replay %.0f us (runs:%s), rest %.0f us\n",
                     level, kept, t1 - t0, t2 - t1, rs.c_str(), now_us() - t2);
    }
    return SAGEICP_OK;
}

// what the kernels of this run flagged (every level has been waited for)
int Prep::refuse_flags() {
    int ovf = 0;
    HIPCHK(hipMemcpy(&ovf, d_overflow.data(), sizeof(int), hipMemcpyDeviceToHost));
    if (ovf & kOccNonFinite)
        return fail(SAGEICP_ERR_INVALID, "key-frame selection is on and a coordinate is not finite (NaN / Inf)");
    if (ovf & 2) return fail(SAGEICP_ERR_INVALID, "a label (or, without the range crop, a coordinate) is not finite (NaN / Inf)");
    if (ovf) return fail(SAGEICP_ERR_CAPACITY, "voxel index beyond +-2^19 in VoxelDownsample");
    return SAGEICP_OK;
}

// through the results' part of the staging buffer, as the raw frame went up through its first part
int Prep::fetch(int level, double *dst) {
    const uint32_t kept = kept_levels[level];
    if (!kept) return SAGEICP_OK;
    HIPCHK(hipSetDevice(device));
    Point4 *hp = h_pin.data() + static_cast<size_t>(1 + level) * cap;
    HIPCHK(hipMemcpyAsync(hp, (level ? d_src : d_fd).data(), kept * sizeof(Point4), hipMemcpyDeviceToHost, stream.get()));
    HIPCHK(hipStreamSynchronize(stream.get()));
    std::memcpy(dst, hp, kept * sizeof(Point4));
    return SAGEICP_OK;
}

}  // namespace sageicp
